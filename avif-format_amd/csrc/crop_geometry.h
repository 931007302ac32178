// crop_geometry.h -- the arithmetic of the cropped open (include/avifgpu.h "cropped open"): the clean-aperture rule, how a
// crop in an oriented view maps back to the stored image, which stored rectangle a range of output rows comes from, what has to be decoded
// for it (the COVERING rectangle) and what the host path uploads for it.  Plain integer arithmetic shared by csrc/crop_kernels.hip and a
// stand-alone host program (tools/crop_geometry_check.cpp) that sweeps it under the sanitizers: no HIP type, no device call.
#pragma once
#include <stdint.h>

#include "../../include/avifgpu.h"
#include "open_geometry.h"
#include "upsample_window.h"

namespace avifgpu {

// the one code table (open_geometry.h) under the names this file and its check program have always used
using CropTurn = OpenTurn;
inline CropTurn crop_turn(int code) { return kOpenTurn[code]; }

// a rectangle of a width x height image: 0 <= x0, 1 <= w, x0 + w <= width, and the same in y
inline bool crop_rect_ok(const avifgpu_rect& r, int width, int height)
{
    return r.x0 >= 0 && r.y0 >= 0 && r.width >= 1 && r.height >= 1 && (int64_t)r.x0 + r.width <= width && (int64_t)r.y0 + r.height <= height;
}
inline bool crop_rect_is_whole(const avifgpu_rect& r, int width, int height) { return r.x0 == 0 && r.y0 == 0 && r.width == width && r.height == height; }

// ---- ISO 14496-12 clean aperture -> rectangle --------------------------------------------------------------------------------------------
// One direction: size, aperture N / D, offset N / D -> first and last sample, exact.  With c = (size - 1) / 2 and a = (ap - 1) / 2 the edges
// are off + c -+ a; over the common denominator 2 offD apD they are integers of at most 96 bits, so __int128 holds every intermediate of
// 32-bit operands: nothing overflows and nothing has to be rejected for its size.  Each edge is rounded half up, floor(v + 1/2), and then
// clamped to [0, size - 1] (still in 128 bits).  false: a denominator or the aperture is not positive, or nothing is left.
inline __int128 crop_floor_div(__int128 n, __int128 d) { __int128 q = n / d; if ((n % d != 0) && ((n < 0) != (d < 0))) --q; return q; }
inline bool clap_edges(int size, int32_t apN, int32_t apD, int32_t offN, int32_t offD, int32_t& first, int32_t& count)
{
    if (size < 1 || apD <= 0 || offD <= 0 || apN <= 0) return false;
    const __int128 den = (__int128)2 * offD * apD;
    const __int128 mid = (__int128)2 * offN * apD + (__int128)(size - 1) * offD * apD;
    const __int128 half = ((__int128)apN - apD) * offD;                  // (ap - 1) / 2 over den; negative for an aperture below one sample
    __int128 lo = crop_floor_div(2 * (mid - half) + den, 2 * den);
    __int128 hi = crop_floor_div(2 * (mid + half) + den, 2 * den);
    if (lo < 0) lo = 0;
    if (hi > size - 1) hi = size - 1;
    if (hi < lo) return false;
    first = (int32_t)lo; count = (int32_t)(hi - lo + 1);
    return true;
}

// clap = { widthN, widthD, heightN, heightD, horizOffN, horizOffD, vertOffN, vertOffD }.  false = formatBadParameters.
inline bool clap_to_rect(int width, int height, const int32_t clap[8], avifgpu_rect& out)
{
    avifgpu_rect r;
    if (!clap_edges(width, clap[0], clap[1], clap[4], clap[5], r.x0, r.width)) return false;
    if (!clap_edges(height, clap[2], clap[3], clap[6], clap[7], r.y0, r.height)) return false;
    out = r;
    return true;
}

// ---- a crop given in the coordinates of view = orient(code, F[current]) -> the stored rectangle ----------------------------------------------
inline void crop_view_size(const avifgpu_rect& r, int code, int& vw, int& vh)
{
    open_view_size(r.width, r.height, code, vw, vh);
}
inline bool crop_compose(const avifgpu_rect& cur, int code, const avifgpu_rect& v, avifgpu_rect& out)
{
    if (!open_code_ok(code) || cur.x0 < 0 || cur.y0 < 0 || cur.width < 1 || cur.height < 1) return false;
    if ((int64_t)cur.x0 + cur.width > 0x7fffffffLL || (int64_t)cur.y0 + cur.height > 0x7fffffffLL) return false;
    int vw, vh;
    crop_view_size(cur, code, vw, vh);
    if (!crop_rect_ok(v, vw, vh)) return false;
    const CropTurn o = crop_turn(code);
    // the view's x' runs along the source's x (row-mapped) or y (transposing); its y' along the other
    const int along_x0 = v.x0, along_xn = v.width, along_y0 = v.y0, along_yn = v.height;
    int sx, sw, sy, sh;
    if (!o.t) {
        sw = along_xn; sx = o.fx ? cur.width - along_x0 - along_xn : along_x0;
        sh = along_yn; sy = o.fy ? cur.height - along_y0 - along_yn : along_y0;
    } else {
        sh = along_xn; sy = o.fy ? cur.height - along_x0 - along_xn : along_x0;
        sw = along_yn; sx = o.fx ? cur.width - along_y0 - along_yn : along_y0;
    }
    out.x0 = cur.x0 + sx; out.y0 = cur.y0 + sy; out.width = sw; out.height = sh;
    return true;
}

// ---- output rows [orow0, orow0 + onrows) of orient(code, F[rect]) -> the stored rectangle they come from ------------------------------------
// a row range of rect for codes 1-4, a column band for codes 5-8; the caller has checked 0 <= orow0, 0 <= onrows, orow0 + onrows <= view height
inline avifgpu_rect crop_tile_rect(const avifgpu_rect& rect, int code, int orow0, int onrows)
{
    const CropTurn o = crop_turn(code);
    avifgpu_rect t = rect;
    if (!o.t) { t.y0 = rect.y0 + (o.fy ? rect.height - orow0 - onrows : orow0); t.height = onrows; }
    else      { t.x0 = rect.x0 + (o.fx ? rect.width - orow0 - onrows : orow0); t.width = onrows; }
    return t;
}

// The nearest open replicates chroma sample (x >> xs, y >> ys): a sub-image decoded from advanced plane pointers sees the right samples
// only if it starts on an even index of every subsampled direction -- or is a single column / row, which is its own chroma sample.  The
// COVERING rectangle starts one column / row earlier where it has to; (px, py) is where the wanted rectangle starts inside it.
struct CropCover { avifgpu_rect c; int px, py; };
inline CropCover crop_cover(const avifgpu_rect& t, int xs, int ys)
{
    CropCover k;
    k.px = (xs && (t.x0 & 1) && t.width > 1) ? 1 : 0;
    k.py = (ys && (t.y0 & 1) && t.height > 1) ? 1 : 0;
    k.c.x0 = t.x0 - k.px; k.c.y0 = t.y0 - k.py; k.c.width = t.width + k.px; k.c.height = t.height + k.py;
    return k;
}

// Device scratch for the stored rectangle t (see avifgpu_read_cropped_scratch_bytes): interp = the two upsampled chroma rectangles are
// needed; s / b = bytes per plane sample / per host pixel.  worst_x / worst_y: count the covering column / row whether t starts odd or not
// (the helper does not know where a tile will start in the cut direction).
inline int64_t crop_scratch_bytes(const avifgpu_rect& t, int xs, int ys, bool interp, int code, int s, int b, bool worst_x, bool worst_y)
{
    if (t.width < 1 || t.height < 1) return 0;
    if (interp) return 2 * align256((int64_t)t.width * s) * t.height + (code == 1 ? 0 : align256((int64_t)t.width * b) * t.height);
    const int px = (xs && t.width > 1 && (worst_x || (t.x0 & 1))) ? 1 : 0;
    const int py = (ys && t.height > 1 && (worst_y || (t.y0 & 1))) ? 1 : 0;
    if (code == 1 && !px && !py) return 0;
    return align256((int64_t)(t.width + px) * b) * (t.height + py);
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------------------------
// Every cut is legal; an odd absolute start of a subsampled cut direction only costs the covering row / column and the mover.  matters =
// nearest open and the cut direction is subsampled.  Unflipped direction: the start of THIS tile is given, so n is chosen such that the
// NEXT tile starts on an even absolute index; flipped direction: a tile's region starts where it ends in output order, so n is chosen such
// that THIS tile's region does (the last tile starts where the rectangle starts).  Never below 1.
inline int crop_next_tile(const avifgpu_rect& rect, int code, bool matters, int orow0, int max_rows)
{
    const CropTurn o = crop_turn(code);
    const int out_h = o.t ? rect.width : rect.height;
    const int a0 = o.t ? rect.x0 : rect.y0;
    const int rest = out_h - orow0;
    int n = max_rows < rest ? max_rows : rest;
    if (!matters || n >= rest || n <= 1) return n;
    const bool flipped = o.t ? o.fx : o.fy;
    const int edge = flipped ? a0 + out_h - orow0 - n : a0 + orow0 + n;      // the absolute index the cut falls on, either way
    if (edge & 1) --n;
    return n;
}

// ---- host path: what goes up for the stored rectangle t --------------------------------------------------------------------------------------
// The STAGED image s is a sub-image of the stored one that the device path can treat as a whole image: it starts on an even index of every
// subsampled direction (so chroma sample (x >> xs) of the stored image is sample ((x - s.x0) >> xs) of the staged planes), and for an
// interpolated open it holds every chroma sample the taps of t touch (up_need, upsample_window.h), so clamping at the staged planes' edge
// IS clamping at the whole plane's edge or never happens.  Its first column is then rounded down to a multiple of 32 (kCropStageColumns).  t sits at (t.x0 - s.x0, t.y0 - s.y0) inside it.
inline avifgpu_rect crop_stage_rect_exact(const avifgpu_rect& t, int width, int height, int xs, int ys, bool interp);
constexpr int kCropStageColumns = 32;           // the staged image starts on a multiple of this many columns: the host side of every plane's upload is 16-byte aligned within its row
inline avifgpu_rect crop_stage_rect(const avifgpu_rect& t, int width, int height, int xs, int ys, bool interp)
{
    avifgpu_rect s = crop_stage_rect_exact(t, width, height, xs, ys, interp);
    const int a = s.x0 / kCropStageColumns * kCropStageColumns;       // more real samples on the left: nothing that was clamped is clamped differently
    s.width += s.x0 - a; s.x0 = a;
    return s;
}
inline avifgpu_rect crop_stage_rect_exact(const avifgpu_rect& t, int width, int height, int xs, int ys, bool interp)
{
    avifgpu_rect s = t;
    if (interp) {
        const int cw = (width + xs) >> xs, ch = (height + ys) >> ys;
        const UpNeed n = up_need(cw, ch, ys, t.x0, t.y0, t.width, t.height);
        const int x1 = 2 * n.hi + 2 < width ? 2 * n.hi + 2 : width;
        s.x0 = 2 * n.lo; s.width = x1 - s.x0;
        if (ys) {
            const int y1 = 2 * n.rhi + 2 < height ? 2 * n.rhi + 2 : height;
            s.y0 = 2 * n.rlo; s.height = y1 - s.y0;
        }
        return s;
    }
    if (xs && (t.x0 & 1)) { s.x0 -= 1; s.width += 1; }
    if (ys && (t.y0 & 1)) { s.y0 -= 1; s.height += 1; }
    return s;
}

// plane `chroma` ? (x >> xs, y >> ys) : (x, y): the sample rectangle of a staged image in one plane
inline avifgpu_rect crop_plane_rect(const avifgpu_rect& s, bool chroma, int xs, int ys)
{
    if (!chroma) return s;
    avifgpu_rect p;
    p.x0 = s.x0 >> xs; p.y0 = s.y0 >> ys; p.width = (s.width + xs) >> xs; p.height = (s.height + ys) >> ys;
    return p;
}

} // namespace avifgpu
