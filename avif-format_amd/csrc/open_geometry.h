// open_geometry.h -- the arithmetic that the oriented, upsampled and cropped opens share: the one table of the eight
// EXIF codes, the size of a view, which source region a range of output rows comes from, and where such a range may be cut.  Plain integer
// arithmetic shared by the three kernel files, crop_geometry.h and a stand-alone host program (tools/open_geometry_check.cpp) that sweeps it
// under the sanitizers: no HIP type, no device call.
#pragma once
#include <stdint.h>

#include "../../include/avifgpu.h"

namespace avifgpu {

// code -> (transpose, flip x, flip y) of the SOURCE coordinate:
//   row-mapped  (codes 1 .. 4)   view(y', x') = src(fy ? H - 1 - y' : y',  fx ? W - 1 - x' : x')
//   transposing (codes 5 .. 8)   view(y', x') = src(fy ? H - 1 - x' : x',  fx ? W - 1 - y' : y')
struct OpenTurn { bool t, fx, fy; };
constexpr OpenTurn kOpenTurn[9] = { { false, false, false }, { false, false, false }, { false, true, false }, { false, true, true }, { false, false, true },
                                    { true, false, false }, { true, false, true }, { true, true, true }, { true, true, false } };
inline bool open_code_ok(int code) { return code >= 1 && code <= 8; }

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// the view of a w x h image under a code
inline void open_view_size(int w, int h, int code, int& vw, int& vh) { vw = kOpenTurn[code].t ? h : w; vh = kOpenTurn[code].t ? w : h; }

// the view as a permutation of w x h labels (host only): the definition the region below is checked against
inline void apply_code(int code, const int* in, int w, int h, int* out, int& ow, int& oh)
{
    const OpenTurn o = kOpenTurn[code];
    open_view_size(w, h, code, ow, oh);
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            const int sy = o.t ? (o.fy ? h - 1 - x : x) : (o.fy ? h - 1 - y : y);
            const int sx = o.t ? (o.fx ? w - 1 - y : y) : (o.fx ? w - 1 - x : x);
            out[y * ow + x] = in[sy * w + sx];
        }
}

// ---- the source region of output rows [orow0, orow0 + onrows): a row range for codes 1-4, a column band for codes 5-8 ----------------------
struct OpenRegion {
    OpenTurn o;
    int out_w, out_h;        // the oriented image
    int start;               // first source row (codes 1-4) / column (codes 5-8) of the region
    int sub_w, sub_h;        // the region = the sub-image that is decoded
    int x0, y0;              // its origin in the stored image
    int bpp;                 // bytes of a host pixel
    bool flipped;            // the cut direction runs backwards: the region starts where the rows end
    bool subsampled;         // the cut direction is subsampled
};

// false, with out_w / out_h filled: the rows are not inside the view.  xs / ys: the image's chroma shifts.
inline bool open_region(int w, int h, int xs, int ys, int bpp, int code, int orow0, int onrows, OpenRegion& r)
{
    r.o = kOpenTurn[code];
    open_view_size(w, h, code, r.out_w, r.out_h);
    r.bpp = bpp;
    if (orow0 < 0 || onrows < 0 || (int64_t)orow0 + onrows > r.out_h) return false;
    r.flipped = r.o.t ? r.o.fx : r.o.fy;
    r.start = r.flipped ? r.out_h - orow0 - onrows : orow0;
    r.sub_w = r.o.t ? onrows : w;
    r.sub_h = r.o.t ? h : onrows;
    r.x0 = r.o.t ? r.start : 0;
    r.y0 = r.o.t ? 0 : r.start;
    r.subsampled = (r.o.t ? xs : ys) != 0;
    return true;
}

// a region of a subsampled direction starts on an even index; a single row / column is its own chroma sample wherever it lies
inline bool legal_cut(const OpenRegion& r, int onrows) { return !r.subsampled || (r.start & 1) == 0 || onrows <= 1; }

inline bool plane_is_chroma(const avifgpu_read_desc* d, int pl) { return d->colorspace == AVIFGPU_COLORSPACE_YCBCR && (pl == 1 || pl == 2); }
inline bool upsampling_ok(int u) { return u >= AVIFGPU_UPSAMPLE_NEAREST && u <= AVIFGPU_UPSAMPLE_BILINEAR_LEFT; }

} // namespace avifgpu
