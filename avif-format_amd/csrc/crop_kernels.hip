// crop_kernels.hip -- the cropped open: the clean aperture (clap) of an image applied on the GPU (include/avifgpu.h "cropped open").
//
// The decode arithmetic is not copied and no existing kernel is touched.  Output rows [orow0, orow0 + onrows) of orient(code, F[rect])
// come from a stored rectangle T (crop_geometry.h); what runs for it is built from the library's own entries on device pointers:
//   * interpolated chroma: chroma_upsample on rectangle T of the WHOLE planes (it clamps against the plane, so a crop sees the samples
//     outside it), the 4:4:4 open on (Y + offset, U(Cb), U(Cr), A + offset), for codes 2-8 the orient kernels behind it;
//   * replicated chroma: the existing open on the COVERING rectangle -- T with its start rounded down to even in every subsampled
//     direction -- from advanced plane pointers; straight into dst where T is its own covering rectangle and the code is 1, otherwise into
//     scratch, and crop_rows (code 1) or the orient kernels (codes 2-8) move the pixels of T from one pixel and / or one row in.
// The entry's shared argument checks and the host-pointer path are staged_open.cpp's, which this file gives its cut rule
// (crop_next_tile), the staged rectangle of a tile and the device path above.
//
// crop_rows.  A 2-D byte mover that knows nothing of colour: `rows` rows of `rb` bytes from src (any byte offset into rows of a pitch that
// is a multiple of 256) to dst (any base, any stride).  A wave owns 1 KiB of a destination row ON THE DESTINATION'S 16-BYTE GRID: chunk k
// of a row is the 16 bytes at head + 16 k, head = the bytes in front of the row's first 16-byte boundary; a lane loads its chunk as 16
// bytes at any address (the source sits wherever the offset pixel puts it, as orient_rows' does for a flipped x) and stores it
// non-temporally, aligned.  The ragged head (< 16 bytes) and tail (< 16 bytes) of a row go byte by byte, one lane each.  Bytes of a dst
// row beyond rb are not touched.  A translation unit -- and so a code object -- of its own: a process that never crops never loads it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "crop_geometry.h"

namespace avifgpu {

namespace {

typedef uint32_t cr_u4 __attribute__((ext_vector_type(4)));
typedef cr_u4 cr_u4_any __attribute__((aligned(1)));            // 16 bytes at any address

struct CropParams {
    const uint8_t* src; int64_t src_stride;
    uint8_t* dst; int64_t dst_stride;
    int64_t rb;                                  // payload bytes of a row
    int32_t rows;
};

constexpr int kCropThreads = 256;                // four waves, four neighbouring spans of a row

__global__ __launch_bounds__(kCropThreads) void crop_rows(const CropParams p)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t span = (int64_t)blockIdx.x * (kCropThreads / 64) + wave;
    const int64_t kc = span * 64 + lane;                                       // the lane's chunk of every row
    for (int row = (int)blockIdx.y; row < p.rows; row += (int)gridDim.y) {
        const uint8_t* const sp = p.src + (int64_t)row * p.src_stride;
        uint8_t* const dp = p.dst + (int64_t)row * p.dst_stride;
        const int64_t head = min((int64_t)((0 - reinterpret_cast<uintptr_t>(dp)) & 15), p.rb);
        const int64_t nc = (p.rb - head) >> 4;                                 // whole chunks behind the head
        if (kc < nc) {
            const int64_t off = head + kc * 16;                                // off + 16 <= rb
            const cr_u4 v = __builtin_nontemporal_load(reinterpret_cast<const cr_u4_any*>(sp + off));
            __builtin_nontemporal_store(v, reinterpret_cast<cr_u4*>(dp + off));
        }
        if (span == 0 && (int64_t)lane < head) dp[lane] = sp[lane];            // the ragged head
        const int64_t tail0 = head + nc * 16;
        if (span == (nc >> 6) && tail0 + (int64_t)lane < p.rb && lane < 16u) dp[tail0 + lane] = sp[tail0 + lane];   // the ragged tail, in the wave behind the last chunk
    }
}

hipError_t launch_crop(const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, int64_t rb, int rows, hipStream_t st)
{
    if (rb <= 0 || rows <= 0) return hipSuccess;
    CropParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.src_stride = src_stride; p.dst = dst; p.dst_stride = dst_stride; p.rb = rb; p.rows = rows;
    const int64_t spans = ((rb >> 4) + 1 + 63) / 64;                           // chunks of a row, + 1: the wave behind the last chunk owns the tail
    const dim3 grid((unsigned)((spans + 3) / 4), (unsigned)std::min(rows, 65535)), block(kCropThreads);
    hipLaunchKernelGGL(crop_rows, grid, block, 0, st, p);
    return hipGetLastError();
}

// the two chroma planes are interpolated: a bilinear mode on a subsampled YCbCr image
bool interpolated(const avifgpu_read_desc* d, const ReadGeom& g, int upsampling)
{
    return upsampling != AVIFGPU_UPSAMPLE_NEAREST && d->colorspace == AVIFGPU_COLORSPACE_YCBCR && g.xs != 0;
}

struct Call {
    ReadGeom g;
    bool interp;
    int ssz, bpp;            // bytes per plane sample / per host pixel
    int out_w, out_h;        // the cropped, oriented image
};

int check_cropped(const avifgpu_read_desc* d, const avifgpu_rect* rect, int upsampling, int code, Call& c, const char* who)
{
    if (!upsampling_ok(upsampling)) return fail(AVIFGPU_formatBadParameters, "%s: chroma upsampling %d is not an AVIFGPU_UPSAMPLE_* value", who, upsampling);
    if (!open_code_ok(code)) return fail(AVIFGPU_formatBadParameters, "%s: orientation %d is not an EXIF code 1..8", who, code);
    const int err = check_read(d, 0, 0, c.g);
    if (err) return err;
    if (!rect) return fail(AVIFGPU_formatBadParameters, "%s: null rectangle", who);
    if (!crop_rect_ok(*rect, d->width, d->height))
        return fail(AVIFGPU_formatBadParameters, "%s: rectangle (%d, %d, %d, %d) is not inside the %d x %d image", who, rect->x0, rect->y0, rect->width, rect->height, d->width, d->height);
    c.interp = interpolated(d, c.g, upsampling);
    c.ssz = d->bit_depth > 8 ? 2 : 1;
    c.bpp = c.g.nch * (d->depth / 8);
    crop_view_size(*rect, code, c.out_w, c.out_h);
    return 0;
}

// descriptor and plane pointers of stored rectangle r as a sub-image (r starts even wherever that matters: crop_cover)
void sub_image(const avifgpu_read_desc* d, const ReadGeom& g, int ssz, const avifgpu_rect& r, const void* const src[4], const int64_t src_stride[4],
               avifgpu_read_desc& sub, const void* out[4])
{
    sub = *d;
    sub.width = r.width; sub.height = r.height;
    for (int pl = 0; pl < 4; ++pl) {
        out[pl] = nullptr;
        if (!read_plane_used(d, g, pl) || !src[pl]) continue;
        const avifgpu_rect pr = crop_plane_rect(r, plane_is_chroma(d, pl), g.xs, g.ys);
        out[pl] = static_cast<const uint8_t*>(src[pl]) + (int64_t)pr.y0 * src_stride[pl] + (int64_t)pr.x0 * ssz;
    }
}

int64_t scratch_need(const avifgpu_read_desc* d, const Call& c, const avifgpu_rect& t, int code)
{
    const bool sub = d->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    return crop_scratch_bytes(t, sub ? c.g.xs : 0, sub ? c.g.ys : 0, c.interp, code, c.ssz, c.bpp, false, false);
}

// orient(code, F[t]) of the image whose WHOLE planes are src, on device pointers: everything is enqueued on st.
int open_rect_device(const avifgpu_read_desc* d, const Call& c, const avifgpu_rect& t, int upsampling, int code,
                     const void* const src[4], const int64_t src_stride[4], uint8_t* dst, int64_t dst_row_bytes, uint8_t* scratch, hipStream_t st)
{
    int err;
    hipError_t e;
    if (c.interp) {
        const int64_t up_pitch = align256((int64_t)t.width * c.ssz);
        void* const up[2] = { scratch, scratch + up_pitch * t.height };
        const void* const cplanes[2] = { src[1], src[2] };
        const int64_t cstrides[2] = { src_stride[1], src_stride[2] };
        if ((err = avifgpu_probe_upsample(c.ssz, d->chroma, upsampling, d->width, d->height, t.x0, t.y0, t.width, t.height, cplanes, cstrides, up, up_pitch, 0, st))) return err;
        avifgpu_read_desc sub = *d;
        sub.chroma = AVIFGPU_CHROMA_444; sub.width = t.width; sub.height = t.height;
        const int64_t yoff = (int64_t)t.y0 * src_stride[0] + (int64_t)t.x0 * c.ssz;
        const int64_t aoff = c.g.alpha ? (int64_t)t.y0 * src_stride[3] + (int64_t)t.x0 * c.ssz : 0;
        const void* const planes[4] = { static_cast<const uint8_t*>(src[0]) + yoff, up[0], up[1], c.g.alpha ? static_cast<const uint8_t*>(src[3]) + aoff : nullptr };
        const int64_t strides[4] = { src_stride[0], up_pitch, up_pitch, c.g.alpha ? src_stride[3] : 0 };
        if (code == 1) return avifgpu_read_rows(&sub, 0, sub.height, planes, strides, dst, dst_row_bytes, AVIFGPU_MEM_DEVICE, st);
        uint8_t* const img = scratch + 2 * up_pitch * t.height;
        const int64_t pitch = align256((int64_t)t.width * c.bpp);
        if ((err = avifgpu_read_rows(&sub, 0, sub.height, planes, strides, img, pitch, AVIFGPU_MEM_DEVICE, st))) return err;
        return avifgpu_probe_orient(code, c.bpp, t.width, t.height, img, pitch, dst, dst_row_bytes, st);
    }
    const bool subsampled = d->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    const CropCover k = crop_cover(t, subsampled ? c.g.xs : 0, subsampled ? c.g.ys : 0);
    avifgpu_read_desc sub; const void* psrc[4];
    sub_image(d, c.g, c.ssz, k.c, src, src_stride, sub, psrc);
    if (code == 1 && !k.px && !k.py)                           // the existing kernels, straight into dst
        return avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, dst, dst_row_bytes, AVIFGPU_MEM_DEVICE, st);
    const int64_t pitch = align256((int64_t)k.c.width * c.bpp);
    if ((err = avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, scratch, pitch, AVIFGPU_MEM_DEVICE, st))) return err;
    const uint8_t* const from = scratch + (int64_t)k.py * pitch + (int64_t)k.px * c.bpp;
    if (code != 1) return avifgpu_probe_orient(code, c.bpp, t.width, t.height, from, pitch, dst, dst_row_bytes, st);
    if ((e = launch_crop(from, pitch, dst, dst_row_bytes, (int64_t)t.width * c.bpp, t.height, st)) != hipSuccess) return hip_fail(e, "crop_rows launch", AVIFGPU_readErr);
    char label[kLabelBytes];
    snprintf(label, sizeof(label), "crop_rows rb=%lld rows=%d", (long long)t.width * c.bpp, t.height);
    set_last_kernel(label);
    return 0;
}

// ---- host path: the staged driver (staged_open.cpp) with the STAGED image of a tile (crop_stage_rect): only its part of each plane goes up,
// as a strided copy, and the device path treats it as a whole image --------------------------------------------------------------------
constexpr size_t kHostTileBytes = (size_t)16 << 20;             // output bytes of one staged tile

bool cut_matters(const avifgpu_read_desc* d, const Call& c, int code)
{
    if (c.interp || d->colorspace != AVIFGPU_COLORSPACE_YCBCR) return false;
    return (crop_turn(code).t ? c.g.xs : c.g.ys) != 0;
}

int read_rows_cropped_host(const avifgpu_read_desc* d, const Call& c, const avifgpu_rect& rect, int upsampling, int code, int orow0, int onrows,
                           const void* const src[4], const int64_t src_stride[4], uint8_t* dst, int64_t dst_row_bytes)
{
    const bool subsampled = d->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    const int xs = subsampled ? c.g.xs : 0, ys = subsampled ? c.g.ys : 0;
    const bool matters = cut_matters(d, c, code);
    const int64_t out_pitch = align256((int64_t)c.out_w * c.bpp);              // every tile's output is c.out_w wide
    avifgpu_read_desc sd = *d;                                 // the staged image
    avifgpu_rect tin;                                          // the tile's rectangle inside it
    const StagedPlan plan = [&](int o0, int left, int max_rows, StagedTile& t) {
        // cut inside the caller's range, on the helper's rule: the range's own end is a cut like any other
        t.n = std::min(crop_next_tile(rect, code, matters, o0, max_rows), left);
        tin = crop_tile_rect(rect, code, o0, t.n);
        const avifgpu_rect sr = crop_stage_rect(tin, d->width, d->height, xs, ys, c.interp);
        sd.width = sr.width; sd.height = sr.height;
        for (int pl = 0; pl < 4; ++pl) {
            if (!read_plane_used(d, c.g, pl) || !src[pl]) continue;
            const avifgpu_rect pr = crop_plane_rect(sr, plane_is_chroma(d, pl), xs, ys);
            const int64_t wbytes = (int64_t)pr.width * c.ssz;
            t.up[pl] = { static_cast<const uint8_t*>(src[pl]) + (int64_t)pr.y0 * src_stride[pl] + (int64_t)pr.x0 * c.ssz, src_stride[pl], wbytes, pr.height, align256(wbytes) };
        }
        tin.x0 -= sr.x0; tin.y0 -= sr.y0;
        t.out_pitch = out_pitch;
        t.scratch_bytes = scratch_need(&sd, c, tin, code);
        return 0;
    };
    const StagedEnqueue enqueue = [&](const StagedBuffers& b) {
        return open_rect_device(&sd, c, tin, upsampling, code, b.plane, b.pitch, static_cast<uint8_t*>(b.out), out_pitch, static_cast<uint8_t*>(b.scratch), b.stream);
    };
    return staged_open("cropped open", kHostTileBytes, (int64_t)c.out_w * c.bpp, orow0, onrows, dst, dst_row_bytes, plan, enqueue);
}

// the call is one the upsampled open serves byte for byte: the whole image, cut where that entry allows
bool hand_on(const avifgpu_read_desc* d, const Call& c, const avifgpu_rect& rect, int code, const avifgpu_rect& t, int onrows)
{
    if (!crop_rect_is_whole(rect, d->width, d->height)) return false;
    const bool subsampled = d->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    const CropTurn o = crop_turn(code);
    const bool cut_sub = subsampled && (o.t ? c.g.xs : c.g.ys) != 0;
    const int start = o.t ? t.x0 : t.y0;
    return !cut_sub || (start & 1) == 0 || onrows <= 1;
}

} // namespace

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_clap_to_rect(int32_t width, int32_t height, const int32_t clap[8], avifgpu_rect* out)
{
    set_error("");
    if (width < 1 || height < 1 || !clap || !out) return fail(AVIFGPU_formatBadParameters, "avifgpu_clap_to_rect: bad size or null argument");
    avifgpu_rect r;
    if (!clap_to_rect(width, height, clap, r))
        return fail(AVIFGPU_formatBadParameters, "avifgpu_clap_to_rect: aperture %d/%d x %d/%d at %d/%d, %d/%d has a denominator or a size <= 0 or lies outside the %d x %d image",
                    clap[0], clap[1], clap[2], clap[3], clap[4], clap[5], clap[6], clap[7], width, height);
    *out = r;
    return 0;
}

int32_t avifgpu_crop_compose(const avifgpu_rect* current, int32_t code, const avifgpu_rect* crop_in_view, avifgpu_rect* out)
{
    set_error("");
    if (!current || !crop_in_view || !out) return fail(AVIFGPU_formatBadParameters, "avifgpu_crop_compose: null argument");
    avifgpu_rect r;
    if (!crop_compose(*current, code, *crop_in_view, r))
        return fail(AVIFGPU_formatBadParameters, "avifgpu_crop_compose: code %d is not 1..8, or a rectangle is empty, negative or outside its view", code);
    *out = r;
    return 0;
}

int32_t avifgpu_read_cropped_geometry(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t orientation, int32_t* out_w, int32_t* out_h)
{
    set_error("");
    Call c;
    const int err = check_cropped(desc, rect, AVIFGPU_UPSAMPLE_NEAREST, orientation, c, "avifgpu_read_cropped_geometry");
    if (err) return err;
    if (!out_w || !out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_cropped_geometry: null argument");
    *out_w = c.out_w; *out_h = c.out_h;
    return 0;
}

int32_t avifgpu_read_cropped_next_tile(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t max_rows)
{
    set_error("");
    Call c;
    const int err = check_cropped(desc, rect, upsampling, orientation, c, "avifgpu_read_cropped_next_tile");
    if (err) return err;
    if (orow0 < 0 || orow0 >= c.out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_cropped_next_tile: row %d outside the %d rows of the image", orow0, c.out_h);
    if (max_rows < 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_cropped_next_tile: max_rows %d < 1", max_rows);
    return crop_next_tile(*rect, orientation, cut_matters(desc, c, orientation), orow0, max_rows);
}

int64_t avifgpu_read_cropped_scratch_bytes(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation, int32_t onrows)
{
    set_error("");
    Call c;
    const int err = check_cropped(desc, rect, upsampling, orientation, c, "avifgpu_read_cropped_scratch_bytes");
    if (err) return err;
    if (onrows < 0 || onrows > c.out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_cropped_scratch_bytes: %d rows of an image of %d", onrows, c.out_h);
    const CropTurn o = crop_turn(orientation);
    avifgpu_rect t = *rect;
    if (o.t) t.width = onrows; else t.height = onrows;
    const bool subsampled = desc->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    return crop_scratch_bytes(t, subsampled ? c.g.xs : 0, subsampled ? c.g.ys : 0, c.interp, orientation, c.ssz, c.bpp, o.t, !o.t);
}

int32_t avifgpu_read_rows_cropped(const avifgpu_read_desc* desc, const avifgpu_rect* rect, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t onrows,
                                  const void* const src[4], const int64_t src_stride[4], void* dst, int64_t dst_row_bytes,
                                  void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream)
{
    set_error("");
    Call c;
    int err = check_cropped(desc, rect, upsampling, orientation, c, "avifgpu_read_rows_cropped");
    if (err) return err;
    if (orow0 < 0 || onrows < 0 || (int64_t)orow0 + onrows > c.out_h)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_cropped: rows [%d, %d + %d) outside the %d rows of the cropped image", orow0, orow0, onrows, c.out_h);
    const avifgpu_rect t = crop_tile_rect(*rect, orientation, orow0, onrows);
    const int64_t need = scratch_need(desc, c, t, orientation);
    const OpenEntry entry = { "avifgpu_read_rows_cropped", "avifgpu_read_cropped_scratch_bytes", desc, &c.g, c.out_w, c.bpp, onrows,
                              src, src_stride, dst, dst_row_bytes, scratch, scratch_bytes, mem_kind };
    err = check_open_entry(entry, need, [&](int step) {
        if (step == 0 && hand_on(desc, c, *rect, orientation, t, onrows)) {      // the existing entries, byte for byte; the new code object is not loaded
            const int rc = avifgpu_read_rows_upsampled(desc, upsampling, orientation, orow0, onrows, src, src_stride, dst, dst_row_bytes, scratch, scratch_bytes, mem_kind, stream);
            return rc ? rc : kOpenEntryOver;
        }
        if (step == 1 && c.interp && ((int64_t)t.height + 31) / 32 > 65535) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_cropped: a region of %d rows (cut it)", t.height);
        return 0;
    });
    if (err) return err == kOpenEntryOver ? 0 : err;

    if (mem_kind == AVIFGPU_MEM_DEVICE)
        return open_rect_device(desc, c, t, upsampling, orientation, src, src_stride, static_cast<uint8_t*>(dst), dst_row_bytes, static_cast<uint8_t*>(scratch), (hipStream_t)stream);
    if (orientation == 1 && need == 0) {
        // nothing to move: avifgpu_read_rows on the sub-image, the tile loop of every bound context -- but only where the advanced HOST
        // pointers stay on the 16-byte grid: from pointers a few bytes off it that path's uploads were measured 1.7x (f32) to 4.7x (8 bit)
        // slower than from aligned ones, while the staged path below copies from an aligned column
        avifgpu_read_desc sub; const void* psrc[4];
        sub_image(desc, c.g, c.ssz, t, src, src_stride, sub, psrc);
        bool on_grid = true;
        for (int pl = 0; pl < 4; ++pl)
            if (psrc[pl]) on_grid = on_grid && ((static_cast<const uint8_t*>(psrc[pl]) - static_cast<const uint8_t*>(src[pl])) % src_stride[pl]) % 16 == 0;
        if (on_grid) return avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, dst, dst_row_bytes, AVIFGPU_MEM_HOST, nullptr);
    }
    return read_rows_cropped_host(desc, c, *rect, upsampling, orientation, orow0, onrows, src, src_stride, static_cast<uint8_t*>(dst), dst_row_bytes);
}

int32_t avifgpu_probe_crop(const void* src, int64_t src_row_bytes, void* dst, int64_t dst_row_bytes, int64_t row_payload_bytes, int32_t rows, void* stream)
{
    set_error("");
    if (!src || !dst || row_payload_bytes < 1 || rows < 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_crop: bad size or null buffer");
    if (src_row_bytes < row_payload_bytes || dst_row_bytes < row_payload_bytes) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_crop: row bytes too small");
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    const hipError_t e = launch_crop(static_cast<const uint8_t*>(src), src_row_bytes, static_cast<uint8_t*>(dst), dst_row_bytes, row_payload_bytes, rows, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_crop", AVIFGPU_readErr);
}

} // extern "C"
