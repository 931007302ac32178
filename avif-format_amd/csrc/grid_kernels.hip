// grid_kernels.hip -- the grid open: a tiled (grid) image opened from its decoded tiles (include/avifgpu.h "grid open").
//
// The decode arithmetic is not copied and no existing kernel is touched.  Output rows [orow0, orow0 + onrows) of the cropped, oriented
// image come from a stored rectangle T; the cropped open's host path already says which STAGED rectangle of every plane it needs for T
// (crop_geometry.h: the region, its covering row / column or bilinear halo, from a column that is a multiple of 32).  Here that rectangle
// of every ASSEMBLED plane is put together from the tiles -- by grid_gather on device pointers, by one strided copy per intersecting tile
// (grid_geometry.h: grid_pieces) on host pointers -- and avifgpu_read_rows_cropped runs on it as on a whole image: what a staged tile of
// the cropped open runs after its upload.
//
// grid_gather<S>.  A byte mover that knows nothing of colour: rectangle [x0, x0 + w) x [y0, y0 + h) of up to four assembled planes (grid.z)
// into contiguous rows whose base and pitch are multiples of 256.  A lane owns 16 bytes of a destination row, a wave 1 KiB, a workgroup
// 4 KiB; grid.y rows with crop_rows' row loop.  The tile row is uniform for a workgroup row; the tile column costs a lane one unsigned
// division.  Where a lane's 16 bytes lie inside one tile it loads them at any address and stores them non-temporally, aligned; where they
// straddle a seam (several, for tiles narrower than 16 bytes) or are the row's tail of fewer than 16 bytes, it places each sample on its
// own.  Bytes of a destination row beyond the payload are not touched.  No LDS, no atomics.  A translation unit -- and so a code object --
// of its own: a process that never opens a grid never loads it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "crop_geometry.h"
#include "grid_geometry.h"

namespace avifgpu {

namespace {

typedef uint32_t gr_u4 __attribute__((ext_vector_type(4)));
typedef gr_u4 gr_u4_any __attribute__((aligned(1)));            // 16 bytes at any address
// A tile's plane pointer comes out of the table, so the compiler cannot know its address space and would emit flat loads; the table holds
// device (global) pointers and nothing else.
#define AG_GRID_GLOBAL __attribute__((address_space(1)))

struct GridPlane {
    uint8_t* dst; int64_t pitch;                 // multiples of 16
    int32_t plane;                               // which pointer of a tile record
    int32_t tw, th;                              // a tile's extent in this plane, samples
    int32_t x0, y0, w, h;                        // the rectangle of the assembled plane; w == 0: nothing
};
struct GridParams {
    const avifgpu_grid_tile* tiles; int32_t columns;
    GridPlane pl[4];
};

constexpr int kGridThreads = 256;                // four waves, four neighbouring spans of a row

template <int S> struct GridSample;
template <> struct GridSample<1> { typedef uint8_t type; };
template <> struct GridSample<2> { typedef uint16_t type; };

template <int S>
__global__ __launch_bounds__(kGridThreads) void grid_gather(const GridParams p)
{
    typedef typename GridSample<S>::type sample_t;
    const GridPlane& q = p.pl[blockIdx.z];
    const int64_t rb = (int64_t)q.w * S;                                       // payload bytes of a row
    const int64_t off = ((int64_t)blockIdx.x * kGridThreads + threadIdx.x) * 16;   // the lane's 16 bytes of every row
    if (off >= rb) return;
    const int n = (int)min((int64_t)16, rb - off) / S;                         // samples of this lane
    const uint32_t x = (uint32_t)q.x0 + (uint32_t)(off / S);                   // the first one's column in the assembled plane
    const uint32_t tw = (uint32_t)q.tw;
    const uint32_t tc = x / tw, tx = x - tc * tw;
    const bool whole = n == 16 / S && tx + 16 / S <= tw;                       // 16 bytes inside one tile
    for (int row = (int)blockIdx.y; row < q.h; row += (int)gridDim.y) {
        const uint32_t y = (uint32_t)q.y0 + (uint32_t)row;
        const uint32_t tr = y / (uint32_t)q.th, ty = y - tr * (uint32_t)q.th;
        const avifgpu_grid_tile* const trow = p.tiles + (int64_t)tr * p.columns;
        uint8_t* const dp = q.dst + (int64_t)row * q.pitch + off;
        if (whole) {
            const avifgpu_grid_tile* const t = trow + tc;
            const uint8_t* const sp = static_cast<const uint8_t*>(t->plane[q.plane]) + (int64_t)ty * t->stride[q.plane] + (int64_t)tx * S;
            const gr_u4 v = __builtin_nontemporal_load((const AG_GRID_GLOBAL gr_u4_any*)sp);
            __builtin_nontemporal_store(v, reinterpret_cast<gr_u4*>(dp));
        } else {
            uint32_t c = tc, cx = tx;
            for (int i = 0; i < n; ++i) {
                const avifgpu_grid_tile* const t = trow + c;
                const uint8_t* const sp = static_cast<const uint8_t*>(t->plane[q.plane]) + (int64_t)ty * t->stride[q.plane];
                reinterpret_cast<sample_t*>(dp)[i] = ((const AG_GRID_GLOBAL sample_t*)sp)[cx];
                if (++cx == tw) { cx = 0; ++c; }
            }
        }
    }
}

// one launch for all planes of p with w > 0 in slots [0, nplanes)
hipError_t launch_gather(const GridParams& p, int nplanes, int s, hipStream_t st)
{
    int64_t rb = 0; int rows = 0;
    for (int i = 0; i < nplanes; ++i) { rb = std::max(rb, (int64_t)p.pl[i].w * s); rows = std::max(rows, (int)p.pl[i].h); }
    if (rb <= 0 || rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((rb + kGridThreads * 16 - 1) / (kGridThreads * 16)), (unsigned)std::min(rows, 65535), (unsigned)nplanes), block(kGridThreads);
    if (s == 1) hipLaunchKernelGGL(grid_gather<1>, grid, block, 0, st, p);
    else        hipLaunchKernelGGL(grid_gather<2>, grid, block, 0, st, p);
    return hipGetLastError();
}

// ---- the entry ---------------------------------------------------------------------------------------------------------------------------
struct Call {
    ReadGeom g;
    bool interp;
    int xs, ys;              // the chroma shifts where they subsample planes (YCbCr), 0 otherwise
    int ssz, bpp;            // bytes per plane sample / per host pixel
    int out_w, out_h;        // the cropped, oriented image
    avifgpu_rect rect;       // the caller's, or the whole canvas
};

int check_grid(const avifgpu_read_desc* d, const avifgpu_grid* grid, const avifgpu_rect* rect, int upsampling, int code, Call& c, const char* who)
{
    if (!upsampling_ok(upsampling)) return fail(AVIFGPU_formatBadParameters, "%s: chroma upsampling %d is not an AVIFGPU_UPSAMPLE_* value", who, upsampling);
    if (!open_code_ok(code)) return fail(AVIFGPU_formatBadParameters, "%s: orientation %d is not an EXIF code 1..8", who, code);
    const int err = check_read(d, 0, 0, c.g);
    if (err) return err;
    if (!grid) return fail(AVIFGPU_formatBadParameters, "%s: null grid", who);
    const bool subsampled = d->colorspace == AVIFGPU_COLORSPACE_YCBCR;
    c.xs = subsampled ? c.g.xs : 0; c.ys = subsampled ? c.g.ys : 0;
    const char* const why = grid_illegal(d->width, d->height, c.xs, c.ys, *grid);
    if (why) return fail(AVIFGPU_formatBadParameters, "%s: %d x %d tiles of %d x %d for a %d x %d canvas: %s", who, grid->columns, grid->rows, grid->tile_width, grid->tile_height, d->width, d->height, why);
    const avifgpu_rect whole = { 0, 0, d->width, d->height };
    c.rect = rect ? *rect : whole;
    if (!crop_rect_ok(c.rect, d->width, d->height))
        return fail(AVIFGPU_formatBadParameters, "%s: rectangle (%d, %d, %d, %d) is not inside the %d x %d canvas", who, c.rect.x0, c.rect.y0, c.rect.width, c.rect.height, d->width, d->height);
    c.interp = upsampling != AVIFGPU_UPSAMPLE_NEAREST && subsampled && c.g.xs != 0;
    c.ssz = d->bit_depth > 8 ? 2 : 1;
    c.bpp = c.g.nch * (d->depth / 8);
    crop_view_size(c.rect, code, c.out_w, c.out_h);
    return 0;
}

// avifgpu_read_grid_scratch_bytes' formula
int64_t grid_scratch_bytes(const avifgpu_read_desc* d, const Call& c, int code, int onrows)
{
    if (onrows < 1) return 0;
    const CropTurn o = crop_turn(code);
    avifgpu_rect t = c.rect;
    if (o.t) t.width = onrows; else t.height = onrows;
    const int gw = grid_stage_bound(t.width, kGridStageColumns, d->width), gh = grid_stage_bound(t.height, kGridStageRows, d->height);
    int64_t total = 256;
    for (int pl = 0; pl < 4; ++pl) {
        if (!read_plane_used(d, c.g, pl)) continue;
        const bool chroma = plane_is_chroma(d, pl);
        total += align256((int64_t)(chroma ? (gw + c.xs) >> c.xs : gw) * c.ssz) * (chroma ? (gh + c.ys) >> c.ys : gh);
    }
    return total + crop_scratch_bytes(t, c.xs, c.ys, c.interp, code, c.ssz, c.bpp, true, true);
}

// The staged image of the output rows [o0, o0 + n): its descriptor, where the rows' region lies inside it, each used plane's rectangle of
// the assembled plane, its pitch and its offset in the gathered block, and the block's bytes.
struct Stage {
    avifgpu_read_desc sd; avifgpu_rect tin; int n;        // the staged image, the rows' region inside it, the rows
    avifgpu_rect pr[4]; int64_t pitch[4], at[4]; bool used[4];
    int64_t bytes;
};
void stage_of(const avifgpu_read_desc* d, const Call& c, int code, int o0, int n, Stage& s)
{
    s.n = n;
    s.tin = crop_tile_rect(c.rect, code, o0, n);
    const avifgpu_rect sr = crop_stage_rect(s.tin, d->width, d->height, c.xs, c.ys, c.interp);
    s.sd = *d; s.sd.width = sr.width; s.sd.height = sr.height;
    s.bytes = 0;
    for (int pl = 0; pl < 4; ++pl) {
        s.used[pl] = read_plane_used(d, c.g, pl);
        s.pitch[pl] = 0; s.at[pl] = 0;
        if (!s.used[pl]) continue;
        s.pr[pl] = crop_plane_rect(sr, plane_is_chroma(d, pl), c.xs, c.ys);
        s.pitch[pl] = align256((int64_t)s.pr[pl].width * c.ssz);
        s.at[pl] = s.bytes;
        s.bytes += s.pitch[pl] * s.pr[pl].height;
    }
    s.tin.x0 -= sr.x0; s.tin.y0 -= sr.y0;
}

// the cropped open of the staged image whose planes sit at base + s.at[]: all of the view of s.tin
int open_staged(const Stage& s, int upsampling, int code, uint8_t* base, uint8_t* dst, int64_t dst_row_bytes,
                uint8_t* scratch, int64_t scratch_bytes, hipStream_t st)
{
    const void* planes[4]; int64_t strides[4];
    for (int pl = 0; pl < 4; ++pl) { planes[pl] = s.used[pl] ? base + s.at[pl] : nullptr; strides[pl] = s.pitch[pl]; }
    return avifgpu_read_rows_cropped(&s.sd, &s.tin, upsampling, code, 0, s.n, planes, strides, dst, dst_row_bytes, scratch, scratch_bytes, AVIFGPU_MEM_DEVICE, st);
}

uint8_t* up256(void* p) { return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }

int read_rows_grid_device(const avifgpu_read_desc* d, const avifgpu_grid& grid, const Call& c, const avifgpu_grid_tile* tiles, int upsampling, int code,
                          int orow0, int onrows, uint8_t* dst, int64_t dst_row_bytes, void* scratch, int64_t scratch_bytes, hipStream_t st)
{
    Stage s;
    stage_of(d, c, code, orow0, onrows, s);
    uint8_t* const base = up256(scratch);
    const int64_t rest = scratch_bytes - (base - static_cast<uint8_t*>(scratch)) - s.bytes;
    if (rest < 0) return fail(AVIFGPU_readErr, "avifgpu_read_rows_grid: the staged planes exceed the scratch bound");      // the helper's bound holds them: not reached
    GridParams p;
    memset(&p, 0, sizeof(p));
    p.tiles = tiles; p.columns = grid.columns;
    int np = 0;
    for (int pl = 0; pl < 4; ++pl) {
        if (!s.used[pl]) continue;
        const bool chroma = plane_is_chroma(d, pl);
        p.pl[np++] = { base + s.at[pl], s.pitch[pl], pl, grid_tile_w(grid, chroma, c.xs), grid_tile_h(grid, chroma, c.ys), s.pr[pl].x0, s.pr[pl].y0, s.pr[pl].width, s.pr[pl].height };
    }
    const hipError_t e = launch_gather(p, np, c.ssz, st);
    if (e != hipSuccess) return hip_fail(e, "grid_gather launch", AVIFGPU_readErr);
    return open_staged(s, upsampling, code, base, dst, dst_row_bytes, base + s.bytes, rest, st);
}

constexpr size_t kHostTileBytes = (size_t)16 << 20;             // output bytes of one staged tile, as for the cropped open

int read_rows_grid_host(const avifgpu_read_desc* d, const avifgpu_grid& grid, const Call& c, const avifgpu_grid_tile* tiles, int upsampling, int code,
                        int orow0, int onrows, uint8_t* dst, int64_t dst_row_bytes)
{
    const bool matters = !c.interp && (crop_turn(code).t ? c.xs : c.ys) != 0;
    const int64_t out_pitch = align256((int64_t)c.out_w * c.bpp);
    Stage s;
    int64_t crop_need = 0;
    const StagedPlan plan = [&](int o0, int left, int max_rows, StagedTile& t) {
        t.n = std::min(crop_next_tile(c.rect, code, matters, o0, max_rows), left);
        stage_of(d, c, code, o0, t.n, s);
        crop_need = crop_scratch_bytes(s.tin, c.xs, c.ys, c.interp, code, c.ssz, c.bpp, true, true);
        t.out_pitch = out_pitch;
        t.scratch_bytes = s.bytes + crop_need;                  // nothing goes up through the driver: the planes are assembled in the slot's scratch
        return 0;
    };
    const StagedEnqueue enqueue = [&](const StagedBuffers& b) {
        uint8_t* const base = static_cast<uint8_t*>(b.scratch);
        for (int pl = 0; pl < 4; ++pl) {
            if (!s.used[pl]) continue;
            const bool chroma = plane_is_chroma(d, pl);
            hipError_t e = hipSuccess;
            grid_pieces(grid.columns, grid_tile_w(grid, chroma, c.xs), grid_tile_h(grid, chroma, c.ys), c.ssz, s.pr[pl].x0, s.pr[pl].y0, s.pr[pl].width, s.pr[pl].height,
                        [&](const GridPiece& k) {
                            if (e != hipSuccess) return;
                            const avifgpu_grid_tile& t = tiles[k.tile];
                            e = hipMemcpy2DAsync(base + s.at[pl] + (int64_t)k.dst_y * s.pitch[pl] + k.dst_x, (size_t)s.pitch[pl],
                                                 static_cast<const uint8_t*>(t.plane[pl]) + (int64_t)k.src_y * t.stride[pl] + k.src_x, (size_t)t.stride[pl],
                                                 (size_t)k.bytes, (size_t)k.rows, hipMemcpyHostToDevice, b.stream);
                        });
            if (e != hipSuccess) return hip_fail(e, "hipMemcpy2DAsync (tile pieces)", AVIFGPU_readErr);
        }
        return open_staged(s, upsampling, code, base, static_cast<uint8_t*>(b.out), out_pitch, base + s.bytes, crop_need, b.stream);
    };
    return staged_open("grid open", kHostTileBytes, (int64_t)c.out_w * c.bpp, orow0, onrows, dst, dst_row_bytes, plan, enqueue);
}

} // namespace

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_grid_parse(const uint8_t* payload, int64_t size, int32_t* rows, int32_t* columns, int32_t* out_w, int32_t* out_h)
{
    set_error("");
    if (!payload || !rows || !columns || !out_w || !out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_parse: null argument");
    int32_t r, c, w, h;
    if (!grid_parse(payload, size, r, c, w, h))
        return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_parse: %lld bytes are no ImageGrid payload (version 0, 8 or 12 bytes, a size of 1..INT32_MAX)", (long long)size);
    *rows = r; *columns = c; *out_w = w; *out_h = h;
    return 0;
}

int32_t avifgpu_grid_check(const avifgpu_read_desc* desc, const avifgpu_grid* grid)
{
    set_error("");
    Call c;
    return check_grid(desc, grid, nullptr, AVIFGPU_UPSAMPLE_NEAREST, 1, c, "avifgpu_grid_check");
}

int64_t avifgpu_read_grid_scratch_bytes(const avifgpu_read_desc* desc, const avifgpu_grid* grid, const avifgpu_rect* rect, int32_t upsampling,
                                        int32_t orientation, int32_t onrows)
{
    set_error("");
    Call c;
    const int err = check_grid(desc, grid, rect, upsampling, orientation, c, "avifgpu_read_grid_scratch_bytes");
    if (err) return err;
    if (onrows < 0 || onrows > c.out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_grid_scratch_bytes: %d rows of an image of %d", onrows, c.out_h);
    return grid_scratch_bytes(desc, c, orientation, onrows);
}

int32_t avifgpu_read_rows_grid(const avifgpu_read_desc* desc, const avifgpu_grid* grid, const avifgpu_grid_tile* tiles,
                               const avifgpu_rect* rect, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t onrows,
                               void* dst, int64_t dst_row_bytes, void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream)
{
    set_error("");
    Call c;
    const int err = check_grid(desc, grid, rect, upsampling, orientation, c, "avifgpu_read_rows_grid");
    if (err) return err;
    if (orow0 < 0 || onrows < 0 || (int64_t)orow0 + onrows > c.out_h)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_grid: rows [%d, %d + %d) outside the %d rows of the image", orow0, orow0, onrows, c.out_h);
    if (mem_kind != AVIFGPU_MEM_HOST && mem_kind != AVIFGPU_MEM_DEVICE) return fail(AVIFGPU_formatBadParameters, "bad mem_kind %d", mem_kind);
    if (!tiles || !dst) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_grid: null buffer");
    const int64_t row_bytes = (int64_t)c.out_w * c.bpp;
    if (row_bytes > 0x7fffffffLL) return fail(AVIFGPU_memFullErr, "rowBytes exceeds int32");
    if (dst_row_bytes < row_bytes) return fail(AVIFGPU_formatBadParameters, "dst_row_bytes %lld < %lld", (long long)dst_row_bytes, (long long)row_bytes);
    if (mem_kind == AVIFGPU_MEM_HOST) {
        for (int k = 0; k < grid->columns * grid->rows; ++k) {
            if (!grid_tile_visible(*grid, desc->width, desc->height, k)) continue;
            for (int pl = 0; pl < 4; ++pl) {
                if (!read_plane_used(desc, c.g, pl)) continue;
                if (!tiles[k].plane[pl]) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_grid: plane %d of tile %d is null", pl, k);
                const int64_t rb = (int64_t)grid_tile_w(*grid, plane_is_chroma(desc, pl), c.xs) * c.ssz;
                if (tiles[k].stride[pl] < rb) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_grid: stride %lld of plane %d of tile %d < %lld", (long long)tiles[k].stride[pl], pl, k, (long long)rb);
            }
        }
    } else {
        const int64_t need = grid_scratch_bytes(desc, c, orientation, onrows);
        if (need > 0 && (!scratch || scratch_bytes < need))
            return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_grid: %lld bytes of scratch, %lld needed (avifgpu_read_grid_scratch_bytes)", (long long)(scratch ? scratch_bytes : 0), (long long)need);
    }
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    if (onrows == 0) return 0;
    if (mem_kind == AVIFGPU_MEM_DEVICE)
        return read_rows_grid_device(desc, *grid, c, tiles, upsampling, orientation, orow0, onrows, static_cast<uint8_t*>(dst), dst_row_bytes, scratch, scratch_bytes, (hipStream_t)stream);
    if (grid->columns == 1 && grid->rows == 1)                 // no seam: the cropped open on tile 0, byte for byte
        return avifgpu_read_rows_cropped(desc, &c.rect, upsampling, orientation, orow0, onrows, tiles[0].plane, tiles[0].stride, dst, dst_row_bytes, nullptr, 0, AVIFGPU_MEM_HOST, nullptr);
    return read_rows_grid_host(desc, *grid, c, tiles, upsampling, orientation, orow0, onrows, static_cast<uint8_t*>(dst), dst_row_bytes);
}

int32_t avifgpu_probe_grid_gather(const avifgpu_grid_tile* tiles_dev, int32_t columns, int32_t plane, int32_t tile_w_samples,
                                  int32_t tile_h_samples, int32_t bytes_per_sample, int32_t x0, int32_t y0, int32_t w, int32_t h,
                                  void* dst, int64_t dst_row_bytes, void* stream)
{
    set_error("");
    if (!tiles_dev || !dst || columns < 1 || columns > kGridMaxSide || plane < 0 || plane > 3 || tile_w_samples < 1 || tile_h_samples < 1)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_gather: bad table, plane or tile size");
    if (bytes_per_sample != 1 && bytes_per_sample != 2) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_gather: %d bytes per sample", bytes_per_sample);
    if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || (int64_t)x0 + w > (int64_t)columns * tile_w_samples || (int64_t)y0 + h > (int64_t)kGridMaxSide * tile_h_samples)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_gather: the rectangle is not inside the tiles");
    if ((reinterpret_cast<uintptr_t>(dst) & 15) || (dst_row_bytes & 15) || dst_row_bytes < (int64_t)w * bytes_per_sample)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_gather: dst and dst_row_bytes must be multiples of 16, and a row must hold the payload");
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    GridParams p;
    memset(&p, 0, sizeof(p));
    p.tiles = tiles_dev; p.columns = columns;
    p.pl[0] = { static_cast<uint8_t*>(dst), dst_row_bytes, plane, tile_w_samples, tile_h_samples, x0, y0, w, h };
    const hipError_t e = launch_gather(p, 1, bytes_per_sample, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_grid_gather", AVIFGPU_readErr);
}

} // extern "C"
