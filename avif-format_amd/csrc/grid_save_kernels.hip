// grid_save_kernels.hip -- the grid save: a save written straight into the padded tiles a grid encoder takes (include/avifgpu.h "grid
// save").  The mirror of grid_kernels.hip.
//
// The conversion arithmetic is not copied and no existing kernel is touched.  On device pointers the unchanged save (and any armed
// statistics behind it) writes canvas-sized planes into the head of the caller's scratch; then grid_scatter (one launch, two where chroma
// is subsampled) puts the band of every used plane into the tiles, padding included.  On host pointers the row-tile scheduler of
// pipeline.hip converts into slot planes of the padded pitch, grid_pad fills the pad cells in place and the band travels down as one
// strided copy per tile piece.
//
// grid_scatter<B>.  A byte mover that knows nothing of colour, destination-driven: the padded row of a plane is columns * tw_p * B bytes;
// a lane owns 16 of them, a wave 1 KiB, a workgroup 4 KiB; grid.y rows with grid_gather's row loop, grid.z planes.  The tile row is uniform
// for a workgroup row; the tile column costs a lane one unsigned division.  Where a lane's 16 bytes lie inside one tile and inside the
// canvas it loads them as one word and stores them -- non-temporally where the tile address is a multiple of 16, as one unaligned word
// otherwise; at a seam (several, for tiles narrower than 16 bytes), at the row's tail and in the padding it places units of 1 or 2 bytes,
// each from the CLAMPED source pixel: that clamp is what writes the padding.  Bytes of a tile row beyond tw_p * B are not touched.  No LDS,
// no atomics.
//
// grid_pad<B>.  The host path's in-place padding: pad columns of every band row, pad rows below the last band.  It reads valid cells only
// (the row's last pixel, the last row) and writes pad cells only: no hazard.
//
// A translation unit -- and so a code object -- of its own: a process that never saves a grid never loads it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "grid_save_geometry.h"
#include "grid_save.h"

namespace avifgpu {

namespace {

typedef uint32_t gs_u4 __attribute__((ext_vector_type(4)));
typedef gs_u4 gs_u4_any __attribute__((aligned(1)));            // 16 bytes at any address
// A tile's plane pointer comes out of the table, so the compiler cannot know its address space and would emit flat stores; the table holds
// device (global) pointers and nothing else.
#define AG_GRID_GLOBAL __attribute__((address_space(1)))

struct ScatterPlane {
    const uint8_t* src; int64_t pitch;           // the band buffer: src_rows rows of pw pixels
    int32_t plane;                               // which pointer of a tile record
    int32_t tw, th;                              // a tile's extent in this plane, pixels
    int32_t pw;                                  // valid pixels of a source row
    int32_t y0, h, src_rows;                     // rows [y0, y0 + h) of the padded plane; row r comes from buffer row min(r, src_rows - 1); h == 0: nothing
};
struct ScatterParams {
    const avifgpu_grid_tile* tiles; int32_t columns;
    ScatterPlane pl[4];
};

constexpr int kScatterThreads = 256;             // four waves, four neighbouring spans of a row

template <int U> struct ScatterUnit;
template <> struct ScatterUnit<1> { typedef uint8_t type; };
template <> struct ScatterUnit<2> { typedef uint16_t type; };

template <int B>
__global__ __launch_bounds__(kScatterThreads) void grid_scatter(const ScatterParams p)
{
    constexpr int U = (B == 2 || B == 6 || B == 8) ? 2 : 1;                    // grid_scatter_unit(B)
    typedef typename ScatterUnit<U>::type unit_t;
    const ScatterPlane& q = p.pl[blockIdx.z];
    const uint64_t twb = (uint64_t)q.tw * B;                                   // bytes of a tile row
    const uint64_t total = twb * (uint64_t)p.columns;                          // ... of a padded row
    const uint64_t off = ((uint64_t)blockIdx.x * kScatterThreads + threadIdx.x) * 16;   // the lane's 16 bytes of every padded row
    if (off >= total) return;
    const int n = (int)min((uint64_t)16, total - off);
    const uint64_t tc = off / twb, tx = off - tc * twb;
    const uint64_t valid = (uint64_t)q.pw * B;                                 // bytes a source row holds
    const bool whole = n == 16 && tx + 16 <= twb && off + 16 <= valid;         // 16 bytes inside one tile and inside the canvas
    for (int row = (int)blockIdx.y; row < q.h; row += (int)gridDim.y) {
        const uint32_t y = (uint32_t)q.y0 + (uint32_t)row;
        const uint32_t tr = y / (uint32_t)q.th, ty = y - tr * (uint32_t)q.th;
        const avifgpu_grid_tile* const trow = p.tiles + (int64_t)tr * p.columns;
        const uint8_t* const sp = q.src + (int64_t)min(row, q.src_rows - 1) * q.pitch;
        if (whole) {
            const avifgpu_grid_tile* const t = trow + tc;
            uint8_t* const dp = static_cast<uint8_t*>(const_cast<void*>(t->plane[q.plane])) + (int64_t)ty * t->stride[q.plane] + (int64_t)tx;
            const gs_u4 v = __builtin_nontemporal_load((const AG_GRID_GLOBAL gs_u4_any*)(sp + off));
            if ((reinterpret_cast<uintptr_t>(dp) & 15) == 0) __builtin_nontemporal_store(v, (AG_GRID_GLOBAL gs_u4*)dp);
            else *(AG_GRID_GLOBAL gs_u4_any*)dp = v;
        } else {
            uint64_t c = tc, cx = tx;
            const avifgpu_grid_tile* t = trow + c;
            uint8_t* dp = static_cast<uint8_t*>(const_cast<void*>(t->plane[q.plane])) + (int64_t)ty * t->stride[q.plane];
            for (int i = 0; i < n; i += U) {
                const uint32_t v = (uint32_t)(off + i);
                const uint32_t pix = v / B, w = v - pix * B;
                const uint32_t spix = min(pix, (uint32_t)q.pw - 1);            // the clamp that writes the pad columns
                *(AG_GRID_GLOBAL unit_t*)(dp + cx) = *(const AG_GRID_GLOBAL unit_t*)(sp + (uint64_t)spix * B + w);
                cx += U;
                if (cx == twb && i + U < n) {
                    cx = 0; ++c;
                    t = trow + c;
                    dp = static_cast<uint8_t*>(const_cast<void*>(t->plane[q.plane])) + (int64_t)ty * t->stride[q.plane];
                }
            }
        }
    }
}

// one launch for the planes of p in slots [0, nplanes) whose padded rows are rb bytes: pixels of b bytes
hipError_t launch_scatter_group(const ScatterParams& p, int nplanes, int64_t rb, int b, hipStream_t st)
{
    int rows = 0;
    for (int i = 0; i < nplanes; ++i) rows = std::max(rows, (int)p.pl[i].h);
    if (rb <= 0 || rows <= 0) return hipSuccess;
    if (rb > 0xffffffffLL) return hipErrorInvalidValue;           // the seam path indexes a padded row in 32 bits
    const dim3 grid((unsigned)((rb + kScatterThreads * 16 - 1) / (kScatterThreads * 16)), (unsigned)std::min(rows, 65535), (unsigned)nplanes), block(kScatterThreads);
    switch (b) {
    case 1: hipLaunchKernelGGL(grid_scatter<1>, grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL(grid_scatter<2>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(grid_scatter<3>, grid, block, 0, st, p); break;
    case 4: hipLaunchKernelGGL(grid_scatter<4>, grid, block, 0, st, p); break;
    case 6: hipLaunchKernelGGL(grid_scatter<6>, grid, block, 0, st, p); break;
    case 8: hipLaunchKernelGGL(grid_scatter<8>, grid, block, 0, st, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// All planes of p with h > 0 in slots [0, nplanes).  Planes whose padded rows have one length share a launch (grid.z); the subsampled chroma
// planes get a launch of their own: in the luma planes' grid half their workgroups would own no byte, and with one 4-KiB span per
// workgroup the kernel runs at the rate workgroups are dispatched -- measured on the 12-bit 4:2:2 save of an 8192^2 document, one launch
// for all three planes took 24 us longer than the three planes launched one by one.
hipError_t launch_scatter(const ScatterParams& p, int nplanes, int b, hipStream_t st)
{
    bool done[4] = {};
    for (int i = 0; i < nplanes; ++i) {
        if (done[i]) continue;
        const int64_t rb = (int64_t)p.pl[i].tw * b * p.columns;
        ScatterParams g = p;
        int n = 0;
        for (int j = i; j < nplanes; ++j) {
            if (done[j] || (int64_t)p.pl[j].tw * b * p.columns != rb) continue;
            g.pl[n++] = p.pl[j];
            done[j] = true;
        }
        const hipError_t e = launch_scatter_group(g, n, rb, b, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- grid_pad: pixel (row, x) of a plane of `full` pixels a row <- pixel (min(row, rows - 1), min(x, pw - 1)), pad cells only --------------
struct PadPlane { uint8_t* base; int64_t pitch; int32_t pw, full, rows, pad_rows; };      // rows == 0: nothing
struct PadParams { PadPlane pl[4]; };

template <int B>
__global__ __launch_bounds__(kScatterThreads) void grid_pad(const PadParams p)
{
    constexpr int U = (B == 2 || B == 6 || B == 8) ? 2 : 1;
    typedef typename ScatterUnit<U>::type unit_t;
    const PadPlane& q = p.pl[blockIdx.z];
    const int64_t i = (int64_t)blockIdx.x * kScatterThreads + threadIdx.x;
    for (int row = (int)blockIdx.y; row < q.rows + q.pad_rows; row += (int)gridDim.y) {
        const int64_t x = row < q.rows ? (int64_t)q.pw + i : i;                // a band row: its pad columns; a pad row: all of it
        if (x >= q.full) continue;
        const unit_t* const s = reinterpret_cast<const unit_t*>(q.base + (int64_t)min(row, q.rows - 1) * q.pitch + min(x, (int64_t)q.pw - 1) * B);
        unit_t* const d = reinterpret_cast<unit_t*>(q.base + (int64_t)row * q.pitch + x * B);
        for (int k = 0; k < B / U; ++k) d[k] = s[k];
    }
}

uint8_t* up256(void* p) { return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(p) + 255) & ~(uintptr_t)255); }
int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

} // namespace

// ---- what pipeline.hip's start_write needs (grid_save.h) -------------------------------------------------------------------------------------
void grid_save_plane(const avifgpu_write_desc* d, const WriteGeom& g, const avifgpu_grid& grid, int pl, int row0, int nrows, GridSavePlane& out)
{
    const bool chroma = d->output == AVIFGPU_OUT_YCBCR && (pl == 1 || pl == 2);
    const int xs = chroma ? g.xs : 0, ys = chroma ? g.ys : 0;
    int rows; int64_t rb;
    write_plane_extent(d, g, pl, nrows, rows, rb);
    out.pw = (d->width + xs) >> xs;
    out.b = (int)(rb / out.pw);
    out.tw = grid_tile_w(grid, chroma, g.xs);
    out.th = grid_tile_h(grid, chroma, g.ys);
    out.band = grid_save_band(grid, d->height, row0, nrows, ys, out.pw, out.tw, out.th);
    out.full_bytes = (int64_t)grid.columns * out.tw * out.b;
}

int check_grid_tiles(const avifgpu_write_desc* d, const WriteGeom& g, const avifgpu_grid& grid, const avifgpu_grid_tile* tiles, const char* who)
{
    if (!tiles) return fail(AVIFGPU_formatBadParameters, "%s: null buffer", who);
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        GridSavePlane s;
        grid_save_plane(d, g, grid, pl, 0, 0, s);
        const int64_t rb = (int64_t)s.tw * s.b;
        const bool wide = grid_scatter_unit(s.b) == 2;                 // 16-bit samples: naturally aligned
        for (int k = 0; k < grid.columns * grid.rows; ++k) {
            if (!tiles[k].plane[pl]) return fail(AVIFGPU_formatBadParameters, "%s: plane %d of tile %d is null", who, pl, k);
            if (tiles[k].stride[pl] < rb) return fail(AVIFGPU_formatBadParameters, "%s: stride %lld of plane %d of tile %d < %lld", who, (long long)tiles[k].stride[pl], pl, k, (long long)rb);
            if (wide && ((reinterpret_cast<uintptr_t>(tiles[k].plane[pl]) | (uintptr_t)tiles[k].stride[pl]) & 1))
                return fail(AVIFGPU_formatBadParameters, "%s: plane %d of tile %d holds 16-bit samples at an odd address or stride", who, pl, k);
        }
    }
    return 0;
}

hipError_t launch_grid_pad(const GridSavePlane gp[4], uint8_t* const base[4], const int64_t pitch[4], hipStream_t st)
{
    PadParams p;
    memset(&p, 0, sizeof(p));
    int np = 0, b = 0, rows = 0; int64_t cells = 0;
    for (int pl = 0; pl < 4; ++pl) {
        if (!base[pl] || gp[pl].band.rows < 1) continue;
        const GridSavePlane& s = gp[pl];
        if (s.band.pad_cols == 0 && s.band.pad_rows == 0) continue;
        p.pl[np++] = { base[pl], pitch[pl], s.pw, s.pw + s.band.pad_cols, s.band.rows, s.band.pad_rows };
        b = s.b;
        rows = std::max(rows, s.band.rows + s.band.pad_rows);
        cells = std::max<int64_t>(cells, s.band.pad_rows ? s.pw + s.band.pad_cols : s.band.pad_cols);
    }
    if (np == 0 || cells <= 0) return hipSuccess;
    const dim3 grid((unsigned)((cells + kScatterThreads - 1) / kScatterThreads), (unsigned)std::min(rows, 65535), (unsigned)np), block(kScatterThreads);
    switch (b) {
    case 1: hipLaunchKernelGGL(grid_pad<1>, grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL(grid_pad<2>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(grid_pad<3>, grid, block, 0, st, p); break;
    case 4: hipLaunchKernelGGL(grid_pad<4>, grid, block, 0, st, p); break;
    case 6: hipLaunchKernelGGL(grid_pad<6>, grid, block, 0, st, p); break;
    case 8: hipLaunchKernelGGL(grid_pad<8>, grid, block, 0, st, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

namespace {

// ---- the entry -------------------------------------------------------------------------------------------------------------------------------
int check_save_grid(const avifgpu_write_desc* d, const avifgpu_grid* grid, int row0, int nrows, WriteGeom& g, const char* who)
{
    const int err = check_write(d, row0, nrows, g);
    if (err) return err;
    if (!grid) return fail(AVIFGPU_formatBadParameters, "%s: null grid", who);
    const char* const why = grid_save_illegal(d->width, d->height, g.xs, g.ys, *grid);
    if (why) return fail(AVIFGPU_formatBadParameters, "%s: %d x %d tiles of %d x %d for a %d x %d canvas: %s", who, grid->columns, grid->rows, grid->tile_width, grid->tile_height, d->width, d->height, why);
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        GridSavePlane s;
        grid_save_plane(d, g, *grid, pl, 0, 0, s);
        if (s.full_bytes > 0x7fffffffLL) return fail(AVIFGPU_memFullErr, "%s: a padded row of plane %d exceeds int32", who, pl);
    }
    return 0;
}

int64_t save_scratch_bytes(const avifgpu_write_desc* d, const WriteGeom& g, int nrows)
{
    if (nrows < 1) return 0;
    int64_t total = 256;
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        int rows; int64_t rb;
        write_plane_extent(d, g, pl, nrows, rows, rb);
        total += align256(rb) * rows;
    }
    return total;
}

int icc_args_of(int kind, const void* icc, IccArgs& a, const char* who)
{
    if (kind == AVIFGPU_ICC_KIND_NONE) {
        if (icc) return fail(AVIFGPU_formatBadParameters, "%s: AVIFGPU_ICC_KIND_NONE takes a NULL icc", who);
        return 0;
    }
    if (kind < AVIFGPU_ICC_KIND_NONE || kind > AVIFGPU_ICC_KIND_PIPELINE32) return fail(AVIFGPU_formatBadParameters, "%s: icc_kind %d is not an AVIFGPU_ICC_KIND_* value", who, kind);
    if (!icc) return fail(AVIFGPU_formatBadParameters, "%s: icc_kind %d with a NULL icc", who, kind);
    switch (kind) {
    case AVIFGPU_ICC_KIND_TRANSFORM:   a.f32 = static_cast<const avifgpu_icc_transform*>(icc); break;
    case AVIFGPU_ICC_KIND_SAMPLED:     a.s32 = static_cast<const avifgpu_icc_sampled32*>(icc); break;
    case AVIFGPU_ICC_KIND_SHAPER8:     a.s8 = static_cast<const avifgpu_icc_shaper8*>(icc); break;
    case AVIFGPU_ICC_KIND_CLUT16:      a.c16 = static_cast<const avifgpu_icc_clut16*>(icc); break;
    case AVIFGPU_ICC_KIND_CLUT8_TABLE: a.c8t = static_cast<const avifgpu_icc_clut16*>(icc); break;
    default:
        a.p32 = static_cast<const avifgpu_icc_pipeline32*>(icc);
        if (!icc_pipeline32_stamped(a.p32))
            return fail(AVIFGPU_formatBadParameters, "the ICC stage program is not proven: unstamped, or altered since avifgpu_icc_pipeline32_prove");
    }
    return 0;
}

int write_rows_grid_device(const avifgpu_write_desc* d, const WriteGeom& g, const IccArgs& icc, const avifgpu_grid& grid, const avifgpu_grid_tile* tiles,
                           int row0, int nrows, const void* src, int64_t src_row_bytes, void* scratch, hipStream_t st)
{
    uint8_t* at = up256(scratch);
    void* planes[4] = {}; int64_t strides[4] = {};
    ScatterParams p;
    memset(&p, 0, sizeof(p));
    p.tiles = tiles; p.columns = grid.columns;
    int np = 0, b = 1;
    for (int pl = 0; pl < 4; ++pl) {
        if (!write_plane_used(d, g, pl)) continue;
        int rows; int64_t rb;
        write_plane_extent(d, g, pl, nrows, rows, rb);
        planes[pl] = at; strides[pl] = align256(rb);
        at += strides[pl] * rows;
        GridSavePlane s;
        grid_save_plane(d, g, grid, pl, row0, nrows, s);
        if (s.band.rows < 1) continue;
        p.pl[np++] = { static_cast<const uint8_t*>(planes[pl]), strides[pl], pl, s.tw, s.th, s.pw, s.band.y0, s.band.rows + s.band.pad_rows, s.band.rows };
        b = s.b;
    }
    const int err = write_rows_with_icc(d, icc, row0, nrows, src, src_row_bytes, planes, strides, AVIFGPU_MEM_DEVICE, st);   // the unchanged save, statistics behind it
    if (err) return err;
    const hipError_t e = launch_scatter(p, np, b, st);
    return e == hipSuccess ? 0 : hip_fail(e, "grid_scatter launch", AVIFGPU_writErr);
}

} // namespace

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_write_grid_check(const avifgpu_write_desc* desc, const avifgpu_grid* grid)
{
    set_error("");
    WriteGeom g;
    return check_save_grid(desc, grid, 0, 0, g, "avifgpu_write_grid_check");
}

int64_t avifgpu_write_grid_scratch_bytes(const avifgpu_write_desc* desc, int32_t nrows)
{
    set_error("");
    WriteGeom g;
    const int err = check_write(desc, 0, 0, g);
    if (err) return err;
    if (nrows < 0 || nrows > desc->height) return fail(AVIFGPU_formatBadParameters, "avifgpu_write_grid_scratch_bytes: %d rows of an image of %d", nrows, desc->height);
    return save_scratch_bytes(desc, g, nrows);
}

int32_t avifgpu_grid_fit(const avifgpu_write_desc* desc, int32_t max_tile_width, int32_t max_tile_height, int32_t align, avifgpu_grid* grid)
{
    set_error("");
    WriteGeom g;
    const int err = check_write(desc, 0, 0, g);
    if (err) return err;
    if (!grid) return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_fit: null grid");
    if (max_tile_width < 1 || max_tile_height < 1 || align < 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_fit: caps and align must be at least 1");
    avifgpu_grid r;
    if (!grid_fit_side(desc->width, max_tile_width, align, g.xs != 0, r.columns, r.tile_width) ||
        !grid_fit_side(desc->height, max_tile_height, align, g.ys != 0, r.rows, r.tile_height))
        return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_fit: no grid of at most 256 x 256 tiles of at most %d x %d, multiples of %d, covers %d x %d", max_tile_width, max_tile_height, align, desc->width, desc->height);
    *grid = r;
    return 0;
}

int32_t avifgpu_grid_payload(const avifgpu_grid* grid, int32_t width, int32_t height, uint8_t* out, int64_t capacity)
{
    set_error("");
    if (!grid || !out) return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_payload: null argument");
    const int n = grid_payload(*grid, width, height, out, capacity);
    if (n == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_grid_payload: %d x %d tiles, a %d x %d canvas, %lld bytes of room: no ImageGrid payload (1..256 tiles a side, a size of at least 1, 8 or 12 bytes)",
                            grid->columns, grid->rows, width, height, (long long)capacity);
    return n;
}

int32_t avifgpu_write_rows_grid(const avifgpu_write_desc* desc, int32_t icc_kind, const void* icc, const avifgpu_grid* grid, const avifgpu_grid_tile* tiles,
                                int32_t row0, int32_t nrows, const void* src, int64_t src_row_bytes, void* scratch, int64_t scratch_bytes,
                                int32_t mem_kind, void* stream)
{
    static const char* const who = "avifgpu_write_rows_grid";
    set_error("");
    WriteGeom g;
    int err = check_save_grid(desc, grid, row0, nrows, g, who);
    if (err) return err;
    IccArgs a;
    if ((err = icc_args_of(icc_kind, icc, a, who))) return err;
    if (mem_kind != AVIFGPU_MEM_HOST && mem_kind != AVIFGPU_MEM_DEVICE) return fail(AVIFGPU_formatBadParameters, "bad mem_kind %d", mem_kind);
    if (!tiles || !src) return fail(AVIFGPU_formatBadParameters, "%s: null buffer", who);
    const int64_t min_src_row = (int64_t)desc->width * desc->planes * (desc->depth / 8);
    if (src_row_bytes < min_src_row) return fail(AVIFGPU_formatBadParameters, "src_row_bytes %lld < %lld", (long long)src_row_bytes, (long long)min_src_row);
    if (mem_kind == AVIFGPU_MEM_HOST) {
        if ((err = check_grid_tiles(desc, g, *grid, tiles, who))) return err;
    } else {
        const int64_t need = save_scratch_bytes(desc, g, nrows);
        if (need > 0 && (!scratch || scratch_bytes < need))
            return fail(AVIFGPU_formatBadParameters, "%s: %lld bytes of scratch, %lld needed (avifgpu_write_grid_scratch_bytes)", who, (long long)(scratch ? scratch_bytes : 0), (long long)need);
    }
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    if (nrows == 0) return 0;
    if (mem_kind == AVIFGPU_MEM_DEVICE)
        return write_rows_grid_device(desc, g, a, *grid, tiles, row0, nrows, src, src_row_bytes, scratch, (hipStream_t)stream);
    const GridDest gd = { *grid, tiles };
    void* const none[4] = {}; const int64_t zero[4] = {};
    if (a.c16 || a.s32 || a.c8t) icc_epoch_for_call(row0, nrows);      // as write_rows_any does for its host path
    return write_rows_host(desc, row0, nrows, src, src_row_bytes, none, zero, a, &gd);
}

int32_t avifgpu_probe_grid_scatter(const avifgpu_grid_tile* tiles_dev, int32_t columns, int32_t plane, int32_t tile_w_pixels, int32_t tile_h_pixels,
                                   int32_t bytes_per_pixel, int32_t plane_w, int32_t plane_h, int32_t y0, int32_t h,
                                   const void* src, int64_t src_row_bytes, void* stream)
{
    set_error("");
    if (!tiles_dev || !src || columns < 1 || columns > kGridMaxSide || plane < 0 || plane > 3 || tile_w_pixels < 1 || tile_h_pixels < 1)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: bad table, plane or tile size");
    const int b = bytes_per_pixel;
    if (b != 1 && b != 2 && b != 3 && b != 4 && b != 6 && b != 8) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: %d bytes per pixel", b);
    if (plane_w < 1 || plane_h < 1 || (int64_t)columns * tile_w_pixels < plane_w || (int64_t)kGridMaxSide * tile_h_pixels < plane_h)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: the tiles do not cover the plane");
    if (y0 < 0 || h < 1 || (int64_t)y0 + h > (int64_t)kGridMaxSide * tile_h_pixels || y0 >= plane_h)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: rows [%d, %d + %d) are not rows of the padded plane that begin inside the plane", y0, y0, h);
    if ((int64_t)columns * tile_w_pixels * b > 0x7fffffffLL || src_row_bytes < (int64_t)plane_w * b)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: a source row must hold plane_w pixels, a padded row must fit int32");
    if (grid_scatter_unit(b) == 2 && ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)src_row_bytes) & 1))
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_grid_scatter: pixels of %d bytes are 16-bit samples: src and src_row_bytes must be even", b);
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    ScatterParams p;
    memset(&p, 0, sizeof(p));
    p.tiles = tiles_dev; p.columns = columns;
    p.pl[0] = { static_cast<const uint8_t*>(src), src_row_bytes, plane, tile_w_pixels, tile_h_pixels, plane_w, y0, h, std::min(h, plane_h - y0) };
    const hipError_t e = launch_scatter(p, 1, b, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_grid_scatter", AVIFGPU_writErr);
}

} // extern "C"
