// staging.h -- internal C++ interface between the host-side translation units of libavifgpu.so:
//   avifgpu_api.hip  validation, descriptor -> kernel parameters, the extern "C" entry points
//   icc_tables.cpp   the ICC stage of a save: its kernel parameters, the per-device cache of its tables
//   pipeline.hip     the bound device contexts: one worker thread + N staging slots per context; row-tile scheduler
//   host_shim.cpp    the FormatRecord tile protocol above them
//   staged_open.cpp  the entry checks and the staged host path of the oriented, upsampled and cropped opens
//   save_stats.cpp   the arming, the per-call check and the launch sequence of a save's three statistics
// Nothing here crosses the C-ABI (include/avifgpu.h is the public surface).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <functional>

#include "../../include/avifgpu.h"
#include "kernel_params.h"
#include "open_geometry.h"

namespace avifgpu {

// The ICC stage of a write call (at most one member set); the pointed-to tables outlive the call.
struct IccArgs {
    const avifgpu_icc_transform* f32 = nullptr;     // 32-bit documents (avifgpu_write_rows_icc)
    const avifgpu_icc_shaper8*   s8 = nullptr;      // 8-bit documents  (avifgpu_write_rows_icc8)
    const avifgpu_icc_clut16*    c16 = nullptr;     // 16-bit documents (avifgpu_write_rows_icc16)
    const avifgpu_icc_sampled32* s32 = nullptr;     // 32-bit documents with sampled curves (avifgpu_write_rows_icc_sampled)
    const avifgpu_icc_clut16*    c8t = nullptr;     // 8-bit documents behind a LUT-based profile: the 33^3 table (avifgpu_write_rows_icc8_table)
    const avifgpu_icc_pipeline32* p32 = nullptr;    // 32-bit documents behind a LUT-based profile: lcms2's stage program (avifgpu_write_rows_icc_pipeline32)
};

// The optional destination of a grid save (include/avifgpu.h "grid save"): the planes go to the padded tiles of `tiles` (host records of
// host pointers, checked with check_grid_tiles of grid_save.h by whoever builds it: avifgpu_write_rows_grid, the shim) instead of dst[] / dst_stride[], which are then ignored.
struct GridDest { avifgpu_grid grid; const avifgpu_grid_tile* tiles; };

struct WriteGeom { bool color, alpha, dst16; int xs, ys, nplanes; };
struct ReadGeom { int xs, ys, nch, transfer; bool alpha; };

// ---- avifgpu_api.hip ------------------------------------------------------------------------------------------------
int  fail(int code, const char* fmt, ...);                         // formats avifgpu_last_error() of the calling thread
int  hip_fail(hipError_t e, const char* what, int code);
void set_error(const char* msg);
const char* last_error();
void set_last_kernel(const char* label);
// ---- icc_pipeline32.cpp ----------------------------------------------------------------------------------------------
bool icc_pipeline32_stamped(const avifgpu_icc_pipeline32* p);      // proven, and unchanged since

int  check_write(const avifgpu_write_desc* d, int row0, int nrows, WriteGeom& g);
// what every avifgpu_write_rows* entry is behind its own checks: validation, the armed statistics, the launch or the host scheduler
int  write_rows_with_icc(const avifgpu_write_desc* d, const IccArgs& icc, int32_t row0, int32_t nrows, const void* src, int64_t src_row_bytes,
                         void* const dst[4], const int64_t dst_stride[4], int32_t mem_kind, void* stream);
int  check_write_buffers(const avifgpu_write_desc* d, const WriteGeom& g, int nrows, const void* src, int64_t src_row_bytes,
                         void* const dst[4], const int64_t dst_stride[4]);
// Kernel parameters of one tile.  Uploads ICC tables to the CURRENT device's cache when they changed.
int  fill_write_params(const avifgpu_write_desc* d, int row0, int nrows, const WriteGeom& g, const IccArgs& icc, WriteParams& p);
void write_plane_extent(const avifgpu_write_desc* d, const WriteGeom& g, int plane, int nrows, int& rows, int64_t& row_bytes);
bool write_plane_used(const avifgpu_write_desc* d, const WriteGeom& g, int plane);

int  check_read(const avifgpu_read_desc* d, int row0, int nrows, ReadGeom& g);
int  check_read_buffers(const avifgpu_read_desc* d, const ReadGeom& g, int nrows, const void* const src[4], const int64_t src_stride[4],
                        const void* dst, int64_t dst_row_bytes);
int  fill_read_params(const avifgpu_read_desc* d, int nrows, const ReadGeom& g, ReadParams& p);
void read_plane_extent(const avifgpu_read_desc* d, const ReadGeom& g, int plane, int nrows, int& rows, int64_t& row_bytes);
bool read_plane_used(const avifgpu_read_desc* d, const ReadGeom& g, int plane);

int  hot_variant();
// ---- save_stats.cpp: the three statistics a save can carry -- the code histogram (avifgpu_histogram_attach), the thumbnail sums
// (avifgpu_thumbnail_attach), the summary of the written planes (avifgpu_summary_attach) -- armed, checked and launched in one place ------
// What is armed for one write call and where it goes.  A null target: not armed, or (the histogram) the descriptor is not counted.
struct SaveStats {
    uint64_t* hist = nullptr;                        // 1 << bit_depth bins
    uint64_t* thumb = nullptr; int tw = 0, th = 0;   // [(ty * tw + tx) * planes + c]
    uint32_t* summary = nullptr;                     // [AVIFGPU_SUMMARY_COUNTERS]
    bool any() const { return hist || thumb || summary; }
};
// The calling thread's arms for a write of `mem_kind`: 0 and *s, or formatBadParameters with a message -- histogram first, then thumbnail,
// then summary -- when an arm's memory kind disagrees, the histogram's bit depth is not the call's (depth-32 documents; others are not
// counted), or the thumbnail is larger than the smallest used plane.
int  save_stats_for_call(const avifgpu_write_desc* d, const WriteGeom& g, int mem_kind, SaveStats* s);
// The calling thread's arms that live in HOST memory, whatever the descriptor (what wait_all() merges into); *nbins: the histogram's
SaveStats save_stats_host(int* nbins);
// The statistics kernels of one tile behind its launch_write() on `st`, in that order, into s's targets on the stream's device: `p` is what
// that kernel was launched with (the histogram reads p.src again, the others the planes p.dst it wrote).  0 or writErr with a message.
int  launch_save_stats(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const WriteParams& p, const SaveStats& s, hipStream_t st);

// ---- thumbnail_kernels.hip: the box-average thumbnail of a save ------------------------------------------------------
constexpr int kThumbMaxSide = 1024;
// thumbnail rows [ty_lo, ty_hi) that source rows [row0, row0 + nrows) add to, over all planes
void thumbnail_rows_of_tile(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, int th, int& ty_lo, int& ty_hi);
// Sum the output codes of one tile into sums[(ty * tw + tx) * planes + c], enqueued behind the tile's launch_write(): `planes` / `stride` are
// the pointers that kernel wrote through (at row row0; chroma: row0 >> ys), sums lives on the stream's device.
hipError_t launch_thumbnail(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const uint8_t* const planes[4],
                            const int64_t stride[4], int tw, int th, unsigned long long* sums, hipStream_t st, int twin = 0);   // twin: avifgpu_probe_thumbnail

// ---- summary_kernels.hip: the summary of a save's written planes -----------------------------------------------------
// Raise counters[AVIFGPU_SUMMARY_COUNTERS] by the output codes of one tile, enqueued behind the tile's launch_write(): `planes` / `stride`
// are the pointers that kernel wrote through (at row row0; chroma: row0 >> ys), counters lives on the stream's device.
hipError_t launch_summary(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const uint8_t* const planes[4],
                          const int64_t stride[4], uint32_t* counters, hipStream_t st, int twin = 0);   // twin: avifgpu_probe_summary

// ---- staged_open.cpp: what avifgpu_read_rows_oriented / _upsampled / _cropped (orient_, upsample_, crop_kernels.hip) share on the host ----
// The region of output rows [orow0, orow0 + onrows) of an oriented image (open_geometry.h), from its descriptor.
inline bool region_of(const avifgpu_read_desc* d, const ReadGeom& g, int code, int orow0, int onrows, OpenRegion& r)
{
    return open_region(d->width, d->height, g.xs, g.ys, g.nch * (d->depth / 8), code, orow0, onrows, r);
}
// The checks the three entries share, with their codes and messages, in the order they have always run: mem_kind, null buffers, the int32
// limit on rowBytes, dst_row_bytes, check_read_buffers on the whole image, own(0), the scratch size against `need`, own(1),
// context_count(), onrows == 0.  own(step) = the entry's own checks in their place; whatever it returns but 0 ends the call.
// Returns 0: go on; kOpenEntryOver: the call is over and returns 0; anything else: the call returns it.
struct OpenEntry {
    const char* who; const char* scratch_helper;     // the entry, and the helper its scratch message names
    const avifgpu_read_desc* desc; const ReadGeom* g;
    int64_t out_w; int bpp; int onrows;              // the output: pixels of a row, bytes of a pixel
    const void* const* src; const int64_t* src_stride; void* dst; int64_t dst_row_bytes; void* scratch; int64_t scratch_bytes; int mem_kind;
};
constexpr int kOpenEntryOver = 1;
int  check_open_entry(const OpenEntry& a, int64_t need, const std::function<int(int)>& own);
// The staged path of a host-pointer call: rows [orow0, orow0 + onrows) of row_bytes payload bytes each, in tiles of at most
// max(2, tile_bytes / row_bytes) rows, through two slots (a stream, four plane buffers, scratch, out) on the first bound context.
//   plan(o0, left, max_rows, t)   the tile that starts at output row o0 with `left` rows of the call to go: its rows, what goes up, what it needs
//   enqueue(b)                    the feature's device path on the slot's buffers and stream; a library error code
// Uploads, the rows' way down to dst, the slot's reuse and the drain of both streams (also after a failure) are the driver's.
struct StagedUpload { const void* host; int64_t host_stride, row_bytes, rows, pitch; };    // host == nullptr: nothing goes up for this plane
struct StagedTile { int n; StagedUpload up[4]; int64_t out_pitch, scratch_bytes; };
struct StagedBuffers { const void* plane[4]; int64_t pitch[4]; void* out; void* scratch; hipStream_t stream; };
typedef std::function<int(int o0, int left, int max_rows, StagedTile& t)> StagedPlan;
typedef std::function<int(const StagedBuffers& b)> StagedEnqueue;
int  staged_open(const char* name, size_t tile_bytes, int64_t row_bytes, int orow0, int onrows, uint8_t* dst, int64_t dst_row_bytes,
                 const StagedPlan& plan, const StagedEnqueue& enqueue);
void release_open_staging();                         // the two slots (avifgpu_shutdown); nothing to do if never used

// ---- write_kernels.hip / read_kernels.hip ---------------------------------------------------------------------------
hipError_t launch_write(const WriteParams& p, int depth, int planes, bool dst16, int output, int xs, int ys,
                        int variant, hipStream_t st, char* label);
// the code histogram of the same tile (depth 32), enqueued behind launch_write(): bins = 1 << bit_depth counters on the stream's device
hipError_t launch_write_hist(const WriteParams& p, int planes, unsigned long long* bins, hipStream_t st, int twin = 0);   // twin: avifgpu_probe_histogram
hipError_t launch_read(const ReadParams& p, int colorspace, int depth, bool alpha, int xs, int ys,
                       hipStream_t st, char* label);
void release_device_caches();                        // read tables + ICC tables of every device (avifgpu_shutdown)

// ---- icc_tables.cpp: the ICC stage of a write call -- its WriteParams fields and the device copies of its tables, cached per HIP device
// (the calling thread's current one) and re-uploaded only when the contents change -------------------------------------
int  fill_icc_params(const avifgpu_write_desc* d, const IccArgs& icc, WriteParams& p);     // p zeroed; the first half of fill_write_params
void icc_epoch_for_call(int row0, int nrows);        // one call per C-ABI write call / shim tile that carries an ICC table (IccVerify, icc_tables.h)
void release_icc_tables();                           // every device's, under hipSetDevice; the caller's device is restored

// ---- pipeline.hip: bound contexts, staging slots, the row-tile scheduler --------------------------------------------
// A context = one HIP device ordinal + one worker thread + kSlots staging slots (device in/out buffers, pinned host in/out
// buffers, one stream and one completion event per slot).  The same ordinal may be bound several times (that is how the
// scheduler is exercised on a 1-GPU box); real deployments bind each GPU of the node once.
int  contexts_init(const int32_t* devices, int count);
void contexts_shutdown();
int  context_count();                               // worker contexts (bound devices x lanes)
int  bound_device_count();                          // entries of the avifgpu_init_devices list
int  context_device(int ctx);
int  slots_per_context();

// Row cut k of `world` over `height` rows, rounded down to even when `even` (same rule as sharding.row_cut).
int  row_cut(int height, int world, int k, bool even);

// Pinned host tile buffer of (ctx, slot), at least `bytes` long (the shim lets the host fill / drain it).  nullptr: out of memory.
void* tile_buffer(int ctx, int slot, size_t bytes);

// Queue one tile on a context; returns at once.  The caller must have waited for the slot (wait_slot) since its last use.
// Host pointers only.  `src` / `dst` may be pinned (DMA goes straight to them) or pageable (the worker bounces them through
// the slot's pinned buffers with its own memcpy, off the calling thread).
int  write_tile_enqueue(int ctx, int slot, const avifgpu_write_desc* d, int row0, int nrows, const void* src, int64_t src_row_bytes,
                        void* const dst[4], const int64_t dst_stride[4], const IccArgs& icc, const GridDest* grid = nullptr);
int  read_tile_enqueue(int ctx, int slot, const avifgpu_read_desc* d, int row0, int nrows, const void* const src[4],
                       const int64_t src_stride[4], void* dst, int64_t dst_row_bytes);
int  wait_slot(int ctx, int slot);                   // the tile last queued on (ctx, slot) has fully landed in host memory
int  wait_all();                                     // every context idle; returns the first error any tile produced.  What the tiles added to their
                                                     // contexts' statistics accumulators is merged into the calling thread's HOST arms (nothing on an error)
// One host-pointer conversion (whole-range call or a shim save / open) at a time per process: they share slots and error state.
void host_call_lock();
void host_call_unlock();
struct HostCallGuard { HostCallGuard() { host_call_lock(); } ~HostCallGuard() { host_call_unlock(); } };
// Topology of the bound devices (avifgpu_device_topology / avifgpu_topology_probe, include/avifgpu.h)
int  device_topology(int index, avifgpu_device_info* out);
int  device_traffic(int index, avifgpu_device_traffic* out, bool reset);
int  topology_plan(const char* sysfs_root, const char* const* bdfs, int count, avifgpu_device_info* out);
int  topology_probe_c(const char* sysfs_root, const char* bdf, int32_t* numa_node, char* cpulist, int32_t cpulist_len);

// Whole-range host conversions: rows [row0, row0 + nrows) are cut into one contiguous row tile per context (even cuts) and
// each tile is pipelined through that context's slots in sub-tiles.  Output bytes do not depend on the number of contexts.
int  write_rows_host(const avifgpu_write_desc* d, int row0, int nrows, const void* src, int64_t src_row_bytes,
                     void* const dst[4], const int64_t dst_stride[4], const IccArgs& icc, const GridDest* grid = nullptr);
int  read_rows_host(const avifgpu_read_desc* d, int row0, int nrows, const void* const src[4], const int64_t src_stride[4],
                    void* dst, int64_t dst_row_bytes);

} // namespace avifgpu
