// thumbnail_kernels.hip -- the box-average thumbnail of a save (include/avifgpu.h "thumbnail of a save").
//
// One kernel, thumb_box_sums<sample type, interleaved channels>, reads the planes the conversion kernel of the same tile has just written
// (the slot's staging buffer on the host path, the caller's planes on the device path) and adds every output code to the 64-bit counter
// of its thumbnail cell and channel.  It knows nothing of document depth, transfer, profile or alpha: whatever was written is averaged.
// A translation unit -- and so a code object -- of its own: a process that never arms a thumbnail never loads it.
//
// Shape.  A workgroup of 256 lanes owns a COLUMN block (256 x 16 bytes of a plane row) and a BAND of consecutive plane rows; the plane is
// grid.z.  A lane keeps its 16 bytes' column position for the whole band, so
//   * its first cell and the cell boundary behind it are worked out once per workgroup (two divisions), and walked from there by
//     adding pw / tw and pw % tw with a carry -- exact, 32-bit, no division per sample;
//   * the rows of the band that share a thumbnail row are summed sample by sample in registers (one 16-byte non-temporal load and 8 / 16
//     adds per row), and only at the end of that run of rows does the lane merge its samples by cell and channel;
//   * a wave whose lanes all lie in one cell reduces across its lanes and adds once per channel; any other wave adds per lane and cell;
//     both go to 64-bit LDS counters (ds_add_u64) that hold the piece of the thumbnail row the column block covers;
//   * the workgroup then flushes the non-zero counters to the global sums, consecutive lanes to consecutive counters (vector atomics).
// Atomic volume per launch is about (bands) x tw x C x 8 bytes.
//
// No wrap for any legal geometry: a lane's per-sample register sum is 32-bit and covers at most band_rows rows of codes <= 65535
// (u16 container), band_rows <= 32768 (launch_thumbnail), 65535 * 32768 < 2^32; everything behind it (lane merge, LDS, global) is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "kernel_params.h"
#include "written_planes.h"

namespace avifgpu {

namespace {

typedef uint32_t tb_u4 __attribute__((ext_vector_type(4)));

constexpr int kThumbThreads = 256;
constexpr int kThumbLaneBytes = 16;
// LDS counters of a workgroup: one per (cell, channel) its column block can touch.  The block holds S = 4096 u8 or 2048 u16 samples; with
// 3 interleaved channels it may start and end inside a pixel, so it touches P <= S / NCH + 2 pixels [a, b], b - a = P - 1, and
// floor(b tw / pw) - floor(a tw / pw) <= floor((P - 1) tw / pw) + 1, that is at most floor((S / NCH + 1) tw / pw) + 2 cells -- and never more
// cells than pixels (tw <= pw): at most 1366 x 3 = 4098 counters.  launch_thumbnail sizes the dynamic LDS by the first bound, capped by this.
constexpr int kThumbEntries = 4096 + 8;
constexpr int kThumbMaxBandRows = 32768;          // see "No wrap" above

// a / b for a < 2^42, b < 2^31: 32-bit when the dividend allows it (every plane narrower than 2^22 pixels)
__device__ __forceinline__ uint32_t tb_div(uint64_t a, uint32_t b)
{
    if ((a >> 32) == 0) return (uint32_t)a / b;
    return (uint32_t)(a / b);
}

template <typename T, int K> __device__ __forceinline__ void tb_add16(uint32_t (&acc)[K], const tb_u4 v)
{
    if constexpr (sizeof(T) == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[4 * i + 0] += v[i] & 0xffu;
            acc[4 * i + 1] += (v[i] >> 8) & 0xffu;
            acc[4 * i + 2] += (v[i] >> 16) & 0xffu;
            acc[4 * i + 3] += v[i] >> 24;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[2 * i + 0] += v[i] & 0xffffu;
            acc[2 * i + 1] += v[i] >> 16;
        }
    }
}

// one sample at any address (planes with a stride or a base that is no multiple of 16, and the ragged end of a row); little-endian u16
template <typename T> __device__ __forceinline__ uint32_t tb_load1(const uint8_t* p)
{
    if constexpr (sizeof(T) == 1) return p[0];
    else return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ unsigned long long tb_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

template <typename T, int NCH>
__global__ __launch_bounds__(kThumbThreads) void thumb_box_sums(const ThumbParams p)
{
    constexpr int K = kThumbLaneBytes / (int)sizeof(T);        // samples of a lane
    constexpr uint32_t BLK = (uint32_t)K * kThumbThreads;      // samples of a column block
    extern __shared__ unsigned long long s_acc[];              // p.lds_entries counters (launch_thumbnail)
    __shared__ int s_tx[2];

    const ThumbPlane pl = p.pl[blockIdx.z];
    const uint32_t pw = (uint32_t)pl.pw, ph = (uint32_t)pl.ph, tw = (uint32_t)p.tw, th = (uint32_t)p.th;
    const uint32_t nsamp = pw * NCH;                           // < 2^31 (launch_thumbnail)
    const uint32_t blk0 = blockIdx.x * BLK;
    const int rb0 = (int)blockIdx.y * p.band_rows;
    if (blk0 >= nsamp || rb0 >= pl.prows) return;              // the grid is sized for the largest plane
    const int rb1 = min(rb0 + p.band_rows, pl.prows);
    const uint32_t tid = threadIdx.x;

    for (uint32_t e = tid; e < (uint32_t)p.lds_entries; e += kThumbThreads) s_acc[e] = 0;
    if (tid == 0) {
        s_tx[0] = (int)tb_div((uint64_t)(blk0 / NCH) * tw, pw);
        s_tx[1] = (int)tb_div((uint64_t)((min(blk0 + BLK, nsamp) - 1u) / NCH) * tw, pw);
    }
    __syncthreads();
    const int txf = s_tx[0];
    const uint32_t nent = (uint32_t)(s_tx[1] - txf + 1) * NCH;

    // the lane's column position: fixed for the whole band
    const uint32_t s0 = blk0 + tid * K;
    const int cnt = s0 < nsamp ? (int)min((uint32_t)K, nsamp - s0) : 0;
    const uint32_t px0 = s0 / NCH;
    const int c0 = (int)(s0 - px0 * NCH);                      // channel of the lane's first sample
    int tx0 = 0;
    uint32_t q0 = 0, r0 = 0;                                   // (tx0 + 1) * pw = q0 * tw + r0: the boundary behind cell tx0 is ceil = q0 + (r0 > 0)
    if (cnt > 0) {
        tx0 = (int)tb_div((uint64_t)px0 * tw, pw);
        const uint64_t a = (uint64_t)(tx0 + 1) * pw;
        q0 = tb_div(a, tw);
        r0 = (uint32_t)(a - (uint64_t)q0 * tw);
    }
    const uint32_t qs = pw / tw, rs = pw - qs * tw;            // one cell further: q += qs, r += rs, carry at tw
    const uint32_t px_last = cnt > 0 ? (s0 + (uint32_t)cnt - 1u) / NCH : 0u;
    const bool lane_one_cell = px_last < q0 + (r0 > 0 ? 1u : 0u);
    // the wave adds once per channel when every lane that holds samples lies in the cell of its first lane
    const int tx_wave = __shfl(tx0, 0, 64);
    const bool wave_one_cell = __all(cnt == 0 || (lane_one_cell && tx0 == tx_wave)) != 0;
    const bool wave_leader = (tid & 63u) == 0;

    const uint8_t* const col = pl.base + (size_t)s0 * sizeof(T);
    const bool vec = pl.aligned != 0 && cnt == K;

    int r = rb0;
    while (r < rb1) {
        // the run of band rows that share thumbnail row ty (wave-uniform)
        const uint32_t prow = (uint32_t)(pl.prow0 + r);
        const uint32_t ty = tb_div((uint64_t)prow * th, ph);
        const uint64_t yb_num = (uint64_t)(ty + 1u) * ph + (th - 1u);
        const uint32_t yb = tb_div(yb_num, th);                // ceil((ty + 1) ph / th) > prow
        const int rend = min(rb1, (int)(yb - (uint32_t)pl.prow0));

        uint32_t acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0;
        if (vec) {
            const uint8_t* cp = col + (int64_t)r * pl.stride;
            int rr = r;
            // four rows per trip.  Keeping a second group of four in flight (two register sets, ping-pong) was measured and lost on every
            // frame, 1-8 % (profiles/thumbnail/load_loop_ab.txt): the loop is not short of loads in flight
            for (; rr + 4 <= rend; rr += 4) {
                const tb_u4 v0 = __builtin_nontemporal_load(reinterpret_cast<const tb_u4*>(cp));
                const tb_u4 v1 = __builtin_nontemporal_load(reinterpret_cast<const tb_u4*>(cp + pl.stride));
                const tb_u4 v2 = __builtin_nontemporal_load(reinterpret_cast<const tb_u4*>(cp + 2 * pl.stride));
                const tb_u4 v3 = __builtin_nontemporal_load(reinterpret_cast<const tb_u4*>(cp + 3 * pl.stride));
                cp += 4 * pl.stride;
                tb_add16<T, K>(acc, v0); tb_add16<T, K>(acc, v1); tb_add16<T, K>(acc, v2); tb_add16<T, K>(acc, v3);
            }
            for (; rr < rend; ++rr) {
                tb_add16<T, K>(acc, __builtin_nontemporal_load(reinterpret_cast<const tb_u4*>(cp)));
                cp += pl.stride;
            }
        } else if (cnt > 0) {
            const uint8_t* cp = col + (int64_t)r * pl.stride;
            for (int rr = r; rr < rend; ++rr) {
#pragma unroll
                for (int k = 0; k < K; ++k) if (k < cnt) acc[k] += tb_load1<T>(cp + k * sizeof(T));
                cp += pl.stride;
            }
        }

        if (p.twin) {
            // avifgpu_probe_thumbnail's atomics-free twin: the loads and the register adds only.  The sums stay alive through an add that
            // codes cannot produce (every per-sample sum at its ceiling)
            uint32_t all = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < K; ++k) all &= acc[k];
            if (all == 0xffffffffu) atomicAdd(p.sums, 1ull);
            r = rend;
            continue;
        }
        // merge the lane's samples.  part[j] sums samples k = j (mod NCH), whose channel is (c0 + j) % NCH
        if (wave_one_cell) {
            unsigned long long part[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) part[j] = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) part[k % NCH] += acc[k];
            unsigned long long ch[NCH];                        // by channel
            if constexpr (NCH == 3) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ch[c] = c0 == 0 ? part[c] : (c0 == 1 ? part[(c + 2) % 3] : part[(c + 1) % 3]);
            } else {                                           // NCH 1 | 4: a lane starts on a pixel (K is a multiple of 4)
#pragma unroll
                for (int c = 0; c < NCH; ++c) ch[c] = part[c];
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const unsigned long long v = tb_wave_sum(ch[c]);
                if (wave_leader && v) atomicAdd(&s_acc[(uint32_t)(tx_wave - txf) * NCH + c], v);
            }
        } else if (cnt > 0) {
            unsigned long long part[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) part[j] = 0;
            int tx = tx0, c = c0;
            uint32_t q = q0, rm = r0, px = px0;
            uint32_t bnd = q + (rm > 0 ? 1u : 0u);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k < cnt) {
                    if (k > 0 && c == 0 && px >= bnd) {        // a new pixel in the next cell (every cell holds a pixel: one step is enough)
#pragma unroll
                        for (int j = 0; j < NCH; ++j) {
                            if (part[j]) atomicAdd(&s_acc[(uint32_t)(tx - txf) * NCH + (uint32_t)((c0 + j) % NCH)], part[j]);
                            part[j] = 0;
                        }
                        ++tx; q += qs; rm += rs;
                        if (rm >= tw) { rm -= tw; ++q; }
                        bnd = q + (rm > 0 ? 1u : 0u);
                    }
                    part[k % NCH] += acc[k];
                    if (++c == NCH) { c = 0; ++px; }
                }
            }
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                if (part[j]) atomicAdd(&s_acc[(uint32_t)(tx - txf) * NCH + (uint32_t)((c0 + j) % NCH)], part[j]);
        }
        __syncthreads();
        // flush this piece of thumbnail row ty: consecutive lanes, consecutive counters
        unsigned long long* const out = p.sums + ((size_t)ty * tw + (uint32_t)txf) * (uint32_t)p.C + (uint32_t)pl.c0;
        for (uint32_t e = tid; e < nent; e += kThumbThreads) {
            const unsigned long long v = s_acc[e];
            if (v) {
                s_acc[e] = 0;
                atomicAdd(out + (size_t)(e / NCH) * (uint32_t)p.C + (e % NCH), v);
            }
        }
        __syncthreads();
        r = rend;
    }
}

} // namespace

void thumbnail_rows_of_tile(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, int th, int& ty_lo, int& ty_hi)
{
    ty_lo = th; ty_hi = 0;
    for (int c = 0; c < d->planes; ++c) {
        int pw, ph;
        const bool chroma = channel_extent(d, g, c, pw, ph);
        const int64_t p0 = chroma ? row0 >> g.ys : row0, pn = chroma ? (nrows + g.ys) >> g.ys : nrows;
        if (pn <= 0) continue;
        ty_lo = std::min<int>(ty_lo, (int)(p0 * th / ph));
        ty_hi = std::max<int>(ty_hi, (int)((p0 + pn - 1) * th / ph) + 1);
    }
    if (ty_hi < ty_lo) ty_lo = ty_hi = 0;
}

hipError_t launch_thumbnail(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const uint8_t* const planes[4],
                            const int64_t stride[4], int tw, int th, unsigned long long* sums, hipStream_t st, int twin)
{
    if (nrows <= 0) return hipSuccess;
    ThumbParams p;
    memset(&p, 0, sizeof(p));
    p.twin = twin;
    p.sums = sums; p.tw = tw; p.th = th; p.C = d->planes;
    const int ssz = g.dst16 ? 2 : 1;
    const bool interleaved = d->output == AVIFGPU_OUT_REFERENCE && g.color;
    const int nch = interleaved ? d->planes : 1;
    int max_rows = 0;
    int64_t max_samples = 0, max_entries = 0;
    const int64_t blk = (int64_t)(kThumbLaneBytes / ssz) * kThumbThreads;
    WrittenPlane wp[4];
    p.nslots = written_planes(d, g, row0, nrows, planes, stride, wp);
    for (int i = 0; i < p.nslots; ++i) {
        const WrittenPlane& w = wp[i];
        ThumbPlane& t = p.pl[i];
        t.base = planes[w.plane]; t.stride = stride[w.plane];
        t.pw = w.pw; t.ph = w.ph; t.prow0 = w.prow0; t.prows = w.prows; t.c0 = w.c0; t.aligned = w.aligned;
        max_rows = std::max(max_rows, t.prows);
        max_samples = std::max<int64_t>(max_samples, (int64_t)t.pw * nch);
        max_entries = std::max<int64_t>(max_entries, (((blk / nch + 1) * tw) / t.pw + 2) * nch);     // see kThumbEntries
    }
    if (max_samples * ssz >= (int64_t)1 << 31) return hipErrorInvalidValue;        // the kernel indexes a row's samples in 32 bits
    p.lds_entries = (int)std::min<int64_t>(max_entries, kThumbEntries);
    const int gx = (int)ceil_div64(max_samples, blk);
    const int64_t band_rows = band_rows_for(gx, p.nslots, max_rows);       // <= kThumbMaxBandRows keeps the 32-bit register sums from wrapping
    if (band_rows > kThumbMaxBandRows) return hipErrorInvalidValue;                // unreachable: max_rows < 2^31 = 65535 * 32768 + ...
    p.band_rows = (int)band_rows;
    const dim3 grid((unsigned)gx, (unsigned)ceil_div64(max_rows, band_rows), (unsigned)p.nslots), block(kThumbThreads);
#define AG_THUMB_LAUNCH(T_, N_) hipLaunchKernelGGL((thumb_box_sums<T_, N_>), grid, block, (size_t)p.lds_entries * sizeof(unsigned long long), st, p)
    if (ssz == 1) { if (nch == 1) AG_THUMB_LAUNCH(uint8_t, 1); else if (nch == 3) AG_THUMB_LAUNCH(uint8_t, 3); else AG_THUMB_LAUNCH(uint8_t, 4); }
    else          { if (nch == 1) AG_THUMB_LAUNCH(uint16_t, 1); else if (nch == 3) AG_THUMB_LAUNCH(uint16_t, 3); else AG_THUMB_LAUNCH(uint16_t, 4); }
#undef AG_THUMB_LAUNCH
    return hipGetLastError();
}

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_thumbnail_fit(const avifgpu_write_desc* desc, int32_t bbox, int32_t* tw, int32_t* th)
{
    set_error("");
    if (!desc || !tw || !th) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_fit: null argument");
    if (bbox < 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_fit: bounding box %d < 1", bbox);
    WriteGeom g;
    const int err = check_write(desc, 0, 0, g);
    if (err) return err;
    const int64_t W = desc->width, H = desc->height;
    int64_t w = W, h = H;
    if (std::max(W, H) > bbox) {
        if (W >= H) { w = bbox; h = std::max<int64_t>(1, (2 * H * bbox + W) / (2 * W)); }
        else        { h = bbox; w = std::max<int64_t>(1, (2 * W * bbox + H) / (2 * H)); }
    }
    int pw, ph;
    smallest_plane(desc, g, pw, ph);
    *tw = (int32_t)std::min<int64_t>(std::min<int64_t>(w, pw), kThumbMaxSide);
    *th = (int32_t)std::min<int64_t>(std::min<int64_t>(h, ph), kThumbMaxSide);
    return 0;
}

int32_t avifgpu_thumbnail_from_sums(const avifgpu_write_desc* desc, int32_t tw, int32_t th, const uint64_t* sums,
                                    void* const dst[4], const int64_t dst_stride[4])
{
    set_error("");
    if (!desc || !sums || !dst || !dst_stride) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_from_sums: null argument");
    WriteGeom g;
    const int err = check_write(desc, 0, 0, g);
    if (err) return err;
    int spw, sph;
    smallest_plane(desc, g, spw, sph);
    if (tw < 1 || th < 1 || tw > kThumbMaxSide || th > kThumbMaxSide || tw > spw || th > sph)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_from_sums: size %dx%d outside 1..%d or above the smallest plane %dx%d", tw, th, kThumbMaxSide, spw, sph);
    const int C = desc->planes, ssz = g.dst16 ? 2 : 1;
    const uint64_t maxcode = (1u << desc->bit_depth) - 1u;
    const bool interleaved = desc->output == AVIFGPU_OUT_REFERENCE && g.color;
    for (int c = 0; c < C; ++c) {
        const int plane = interleaved ? 0 : (desc->output == AVIFGPU_OUT_REFERENCE ? (c == 0 ? 0 : 3) : c);
        const int64_t min_row = (int64_t)tw * (interleaved ? C : 1) * ssz;
        if (!dst[plane]) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_from_sums: destination plane %d is null", plane);
        if (dst_stride[plane] < min_row) return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_from_sums: dst_stride[%d] %lld < %lld", plane, (long long)dst_stride[plane], (long long)min_row);
    }
    // first pass: every sum within n * maxcode, so that nothing is written for a frame that was not fed exactly once
    for (int pass = 0; pass < 2; ++pass) {
        for (int c = 0; c < C; ++c) {
            int pw, ph; channel_extent(desc, g, c, pw, ph);
            const int plane = interleaved ? 0 : (desc->output == AVIFGPU_OUT_REFERENCE ? (c == 0 ? 0 : 3) : c);
            uint8_t* const base = static_cast<uint8_t*>(dst[plane]);
            for (int ty = 0; ty < th; ++ty) {
                const uint64_t ny = (uint64_t)(ceil_div64((int64_t)(ty + 1) * ph, th) - ceil_div64((int64_t)ty * ph, th));
                for (int tx = 0; tx < tw; ++tx) {
                    const uint64_t n = ny * (uint64_t)(ceil_div64((int64_t)(tx + 1) * pw, tw) - ceil_div64((int64_t)tx * pw, tw));
                    const uint64_t s = sums[((size_t)ty * tw + tx) * C + c];
                    if (pass == 0) {
                        if (s > n * maxcode)
                            return fail(AVIFGPU_formatBadParameters, "avifgpu_thumbnail_from_sums: sum %llu of cell (%d,%d) channel %d exceeds %llu samples x %llu: "
                                        "the frame was not summed exactly once", (unsigned long long)s, tx, ty, c, (unsigned long long)n, (unsigned long long)maxcode);
                        continue;
                    }
                    const uint32_t code = (uint32_t)((2 * s + n) / (2 * n));
                    uint8_t* const o = base + (int64_t)ty * dst_stride[plane] + (int64_t)(interleaved ? tx * C + c : tx) * ssz;
                    o[0] = (uint8_t)(code & 0xffu);
                    if (ssz == 2) o[1] = (uint8_t)(code >> 8);
                }
            }
        }
    }
    return 0;
}

int32_t avifgpu_probe_thumbnail(const avifgpu_write_desc* desc, int32_t twin, int32_t tw, int32_t th, const void* const planes[4],
                                const int64_t stride[4], uint64_t* sums, void* stream)
{
    set_error("");
    WriteGeom g;
    int err = check_write(desc, 0, desc ? desc->height : 0, g);
    if (err) return err;
    if (!planes || !stride || !sums) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_thumbnail: null argument");
    if (twin < 0 || twin > 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_thumbnail: twin %d is not 0 or 1", twin);
    int pw, ph;
    smallest_plane(desc, g, pw, ph);
    if (tw < 1 || th < 1 || tw > kThumbMaxSide || th > kThumbMaxSide || tw > pw || th > ph)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_thumbnail: size %dx%d outside 1..%d or above the smallest plane %dx%d", tw, th, kThumbMaxSide, pw, ph);
    const uint8_t* pp[4];
    if ((err = check_probe_planes("avifgpu_probe_thumbnail", desc, g, planes, stride, pp))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    const hipError_t e = launch_thumbnail(desc, g, 0, desc->height, pp, stride, tw, th, reinterpret_cast<unsigned long long*>(sums), (hipStream_t)stream, twin);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_thumbnail", AVIFGPU_writErr);
}

} // extern "C"
