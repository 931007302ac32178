// summary_kernels.hip -- the summary of a save's written planes (include/avifgpu.h "summary of a save").
//
// One kernel, plane_summary<sample type, layout>, reads the planes the conversion kernel of the same tile has just written (the slot's
// staging buffer on the host path, the caller's planes on the device path) and keeps, per output channel, the largest code and the largest
// 65535 - code, and for colour in R,G,B form the largest max(R,G,B) - min(R,G,B) of a pixel.  Every counter is a running maximum of 32-bit
// unsigned values: all-zero is the empty summary, merging is an element-wise max, feeding a row twice changes nothing.  It knows nothing
// of document depth, transfer, profile or alpha.  A translation unit -- and so a code object -- of its own: a process that never arms a
// summary never loads it.
//
// Shape (the thumbnail kernel's).  A workgroup of 256 lanes owns a COLUMN block and a BAND of consecutive plane rows; grid.z picks the
// plane.  A lane keeps its column position for the whole band and reads whole pixels, so that the spread needs no neighbour:
//   planar          one 16-byte load per row                      (16 u8 | 8 u16 samples)
//   3 interleaved   three 16-byte loads = 48 bytes per row        (16 u8 | 8 u16 pixels)
//   4 interleaved   one 16-byte load per row                      (4 u8 | 2 u16 pixels)
//   G,B,R planes    the same 16 bytes of each of the three planes (16 u8 | 8 u16 pixels)
// as non-temporal loads when the planes' bases and strides are multiples of 16 and the lane's bytes lie inside the row.  Any other lane
// -- the ragged end of a row, unaligned planes -- reads its samples one by one, and ONLY samples inside pw x prows: a sample slot that
// lies beyond the row repeats the same channel of the lane's first pixel, which changes no maximum.
// Per row the lane takes a packed 16-bit max and min per sample slot (u8 samples are first split into their even and odd bytes), and,
// where the spread is defined, max3 / min3 per pixel.  At the end of the band it folds the slots by channel, the wave reduces with
// shuffles, the waves meet in 9 LDS words (ds_max_u32), and the workgroup sends one atomicMax per counter that it would raise to device
// memory: ordinary vector atomics, at most 9 per workgroup, and none once the counters have reached the workgroup's values.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "kernel_params.h"
#include "written_planes.h"

namespace avifgpu {

namespace {

typedef uint32_t sm_u4 __attribute__((ext_vector_type(4)));
typedef uint16_t sm_h2 __attribute__((ext_vector_type(2)));
typedef const sm_u4 __attribute__((address_space(1)))* sm_gptr;

constexpr int kSumThreads = 256;
constexpr int kSumCounters = AVIFGPU_SUMMARY_COUNTERS;
constexpr int kSumHi = 0, kSumLoInv = 4, kSumSpread = 8;          // the layout of the counters (include/avifgpu.h)
enum { kPlanar = 1, kInter3 = 3, kInter4 = 4, kGbr = 5 };         // what a lane reads per row, see above

__device__ __forceinline__ uint32_t sm_pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(sm_h2, a), __builtin_bit_cast(sm_h2, b)));
}
__device__ __forceinline__ uint32_t sm_pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(sm_h2, a), __builtin_bit_cast(sm_h2, b)));
}

template <typename T, int LAYOUT> struct SumShape {
    static constexpr int NLOAD = (LAYOUT == kInter3 || LAYOUT == kGbr) ? 3 : 1;        // 16-byte loads of a lane per row
    static constexpr int K = 16 / (int)sizeof(T);                                      // samples of one load
    static constexpr int NS = NLOAD * K;                                               // sample slots of a lane
    static constexpr int NW = NLOAD * 4;                                               // their dwords
    static constexpr int NACC = sizeof(T) == 1 ? 2 * NW : NW;                          // packed accumulators: two 16-bit slots each
    static constexpr int NCH = LAYOUT == kInter3 ? 3 : (LAYOUT == kInter4 ? 4 : 1);    // interleaved channels of a plane
    static constexpr int NC = LAYOUT == kGbr ? 3 : NCH;                                // channels a lane sees
    static constexpr int CHUNK = (LAYOUT == kInter3 ? 3 : 1) * 16;                     // consecutive bytes of a lane in one plane row
    static constexpr int NPX = LAYOUT == kPlanar ? 0 : (LAYOUT == kInter4 ? K / 4 : K); // whole pixels of a lane (where the spread is defined)
    static constexpr int channel(int s) { return LAYOUT == kGbr ? s / K : s % NCH; }
    static constexpr int slot(int px, int c) { return LAYOUT == kGbr ? c * K + px : px * NCH + c; }
};

// sample slot s of the lane's dwords
template <typename T, int NW> __device__ __forceinline__ uint32_t sm_sample(const uint32_t (&w)[NW], int s)
{
    if constexpr (sizeof(T) == 1) return (w[s / 4] >> (8 * (s % 4))) & 0xffu;
    else return (w[s / 2] >> (16 * (s % 2))) & 0xffffu;
}
// sample slot s of the packed accumulators (u8: dword j of the row went to acc[2j] = bytes 0, 2 and acc[2j + 1] = bytes 1, 3)
template <typename T, int NACC> __device__ __forceinline__ uint32_t sm_slot(const uint32_t (&acc)[NACC], int s)
{
    if constexpr (sizeof(T) == 1) return (acc[2 * (s / 4) + (s & 1)] >> (16 * ((s % 4) >> 1))) & 0xffffu;
    else return (acc[s / 2] >> (16 * (s % 2))) & 0xffffu;
}

// one row of the lane: the per-slot packed max / min, and the spread of its whole pixels
template <typename T, int LAYOUT>
__device__ __forceinline__ void sm_row(const uint32_t (&w)[SumShape<T, LAYOUT>::NW], uint32_t (&hi)[SumShape<T, LAYOUT>::NACC],
                                       uint32_t (&mn)[SumShape<T, LAYOUT>::NACC], uint32_t& spread)
{
    using S = SumShape<T, LAYOUT>;
#pragma unroll
    for (int j = 0; j < S::NW; ++j) {
        if constexpr (sizeof(T) == 1) {
            const uint32_t e = w[j] & 0x00ff00ffu, o = (w[j] >> 8) & 0x00ff00ffu;
            hi[2 * j] = sm_pk_max(hi[2 * j], e);         mn[2 * j] = sm_pk_min(mn[2 * j], e);
            hi[2 * j + 1] = sm_pk_max(hi[2 * j + 1], o); mn[2 * j + 1] = sm_pk_min(mn[2 * j + 1], o);
        } else {
            hi[j] = sm_pk_max(hi[j], w[j]);
            mn[j] = sm_pk_min(mn[j], w[j]);
        }
    }
#pragma unroll
    for (int px = 0; px < S::NPX; ++px) {
        const uint32_t a = sm_sample<T, S::NW>(w, S::slot(px, 0)), b = sm_sample<T, S::NW>(w, S::slot(px, 1)), c = sm_sample<T, S::NW>(w, S::slot(px, 2));
        spread = max(spread, max(max(a, b), c) - min(min(a, b), c));
    }
}

template <typename T> __device__ __forceinline__ uint32_t sm_load1(const uint8_t* p)          // any address; little-endian u16
{
    if constexpr (sizeof(T) == 1) return p[0];
    else return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ uint32_t sm_wave_max(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

template <typename T, int LAYOUT>
__global__ __launch_bounds__(kSumThreads) void plane_summary(const SummaryParams p)
{
    using S = SumShape<T, LAYOUT>;
    __shared__ uint32_t s_cnt[kSumCounters];

    const SummaryPlane pl = p.pl[blockIdx.z];
    const uint32_t row_bytes = (uint32_t)pl.pw * S::NCH * (uint32_t)sizeof(T);        // < 2^31 (launch_summary)
    const uint32_t blk0 = blockIdx.x * (uint32_t)(kSumThreads * S::CHUNK);
    const int rb0 = (int)blockIdx.y * p.band_rows;
    if (blk0 >= row_bytes || rb0 >= pl.prows) return;              // the grid is sized for the largest plane
    const int rb1 = min(rb0 + p.band_rows, pl.prows);
    const uint32_t tid = threadIdx.x;
    if (tid < (uint32_t)kSumCounters) s_cnt[tid] = 0;
    __syncthreads();

    // the lane's column position: fixed for the whole band.  off and row_bytes are whole pixels, so cnt is
    const uint32_t off = blk0 + tid * S::CHUNK;
    const int cnt = off < row_bytes ? (int)(min((uint32_t)S::CHUNK, row_bytes - off) / sizeof(T)) : 0;      // samples of the lane inside the row, per plane
    const bool vec = pl.aligned != 0 && cnt * (int)sizeof(T) == S::CHUNK;

    uint32_t hi[S::NACC], mn[S::NACC], spread = 0;
#pragma unroll
    for (int j = 0; j < S::NACC; ++j) { hi[j] = 0; mn[j] = 0xffffffffu; }

    constexpr int ROWS = S::NLOAD == 3 ? 2 : 4;
    if (vec) {
        const uint8_t* cp[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) cp[l] = pl.base[LAYOUT == kGbr ? l : 0] + (int64_t)rb0 * pl.stride[LAYOUT == kGbr ? l : 0] + off + (LAYOUT == kGbr ? 0 : 16 * l);
        // rows in flight: 4 x 16 bytes per lane, or 2 x 48 (four rows of 48 bytes cost the u8 kernels half their waves)
#pragma unroll ROWS
        for (int r = rb0; r < rb1; ++r) {
            uint32_t w[S::NW];
#pragma unroll
            for (int l = 0; l < S::NLOAD; ++l) {
                const sm_u4 v = __builtin_nontemporal_load((sm_gptr)cp[l]);       // the planes are device memory: global, not flat, loads
                w[4 * l] = v[0]; w[4 * l + 1] = v[1]; w[4 * l + 2] = v[2]; w[4 * l + 3] = v[3];
                cp[l] += pl.stride[LAYOUT == kGbr ? l : 0];
            }
            sm_row<T, LAYOUT>(w, hi, mn, spread);
        }
    } else if (cnt > 0) {
        for (int r = rb0; r < rb1; ++r) {
            uint32_t w[S::NW];
#pragma unroll
            for (int j = 0; j < S::NW; ++j) w[j] = 0;
#pragma unroll
            for (int s = 0; s < S::NS; ++s) {
                // a slot beyond the row repeats the same channel of the lane's first pixel (slot s % NCH of the same plane, read before it)
                const int pln = LAYOUT == kGbr ? s / S::K : 0;
                const int i = LAYOUT == kGbr ? s % S::K : s;
                uint32_t v;
                if (i < cnt) v = sm_load1<T>(pl.base[pln] + (int64_t)r * pl.stride[pln] + off + i * (int)sizeof(T));
                else v = sm_sample<T, S::NW>(w, s - i + i % S::NCH);
                w[s * (int)sizeof(T) / 4] |= v << (8 * ((s * (int)sizeof(T)) % 4));
            }
            sm_row<T, LAYOUT>(w, hi, mn, spread);
        }
    }

    if (p.twin) {
        // avifgpu_probe_summary's atomics-free twin: the loads and the per-row register work only.  The registers stay alive through a
        // store that codes cannot cause (every packed maximum all ones)
        uint32_t all = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < S::NACC; ++j) all &= hi[j];
        if (all == 0xffffffffu && spread == 0xffffffffu) atomicMax(p.counters, 1u);
        return;
    }

    // fold the slots by channel; a lane that read nothing keeps hi = 0 and mn = 0xffff, that is 0 and 0: the identity
    uint32_t chi[S::NC], cmn[S::NC];
#pragma unroll
    for (int c = 0; c < S::NC; ++c) { chi[c] = 0; cmn[c] = 0xffffu; }
#pragma unroll
    for (int s = 0; s < S::NS; ++s) {
        chi[S::channel(s)] = max(chi[S::channel(s)], sm_slot<T, S::NACC>(hi, s));
        cmn[S::channel(s)] = min(cmn[S::channel(s)], sm_slot<T, S::NACC>(mn, s));
    }
    const bool leader = (tid & 63u) == 0;
#pragma unroll
    for (int c = 0; c < S::NC; ++c) {
        const uint32_t h = sm_wave_max(chi[c]), l = sm_wave_max(0xffffu - cmn[c]);
        if (leader && h) atomicMax(&s_cnt[kSumHi + pl.c0 + c], h);
        if (leader && l) atomicMax(&s_cnt[kSumLoInv + pl.c0 + c], l);
    }
    if constexpr (S::NPX > 0) {
        const uint32_t sp = sm_wave_max(spread);
        if (leader && sp) atomicMax(&s_cnt[kSumSpread], sp);
    }
    __syncthreads();
    if (tid < (uint32_t)kSumCounters) {
        const uint32_t v = s_cnt[tid];
        // a counter only grows, so what is read here is never above it: a workgroup whose value is reached already sends nothing.  Without
        // the look, 8192 workgroups x 9 atomics on the same nine words took 47 of the kernel's 107 us on 10-bit 4:4:4 planes
        if (v && v > __hip_atomic_load(p.counters + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.counters + tid, v);
    }
}

bool gbr_planes(const avifgpu_write_desc* d, const WriteGeom& g)
{
    return d->output == AVIFGPU_OUT_YCBCR && d->matrix_coefficients == AVIFGPU_MATRIX_RGB_GBR && g.xs == 0 && g.ys == 0;
}
// the spread is defined: R,G,B of a pixel are there to be compared
bool spread_defined(const avifgpu_write_desc* d, const WriteGeom& g)
{
    return g.color && (d->output == AVIFGPU_OUT_REFERENCE || gbr_planes(d, g));
}

template <typename T, int LAYOUT>
hipError_t launch_layout(SummaryParams& p, hipStream_t st)
{
    using S = SumShape<T, LAYOUT>;
    int max_rows = 0;
    int64_t max_bytes = 0;
    for (int i = 0; i < p.nslots; ++i) {
        max_rows = std::max(max_rows, p.pl[i].prows);
        max_bytes = std::max<int64_t>(max_bytes, (int64_t)p.pl[i].pw * S::NCH * (int64_t)sizeof(T));
    }
    if (max_rows <= 0 || max_bytes <= 0) return hipSuccess;
    if (max_bytes >= (int64_t)1 << 31) return hipErrorInvalidValue;               // the kernel indexes a row's bytes in 32 bits
    const int gx = (int)ceil_div64(max_bytes, (int64_t)kSumThreads * S::CHUNK);
    const int64_t band_rows = band_rows_for(gx, p.nslots, max_rows);
    p.band_rows = (int)band_rows;
    const dim3 grid((unsigned)gx, (unsigned)ceil_div64(max_rows, band_rows), (unsigned)p.nslots), block(kSumThreads);
    hipLaunchKernelGGL((plane_summary<T, LAYOUT>), grid, block, 0, st, p);
    return hipGetLastError();
}

template <int LAYOUT> hipError_t launch_layout_t(bool dst16, SummaryParams& p, hipStream_t st)
{
    return dst16 ? launch_layout<uint16_t, LAYOUT>(p, st) : launch_layout<uint8_t, LAYOUT>(p, st);
}

} // namespace

hipError_t launch_summary(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const uint8_t* const planes[4],
                          const int64_t stride[4], uint32_t* counters, hipStream_t st, int twin)
{
    if (nrows <= 0) return hipSuccess;
    SummaryParams p;
    memset(&p, 0, sizeof(p));
    p.counters = counters; p.twin = twin;
    WrittenPlane wp[4];
    const int n = written_planes(d, g, row0, nrows, planes, stride, wp);
    auto add = [&](int first, int joined) {                                       // joined 3: the G,B,R planes read together as one slot
        SummaryPlane& t = p.pl[p.nslots++];
        t.pw = wp[first].pw; t.prows = wp[first].prows; t.c0 = wp[first].c0; t.aligned = 1;
        for (int l = 0; l < joined; ++l) {
            const WrittenPlane& w = wp[first + l];
            t.base[l] = planes[w.plane]; t.stride[l] = stride[w.plane];
            t.aligned &= (int)w.aligned;
        }
    };
    if (d->output == AVIFGPU_OUT_REFERENCE && g.color) {
        add(0, 1);
        return d->planes == 3 ? launch_layout_t<kInter3>(g.dst16, p, st) : launch_layout_t<kInter4>(g.dst16, p, st);
    }
    if (!gbr_planes(d, g)) {
        for (int i = 0; i < n; ++i) add(i, 1);
        return launch_layout_t<kPlanar>(g.dst16, p, st);
    }
    add(0, 3);
    const hipError_t e = launch_layout_t<kGbr>(g.dst16, p, st);
    if (e != hipSuccess || !g.alpha) return e;
    p.nslots = 0;
    add(3, 1);
    return launch_layout_t<kPlanar>(g.dst16, p, st);
}

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_summary_merge(uint32_t* into, const uint32_t* from)
{
    set_error("");
    if (!into || !from) return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_merge: null argument");
    for (int k = 0; k < kSumCounters; ++k) into[k] = std::max(into[k], from[k]);
    return 0;
}

int32_t avifgpu_summary_read(const avifgpu_write_desc* desc, const uint32_t* counters, avifgpu_save_summary* out)
{
    set_error("");
    if (!desc || !counters || !out) return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_read: null argument");
    WriteGeom g;
    const int err = check_write(desc, 0, 0, g);
    if (err) return err;
    const int C = desc->planes;
    const uint32_t maxcode = (1u << desc->bit_depth) - 1u;
    const bool has_spread = spread_defined(desc, g);
    for (int c = 0; c < C; ++c) {
        if (counters[kSumLoInv + c] == 0)
            return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_read: channel %d was never fed", c);
        if (counters[kSumHi + c] > maxcode || counters[kSumLoInv + c] > 65535u)
            return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_read: channel %d reaches code %u above %u: the counters are not of this descriptor",
                        c, counters[kSumHi + c], maxcode);
    }
    if (has_spread && counters[kSumSpread] > maxcode)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_summary_read: spread %u above %u: the counters are not of this descriptor", counters[kSumSpread], maxcode);
    avifgpu_save_summary s;
    memset(&s, 0, sizeof(s));
    s.channels = C;
    for (int c = 0; c < C; ++c) { s.max_code[c] = (int32_t)counters[kSumHi + c]; s.min_code[c] = (int32_t)(65535u - counters[kSumLoInv + c]); }
    s.spread = has_spread ? (int32_t)counters[kSumSpread] : -1;
    s.alpha_opaque = s.alpha_clear = -1;
    if (g.alpha) {
        s.alpha_opaque = s.min_code[C - 1] == (int32_t)maxcode;
        s.alpha_clear = s.max_code[C - 1] == 0;
    }
    const int32_t half = 1 << (desc->bit_depth - 1);
    if (!g.color) s.neutral = 1;
    else if (has_spread) s.neutral = s.spread == 0;
    else {
        const int32_t lo = desc->chroma_zero_point == AVIFGPU_CHROMA_ZERO_DECODER ? half - 1 : half;    // the DECODER zero point is half - 0.5
        s.neutral = s.min_code[1] >= lo && s.max_code[1] <= half && s.min_code[2] >= lo && s.max_code[2] <= half;
    }
    if (s.alpha_opaque == 1) s.advice |= AVIFGPU_ADVICE_DROP_ALPHA;
    if (g.color && s.neutral) s.advice |= AVIFGPU_ADVICE_MONOCHROME;
    *out = s;
    return 0;
}

int32_t avifgpu_probe_summary(const avifgpu_write_desc* desc, int32_t twin, const void* const planes[4], const int64_t stride[4],
                              uint32_t* counters, void* stream)
{
    set_error("");
    WriteGeom g;
    int err = check_write(desc, 0, desc ? desc->height : 0, g);
    if (err) return err;
    if (!planes || !stride || !counters) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_summary: null argument");
    if (twin < 0 || twin > 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_summary: twin %d is not 0 or 1", twin);
    const uint8_t* pp[4];
    if ((err = check_probe_planes("avifgpu_probe_summary", desc, g, planes, stride, pp))) return err;
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    const hipError_t e = launch_summary(desc, g, 0, desc->height, pp, stride, counters, (hipStream_t)stream, twin);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_summary", AVIFGPU_writErr);
}

} // extern "C"
