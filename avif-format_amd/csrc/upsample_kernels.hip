// upsample_kernels.hip -- bilinear chroma upsampling of a 4:2:0 / 4:2:2 open, on the GPU (include/avifgpu.h "upsampled open").
//
// The decode arithmetic is not copied and no existing kernel is touched.  chroma_upsample writes the two full-resolution chroma planes
// U(Cb), U(Cr) of a source REGION into scratch, and the existing 4:4:4 open (avifgpu_read_rows, behind it the existing orient kernels for
// codes 2-8) then runs on (Y, U(Cb), U(Cr), A) with a copy of the descriptor.  A translation unit -- and so a code object -- of its own: a
// process that never asks for interpolation never loads it.  The region is open_geometry.h's; the entry's shared argument checks and the
// host-pointer path are staged_open.cpp's, which this file tells what goes up for a tile (Y, A, the chroma windows) and what is enqueued.
//
// The definition is integer and exact (avifgpu.h): per direction two taps with weights in quarters, indices clamped to the WHOLE plane,
//     U[y, x] = (sum_a sum_b wy_a wx_b C[jy_a, ix_b] + 8) >> 4        -- ONE rounding of the joint sum.
//
// chroma_upsample<T, YS, SITING>.  The kernel produces an arbitrary rectangle [x0, x0 + w) x [y0, y0 + h) of U from a RESIDENT WINDOW of C
// (base, stride, origin in chroma coordinates) and clamps against the whole plane's cw, ch -- so a tile's bytes do not depend on the
// tiling, and the host path uploads only a region's chroma plus a few samples of halo on each side that exists.
//   * a lane owns 16 bytes of an output row (16 u8 / 8 u16 samples), stored non-temporally; a wave owns 1024 contiguous output bytes;
//   * a wave walks DOWN a band of 32 output rows: every chroma row of the band is loaded once (8 bytes per lane where base, stride and
//     window origin allow, sample by sample otherwise), turned into the lane's 16 / 8 UNROUNDED horizontal sums, and kept in registers
//     together with the row below it; each output row is then one combine (3 A + B or A + 3 B; 4 A for 4:2:2), + 8, >> 4;
//   * the neighbour samples i - 1 / i + 1 at a lane's edges come from the adjacent lane by a cross-lane move, at a wave's edges from one
//     extra clamped load.  No LDS memory, no barrier: the four waves of a workgroup are independent (four neighbouring spans).
// Every index that is loaded is clamped to the samples the rectangle needs, which are inside the window by contract: a lane or wave that
// hangs over the rectangle's right edge reads nothing beyond them and stores only its valid samples, one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "staging.h"
#include "upsample_window.h"

namespace avifgpu {

namespace {

typedef uint32_t up_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t up_u2 __attribute__((ext_vector_type(2)));

struct UpsampleParams {
    const uint8_t* src[2]; int64_t src_stride[2];   // the resident window of Cb, Cr: src[i] is sample (wy0, wx0)
    uint8_t* dst[2]; int64_t dst_stride;            // the rectangle of U(Cb), U(Cr): dst[i] is sample (y0, x0)
    int32_t wx0, wy0;                               // origin of the window in chroma coordinates
    int32_t cw, ch;                                 // the WHOLE chroma plane: what indices are clamped against
    int32_t x0, y0, w, h;                           // the rectangle, in luma coordinates
    int32_t vec_src[2];                             // the lanes' 8-byte source loads are aligned
    int32_t vec_dst;                                // dst bases and stride are multiples of 16
};

constexpr int kUpThreads = 256;                     // four waves, four neighbouring spans of a row
constexpr int kUpBand = 32;                         // output rows a wave walks down

// the N unrounded horizontal sums (weights in quarters) of a lane from its N / 2 + 2 chroma samples c[0] = C[ibase - 1] .. c[N / 2 + 1]
template <int N, int SITING, bool ODD0> __device__ __forceinline__ void up_hsums(const uint32_t (&c)[N / 2 + 2], uint32_t (&h)[N])
{
#pragma unroll
    for (int t = 0; t < N; ++t) {
        const bool xodd = ((t & 1) != 0) != ODD0;
        const int m = (ODD0 ? ((t + 1) >> 1) : (t >> 1)) + 1;            // c[m] = C[x >> 1]
        const int mn = xodd ? m + 1 : m - 1;                             // the other tap: the neighbour on the pixel's side
        if constexpr (SITING == AVIFGPU_UPSAMPLE_BILINEAR_CENTER) h[t] = 3u * c[m] + c[mn];
        else h[t] = xodd ? 2u * c[m] + 2u * c[mn] : 4u * c[m];
    }
}

// TWIN (avifgpu_probe_upsample, attribution only): 1 = store-only (no source load, no cross-lane move, the same combine and stores);
// 2 = math-free (the same loads and stores; no neighbour samples, no sums: a lane stores the samples it loaded, each twice).
template <typename T, int YS, int SITING, int TWIN = 0>
__global__ __launch_bounds__(kUpThreads) void chroma_upsample(const UpsampleParams p)
{
    constexpr int N = 16 / (int)sizeof(T);                     // samples of a lane
    constexpr int HN = N / 2;                                  // chroma samples under them
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int pl = (int)blockIdx.z;
    const int64_t span = (int64_t)blockIdx.x * (kUpThreads / 64) + wave;
    if (span * 64 * N >= p.w) return;                          // wave-uniform; there is no barrier below
    const int64_t t0 = (span * 64 + lane) * N;                 // the lane's first sample, relative to x0
    const int nvalid = (int)min((int64_t)N, max((int64_t)0, (int64_t)p.w - t0));
    const bool full = nvalid == N;
    const bool odd0 = (p.x0 & 1) != 0;
    const int ibase = (int)(((int64_t)p.x0 + t0) >> 1);
    // what the rectangle needs, and so what the window holds
    const UpNeed need = up_need(p.cw, p.ch, YS, p.x0, p.y0, p.w, p.h);
    const int lo = need.lo, hi = need.hi, rlo = need.rlo, rhi = need.rhi;
    const uint8_t* const src = p.src[pl];
    const int64_t stride = p.src_stride[pl];
    const bool vec = p.vec_src[pl] != 0 && full && !odd0;
    const int yb = p.y0 + (int)blockIdx.y * kUpBand, ye = min(p.y0 + p.h, yb + kUpBand);
    uint8_t* const dcol = p.dst[pl] + t0 * (int64_t)sizeof(T);

    // the lane's horizontal sums of chroma row jr (any integer: clamped)
    auto hrow = [&](int jr, uint32_t (&h)[N]) {
        jr = min(max(jr, rlo), rhi);
        const T* const row = reinterpret_cast<const T*>(src + (int64_t)(jr - p.wy0) * stride);
        auto at = [&](int i) -> uint32_t { return (uint32_t)row[min(max(i, lo), hi) - p.wx0]; };
        uint32_t c[HN + 2];
        if constexpr (TWIN == 1) {
#pragma unroll
            for (int s = 0; s < HN + 2; ++s) c[s] = (uint32_t)(jr + s) + lane;
            if (odd0) up_hsums<N, SITING, true>(c, h); else up_hsums<N, SITING, false>(c, h);
            return;
        }
        if (vec) {
            const up_u2 v = *reinterpret_cast<const up_u2*>(row + (ibase - p.wx0));
#pragma unroll
            for (int s = 0; s < HN; ++s) {
                if constexpr (sizeof(T) == 1) c[1 + s] = (v[s >> 2] >> (8 * (s & 3))) & 0xffu;
                else c[1 + s] = (v[s >> 1] >> (16 * (s & 1))) & 0xffffu;
            }
        } else {
#pragma unroll
            for (int s = 0; s < HN; ++s) c[1 + s] = at(ibase + s);
        }
        if constexpr (TWIN == 2) {
#pragma unroll
            for (int t = 0; t < N; ++t) h[t] = c[1 + (t >> 1)];
            return;
        }
        uint32_t left = (uint32_t)__shfl_up((int)c[HN], 1), right = (uint32_t)__shfl_down((int)c[1], 1);
        if (lane == 0) left = at(ibase - 1);
        if (lane == 63) right = at(ibase + HN);
        c[0] = left; c[HN + 1] = right;
        if (odd0) up_hsums<N, SITING, true>(c, h); else up_hsums<N, SITING, false>(c, h);
    };

    // one output row: (wa a + wb b + 8) >> 4 per sample
    auto emit = [&](int y, const uint32_t (&a)[N], const uint32_t (&b)[N], uint32_t wa, uint32_t wb) {
        uint32_t v[N];
#pragma unroll
        for (int t = 0; t < N; ++t) v[t] = TWIN == 2 ? (a[t] | b[t]) : (wa * a[t] + wb * b[t] + 8u) >> 4;
        uint8_t* const d = dcol + (int64_t)(y - p.y0) * p.dst_stride;
        if (full && p.vec_dst) {
            up_u4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (sizeof(T) == 1) o[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
                else o[k] = v[2 * k] | (v[2 * k + 1] << 16);
            }
            __builtin_nontemporal_store(o, reinterpret_cast<up_u4*>(d));
        } else {
#pragma unroll
            for (int t = 0; t < N; ++t) if (t < nvalid) reinterpret_cast<T*>(d)[t] = (T)v[t];
        }
    };

    uint32_t A[N], B[N];
    if (YS) {
        // rows (q, q + 1) give y = 2 q + 1 (3 A + B) and y = 2 q + 2 (A + 3 B): every chroma row of the band is loaded once
        const int qlo = (yb - 1) >> 1, qhi = (ye - 2) >> 1;
        hrow(qlo, A);
        for (int q = qlo; q <= qhi; ++q) {
            hrow(q + 1, B);
            const int y1 = 2 * q + 1, y2 = y1 + 1;
            if (y1 >= yb && y1 < ye) emit(y1, A, B, 3u, 1u);
            if (y2 >= yb && y2 < ye) emit(y2, A, B, 1u, 3u);
#pragma unroll
            for (int t = 0; t < N; ++t) A[t] = B[t];
        }
    } else {
        for (int y = yb; y < ye; ++y) {
            hrow(y, A);
            emit(y, A, A, 4u, 0u);
        }
    }
}

// Enqueue the upsample of both chroma planes.  win[i] / win_stride[i] / (wx0, wy0): the resident window; it must hold what
// up_need(cw, ch, ys, x0, y0, w, h) names (upsample_window.h).
hipError_t launch_upsample(int ssz, int ys, int siting, const uint8_t* const win[2], const int64_t win_stride[2], int wx0, int wy0, int cw, int ch,
                           int x0, int y0, int w, int h, uint8_t* const dst[2], int64_t dst_stride, hipStream_t st, int twin = 0)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    UpsampleParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < 2; ++i) {
        p.src[i] = win[i]; p.src_stride[i] = win_stride[i]; p.dst[i] = dst[i];
        const uintptr_t first = reinterpret_cast<uintptr_t>(win[i]) + (uintptr_t)((int64_t)((x0 >> 1) - wx0) * ssz);
        p.vec_src[i] = (x0 & 1) == 0 && (first & 7) == 0 && (win_stride[i] & 7) == 0;
    }
    p.dst_stride = dst_stride;
    p.vec_dst = ((reinterpret_cast<uintptr_t>(dst[0]) | reinterpret_cast<uintptr_t>(dst[1]) | (uintptr_t)dst_stride) & 15) == 0;
    p.wx0 = wx0; p.wy0 = wy0; p.cw = cw; p.ch = ch; p.x0 = x0; p.y0 = y0; p.w = w; p.h = h;
    const int64_t spans = ((int64_t)w * ssz + 1023) / 1024;
    const int64_t bands = ((int64_t)h + kUpBand - 1) / kUpBand;
    if (bands > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((spans + 3) / 4), (unsigned)bands, 2), block(kUpThreads);
    // [bytes per sample - 1][ys][siting - 1], and the CENTER kernel's attribution twins [..][..][twin - 1]
    typedef void (*Kernel)(const UpsampleParams);
    static const Kernel kKernels[2][2][2] = {
        { { chroma_upsample<uint8_t, 0, 1>, chroma_upsample<uint8_t, 0, 2> }, { chroma_upsample<uint8_t, 1, 1>, chroma_upsample<uint8_t, 1, 2> } },
        { { chroma_upsample<uint16_t, 0, 1>, chroma_upsample<uint16_t, 0, 2> }, { chroma_upsample<uint16_t, 1, 1>, chroma_upsample<uint16_t, 1, 2> } } };
    static const Kernel kTwins[2][2][2] = {
        { { chroma_upsample<uint8_t, 0, 1, 1>, chroma_upsample<uint8_t, 0, 1, 2> }, { chroma_upsample<uint8_t, 1, 1, 1>, chroma_upsample<uint8_t, 1, 1, 2> } },
        { { chroma_upsample<uint16_t, 0, 1, 1>, chroma_upsample<uint16_t, 0, 1, 2> }, { chroma_upsample<uint16_t, 1, 1, 1>, chroma_upsample<uint16_t, 1, 1, 2> } } };
    static_assert(AVIFGPU_UPSAMPLE_BILINEAR_CENTER == 1 && AVIFGPU_UPSAMPLE_BILINEAR_LEFT == 2, "the tables are indexed by siting - 1");
    const Kernel kernel = twin ? kTwins[ssz - 1][ys ? 1 : 0][twin - 1] : kKernels[ssz - 1][ys ? 1 : 0][siting - 1];
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p);
    return hipGetLastError();
}

// ---- the source region of output rows [orow0, orow0 + onrows): the oriented open's OpenRegion (open_geometry.h), and what is sized by it ----
struct Plan : OpenRegion {
    int ssz;
    int64_t up_pitch;        // bytes of a scratch row of U
    int64_t orient_bytes;    // the oriented 4:4:4 open's own scratch (0 for code 1)
};

// the call is one of the existing entry points: nothing to interpolate
bool degenerate(const avifgpu_read_desc* d, const ReadGeom& g, int upsampling)
{
    return upsampling == AVIFGPU_UPSAMPLE_NEAREST || d->colorspace != AVIFGPU_COLORSPACE_YCBCR || g.xs == 0;
}

int plan_of(const avifgpu_read_desc* d, const ReadGeom& g, int code, int orow0, int onrows, Plan& r)
{
    if (!region_of(d, g, code, orow0, onrows, r))
        return fail(AVIFGPU_formatBadParameters, "upsampled rows [%d, %d + %d) outside the %d rows of the image", orow0, orow0, onrows, r.out_h);
    r.ssz = d->bit_depth > 8 ? 2 : 1;
    r.up_pitch = align256((int64_t)r.sub_w * r.ssz);
    r.orient_bytes = code == 1 ? 0 : align256((int64_t)r.sub_w * r.bpp) * r.sub_h;
    return 0;
}

int64_t scratch_need(const Plan& r) { return 2 * r.up_pitch * r.sub_h + r.orient_bytes; }

// The upsampled open of one region on device pointers: upsample, the existing 4:4:4 open on (Y, U(Cb), U(Cr), A) with a copy of the
// descriptor, and for codes 2-8 the existing orient kernels behind it -- all enqueued on st.  y / a: the region's first sample.
int open_region_device(const avifgpu_read_desc* d, const ReadGeom& g, int upsampling, int code, const Plan& r, int onrows,
                       const uint8_t* y, int64_t y_stride, const uint8_t* a, int64_t a_stride,
                       const uint8_t* const win[2], const int64_t win_stride[2], int wx0, int wy0,
                       void* dst, int64_t dst_row_bytes, uint8_t* scratch, hipStream_t st)
{
    uint8_t* const up[2] = { scratch, scratch + r.up_pitch * r.sub_h };
    const int cw = (d->width + g.xs) >> g.xs, ch = (d->height + g.ys) >> g.ys;
    const hipError_t e = launch_upsample(r.ssz, g.ys, upsampling, win, win_stride, wx0, wy0, cw, ch, r.x0, r.y0, r.sub_w, r.sub_h, up, r.up_pitch, st);
    if (e != hipSuccess) return hip_fail(e, "chroma_upsample launch", AVIFGPU_readErr);
    avifgpu_read_desc sub = *d;
    sub.chroma = AVIFGPU_CHROMA_444; sub.width = r.sub_w; sub.height = r.sub_h;
    const void* const planes[4] = { y, up[0], up[1], g.alpha ? a : nullptr };
    const int64_t strides[4] = { y_stride, r.up_pitch, r.up_pitch, g.alpha ? a_stride : 0 };
    if (code == 1) return avifgpu_read_rows(&sub, 0, sub.height, planes, strides, dst, dst_row_bytes, AVIFGPU_MEM_DEVICE, st);
    return avifgpu_read_rows_oriented(&sub, code, 0, onrows, planes, strides, dst, dst_row_bytes, scratch + 2 * r.up_pitch * r.sub_h, r.orient_bytes,
                                      AVIFGPU_MEM_DEVICE, st);
}

// ---- host path: the staged driver (staged_open.cpp).  Y and A: the region.  Chroma: the window stage_window() names (upsample_window.h),
// the region's samples plus the halo, in the place of the plane ------------------------------------------------------------------------
constexpr size_t kHostTileBytes = (size_t)32 << 20;             // output bytes of one staged tile, as the oriented open's

int read_rows_upsampled_host(const avifgpu_read_desc* d, const ReadGeom& g, int upsampling, int code, int orow0, int onrows,
                             const void* const src[4], const int64_t src_stride[4], uint8_t* dst, int64_t dst_row_bytes)
{
    Plan whole, r;
    plan_of(d, g, code, 0, 0, whole);
    const int cw = (d->width + g.xs) >> g.xs, ch = (d->height + g.ys) >> g.ys;
    const int64_t out_pitch = align256((int64_t)whole.out_w * whole.bpp);
    UpStage sw;
    const StagedPlan plan = [&](int o0, int left, int max_rows, StagedTile& t) {
        t.n = avifgpu_read_oriented_next_tile(d, code, o0, std::min(max_rows, left));
        if (t.n <= 0) return t.n;                              // 0: the driver's "empty tile"
        const int err = plan_of(d, g, code, o0, t.n, r);
        if (err) return err;
        for (int pl = 0; pl < 4; pl += 3) {
            if (pl == 3 && !g.alpha) continue;
            const uint8_t* const h = static_cast<const uint8_t*>(src[pl]) + (int64_t)r.y0 * src_stride[pl] + (int64_t)r.x0 * r.ssz;
            t.up[pl] = { h, src_stride[pl], (int64_t)r.sub_w * r.ssz, r.sub_h, r.up_pitch };
        }
        sw = stage_window(cw, ch, g.ys, r.ssz, r.x0, r.y0, r.sub_w, r.sub_h);
        for (int pl = 1; pl <= 2; ++pl)
            t.up[pl] = { static_cast<const uint8_t*>(src[pl]) + stage_host_offset(sw, src_stride[pl], r.ssz), src_stride[pl], sw.row_bytes, sw.rows, sw.pitch };
        t.out_pitch = out_pitch;
        t.scratch_bytes = scratch_need(r);
        return 0;
    };
    const StagedEnqueue enqueue = [&](const StagedBuffers& b) {
        const uint8_t* const win[2] = { static_cast<const uint8_t*>(b.plane[1]), static_cast<const uint8_t*>(b.plane[2]) };
        return open_region_device(d, g, upsampling, code, r, r.o.t ? r.sub_w : r.sub_h, static_cast<const uint8_t*>(b.plane[0]), b.pitch[0],
                                  static_cast<const uint8_t*>(b.plane[3]), b.pitch[3], win, b.pitch + 1, sw.need.lo, sw.need.rlo,
                                  b.out, out_pitch, static_cast<uint8_t*>(b.scratch), b.stream);
    };
    return staged_open("upsampled open", kHostTileBytes, (int64_t)whole.out_w * whole.bpp, orow0, onrows, dst, dst_row_bytes, plan, enqueue);
}

int check_upsampled(const avifgpu_read_desc* d, int upsampling, int code, ReadGeom& g, const char* who)
{
    if (!upsampling_ok(upsampling)) return fail(AVIFGPU_formatBadParameters, "%s: chroma upsampling %d is not an AVIFGPU_UPSAMPLE_* value", who, upsampling);
    if (!open_code_ok(code)) return fail(AVIFGPU_formatBadParameters, "%s: orientation %d is not an EXIF code 1..8", who, code);
    return check_read(d, 0, 0, g);
}

} // namespace

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int64_t avifgpu_read_upsampled_scratch_bytes(const avifgpu_read_desc* desc, int32_t upsampling, int32_t orientation, int32_t onrows)
{
    set_error("");
    ReadGeom g;
    const int err = check_upsampled(desc, upsampling, orientation, g, "avifgpu_read_upsampled_scratch_bytes");
    if (err) return err;
    Plan r;
    if (plan_of(desc, g, orientation, 0, onrows, r)) return AVIFGPU_formatBadParameters;
    if (degenerate(desc, g, upsampling)) return 0;
    return scratch_need(r);
}

int32_t avifgpu_read_rows_upsampled(const avifgpu_read_desc* desc, int32_t upsampling, int32_t orientation, int32_t orow0, int32_t onrows,
                                    const void* const src[4], const int64_t src_stride[4], void* dst, int64_t dst_row_bytes,
                                    void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream)
{
    set_error("");
    ReadGeom g;
    int err = check_upsampled(desc, upsampling, orientation, g, "avifgpu_read_rows_upsampled");
    if (err) return err;
    if (degenerate(desc, g, upsampling))                       // today's entry points, byte for byte
        return avifgpu_read_rows_oriented(desc, orientation, orow0, onrows, src, src_stride, dst, dst_row_bytes, scratch, scratch_bytes, mem_kind, stream);
    Plan r;
    if ((err = plan_of(desc, g, orientation, orow0, onrows, r))) return err;
    const OpenEntry entry = { "avifgpu_read_rows_upsampled", "avifgpu_read_upsampled_scratch_bytes", desc, &g, r.out_w, r.bpp, onrows,
                              src, src_stride, dst, dst_row_bytes, scratch, scratch_bytes, mem_kind };
    err = check_open_entry(entry, scratch_need(r), [&](int step) {
        if (step == 0 && !legal_cut(r, onrows))
            return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_upsampled: output rows [%d, %d) start at odd source %s %d of a subsampled direction (cut with avifgpu_read_oriented_next_tile)",
                        orow0, orow0 + onrows, r.o.t ? "column" : "row", r.start);
        if (step == 1 && ((int64_t)r.sub_h + kUpBand - 1) / kUpBand > 65535) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_upsampled: a region of %d rows (cut it)", r.sub_h);
        return 0;
    });
    if (err) return err == kOpenEntryOver ? 0 : err;

    if (mem_kind == AVIFGPU_MEM_HOST)
        return read_rows_upsampled_host(desc, g, upsampling, orientation, orow0, onrows, src, src_stride, static_cast<uint8_t*>(dst), dst_row_bytes);
    const uint8_t* const win[2] = { static_cast<const uint8_t*>(src[1]), static_cast<const uint8_t*>(src[2]) };
    const int64_t win_stride[2] = { src_stride[1], src_stride[2] };
    const int64_t yoff = (int64_t)r.y0 * src_stride[0] + (int64_t)r.x0 * r.ssz;
    const int64_t aoff = g.alpha ? (int64_t)r.y0 * src_stride[3] + (int64_t)r.x0 * r.ssz : 0;
    return open_region_device(desc, g, upsampling, orientation, r, onrows, static_cast<const uint8_t*>(src[0]) + yoff, src_stride[0],
                              g.alpha ? static_cast<const uint8_t*>(src[3]) + aoff : nullptr, g.alpha ? src_stride[3] : 0,
                              win, win_stride, 0, 0, dst, dst_row_bytes, static_cast<uint8_t*>(scratch), (hipStream_t)stream);
}

int32_t avifgpu_probe_upsample(int32_t bytes_per_sample, int32_t chroma, int32_t upsampling, int32_t width, int32_t height,
                               int32_t x0, int32_t y0, int32_t w, int32_t h, const void* const src[2], const int64_t src_stride[2],
                               void* const dst[2], int64_t dst_row_bytes, int32_t twin, void* stream)
{
    set_error("");
    if (bytes_per_sample != 1 && bytes_per_sample != 2) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: %d bytes per sample", bytes_per_sample);
    if (chroma != AVIFGPU_CHROMA_420 && chroma != AVIFGPU_CHROMA_422) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: chroma %d is not 4:2:0 / 4:2:2", chroma);
    if (upsampling != AVIFGPU_UPSAMPLE_BILINEAR_CENTER && upsampling != AVIFGPU_UPSAMPLE_BILINEAR_LEFT)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: upsampling %d is not a bilinear mode", upsampling);
    if (width < 1 || height < 1 || x0 < 0 || y0 < 0 || w < 1 || h < 1 || (int64_t)x0 + w > width || (int64_t)y0 + h > height)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: bad size or rectangle");
    if (!src || !src_stride || !dst || !src[0] || !src[1] || !dst[0] || !dst[1]) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: null buffer");
    const int ys = chroma == AVIFGPU_CHROMA_420 ? 1 : 0;
    const int cw = (width + 1) >> 1, ch = (height + ys) >> ys;
    if (src_stride[0] < (int64_t)cw * bytes_per_sample || src_stride[1] < (int64_t)cw * bytes_per_sample || dst_row_bytes < (int64_t)w * bytes_per_sample)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: row bytes too small");
    if (((int64_t)h + kUpBand - 1) / kUpBand > 65535) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: %d rows", h);
    if (twin < 0 || twin > 2 || (twin && upsampling != AVIFGPU_UPSAMPLE_BILINEAR_CENTER)) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_upsample: twin %d (0, or 1 / 2 with the CENTER mode)", twin);
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    const uint8_t* const win[2] = { static_cast<const uint8_t*>(src[0]), static_cast<const uint8_t*>(src[1]) };
    uint8_t* const out[2] = { static_cast<uint8_t*>(dst[0]), static_cast<uint8_t*>(dst[1]) };
    const hipError_t e = launch_upsample(bytes_per_sample, ys, upsampling, win, src_stride, 0, 0, cw, ch, x0, y0, w, h, out, dst_row_bytes, (hipStream_t)stream, twin);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_upsample", AVIFGPU_readErr);
}

} // extern "C"
