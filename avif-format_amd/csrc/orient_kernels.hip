// orient_kernels.hip -- irot / imir orientation of an open, applied on the GPU (include/avifgpu.h "oriented open").
//
// The decode arithmetic is not copied.  Output rows [orow0, orow0 + onrows) of the oriented image correspond to a source REGION -- a row
// range for EXIF codes 1-4, a column band for codes 5-8 -- which the existing read kernels decode as a sub-image (the same descriptor with
// the region's size, plane pointers advanced, the same strides) into scratch; one of the two kernels below then MOVES whole host pixels
// from scratch to dst.  They know nothing of colour: a pixel is BPP bytes, BPP in {1, 2, 3, 4, 6, 8, 12, 16} (gray / gray+A / RGB / RGBA at
// 8 / 16 / 32 bit).  A translation unit -- and so a code object -- of its own: a process that never opens an oriented image never loads it.
// The code table and the region are open_geometry.h's; the entry's shared argument checks and the host-pointer path (tiles through two
// staging slots) are staged_open.cpp's, which this file gives its cut rule, what goes up for a tile and what is enqueued.
//
// Every code is (transpose, flip x, flip y) of the SOURCE coordinate:
//   row-mapped  (codes 2, 3, 4)   dst(y', x') = src(fy ? R - 1 - y' : y',  fx ? W - 1 - x' : x')
//   transposing (codes 5 .. 8)    dst(y', x') = src(fy ? H - 1 - x' : x',  fx ? W - 1 - y' : y')
//
// orient_rows<BPP>.  A wave owns a span of one destination row: 64 lanes x 16 bytes (x 3 for 3-, 6- and 12-byte pixels, so that a span is a
// whole number of pixels).  Pixel sizes that divide 16 reverse in registers: destination chunk k of a row of N chunks is source chunk
// N - 1 - k with its pixels swapped end for end.  The other three go through the wave's LDS strip: the span is written as it was loaded
// and read back unit by unit (1, 2 or 4 bytes: the largest power of two that divides the pixel) from the mirrored pixel.  The ragged
// last span of a row takes the strip too, chunk by chunk in a loop.
//
// orient_transpose<BPP>.  A workgroup of 256 lanes owns a square tile of T x T pixels of the DESTINATION (T = 64 up to 4-byte pixels, 32
// above: a tile row is a multiple of 16 bytes either way), reads the matching source tile row-wise with 16-byte loads into an LDS image of
// whole pixels whose pitch is the tile row + one dword, and writes destination rows of 16 bytes per lane, 8 (4) consecutive lanes on 128
// (64) consecutive bytes, gathering each lane's 16 bytes unit by unit from one LDS column.  Tiles are anchored on the destination so
// that its stores are always aligned.  With a flipped x the source chunks of both kernels sit ws * BPP % 16 bytes off the 16-byte grid
// (the width of a column band is whatever the caller's tile is): they are loaded as 16 bytes at any address, so whole tiles and spans
// stay on these paths for every width.  Only a ragged tile or span at the edge and unaligned bases or strides take the per-pixel path:
// plain byte copies, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "staging.h"

namespace avifgpu {

namespace {

typedef uint32_t or_u4 __attribute__((ext_vector_type(4)));
typedef or_u4 or_u4_any __attribute__((aligned(1)));            // 16 bytes at any address: a flipped x puts the source chunk wherever the row's length puts it

__device__ __forceinline__ or_u4 or_load16_any(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const or_u4_any*>(p)); }

struct OrientParams {
    const uint8_t* src; int64_t src_stride;      // the decoded sub-image: ws x hs pixels
    uint8_t* dst; int64_t dst_stride;            // row-mapped: ws x hs; transposing: hs x ws
    int32_t ws, hs;
    int32_t fx, fy;                              // source x / y runs backwards
    int32_t fast;                                // bases and strides are multiples of 16
};

constexpr int kOrientThreads = 256;

template <int BPP> struct PixelUnit { static constexpr int U = (BPP % 4 == 0) ? 4 : ((BPP % 2 == 0) ? 2 : 1); };

template <int BPP> __device__ __forceinline__ void or_copy_pixel(uint8_t* d, const uint8_t* s)
{
#pragma unroll
    for (int b = 0; b < BPP; ++b) d[b] = s[b];
}

// the pixels of a 16-byte chunk end for end (BPP divides 16)
template <int BPP> __device__ __forceinline__ or_u4 or_reverse16(const or_u4 v)
{
    if constexpr (BPP == 16) return v;
    else if constexpr (BPP == 8) { or_u4 r; r[0] = v[2]; r[1] = v[3]; r[2] = v[0]; r[3] = v[1]; return r; }
    else {
        or_u4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w = v[3 - i];
            if constexpr (BPP == 4) r[i] = w;
            else if constexpr (BPP == 2) r[i] = (w >> 16) | (w << 16);
            else r[i] = __builtin_bswap32(w);
        }
        return r;
    }
}

// unit `u` (U bytes, at byte offset u * U) of an LDS image, into byte position (i * U) of a 16-byte chunk held as four dwords
template <int U> __device__ __forceinline__ void or_put_unit(uint32_t (&out)[4], int i, const uint8_t* lds, uint32_t byte_off)
{
    if constexpr (U == 4) out[i] = *reinterpret_cast<const uint32_t*>(lds + byte_off);
    else if constexpr (U == 2) out[i >> 1] |= (uint32_t)*reinterpret_cast<const uint16_t*>(lds + byte_off) << (16 * (i & 1));
    else out[i >> 2] |= (uint32_t)lds[byte_off] << (8 * (i & 3));
}

template <int BPP>
__global__ __launch_bounds__(kOrientThreads) void orient_rows(const OrientParams p)
{
    constexpr bool REG = (16 % BPP) == 0;
    constexpr int K = REG ? 1 : 3;                             // 16-byte chunks of a lane
    constexpr int SPANB = 64 * 16 * K, SPANPX = SPANB / BPP;   // a wave's span
    constexpr int U = PixelUnit<BPP>::U, CP = BPP / U;         // unit bytes, units of a pixel
    __shared__ or_u4 s_strip[REG ? 1 : (kOrientThreads / 64) * 64 * K];

    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const int64_t span = (int64_t)blockIdx.x * (kOrientThreads / 64) + wave;
    const int64_t rb = (int64_t)p.ws * BPP;
    const int64_t px0 = span * SPANPX;
    const bool in = px0 < p.ws;
    const int npx = in ? (int)min((int64_t)SPANPX, (int64_t)p.ws - px0) : 0;

    for (int row = (int)blockIdx.y; row < p.hs; row += (int)gridDim.y) {
        const uint8_t* const sp = p.src + (int64_t)(p.fy ? p.hs - 1 - row : row) * p.src_stride;
        uint8_t* const dp = p.dst + (int64_t)row * p.dst_stride;
        if (p.fast && !p.fx) {                                 // rows move, pixels stay: 16-byte chunks, the row's last bytes one by one
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int64_t off = span * SPANB + (int64_t)(j * 64 + (int)lane) * 16;
                if (off + 16 <= rb) {
                    const or_u4 v = __builtin_nontemporal_load(reinterpret_cast<const or_u4*>(sp + off));
                    __builtin_nontemporal_store(v, reinterpret_cast<or_u4*>(dp + off));
                } else if (off < rb) {
                    for (int64_t b = off; b < rb; ++b) dp[b] = sp[b];
                }
            }
        } else if (p.fast && REG) {                            // reversed in registers; the source chunk sits rb % 16 bytes off the 16-byte grid
            const int64_t nc = rb >> 4, kc = span * 64 + lane;
            if (kc < nc) {
                const or_u4 v = or_load16_any(sp + (rb - (kc + 1) * 16));
                __builtin_nontemporal_store(or_reverse16<BPP>(v), reinterpret_cast<or_u4*>(dp + kc * 16));
            } else if (kc == nc) {                             // the row's last rb % 16 bytes: the source row's first pixels
                const int tail = (int)(rb & 15) / BPP;
                for (int i = 0; i < tail; ++i) or_copy_pixel<BPP>(dp + nc * 16 + i * BPP, sp + (tail - 1 - i) * BPP);
            }
        } else if (p.fast) {                                   // reversed through the wave's LDS strip; the source span sits anywhere
            if constexpr (!REG) {
                // a whole span: SPANB source bytes from rb - (span + 1) * SPANB, everything a compile-time constant.  The ragged last span
                // of a row (nb < SPANB bytes: the source row's FIRST nb bytes) takes the same way chunk by chunk in a loop, its last,
                // partial chunk byte by byte -- it is up to an eighth of a row, too much for a byte loop from global memory
                const bool full = npx == SPANPX;
                or_u4* const strip = s_strip + wave * 64 * K;
                uint8_t* const lds = reinterpret_cast<uint8_t*>(strip);
                const int nb = npx * BPP;
                if (full) {
                    const uint8_t* const s0 = sp + (rb - (span + 1) * SPANB);
#pragma unroll
                    for (int j = 0; j < K; ++j) strip[j * 64 + lane] = or_load16_any(s0 + (j * 64 + (int)lane) * 16);
                } else {
#pragma unroll 1
                    for (int c = (int)lane; c * 16 < nb; c += 64) {
                        if (c * 16 + 16 <= nb) strip[c] = or_load16_any(sp + c * 16);
                        else for (int b = c * 16; b < nb; ++b) lds[b] = sp[b];
                    }
                }
                __syncthreads();
                if (full) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const uint32_t c = (uint32_t)j * 64u + lane;
                        uint32_t out[4] = { 0, 0, 0, 0 };
#pragma unroll
                        for (int i = 0; i < 16 / U; ++i) {
                            const uint32_t unit = c * (16 / U) + (uint32_t)i;
                            const uint32_t px = unit / CP, comp = unit - px * CP;
                            or_put_unit<U>(out, i, lds, ((uint32_t)(SPANPX - 1) - px) * BPP + comp * U);
                        }
                        or_u4 v; v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3];
                        __builtin_nontemporal_store(v, reinterpret_cast<or_u4*>(dp + span * SPANB + (int64_t)c * 16));
                    }
                } else {
#pragma unroll 1
                    for (int c = (int)lane; c * 16 < nb; c += 64) {
                        if (c * 16 + 16 <= nb) {
                            uint32_t out[4] = { 0, 0, 0, 0 };
#pragma unroll
                            for (int i = 0; i < 16 / U; ++i) {
                                const uint32_t unit = (uint32_t)c * (16 / U) + (uint32_t)i;
                                const uint32_t px = unit / CP, comp = unit - px * CP;
                                or_put_unit<U>(out, i, lds, ((uint32_t)(npx - 1) - px) * BPP + comp * U);
                            }
                            or_u4 v; v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3];
                            __builtin_nontemporal_store(v, reinterpret_cast<or_u4*>(dp + span * SPANB + (int64_t)c * 16));
                        } else {
                            for (int b = c * 16; b < nb; ++b) {
                                const int px = b / BPP;
                                dp[span * SPANB + b] = lds[(npx - 1 - px) * BPP + (b - px * BPP)];
                            }
                        }
                    }
                }
                __syncthreads();                               // the strip is rewritten for the next row
            }
        } else {                                               // any base, any stride: pixel by pixel
            for (int k = (int)lane; k < npx; k += 64) {
                const int64_t x = px0 + k;
                or_copy_pixel<BPP>(dp + x * BPP, sp + (p.fx ? (int64_t)p.ws - 1 - x : x) * BPP);
            }
        }
    }
}

template <int BPP>
__global__ __launch_bounds__(kOrientThreads) void orient_transpose(const OrientParams p)
{
    constexpr int T = BPP <= 4 ? 64 : 32;                      // tile side in pixels
    constexpr int TRB = T * BPP, CH = TRB / 16;                // bytes / 16-byte chunks of a tile row
    constexpr int PITCH = TRB + 4;                             // LDS pitch: one dword of padding
    constexpr int U = PixelUnit<BPP>::U, CP = BPP / U;
    constexpr int J = (CH % 8 == 0) ? 8 : 4;                   // consecutive lanes on one destination row
    __shared__ uint32_t s_tile[T * PITCH / 4];

    const uint32_t tid = threadIdx.x;
    const int dw = p.hs, dh = p.ws;                            // the destination's size
    const int dx0 = (int)blockIdx.x * T;
    for (int dy0 = (int)blockIdx.y * T; dy0 < dh; dy0 += (int)gridDim.y * T) {
        const int tw = min(T, dw - dx0), th = min(T, dh - dy0);
        const int sy0 = p.fy ? p.hs - dx0 - tw : dx0;          // the source tile: tw rows from sy0, th columns from sx0
        const int sx0 = p.fx ? p.ws - dy0 - th : dy0;
        const bool whole = p.fast && tw == T && th == T;       // uniform over the workgroup
        if (whole) {
            const uint8_t* const s0 = p.src + (int64_t)sy0 * p.src_stride + (int64_t)sx0 * BPP;
            for (uint32_t idx = tid; idx < (uint32_t)(T * CH); idx += kOrientThreads) {
                const uint32_t r = idx / CH, c = idx - r * CH;
                const or_u4 v = or_load16_any(s0 + (int64_t)r * p.src_stride + c * 16);      // with fx, sx0 * BPP is off the 16-byte grid by ws * BPP % 16
                uint32_t* const w = s_tile + (r * PITCH + c * 16) / 4;
                w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
            }
            __syncthreads();
            const uint8_t* const lds = reinterpret_cast<const uint8_t*>(s_tile);
            uint8_t* const d0 = p.dst + (int64_t)dy0 * p.dst_stride + (int64_t)dx0 * BPP;
            for (uint32_t idx = tid; idx < (uint32_t)(T * CH); idx += kOrientThreads) {
                const uint32_t j = idx % J, t = idx / J;
                const uint32_t yy = t % T, g = t / T;                              // destination row of the tile, group of J chunks (CH / J of them)
                const uint32_t c = g * J + j;
                const uint32_t lc = p.fx ? (uint32_t)(T - 1) - yy : yy;            // LDS column = source x
                uint32_t out[4] = { 0, 0, 0, 0 };
#pragma unroll
                for (int i = 0; i < 16 / U; ++i) {
                    const uint32_t unit = c * (16 / U) + (uint32_t)i;
                    const uint32_t xx = unit / CP, comp = unit - xx * CP;          // destination pixel of the tile row
                    const uint32_t lr = p.fy ? (uint32_t)(T - 1) - xx : xx;        // LDS row = source y
                    or_put_unit<U>(out, i, lds, lr * PITCH + lc * BPP + comp * U);
                }
                or_u4 v; v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3];
                __builtin_nontemporal_store(v, reinterpret_cast<or_u4*>(d0 + (int64_t)yy * p.dst_stride + c * 16));
            }
            __syncthreads();                                   // the tile is rewritten for the next dy0
        } else {
            for (int k = (int)tid; k < tw * th; k += kOrientThreads) {
                const int yy = k / tw, xx = k - yy * tw;
                const int x = dx0 + xx, y = dy0 + yy;          // destination pixel
                const int sy = p.fy ? p.hs - 1 - x : x, sx = p.fx ? p.ws - 1 - y : y;
                or_copy_pixel<BPP>(p.dst + (int64_t)y * p.dst_stride + (int64_t)x * BPP, p.src + (int64_t)sy * p.src_stride + (int64_t)sx * BPP);
            }
        }
    }
}

hipError_t launch_orient(int code, int bpp, const uint8_t* src, int64_t src_stride, int ws, int hs, uint8_t* dst, int64_t dst_stride, hipStream_t st)
{
    if (ws <= 0 || hs <= 0) return hipSuccess;
    const OpenTurn o = kOpenTurn[code];
    OrientParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.src_stride = src_stride; p.dst = dst; p.dst_stride = dst_stride; p.ws = ws; p.hs = hs; p.fx = o.fx; p.fy = o.fy;
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)src_stride | (uintptr_t)dst_stride) & 15) == 0;
    const dim3 block(kOrientThreads);
    if (!o.t) {
        p.fast = aligned;
        const int spanb = (16 % bpp) == 0 ? 1024 : 3072;
        const int64_t spans = ((int64_t)ws * bpp + spanb - 1) / spanb;
        const dim3 grid((unsigned)((spans + 3) / 4), (unsigned)std::min(hs, 65535));
#define AG_ORIENT_ROWS(B_) case B_: hipLaunchKernelGGL((orient_rows<B_>), grid, block, 0, st, p); break
        switch (bpp) {
            AG_ORIENT_ROWS(1); AG_ORIENT_ROWS(2); AG_ORIENT_ROWS(3); AG_ORIENT_ROWS(4); AG_ORIENT_ROWS(6); AG_ORIENT_ROWS(8); AG_ORIENT_ROWS(12); AG_ORIENT_ROWS(16);
            default: return hipErrorInvalidValue;
        }
#undef AG_ORIENT_ROWS
    } else {
        p.fast = aligned;
        const int T = bpp <= 4 ? 64 : 32;
        const dim3 grid((unsigned)((hs + T - 1) / T), (unsigned)std::min((ws + T - 1) / T, 65535));
#define AG_ORIENT_TR(B_) case B_: hipLaunchKernelGGL((orient_transpose<B_>), grid, block, 0, st, p); break
        switch (bpp) {
            AG_ORIENT_TR(1); AG_ORIENT_TR(2); AG_ORIENT_TR(3); AG_ORIENT_TR(4); AG_ORIENT_TR(6); AG_ORIENT_TR(8); AG_ORIENT_TR(12); AG_ORIENT_TR(16);
            default: return hipErrorInvalidValue;
        }
#undef AG_ORIENT_TR
    }
    return hipGetLastError();
}

// ---- the source region of output rows [orow0, orow0 + onrows): OpenRegion (open_geometry.h) -------------------------------------------
int oriented_region(const avifgpu_read_desc* d, const ReadGeom& g, int code, int orow0, int onrows, OpenRegion& r)
{
    if (region_of(d, g, code, orow0, onrows, r)) return 0;
    return fail(AVIFGPU_formatBadParameters, "oriented rows [%d, %d + %d) outside the %d rows of the image", orow0, orow0, onrows, r.out_h);
}

// The oriented open's cut rule.  NOT crop_next_tile (crop_geometry.h): behind a caller's own odd start of an unflipped subsampled direction
// this one answers 1, that one the n that makes the next start even.  Both are public behaviour.
int next_tile(const OpenRegion& whole, int orow0, int max_rows)
{
    const int rest = whole.out_h - orow0;
    int n = std::min(max_rows, rest);
    if (!whole.subsampled || n <= 1) return n;
    if (whole.flipped) {
        if ((whole.out_h - orow0 - n) & 1) --n;                 // n == rest starts at 0
        return n;
    }
    if (orow0 & 1) return 1;                                    // only reached behind a caller's own odd cut
    if (n < rest && (n & 1)) --n;                               // leave the next tile an even start
    return n;
}

// descriptor and plane pointers of the region's sub-image
void sub_image(const avifgpu_read_desc* d, const ReadGeom& g, const OpenRegion& r, const void* const src[4], const int64_t src_stride[4],
               avifgpu_read_desc& sub, const void* out[4])
{
    sub = *d;
    sub.width = r.sub_w; sub.height = r.sub_h;
    const int ssz = d->bit_depth > 8 ? 2 : 1;
    for (int pl = 0; pl < 4; ++pl) {
        out[pl] = nullptr;
        if (!read_plane_used(d, g, pl) || !src[pl]) continue;
        const bool chroma = plane_is_chroma(d, pl);
        const int64_t off = r.o.t ? (int64_t)(r.start >> (chroma ? g.xs : 0)) * ssz : (int64_t)(r.start >> (chroma ? g.ys : 0)) * src_stride[pl];
        out[pl] = static_cast<const uint8_t*>(src[pl]) + off;
    }
}

int64_t scratch_pitch(const OpenRegion& r) { return align256((int64_t)r.sub_w * r.bpp); }

// ---- host path: the staged driver (staged_open.cpp) with what goes up for a tile -- the region's part of every plane -- and what runs ---
constexpr size_t kHostTileBytes = (size_t)32 << 20;             // output bytes of one staged tile

int read_rows_oriented_host(const avifgpu_read_desc* d, const ReadGeom& g, int code, int orow0, int onrows,
                            const void* const src[4], const int64_t src_stride[4], uint8_t* dst, int64_t dst_row_bytes)
{
    OpenRegion whole, r;
    region_of(d, g, code, 0, 0, whole);
    const int ssz = d->bit_depth > 8 ? 2 : 1;
    avifgpu_read_desc sub;
    const int64_t out_pitch = align256((int64_t)whole.out_w * whole.bpp);
    const StagedPlan plan = [&](int o0, int left, int max_rows, StagedTile& t) {
        t.n = next_tile(whole, o0, std::min(max_rows, left));
        const int err = oriented_region(d, g, code, o0, t.n, r);
        if (err) return err;
        const void* hsrc[4];
        sub_image(d, g, r, src, src_stride, sub, hsrc);
        for (int pl = 0; pl < 4; ++pl) {
            const bool chroma = plane_is_chroma(d, pl);
            const int64_t wbytes = (int64_t)(chroma ? (sub.width + g.xs) >> g.xs : sub.width) * ssz;
            t.up[pl] = { hsrc[pl], src_stride[pl], wbytes, chroma ? (sub.height + g.ys) >> g.ys : sub.height, align256(wbytes) };
        }
        t.out_pitch = out_pitch;
        t.scratch_bytes = scratch_pitch(r) * r.sub_h;
        return 0;
    };
    const StagedEnqueue enqueue = [&](const StagedBuffers& b) {
        const int64_t sp = scratch_pitch(r);
        const int err = avifgpu_read_rows(&sub, 0, sub.height, b.plane, b.pitch, b.scratch, sp, AVIFGPU_MEM_DEVICE, b.stream);
        if (err) return err;
        const hipError_t e = launch_orient(code, r.bpp, static_cast<const uint8_t*>(b.scratch), sp, r.sub_w, r.sub_h, static_cast<uint8_t*>(b.out), out_pitch, b.stream);
        return e == hipSuccess ? 0 : hip_fail(e, "orient kernel launch", AVIFGPU_readErr);
    };
    return staged_open("oriented open", kHostTileBytes, (int64_t)whole.out_w * whole.bpp, orow0, onrows, dst, dst_row_bytes, plan, enqueue);
}

int check_oriented(const avifgpu_read_desc* d, int code, ReadGeom& g, const char* who)
{
    if (!open_code_ok(code)) return fail(AVIFGPU_formatBadParameters, "%s: orientation %d is not an EXIF code 1..8", who, code);
    return check_read(d, 0, 0, g);
}

} // namespace

} // namespace avifgpu

// ======================================================================================================
using namespace avifgpu;

extern "C" {

int32_t avifgpu_orientation_compose(int32_t first, int32_t then)
{
    set_error("");
    if (!open_code_ok(first) || !open_code_ok(then)) return fail(AVIFGPU_formatBadParameters, "avifgpu_orientation_compose: %d, %d: not EXIF codes 1..8", first, then);
    const int label[6] = { 0, 1, 2, 3, 4, 5 };
    int a[6], b[6], c[6], aw, ah, bw, bh, cw, ch;
    apply_code(first, label, 3, 2, a, aw, ah);
    apply_code(then, a, aw, ah, b, bw, bh);
    for (int code = 1; code <= 8; ++code) {
        apply_code(code, label, 3, 2, c, cw, ch);
        if (cw == bw && ch == bh && memcmp(b, c, sizeof(b)) == 0) return code;
    }
    return fail(AVIFGPU_formatBadParameters, "avifgpu_orientation_compose: not closed");      // unreachable: the eight codes are a group
}

int32_t avifgpu_read_oriented_geometry(const avifgpu_read_desc* desc, int32_t orientation, int32_t* out_w, int32_t* out_h)
{
    set_error("");
    ReadGeom g;
    const int err = check_oriented(desc, orientation, g, "avifgpu_read_oriented_geometry");
    if (err) return err;
    if (!out_w || !out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_oriented_geometry: null argument");
    open_view_size(desc->width, desc->height, orientation, *out_w, *out_h);
    return 0;
}

int32_t avifgpu_read_oriented_next_tile(const avifgpu_read_desc* desc, int32_t orientation, int32_t orow0, int32_t max_rows)
{
    set_error("");
    ReadGeom g;
    const int err = check_oriented(desc, orientation, g, "avifgpu_read_oriented_next_tile");
    if (err) return err;
    OpenRegion whole;
    region_of(desc, g, orientation, 0, 0, whole);
    if (orow0 < 0 || orow0 >= whole.out_h) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_oriented_next_tile: row %d outside the %d rows of the image", orow0, whole.out_h);
    if (max_rows < 1) return fail(AVIFGPU_formatBadParameters, "avifgpu_read_oriented_next_tile: max_rows %d < 1", max_rows);
    return next_tile(whole, orow0, max_rows);
}

int64_t avifgpu_read_oriented_scratch_bytes(const avifgpu_read_desc* desc, int32_t orientation, int32_t onrows)
{
    set_error("");
    ReadGeom g;
    const int err = check_oriented(desc, orientation, g, "avifgpu_read_oriented_scratch_bytes");
    if (err) return err;
    OpenRegion r;
    if (oriented_region(desc, g, orientation, 0, onrows, r)) return AVIFGPU_formatBadParameters;
    if (orientation == 1) return 0;
    return scratch_pitch(r) * r.sub_h;
}

int32_t avifgpu_read_rows_oriented(const avifgpu_read_desc* desc, int32_t orientation, int32_t orow0, int32_t onrows,
                                   const void* const src[4], const int64_t src_stride[4], void* dst, int64_t dst_row_bytes,
                                   void* scratch, int64_t scratch_bytes, int32_t mem_kind, void* stream)
{
    set_error("");
    ReadGeom g;
    int err = check_oriented(desc, orientation, g, "avifgpu_read_rows_oriented");
    if (err) return err;
    OpenRegion r;
    if ((err = oriented_region(desc, g, orientation, orow0, onrows, r))) return err;
    const OpenEntry entry = { "avifgpu_read_rows_oriented", "avifgpu_read_oriented_scratch_bytes", desc, &g, r.out_w, r.bpp, onrows,
                              src, src_stride, dst, dst_row_bytes, scratch, scratch_bytes, mem_kind };
    err = check_open_entry(entry, orientation == 1 ? 0 : scratch_pitch(r) * r.sub_h, [&](int step) {
        if (step == 0 && !legal_cut(r, onrows))
            return fail(AVIFGPU_formatBadParameters, "avifgpu_read_rows_oriented: output rows [%d, %d) start at odd source %s %d of a subsampled direction (cut with avifgpu_read_oriented_next_tile)",
                        orow0, orow0 + onrows, r.o.t ? "column" : "row", r.start);
        return 0;
    });
    if (err) return err == kOpenEntryOver ? 0 : err;

    if (mem_kind == AVIFGPU_MEM_HOST) {
        if (orientation == 1) {                                // avifgpu_read_rows: the tile loop of every bound context
            avifgpu_read_desc sub; const void* psrc[4];
            sub_image(desc, g, r, src, src_stride, sub, psrc);
            return avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, dst, dst_row_bytes, AVIFGPU_MEM_HOST, nullptr);
        }
        return read_rows_oriented_host(desc, g, orientation, orow0, onrows, src, src_stride, static_cast<uint8_t*>(dst), dst_row_bytes);
    }
    avifgpu_read_desc sub; const void* psrc[4];
    sub_image(desc, g, r, src, src_stride, sub, psrc);
    if (orientation == 1) return avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, dst, dst_row_bytes, AVIFGPU_MEM_DEVICE, stream);
    const int64_t sp = scratch_pitch(r);
    if ((err = avifgpu_read_rows(&sub, 0, sub.height, psrc, src_stride, scratch, sp, AVIFGPU_MEM_DEVICE, stream))) return err;
    const hipError_t e = launch_orient(orientation, r.bpp, static_cast<const uint8_t*>(scratch), sp, r.sub_w, r.sub_h, static_cast<uint8_t*>(dst), dst_row_bytes, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "orient kernel launch", AVIFGPU_readErr);
}

int32_t avifgpu_probe_orient(int32_t orientation, int32_t bytes_per_pixel, int32_t width, int32_t height, const void* src, int64_t src_row_bytes,
                             void* dst, int64_t dst_row_bytes, void* stream)
{
    set_error("");
    if (orientation < 2 || orientation > 8) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_orient: orientation %d is not 2..8", orientation);
    bool ok = false;
    for (int b : { 1, 2, 3, 4, 6, 8, 12, 16 }) ok = ok || b == bytes_per_pixel;
    if (!ok) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_orient: %d bytes per pixel", bytes_per_pixel);
    if (width < 1 || height < 1 || !src || !dst) return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_orient: bad size or null buffer");
    const int64_t out_w = kOpenTurn[orientation].t ? height : width;
    if (src_row_bytes < (int64_t)width * bytes_per_pixel || dst_row_bytes < out_w * bytes_per_pixel)
        return fail(AVIFGPU_formatBadParameters, "avifgpu_probe_orient: row bytes too small");
    if (context_count() == 0) return fail(AVIFGPU_formatBadParameters, "avifgpu_init has not succeeded: no HIP device bound (no CPU fallback)");
    const hipError_t e = launch_orient(orientation, bytes_per_pixel, static_cast<const uint8_t*>(src), src_row_bytes, width, height, static_cast<uint8_t*>(dst), dst_row_bytes, (hipStream_t)stream);
    return e == hipSuccess ? 0 : hip_fail(e, "avifgpu_probe_orient", AVIFGPU_readErr);
}

} // extern "C"
