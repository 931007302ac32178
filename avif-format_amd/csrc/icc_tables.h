// icc_tables.h -- the parts of the ICC device-table cache (icc_tables.cpp) that make no HIP call: the fingerprint of a caller's table, the
// staleness decision, the device layouts of the 33^3 table.  A plain C++ program can include this (tools/icc_tables_check.cpp does).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/avifgpu.h"
#include "kernel_params.h"

namespace avifgpu {

// 4096 strided words of a table, its last word and its size.  A prepared table is immutable while it is in use (include/avifgpu.h); this is
// the guard against a caller that rewrites one in place anyway, and it is trusted WITHIN an epoch only (icc_staleness): a change the stride
// misses -- 32 consecutive floats of a 4096-entry curve -- is what the byte-for-byte comparison of the next epoch finds.
inline uint64_t table_fingerprint(const void* base, size_t bytes)
{
    const uint32_t* w = static_cast<const uint32_t*>(base);
    const size_t n = bytes / 4, step = n / 4096 ? n / 4096 : 1;
    uint64_t h = 1469598103934665603ull ^ (uint64_t)bytes;
    for (size_t i = 0; i < n; i += step) h = (h ^ w[i]) * 1099511628211ull;
    if (n) h = (h ^ w[n - 1]) * 1099511628211ull;
    return h;
}

// What a cache record remembers of its last upload, and the same four facts of the call at hand.
struct IccStamp { const void* src = nullptr; uint64_t fp = 0, epoch = 0; size_t size = 0; };
// EveryCall: the caller's bytes are compared with the stored image on every call (the small tables: 8-bit shaper, stage program, pow bins).
// OncePerEpoch: a tile that passes the same table again (every tile of an image does) skips the comparison of 216-792 KiB under the
// cache's mutex -- same address, same fingerprint, same size, same EPOCH.  A caller may legally rewrite or reallocate a table at the same
// address between two saves, so address and fingerprint prove nothing across epochs; and the epoch is compared per record, hence per
// device: a multi-GPU save hands row 0 to one device only, and the first tile EACH device sees in an epoch takes the full comparison.
enum class IccVerify { EveryCall, OncePerEpoch };
enum class IccStale { Trusted, CompareBytes, Upload };
inline IccStale icc_staleness(const IccStamp& rec, const IccStamp& call, IccVerify policy)
{
    if (rec.size != call.size) return IccStale::Upload;          // also: nothing uploaded yet (no image is empty)
    if (policy == IccVerify::OncePerEpoch && rec.epoch == call.epoch && rec.src == call.src && rec.fp == call.fp) return IccStale::Trusted;
    return IccStale::CompareBytes;
}

// Device image of the 33^3 table; kernel_params.h (AG_ICC16_DOT2) describes both layouts and what they cost.  Layout 2: the four nodes of
// a pixel's tetrahedron arrive in two 12-byte gathers, {p0, p3} from table A and {p1, p2} from table B, each pair stored channel by
// channel (lo | hi << 16).  Nodes beyond the grid are zero: the fraction of an axis at its end is 0 and so is their weight, which is what
// the library's zeroed strides amount to.  Layout 1 (one 128-byte record per cell) is kept for A/B (tools/ab_variants.sh).
constexpr size_t kIcc16DeviceBytes = AG_ICC16_DOT2 == 2 ? (size_t)kIcc16PairTablesBytes : (size_t)kIcc16Nodes * kIcc16RecBytes;
// table: [33^3][4] as in avifgpu_icc_clut16; out: kIcc16DeviceBytes / 2 ZEROED words
inline void icc16_device_image(const uint16_t (*table)[4], uint16_t* out)
{
    constexpr size_t G = AVIFGPU_ICC_CLUT_GRID;
#if AG_ICC16_DOT2 == 2
    // A[n] = {node n, node n + (1,1,1)}, B[3 m + k] = {node m, node m + e_k}
    auto node_at = [&](size_t r, size_t g, size_t b) -> const uint16_t* {
        return (r < G && g < G && b < G) ? table[(r * G + g) * G + b] : nullptr;
    };
    auto put_pair = [](uint16_t* dst, const uint16_t* lo, const uint16_t* hi) {
        for (int ch = 0; ch < 3; ++ch) { dst[2 * ch] = lo ? lo[ch] : 0; dst[2 * ch + 1] = hi ? hi[ch] : 0; }
    };
    uint16_t* A = out;
    uint16_t* B = out + kIcc16TableABytes / 2;
    for (size_t r = 0; r < G; ++r)
        for (size_t g = 0; g < G; ++g)
            for (size_t b = 0; b < G; ++b) {
                const size_t n = (r * G + g) * G + b;
                put_pair(A + 6 * n, node_at(r, g, b), node_at(r + 1, g + 1, b + 1));
                put_pair(B + 6 * (3 * n + 0), node_at(r, g, b), node_at(r + 1, g, b));
                put_pair(B + 6 * (3 * n + 1), node_at(r, g, b), node_at(r, g + 1, b));
                put_pair(B + 6 * (3 * n + 2), node_at(r, g, b), node_at(r, g, b + 1));
            }
#else
    constexpr size_t kRecU16 = kIcc16RecBytes / 2;
    for (size_t r = 0; r < G; ++r)
        for (size_t g = 0; g < G; ++g)
            for (size_t b = 0; b < G; ++b) {
                uint16_t* dst = out + ((r * G + g) * G + b) * kRecU16;
                auto put = [&](int unit, int half, int j) {            // node of corner j -> its place in the unit
                    const size_t rr = r + ((j >> 2) & 1), gg = g + ((j >> 1) & 1), bb = b + (j & 1);
                    if (!(rr < G && gg < G && bb < G)) return;
                    const uint16_t* node = table[(rr * G + gg) * G + bb];
                    for (int ch = 0; ch < 3; ++ch) dst[(kIcc16UnitBytes / 2) * unit + 2 * ch + half] = node[ch];      // {a.R, b.R, a.G, b.G, a.B, b.B, 0, 0}
                };
                put(kIcc16BaseUnit, 0, 0); put(kIcc16BaseUnit, 1, 7);
                for (int idx = 0; idx < 8; ++idx) {
                    const int amax = kIcc16AxesOfIdx[idx][0], amin = kIcc16AxesOfIdx[idx][1];
                    if (amax < 0) continue;
                    put(idx, 0, 4 >> amax); put(idx, 1, 7 - (4 >> amin));
                }
            }
#endif
}

} // namespace avifgpu
