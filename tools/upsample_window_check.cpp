// upsample_window_check.cpp -- the tile and halo arithmetic of the upsampled open's host path (csrc/upsample_window.h), run on the CPU.
// A stand-alone host program for the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o upsample_window_check tools/upsample_window_check.cpp && ./upsample_window_check
// For every small image size, chroma format, sample size and siting, and for every source region the library can stage (row ranges and
// column bands of every start and length), it stages the chroma window exactly as read_rows_upsampled_host does -- from a host plane
// that ends at its last sample into a buffer that ends at the window's last byte, so that any byte too many is a sanitizer report --
// evaluates the rectangle through the window with the kernel's rule (indices clamped to up_need(), minus the window's origin) and
// compares every sample with the definition evaluated on the whole plane.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../avif-format_amd/csrc/upsample_window.h"

using namespace avifgpu;

namespace {

int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Taps { int i0, w0, i1, w1; };
Taps taps_x(int x, int siting)
{
    const int i = x >> 1;
    if (siting == 1) return (x & 1) ? Taps{ i, 3, i + 1, 1 } : Taps{ i - 1, 1, i, 3 };
    return (x & 1) ? Taps{ i, 2, i + 1, 2 } : Taps{ i, 4, i, 0 };
}
Taps taps_y(int y, int ys)
{
    if (!ys) return Taps{ y, 4, y, 0 };
    const int j = y >> 1;
    return (y & 1) ? Taps{ j, 3, j + 1, 1 } : Taps{ j - 1, 1, j, 3 };
}

template <typename T> uint32_t sample(const uint8_t* base, int64_t stride, int row, int col) { T v; memcpy(&v, base + (int64_t)row * stride + (int64_t)col * sizeof(T), sizeof(T)); return v; }

template <typename T> long check_region(const uint8_t* plane, int64_t stride, int cw, int ch, int ys, int siting, int x0, int y0, int w, int h)
{
    const int ssz = (int)sizeof(T);
    const UpStage sw = stage_window(cw, ch, ys, ssz, x0, y0, w, h);
    // the upload: sw.rows rows of sw.row_bytes bytes into a buffer that ends at the window's last byte
    uint8_t* const win = static_cast<uint8_t*>(malloc((size_t)((sw.rows - 1) * sw.pitch + sw.row_bytes)));
    const uint8_t* const host = plane + stage_host_offset(sw, stride, ssz);
    for (int64_t r = 0; r < sw.rows; ++r) memcpy(win + r * sw.pitch, host + r * stride, (size_t)sw.row_bytes);
    const UpNeed need = up_need(cw, ch, ys, x0, y0, w, h);             // what the kernel clamps its loads to
    if (need.lo < sw.need.lo || need.hi > sw.need.hi || need.rlo < sw.need.rlo || need.rhi > sw.need.rhi) { printf("window smaller than the need\n"); exit(1); }
    if (x0 % 2 == 0 && (x0 >> 1) >= 8 / ssz && ((int64_t)((x0 >> 1) - sw.need.lo) * ssz) % 8 != 0) { printf("sample under x0 off the 8-byte grid\n"); exit(1); }
    long n = 0;
    for (int y = y0; y < y0 + h; ++y)
        for (int x = x0; x < x0 + w; ++x) {
            const Taps tx = taps_x(x, siting), ty = taps_y(y, ys);
            uint32_t want = 0, got = 0;
            const int ix[2] = { tx.i0, tx.i1 }, wx[2] = { tx.w0, tx.w1 }, jy[2] = { ty.i0, ty.i1 }, wy[2] = { ty.w0, ty.w1 };
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    if (!wy[a] || !wx[b]) continue;
                    want += (uint32_t)(wy[a] * wx[b]) * sample<T>(plane, stride, clampi(jy[a], 0, ch - 1), clampi(ix[b], 0, cw - 1));
                    got += (uint32_t)(wy[a] * wx[b]) * sample<T>(win, sw.pitch, clampi(jy[a], need.rlo, need.rhi) - sw.need.rlo, clampi(ix[b], need.lo, need.hi) - sw.need.lo);
                }
            if (((want + 8) >> 4) != ((got + 8) >> 4)) { printf("mismatch at (%d, %d) of region %d,%d %dx%d, plane %dx%d\n", x, y, x0, y0, w, h, cw, ch); exit(1); }
            ++n;
        }
    free(win);
    return n;
}

template <typename T> long check_image(int W, int H, int ys, int siting, uint32_t seed)
{
    const int cw = (W + 1) >> 1, ch = (H + ys) >> ys;
    const int64_t stride = (int64_t)(cw + 3) * sizeof(T);            // no multiple of 8
    const size_t bytes = (size_t)((ch - 1) * stride + cw * (int64_t)sizeof(T));   // the plane ends at its last sample
    uint8_t* const plane = static_cast<uint8_t*>(malloc(bytes));
    for (size_t i = 0; i < bytes; ++i) { seed = seed * 1664525u + 1013904223u; plane[i] = (uint8_t)(seed >> 24); }
    long n = 0;
    for (int y0 = 0; y0 < H; ++y0)                                     // row ranges (codes 1-4)
        for (int h = 1; y0 + h <= H; h += (h < 4 ? 1 : 5)) n += check_region<T>(plane, stride, cw, ch, ys, siting, 0, y0, W, h);
    for (int x0 = 0; x0 < W; ++x0)                                     // column bands (codes 5-8)
        for (int w = 1; x0 + w <= W; w += (w < 4 ? 1 : 7)) n += check_region<T>(plane, stride, cw, ch, ys, siting, x0, 0, w, H);
    free(plane);
    return n;
}

} // namespace

int main()
{
    long n = 0;
    const int sizes[][2] = { { 1, 1 }, { 2, 2 }, { 1, 9 }, { 9, 1 }, { 3, 5 }, { 17, 12 }, { 33, 31 }, { 34, 32 }, { 67, 35 } };
    for (const auto& s : sizes)
        for (int ys = 0; ys < 2; ++ys)
            for (int siting = 1; siting <= 2; ++siting) {
                n += check_image<uint8_t>(s[0], s[1], ys, siting, 1u + (uint32_t)s[0]);
                n += check_image<uint16_t>(s[0], s[1], ys, siting, 7u + (uint32_t)s[1]);
            }
    printf("upsample window arithmetic: %ld samples through staged windows equal the whole-plane definition\n", n);
    return 0;
}
