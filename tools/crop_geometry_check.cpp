// crop_geometry_check -- sweeps the arithmetic of the cropped open (avif-format_amd/csrc/crop_geometry.h) on the host: every rectangle of
// small images x every code x every cut x both kinds of open, with every invariant the device and host paths rely on asserted, and the
// clean-aperture rule at the extremes of its 32-bit operands.  A stand-alone program with its own main, meant to be built with the
// sanitizers and run on the CPU (no device, no HIP):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/crop_geometry_check.cpp -o crop_geometry_check && ./crop_geometry_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../avif-format_amd/csrc/crop_geometry.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "crop_geometry_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static bool inside(const avifgpu_rect& a, const avifgpu_rect& b)      // a inside b
{
    return a.x0 >= b.x0 && a.y0 >= b.y0 && a.x0 + a.width <= b.x0 + b.width && a.y0 + a.height <= b.y0 + b.height;
}

// orient(code, L[r]) of a label image of width W, read through a touch-map so that every access is bounds-checked by the sanitizer
static std::vector<int> oriented(const std::vector<int>& L, int W, const avifgpu_rect& r, int code)
{
    const CropTurn o = crop_turn(code);
    int vw, vh;
    crop_view_size(r, code, vw, vh);
    std::vector<int> out((size_t)vw * vh);
    for (int y = 0; y < vh; ++y)
        for (int x = 0; x < vw; ++x) {
            const int sy = o.t ? (o.fy ? r.height - 1 - x : x) : (o.fy ? r.height - 1 - y : y);
            const int sx = o.t ? (o.fx ? r.width - 1 - y : y) : (o.fx ? r.width - 1 - x : x);
            out[(size_t)y * vw + x] = L.at((size_t)(r.y0 + sy) * W + (r.x0 + sx));
        }
    return out;
}

static void sweep_image(int W, int H, int xs, int ys)
{
    const avifgpu_rect image = { 0, 0, W, H };
    std::vector<int> L((size_t)W * H);
    for (size_t i = 0; i < L.size(); ++i) L[i] = (int)i;
    const int cw = (W + xs) >> xs, ch = (H + ys) >> ys;
    for (int x0 = 0; x0 < W; ++x0) for (int y0 = 0; y0 < H; ++y0)
    for (int w = 1; x0 + w <= W; ++w) for (int h = 1; y0 + h <= H; ++h) {
        const avifgpu_rect rect = { x0, y0, w, h };
        CHECK(crop_rect_ok(rect, W, H));
        for (int code = 1; code <= 8; ++code) {
            int vw, vh;
            crop_view_size(rect, code, vw, vh);
            const std::vector<int> view = oriented(L, W, rect, code);
            // a crop of the view maps to a stored rectangle with the same pixels (one crop per view: its inner part, or all of it)
            {
                avifgpu_rect v = { vw > 2 ? 1 : 0, vh > 2 ? 1 : 0, vw > 2 ? vw - 2 : vw, vh > 2 ? vh - 1 : vh }, out;
                CHECK(crop_compose(rect, code, v, out) && inside(out, rect));
                const std::vector<int> got = oriented(L, W, out, code);
                int gw, gh;
                crop_view_size(out, code, gw, gh);
                CHECK(gw == v.width && gh == v.height);
                for (int y = 0; y < gh; ++y) for (int x = 0; x < gw; ++x) CHECK(got[(size_t)y * gw + x] == view[(size_t)(v.y0 + y) * vw + v.x0 + x]);
            }
            for (int interp = 0; interp <= (xs ? 1 : 0); ++interp) {
                const bool matters = !interp && (crop_turn(code).t ? xs : ys) != 0;
                for (int max_rows : { 1, 2, 3, 7 }) {
                    int covered = 0;
                    for (int o = 0; o < vh;) {
                        const int n = crop_next_tile(rect, code, matters, o, max_rows);
                        CHECK(n >= 1 && n <= max_rows && o + n <= vh);
                        const avifgpu_rect t = crop_tile_rect(rect, code, o, n);
                        CHECK(inside(t, rect) && t.width >= 1 && t.height >= 1);
                        covered += crop_turn(code).t ? t.width : t.height;
                        // the tile's pixels are the view's rows [o, o + n)
                        const std::vector<int> tv = oriented(L, W, t, code);
                        for (int y = 0; y < n; ++y) for (int x = 0; x < vw; ++x) CHECK(tv[(size_t)y * vw + x] == view[(size_t)(o + y) * vw + x]);
                        // what is decoded: the covering rectangle starts even in every subsampled direction (or is single) and stays inside the image
                        const CropCover k = crop_cover(t, xs, ys);
                        CHECK(inside(k.c, image) && inside(t, k.c) && k.c.x0 + k.px == t.x0 && k.c.y0 + k.py == t.y0);
                        CHECK(!xs || (k.c.x0 & 1) == 0 || k.c.width == 1);
                        CHECK(!ys || (k.c.y0 & 1) == 0 || k.c.height == 1);
                        // its planes stay inside the whole planes
                        const avifgpu_rect kp = crop_plane_rect(k.c, true, xs, ys);
                        CHECK(kp.x0 + kp.width <= cw && kp.y0 + kp.height <= ch && kp.width >= 1 && kp.height >= 1);
                        // chroma sample of every pixel of t through the sub-image == through the whole image
                        for (int x = 0; x < t.width; ++x) CHECK(kp.x0 + ((x + k.px) >> xs) == (t.x0 + x) >> xs);
                        for (int y = 0; y < t.height; ++y) CHECK(kp.y0 + ((y + k.py) >> ys) == (t.y0 + y) >> ys);
                        // the scratch of the call never exceeds what the helper promises for n rows
                        const int64_t need = crop_scratch_bytes(t, xs, ys, interp != 0, code, 2, 12, false, false);
                        avifgpu_rect bound_t = rect;
                        if (crop_turn(code).t) bound_t.width = n; else bound_t.height = n;
                        CHECK(need <= crop_scratch_bytes(bound_t, xs, ys, interp != 0, code, 2, 12, crop_turn(code).t, !crop_turn(code).t));
                        // the host path's staged image: inside the image, even starts, holds t and (interpolated) every tap of t
                        const avifgpu_rect s = crop_stage_rect(t, W, H, xs, ys, interp != 0);
                        CHECK(inside(s, image) && inside(t, s));
                        CHECK(s.x0 % kCropStageColumns == 0 && s.x0 <= t.x0 && t.x0 - s.x0 < kCropStageColumns + 2);
                        CHECK(!ys || (s.y0 & 1) == 0);
                        const avifgpu_rect sp = crop_plane_rect(s, true, xs, ys);
                        CHECK(sp.x0 + sp.width <= cw && sp.y0 + sp.height <= ch);
                        if (interp) {
                            const UpNeed nd = up_need(cw, ch, ys, t.x0, t.y0, t.width, t.height);
                            CHECK(sp.x0 <= nd.lo && (sp.x0 == 0 || nd.lo - sp.x0 < kCropStageColumns / 2) && sp.x0 + sp.width - 1 == nd.hi);
                            if (ys) CHECK(sp.y0 == nd.rlo && sp.y0 + sp.height - 1 == nd.rhi);
                            else CHECK(sp.y0 == t.y0 && sp.height == t.height);
                            // the staged image as a whole image asks for exactly its own planes
                            const int scw = (s.width + xs) >> xs, sch = (s.height + ys) >> ys;
                            const UpNeed in = up_need(scw, sch, ys, t.x0 - s.x0, t.y0 - s.y0, t.width, t.height);
                            CHECK(in.lo == nd.lo - sp.x0 && in.hi == scw - 1 && in.rlo + (ys ? 0 : s.y0) >= 0 && in.rhi <= sch - 1);
                        }
                        if (matters && n < vh - o && n > 1) {
                            const CropTurn tr = crop_turn(code);
                            const int a0 = tr.t ? rect.x0 : rect.y0;
                            const bool flipped = tr.t ? tr.fx : tr.fy;
                            CHECK(((flipped ? a0 + vh - o - n : a0 + o + n) & 1) == 0);
                        }
                        o += n;
                    }
                    CHECK(covered == vh);
                }
            }
        }
    }
}

static void clap_extremes()
{
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    const int32_t vals[] = { lo, lo + 1, -3, -1, 0, 1, 2, 3, 50, 65536, hi - 1, hi };
    const int sizes[] = { 1, 2, 100, 101, hi };
    avifgpu_rect r;
    for (int size : sizes) for (int32_t an : vals) for (int32_t ad : vals) for (int32_t on : vals) for (int32_t od : vals) {
        const int32_t clap[8] = { an, ad, an, ad, on, od, on, od };
        const bool ok = clap_to_rect(size, size, clap, r);
        if (ad <= 0 || od <= 0 || an <= 0) CHECK(!ok);
        if (ok) CHECK(crop_rect_ok(r, size, size) && r.x0 == r.y0 && r.width == r.height);
    }
    // the hand-checked rows of the issue
    const int32_t a[8] = { 50, 1, 40, 1, 0, 1, 0, 1 };
    CHECK(clap_to_rect(100, 80, a, r) && r.x0 == 25 && r.y0 == 20 && r.width == 50 && r.height == 40);
    CHECK(clap_to_rect(101, 80, a, r) && r.x0 == 26 && r.x0 + r.width - 1 == 75);
    const int32_t b[8] = { 50, 1, 40, 1, -1, 2, 0, 1 };
    CHECK(clap_to_rect(100, 80, b, r) && r.x0 == 25 && r.x0 + r.width - 1 == 74);
    const int32_t c[8] = { 20, 1, 40, 1, 0, 1, 0, 1 };
    CHECK(clap_to_rect(10, 80, c, r) && r.x0 == 0 && r.width == 10);
    const int32_t d[8] = { 10, 1, 10, 1, 200, 1, 0, 1 };
    CHECK(!clap_to_rect(100, 80, d, r));
}

int main()
{
    for (int xs = 0; xs <= 1; ++xs)
        for (int ys = 0; ys <= xs; ++ys)
            for (int W : { 1, 2, 5, 6 }) for (int H : { 1, 3, 4 }) sweep_image(W, H, xs, ys);
    sweep_image(7, 6, 1, 1);
    clap_extremes();
    printf("crop_geometry_check: ok, %lld checks\n", g_checks);
    return 0;
}
