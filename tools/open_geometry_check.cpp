// open_geometry_check -- sweeps the arithmetic the oriented, upsampled and cropped opens share (avif-format_amd/csrc/open_geometry.h) on
// the host: every code 1..8 x every image of 1..9 x 1..9 pixels x every range of output rows x every subsampling, the region the filler
// returns against a brute-force pixel mapping of the code (apply_code: the permutation of labels that defines the eight codes), and
// legal_cut against the parity of that region's start.  A stand-alone program with its own main, meant to be built with the sanitizers and
// run on the CPU (no device, no HIP):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/open_geometry_check.cpp -o open_geometry_check && ./open_geometry_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../avif-format_amd/csrc/open_geometry.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "open_geometry_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

int main()
{
    long long regions = 0;
    for (int code = 1; code <= 8; ++code) {
        CHECK(open_code_ok(code));
        for (int w = 1; w <= 9; ++w) for (int h = 1; h <= 9; ++h) {
            std::vector<int> label((size_t)w * h), view((size_t)w * h);
            for (size_t i = 0; i < label.size(); ++i) label[i] = (int)i;
            int vw, vh, ow, oh;
            apply_code(code, label.data(), w, h, view.data(), ow, oh);
            open_view_size(w, h, code, vw, vh);
            CHECK(vw == ow && vh == oh && (int64_t)vw * vh == (int64_t)w * h);
            const bool t = kOpenTurn[code].t;
            CHECK(t == (code >= 5) && vw == (t ? h : w));
            for (int orow0 = 0; orow0 <= vh; ++orow0) for (int onrows = 0; orow0 + onrows <= vh; ++onrows)
            for (int xs = 0; xs <= 1; ++xs) for (int ys = 0; ys <= xs; ++ys) {
                OpenRegion r;
                CHECK(open_region(w, h, xs, ys, 3, code, orow0, onrows, r));
                ++regions;
                CHECK(r.out_w == vw && r.out_h == vh && r.bpp == 3 && r.o.t == t);
                CHECK(r.sub_w == (t ? onrows : w) && r.sub_h == (t ? h : onrows));
                CHECK(r.x0 == (t ? r.start : 0) && r.y0 == (t ? 0 : r.start));
                CHECK(r.subsampled == ((t ? xs : ys) != 0));
                // the source rows (codes 1-4) / columns (codes 5-8) the mapping assigns to these output rows
                std::set<int> touched;
                for (int y = orow0; y < orow0 + onrows; ++y)
                    for (int x = 0; x < vw; ++x) {
                        const int src = view.at((size_t)y * vw + x);
                        touched.insert(t ? src % w : src / w);
                    }
                CHECK((int)touched.size() == onrows);
                if (onrows > 0) {
                    CHECK(*touched.begin() == r.start && *touched.rbegin() == r.start + onrows - 1);
                    // flipped: the first output row is the region's LAST source row / column
                    const int first = view.at((size_t)orow0 * vw);
                    CHECK((t ? first % w : first / w) == (r.flipped ? r.start + onrows - 1 : r.start));
                    // the whole region is what the rows show: sub_w x sub_h pixels from (x0, y0), nothing else
                    std::set<int> want, got;
                    for (int y = 0; y < r.sub_h; ++y) for (int x = 0; x < r.sub_w; ++x) want.insert((r.y0 + y) * w + r.x0 + x);
                    for (int y = orow0; y < orow0 + onrows; ++y) for (int x = 0; x < vw; ++x) got.insert(view.at((size_t)y * vw + x));
                    CHECK(want == got);
                    const bool even_start = (*touched.begin() & 1) == 0;
                    CHECK(legal_cut(r, onrows) == (!r.subsampled || even_start || onrows <= 1));
                } else {
                    CHECK(legal_cut(r, onrows));
                }
            }
            OpenRegion r;
            CHECK(!open_region(w, h, 1, 1, 3, code, 0, vh + 1, r) && r.out_h == vh);
            CHECK(!open_region(w, h, 1, 1, 3, code, -1, 1, r) && !open_region(w, h, 1, 1, 3, code, 1, -1, r));
            CHECK(!open_region(w, h, 1, 1, 3, code, vh, 0x7fffffff, r));
        }
    }
    CHECK(!open_code_ok(0) && !open_code_ok(9) && !open_code_ok(-1));
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512 && align256(0x7fffffffLL * 16) % 256 == 0);
    printf("open_geometry_check: %lld regions of 8 codes x 81 sizes x 3 subsamplings, %lld checks, all passed\n", regions, g_checks);
    return 0;
}
