// grid_geometry_check -- sweeps the arithmetic of the grid open (avif-format_amd/csrc/grid_geometry.h) on the host: the legality rule
// against a restatement, the pieces of every rectangle of small grids against the per-sample definition of an assembled plane, a model
// of what a lane of grid_gather reads and writes, the bound the scratch helper puts on the cropped open's staged rectangle, and the
// ImageGrid payload parser on exact-size heap buffers of random bytes.  A stand-alone program with its own main, meant to be built with
// the sanitizers and run on the CPU (no device, no HIP):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/grid_geometry_check.cpp -o grid_geometry_check && ./grid_geometry_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../avif-format_amd/csrc/crop_geometry.h"
#include "../avif-format_amd/csrc/grid_geometry.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "grid_geometry_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static uint32_t g_rng = 20261020u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// ---- legality -----------------------------------------------------------------------------------------------------------------------------
static bool legal_restated(int64_t W, int64_t H, int xs, int ys, int64_t cols, int64_t rows, int64_t tw, int64_t th)
{
    if (W < 1 || H < 1 || cols < 1 || cols > 256 || rows < 1 || rows > 256 || tw < 1 || th < 1) return false;
    if (cols * tw < W || rows * th < H) return false;
    if (xs == 1 && cols > 1 && tw % 2 != 0) return false;
    if (ys == 1 && rows > 1 && th % 2 != 0) return false;
    return true;
}

static void sweep_legality()
{
    const int sizes[] = { 0, 1, 2, 7, 8, 12, 13 }, counts[] = { 0, 1, 2, 3, 256, 257 }, tiles[] = { 0, 1, 2, 3, 4, 6, 7, 13 };
    for (int W : sizes) for (int H : sizes) for (int xs = 0; xs < 2; ++xs) for (int ys = 0; ys <= xs; ++ys)
        for (int c : counts) for (int r : counts) for (int tw : tiles) for (int th : tiles) {
            const avifgpu_grid g = { c, r, tw, th };
            CHECK((grid_illegal(W, H, xs, ys, g) == nullptr) == legal_restated(W, H, xs, ys, c, r, tw, th));
        }
    // the products are taken in 64 bits
    const avifgpu_grid big = { 256, 256, 0x7fffffff, 0x7fffffff };
    CHECK(grid_illegal(0x7fffffff, 0x7fffffff, 0, 0, big) == nullptr);
    const avifgpu_grid wrap = { 4, 1, 0x40000000, 8 };          // 4 * 2^30 wraps to 0 in 32 bits
    CHECK(grid_illegal(0x7fffffff, 8, 0, 0, wrap) == nullptr);
    const avifgpu_grid shy = { 2, 1, 0x3fffffff, 8 };
    CHECK(grid_illegal(0x7fffffff, 8, 0, 0, shy) != nullptr);
}

// ---- pieces and lanes against the per-sample definition -----------------------------------------------------------------------------------
// A plane of cols x rows tiles of tw x th samples of s bytes.  Every tile is a heap buffer of exactly th rows of tw * s bytes (stride ==
// row: one byte too far is the sanitizer's); byte b of sample (ty, tx) of tile k holds a value the definition can name.
struct Plane {
    int cols, rows, tw, th, s;
    std::vector<std::vector<uint8_t>> tile;
    static uint8_t value(int k, int ty, int tx, int b) { return (uint8_t)(k * 131 + ty * 31 + tx * 7 + b * 3 + 1); }
    Plane(int cols_, int rows_, int tw_, int th_, int s_) : cols(cols_), rows(rows_), tw(tw_), th(th_), s(s_), tile((size_t)cols_ * rows_)
    {
        for (int k = 0; k < cols * rows; ++k) {
            tile[k].resize((size_t)th * tw * s);
            for (int ty = 0; ty < th; ++ty) for (int tx = 0; tx < tw; ++tx) for (int b = 0; b < s; ++b) tile[k][((size_t)ty * tw + tx) * s + b] = value(k, ty, tx, b);
        }
    }
    // P[y, x] = tile[(y / th) * cols + x / tw][y % th, x % tw]
    uint8_t defined(int y, int x, int b) const { return value((y / th) * cols + x / tw, y % th, x % tw, b); }
};

static void check_rect(const Plane& p, int x0, int y0, int w, int h)
{
    const int64_t rb = (int64_t)w * p.s;
    const int64_t pitch = (rb + 15) / 16 * 16;
    // the pieces: the host path's copies
    std::vector<uint8_t> dst((size_t)pitch * h, 0);
    std::vector<uint8_t> hit((size_t)pitch * h, 0);
    int pieces = 0;
    grid_pieces(p.cols, p.tw, p.th, p.s, x0, y0, w, h, [&](const GridPiece& k) {
        ++pieces;
        CHECK(k.tile >= 0 && k.tile < p.cols * p.rows && k.rows >= 1 && k.bytes >= p.s && k.bytes % p.s == 0);
        CHECK(k.src_x >= 0 && k.src_x + k.bytes <= (int64_t)p.tw * p.s && k.src_y >= 0 && k.src_y + k.rows <= p.th);
        CHECK(k.dst_x >= 0 && k.dst_x + k.bytes <= rb && k.dst_y >= 0 && k.dst_y + k.rows <= h);
        for (int r = 0; r < k.rows; ++r)
            for (int64_t b = 0; b < k.bytes; ++b) {
                const size_t at = (size_t)(k.dst_y + r) * pitch + k.dst_x + b;
                CHECK(!hit[at]);
                hit[at] = 1;
                dst[at] = p.tile[k.tile][(size_t)(k.src_y + r) * p.tw * p.s + k.src_x + b];
            }
    });
    const int tiles_x = (x0 + w - 1) / p.tw - x0 / p.tw + 1, tiles_y = (y0 + h - 1) / p.th - y0 / p.th + 1;
    CHECK(pieces == tiles_x * tiles_y);                          // one per intersecting tile
    for (int y = 0; y < h; ++y)
        for (int64_t b = 0; b < pitch; ++b) {
            CHECK(hit[(size_t)y * pitch + b] == (b < rb));
            if (b < rb) CHECK(dst[(size_t)y * pitch + b] == p.defined(y0 + y, x0 + (int)(b / p.s), (int)(b % p.s)));
        }
    // the lanes: grid_gather's own arithmetic, restated with its names -- a lane owns 16 destination bytes of every row
    std::vector<uint8_t> out((size_t)pitch * h, 0xEE);
    const int S = p.s;
    for (int64_t off = 0; off < pitch + 16; off += 16) {
        if (off >= rb) continue;
        const int n = (int)((rb - off < 16 ? rb - off : 16) / S);
        const uint32_t x = (uint32_t)x0 + (uint32_t)(off / S);
        const uint32_t tw = (uint32_t)p.tw, tc = x / tw, tx = x - tc * tw;
        const bool whole = n == 16 / S && tx + 16 / S <= tw;
        for (int row = 0; row < h; ++row) {
            const uint32_t y = (uint32_t)y0 + (uint32_t)row, tr = y / (uint32_t)p.th, ty = y - tr * (uint32_t)p.th;
            CHECK(tr < (uint32_t)p.rows);
            uint8_t* const dp = out.data() + (size_t)row * pitch + off;
            if (whole) {
                CHECK(tc < (uint32_t)p.cols);
                const std::vector<uint8_t>& t = p.tile[tr * p.cols + tc];
                const size_t at = ((size_t)ty * p.tw + tx) * S;
                CHECK(at + 16 <= t.size() && (size_t)tx * S + 16 <= (size_t)p.tw * S);      // inside the tile's ROW, not only its buffer
                memcpy(dp, t.data() + at, 16);
            } else {
                uint32_t c = tc, cx = tx;
                for (int i = 0; i < n; ++i) {
                    CHECK(c < (uint32_t)p.cols);
                    const std::vector<uint8_t>& t = p.tile[tr * p.cols + c];
                    memcpy(dp + (size_t)i * S, &t.at(((size_t)ty * p.tw + cx) * S), S);
                    if (++cx == tw) { cx = 0; ++c; }
                }
            }
        }
    }
    for (int y = 0; y < h; ++y)
        for (int64_t b = 0; b < pitch; ++b) {
            const uint8_t got = out[(size_t)y * pitch + b];
            if (b < rb) CHECK(got == dst[(size_t)y * pitch + b]); else CHECK(got == 0xEE);   // bytes beyond the payload are not touched
        }
}

static void sweep_pieces()
{
    const int shapes[][4] = { { 3, 3, 2, 2 }, { 3, 2, 6, 4 }, { 3, 3, 18, 10 }, { 2, 2, 64, 5 }, { 2, 2, 130, 3 }, { 1, 1, 37, 9 }, { 5, 1, 7, 3 }, { 1, 4, 33, 2 }, { 9, 2, 1, 1 } };
    for (const auto& sh : shapes)
        for (int s = 1; s <= 2; ++s) {
            const Plane p(sh[0], sh[1], sh[2], sh[3], s);
            const int PW = sh[0] * sh[2], PH = sh[1] * sh[3];
            const int xs[] = { 0, 1, sh[2] - 1, sh[2], 17 }, ys[] = { 0, sh[3] - 1, sh[3] };
            for (int x0 : xs) for (int y0 : ys) {
                if (x0 < 0 || x0 >= PW || y0 >= PH) continue;
                for (int w = 1; x0 + w <= PW; w += (w < 40 || x0 + w + 1 >= PW - 2) ? 1 : 13)
                    for (int h : { 1, 2, sh[3], PH - y0 })
                        if (h >= 1 && y0 + h <= PH) check_rect(p, x0, y0, w, h);
            }
        }
    for (int i = 0; i < 3000; ++i) {                             // random shapes and rectangles
        const int cols = 1 + rnd() % 5, rows = 1 + rnd() % 4, tw = 1 + rnd() % 40, th = 1 + rnd() % 7, s = 1 + rnd() % 2;
        const Plane p(cols, rows, tw, th, s);
        const int x0 = rnd() % (cols * tw), y0 = rnd() % (rows * th);
        const int w = 1 + rnd() % (cols * tw - x0), h = 1 + rnd() % (rows * th - y0);
        check_rect(p, x0, y0, w, h);
    }
}

// ---- what is gathered for a call: the cropped open's staged rectangle lies inside the scratch helper's bound and inside the planes -----------
static void sweep_stage_bound()
{
    const int sizes[][2] = { { 1, 1 }, { 2, 3 }, { 9, 8 }, { 70, 5 }, { 67, 6 }, { 101, 3 } };
    for (const auto& sz : sizes) {
        const int W = sz[0], H = sz[1];
        for (int xs = 0; xs < 2; ++xs) for (int ys = 0; ys <= xs; ++ys) for (int interp = 0; interp <= xs; ++interp)
            for (int x0 = 0; x0 < W; ++x0) for (int y0 = 0; y0 < H; ++y0)
                for (int w = 1; x0 + w <= W; w += (w < 6 || x0 + w + 4 > W) ? 1 : 9) for (int h = 1; y0 + h <= H; ++h) {
                    const avifgpu_rect t = { x0, y0, w, h };
                    const avifgpu_rect sr = crop_stage_rect(t, W, H, xs, ys, interp != 0);
                    CHECK(sr.x0 >= 0 && sr.y0 >= 0 && sr.x0 + sr.width <= W && sr.y0 + sr.height <= H);
                    CHECK(sr.x0 <= x0 && sr.y0 <= y0 && sr.x0 + sr.width >= x0 + w && sr.y0 + sr.height >= y0 + h);
                    CHECK(!xs || sr.x0 % 2 == 0); CHECK(!ys || sr.y0 % 2 == 0);
                    const int gw = grid_stage_bound(w, kGridStageColumns, W), gh = grid_stage_bound(h, kGridStageRows, H);
                    CHECK(sr.width <= gw && sr.height <= gh);
                    const avifgpu_rect pr = crop_plane_rect(sr, true, xs, ys);
                    CHECK(pr.width <= ((gw + xs) >> xs) && pr.height <= ((gh + ys) >> ys));
                    CHECK(pr.x0 >= 0 && pr.y0 >= 0 && pr.x0 + pr.width <= ((W + xs) >> xs) && pr.y0 + pr.height <= ((H + ys) >> ys));
                }
    }
    CHECK(grid_stage_bound(0x7fffffff, kGridStageColumns, 0x7fffffff) == 0x7fffffff);       // no overflow at the top
}

// ---- tiles and extents ----------------------------------------------------------------------------------------------------------------------
static void sweep_extents()
{
    for (int W = 1; W <= 40; W += 3) for (int H = 1; H <= 20; H += 3) for (int xs = 0; xs < 2; ++xs) for (int ys = 0; ys <= xs; ++ys)
        for (int c = 1; c <= 4; ++c) for (int r = 1; r <= 3; ++r) for (int tw = 1; tw <= 41; tw += 2 - (c == 1)) for (int th = 1; th <= 21; th += 4) {
            const avifgpu_grid g = { c, r, tw, th };
            if (grid_illegal(W, H, xs, ys, g)) continue;
            const int cw = (W + xs) >> xs, ch = (H + ys) >> ys, twc = grid_tile_w(g, true, xs), thc = grid_tile_h(g, true, ys);
            CHECK(grid_tile_w(g, false, xs) == tw && grid_tile_h(g, false, ys) == th);
            CHECK((int64_t)c * twc >= cw && (int64_t)r * thc >= ch);                        // the chroma tiles cover the chroma canvas
            for (int k = 0; k < c * r; ++k) {
                const bool vis = grid_tile_visible(g, W, H, k);
                const int kc = k % c, kr = k / c;
                CHECK(vis == (kc * tw < W && kr * th < H));
                // a luma sample is visible in a tile exactly where a chroma sample is: the same tiles are read in every plane
                CHECK(vis == ((int64_t)kc * twc < cw && (int64_t)kr * thc < ch));
            }
            // chroma sample (y >> ys, x >> xs) of luma (y, x) lies in the same tile as the luma sample
            for (int x = 0; x < W; ++x) CHECK((x >> xs) / twc == x / tw);
            for (int y = 0; y < H; ++y) CHECK((y >> ys) / thc == y / th);
        }
}

// ---- the payload parser on exact-size heap buffers -------------------------------------------------------------------------------------------
static void fuzz_parse()
{
    int32_t r, c, w, h;
    CHECK(!grid_parse(nullptr, 8, r, c, w, h));
    int ok = 0;
    for (int i = 0; i < 200000; ++i) {
        const int size = rnd() % 15;
        std::vector<uint8_t> buf((size_t)size);                  // size 0: data() may be null or not; both are rejected
        for (uint8_t& b : buf) b = (uint8_t)rnd();
        if (size > 0 && i % 2) buf[0] = 0;
        if (size > 1 && i % 3 == 0) buf[1] = (uint8_t)(rnd() & 1);
        if (size > 4 && i % 5 == 0) buf[4] &= 0x7f;
        r = c = w = h = -7;
        const bool got = grid_parse(buf.data(), size, r, c, w, h);
        // restated
        bool want = size >= 8 && buf[0] == 0 && (!(buf[1] & 1) || size >= 12);
        uint64_t ww = 0, hh = 0;
        if (want) {
            if (buf[1] & 1) { for (int k = 0; k < 4; ++k) { ww = ww << 8 | buf[4 + k]; hh = hh << 8 | buf[8 + k]; } }
            else { ww = (uint64_t)buf[4] << 8 | buf[5]; hh = (uint64_t)buf[6] << 8 | buf[7]; }
            want = ww >= 1 && hh >= 1 && ww <= 0x7fffffffu && hh <= 0x7fffffffu;
        }
        CHECK(got == want);
        if (got) { CHECK(r == buf[2] + 1 && c == buf[3] + 1 && (uint64_t)w == ww && (uint64_t)h == hh); ++ok; }
        else CHECK(r == -7 && c == -7 && w == -7 && h == -7);
    }
    CHECK(ok > 10000);
    CHECK(!grid_parse(reinterpret_cast<const uint8_t*>("\0\0\0\0\0\1\0\1"), -1, r, c, w, h));
}

int main()
{
    sweep_legality();
    sweep_extents();
    sweep_pieces();
    sweep_stage_bound();
    fuzz_parse();
    printf("grid_geometry_check: ok, %lld checks\n", g_checks);
    return 0;
}
