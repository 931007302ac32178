// grid_save_geometry_check -- sweeps the arithmetic of the grid save (avif-format_amd/csrc/grid_save_geometry.h) on the host: the legality
// rule against a restatement, the bands of every row cut of small grids and their pad rectangles, the pieces of every band against the
// per-pixel definition of the padded plane (every byte of every tile exactly once), the rule of avifgpu_grid_fit against a brute-force
// search, the ImageGrid payload against grid_parse on exact-size heap buffers, and a lane model of grid_scatter that writes into heap
// tiles of exactly the bytes a tile holds.  A stand-alone program with its own main, meant to be built with the sanitizers and run on the
// CPU (no device, no HIP):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/grid_save_geometry_check.cpp -o grid_save_geometry_check && ./grid_save_geometry_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../avif-format_amd/csrc/grid_save_geometry.h"

using namespace avifgpu;

static long long g_checks = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { fprintf(stderr, "grid_save_geometry_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

// ---- legality -----------------------------------------------------------------------------------------------------------------------------
static bool legal_restated(int64_t W, int64_t H, int xs, int ys, int64_t cols, int64_t rows, int64_t tw, int64_t th)
{
    if (W < 1 || H < 1 || cols < 1 || cols > 256 || rows < 1 || rows > 256 || tw < 1 || th < 1) return false;
    if (cols * tw < W || rows * th < H) return false;
    if (xs == 1 && cols > 1 && tw % 2 != 0) return false;
    if (ys == 1 && rows > 1 && th % 2 != 0) return false;
    return (cols - 1) * tw < W && (rows - 1) * th < H;
}

static void sweep_legality()
{
    const int sizes[] = { 0, 1, 2, 7, 8, 12, 13 }, counts[] = { 0, 1, 2, 3, 256, 257 }, tiles[] = { 0, 1, 2, 3, 4, 6, 7, 13 };
    for (int W : sizes) for (int H : sizes) for (int xs = 0; xs < 2; ++xs) for (int ys = 0; ys <= xs; ++ys)
        for (int c : counts) for (int r : counts) for (int tw : tiles) for (int th : tiles) {
            const avifgpu_grid g = { c, r, tw, th };
            CHECK((grid_save_illegal(W, H, xs, ys, g) == nullptr) == legal_restated(W, H, xs, ys, c, r, tw, th));
        }
    const avifgpu_grid wrap = { 4, 1, 0x40000000, 8 };          // 3 * 2^30 wraps negative in 32 bits
    CHECK(grid_save_illegal(0x7fffffff, 8, 0, 0, wrap) != nullptr);
    const avifgpu_grid fits = { 2, 1, 0x40000000, 8 };
    CHECK(grid_save_illegal(0x7fffffff, 8, 0, 0, fits) == nullptr);
}

// ---- a plane of a save: canvas, tiles, the definition ---------------------------------------------------------------------------------------
struct Plane {
    avifgpu_grid g; int pw, ph, tw, th, b, ys, height;
    std::vector<std::vector<uint8_t>> tile;      // exactly th rows of tw * b bytes each: one byte too far is the sanitizer's
    std::vector<std::vector<int>> hits;
    static uint8_t value(int y, int x, int k) { return (uint8_t)(y * 37 + x * 11 + k * 5 + 1); }      // byte k of canvas pixel (y, x)
    Plane(const avifgpu_grid& g_, int width, int height_, bool chroma, int xs, int ys_, int b_) : g(g_), b(b_), ys(chroma ? ys_ : 0), height(height_)
    {
        const int x = chroma ? xs : 0;
        pw = (width + x) >> x; ph = (height + ys) >> ys;
        tw = grid_tile_w(g, chroma, xs); th = grid_tile_h(g, chroma, ys_);
        tile.assign((size_t)g.columns * g.rows, std::vector<uint8_t>((size_t)th * tw * b, 0xEE));
        hits.assign((size_t)g.columns * g.rows, std::vector<int>((size_t)th * tw * b, 0));
    }
    void put(int k, int64_t x_bytes, int y, uint8_t v) { const size_t at = (size_t)y * tw * b + (size_t)x_bytes; CHECK(k >= 0 && k < (int)tile.size() && x_bytes >= 0 && x_bytes < (int64_t)tw * b && y >= 0 && y < th); tile[k][at] = v; ++hits[k][at]; }
    void verify() const
    {
        for (int r = 0; r < g.rows; ++r) for (int c = 0; c < g.columns; ++c) for (int y = 0; y < th; ++y) for (int x = 0; x < tw; ++x) for (int k = 0; k < b; ++k) {
            const int qy = r * th + y, qx = c * tw + x;
            const size_t at = ((size_t)y * tw + x) * b + k;
            CHECK(hits[r * g.columns + c][at] == 1);
            CHECK(tile[r * g.columns + c][at] == value(qy < ph ? qy : ph - 1, qx < pw ? qx : pw - 1, k));
        }
    }
};

// the band buffer of a call, as the conversion leaves it: band.rows rows of pw pixels (+ room for the pads when `padded`)
static std::vector<uint8_t> band_buffer(const Plane& p, const GridBand& bd, int64_t pitch, bool padded)
{
    std::vector<uint8_t> buf((size_t)pitch * (bd.rows + (padded ? bd.pad_rows : 0)), 0xCC);
    for (int y = 0; y < bd.rows; ++y) for (int x = 0; x < p.pw; ++x) for (int k = 0; k < p.b; ++k) buf[(size_t)y * pitch + (size_t)x * p.b + k] = Plane::value(bd.y0 + y, x, k);
    return buf;
}

// grid_pad as the kernel does it: pad cells only, from valid cells only
static void model_pad(const Plane& p, const GridBand& bd, std::vector<uint8_t>& buf, int64_t pitch)
{
    const int full = p.pw + bd.pad_cols;
    for (int row = 0; row < bd.rows + bd.pad_rows; ++row)
        for (int x = row < bd.rows ? p.pw : 0; x < full; ++x)
            for (int k = 0; k < p.b; ++k)
                buf[(size_t)row * pitch + (size_t)x * p.b + k] = buf[(size_t)(row < bd.rows ? row : bd.rows - 1) * pitch + (size_t)(x < p.pw ? x : p.pw - 1) * p.b + k];
}

// the host path: pad in place, then one strided copy per piece
static void model_pieces(Plane& p, const GridBand& bd)
{
    const int64_t pitch = (int64_t)p.g.columns * p.tw * p.b + 3;
    std::vector<uint8_t> buf = band_buffer(p, bd, pitch, true);
    model_pad(p, bd, buf, pitch);
    grid_save_pieces(p.g, bd, p.tw, p.th, p.b, [&](const GridPiece& k) {
        CHECK(k.bytes > 0 && k.rows > 0 && k.dst_y + k.rows <= bd.rows + bd.pad_rows && k.dst_x + k.bytes <= (int64_t)p.g.columns * p.tw * p.b);
        for (int y = 0; y < k.rows; ++y) for (int64_t x = 0; x < k.bytes; ++x) p.put(k.tile, k.src_x + x, k.src_y + y, buf[(size_t)(k.dst_y + y) * pitch + (size_t)(k.dst_x + x)]);
    });
}

// the device path: the lanes of grid_scatter on the unpadded band buffer
static void model_lanes(Plane& p, const GridBand& bd)
{
    const int64_t pitch = (int64_t)p.pw * p.b;                   // exactly the payload: a lane that reads past pw * b leaves the buffer
    const std::vector<uint8_t> buf = band_buffer(p, bd, pitch, false);
    const int64_t twb = (int64_t)p.tw * p.b, total = twb * p.g.columns, valid = (int64_t)p.pw * p.b;
    const int U = grid_scatter_unit(p.b);
    for (int row = 0; row < bd.rows + bd.pad_rows; ++row) {
        const int y = bd.y0 + row, tr = y / p.th, ty = y - tr * p.th;
        const uint8_t* sp = buf.data() + (size_t)(row < bd.rows ? row : bd.rows - 1) * pitch;
        for (int64_t off = 0; off < total; off += 16) {
            const int n = (int)(total - off < 16 ? total - off : 16);
            int64_t c = off / twb, cx = off - c * twb;
            if (grid_scatter_whole(off, twb, total, valid)) {
                CHECK(n == 16);
                for (int i = 0; i < 16; ++i) p.put(tr * p.g.columns + (int)c, cx + i, ty, sp[off + i]);
                continue;
            }
            CHECK(n % U == 0 && cx % U == 0);
            for (int i = 0; i < n; i += U) {
                const int64_t s = grid_scatter_source(off + i, p.b, p.pw);
                CHECK(s + U <= valid);
                for (int u = 0; u < U; ++u) p.put(tr * p.g.columns + (int)c, cx + u, ty, sp[s + u]);
                cx += U;
                if (cx == twb) { cx = 0; ++c; }
            }
        }
    }
}

static void sweep_bands_pieces_lanes()
{
    struct Case { int W, H, xs, ys; avifgpu_grid g; };
    const Case cases[] = {
        { 37, 23, 1, 1, { 3, 2, 14, 12 } }, { 37, 23, 1, 1, { 19, 12, 2, 2 } }, { 70, 41, 1, 0, { 3, 3, 32, 16 } }, { 67, 45, 0, 0, { 3, 3, 32, 16 } },
        { 5, 3, 1, 1, { 1, 1, 9, 7 } }, { 31, 9, 0, 0, { 2, 2, 16, 5 } }, { 17, 6, 0, 0, { 2, 1, 16, 6 } }, { 33, 7, 1, 1, { 2, 1, 32, 7 } }, { 1, 1, 1, 1, { 1, 1, 1, 1 } },
    };
    const int bs[] = { 1, 2, 3, 4, 6, 8 };
    for (const Case& k : cases) {
        CHECK(grid_save_illegal(k.W, k.H, k.xs, k.ys, k.g) == nullptr);
        for (int b : bs) for (int chroma = 0; chroma < 2; ++chroma) {
            if (chroma && (b > 2 || (!k.xs && !k.ys))) continue;
            // row cuts: whole, bands of 2, an uneven list (even starts where rows are subsampled)
            std::vector<std::vector<int>> cuts;
            cuts.push_back({ 0, k.H });
            std::vector<int> two; for (int r = 0; r < k.H; r += 2) two.push_back(r); two.push_back(k.H); cuts.push_back(two);
            std::vector<int> odd = { 0 }; const int steps[] = { 6, 2, 14, 4, 10 }; for (int i = 0; odd.back() < k.H; ++i) odd.push_back(odd.back() + steps[i % 5] < k.H ? odd.back() + steps[i % 5] : k.H); cuts.push_back(odd);
            for (int model = 0; model < 2; ++model) for (const std::vector<int>& cut : cuts) {
                Plane p(k.g, k.W, k.H, chroma != 0, k.xs, k.ys, b);
                int next = 0, pad_rows_seen = 0;
                for (size_t i = 0; i + 1 < cut.size(); ++i) {
                    const GridBand bd = grid_save_band(k.g, k.H, cut[i], cut[i + 1] - cut[i], p.ys, p.pw, p.tw, p.th);
                    CHECK(bd.y0 == next && bd.rows >= 1 && bd.pad_cols == k.g.columns * p.tw - p.pw && bd.pad_cols >= 0 && bd.pad_cols < p.tw);
                    next = bd.y0 + bd.rows;
                    CHECK((bd.pad_rows != 0) <= (cut[i + 1] == k.H));
                    if (cut[i + 1] == k.H) { CHECK(next == p.ph && bd.pad_rows == k.g.rows * p.th - p.ph && bd.pad_rows >= 0 && bd.pad_rows < p.th); pad_rows_seen = 1; }
                    if (model == 0) model_pieces(p, bd); else model_lanes(p, bd);
                }
                CHECK(pad_rows_seen == 1);
                p.verify();
            }
        }
    }
}

// ---- avifgpu_grid_fit against a brute-force search -----------------------------------------------------------------------------------------
static void sweep_fit()
{
    const int caps[] = { 1, 2, 3, 16, 17, 64, 100, 300, 4096 }, aligns[] = { 1, 2, 3, 16, 64 };
    for (int size = 1; size <= 300; ++size) for (int cap : caps) for (int align : aligns) for (int sub = 0; sub < 2; ++sub) {
        int n = -1, t = -1;
        const bool ok = grid_fit_side(size, cap, align, sub != 0, n, t);
        int bn = -1, bt = -1;
        for (int c = 1; c <= 256 && bn < 0; ++c) {
            const int a = (sub && c > 1 && (align & 1)) ? align * 2 : align;
            for (int m = a; m <= cap; m += a) if ((int64_t)m * c >= size) { bn = c; bt = m; break; }
        }
        CHECK(ok == (bn > 0));
        if (!ok) continue;
        CHECK(n == bn && t == bt && t % align == 0 && t <= cap && (int64_t)n * t >= size && (int64_t)(n - 1) * t < size);
        CHECK(!(sub && n > 1) || t % 2 == 0);
    }
    int n, t;
    CHECK(!grid_fit_side(257 * 4, 4, 1, false, n, t) && grid_fit_side(256 * 4, 4, 1, false, n, t) && n == 256 && t == 4);
    CHECK(grid_fit_side(0x7fffffff, 0x7fffffff, 64, true, n, t) && n == 2 && t == 0x40000000);   // the one multiple of 64 that covers it alone exceeds the cap (64-bit arithmetic)
    CHECK(grid_fit_side(0x7fffffff, 0x7fffffff, 1, true, n, t) && n == 1 && t == 0x7fffffff);
    CHECK(!grid_fit_side(0, 4, 1, false, n, t) && !grid_fit_side(4, 0, 1, false, n, t) && !grid_fit_side(4, 4, 0, false, n, t));
}

// ---- the payload and its parser ------------------------------------------------------------------------------------------------------------
static void sweep_payload()
{
    const int sizes[] = { 1, 2, 255, 65535, 65536, 70000, 0x7fffffff };
    for (int cols : { 1, 2, 16, 256 }) for (int rows : { 1, 3, 256 }) for (int w : sizes) for (int h : sizes) {
        const avifgpu_grid g = { cols, rows, 64, 64 };
        const int want = (w > 65535 || h > 65535) ? 12 : 8;
        for (int cap = 0; cap <= 13; ++cap) {
            uint8_t* buf = (uint8_t*)malloc(cap ? cap : 1);      // exact size: one byte too far is the sanitizer's
            const int n = grid_payload(g, w, h, buf, cap);
            CHECK(n == (cap >= want ? want : 0));
            if (n) {
                int32_t r, c, ow, oh;
                CHECK(grid_parse(buf, n, r, c, ow, oh) && r == rows && c == cols && ow == w && oh == h);
                CHECK((buf[1] & 1) == (want == 12));
            }
            free(buf);
        }
    }
    uint8_t buf[12];
    const avifgpu_grid bad = { 257, 1, 4, 4 }, ok = { 1, 1, 4, 4 };
    CHECK(grid_payload(bad, 4, 4, buf, 12) == 0 && grid_payload(ok, 0, 4, buf, 12) == 0 && grid_payload(ok, 4, 4, nullptr, 12) == 0 && grid_payload(ok, 4, 4, buf, 12) == 8);
}

int main()
{
    sweep_legality();
    sweep_bands_pieces_lanes();
    sweep_fit();
    sweep_payload();
    printf("grid_save_geometry_check: %lld checks passed\n", g_checks);
    return 0;
}
