// grid_geometry.h -- the arithmetic of the grid open (include/avifgpu.h "grid open"): which grids are legal, the extent of a
// tile in each plane, the ImageGrid payload, and the PIECES -- one per intersecting tile -- that cover a rectangle of an assembled plane.
// Plain integer arithmetic shared by csrc/grid_kernels.hip (the host path copies piece by piece; the kernel computes the same per lane) and
// a stand-alone host program (tools/grid_geometry_check.cpp) that sweeps it under the sanitizers: no HIP type, no device call.
#pragma once
#include <stdint.h>

#include "../../include/avifgpu.h"

namespace avifgpu {

constexpr int kGridMaxSide = 256;                // rows_minus_one / columns_minus_one are 8-bit fields

// ---- legality (ISO 23008-12 6.6.2.3, and what the assembled chroma planes need) ---------------------------------------------------------
// xs / ys: the chroma shifts of a subsampled YCbCr image, 0 otherwise.  A tile's chroma plane has (tile_width + xs) >> xs columns; only for
// an even tile_width does chroma column x of the canvas lie in tile column x / (tile_width >> 1) for every x -- a single column of tiles
// has no seam and may be odd.  Rows alike.  nullptr: legal; otherwise what is wrong.
inline const char* grid_illegal(int width, int height, int xs, int ys, const avifgpu_grid& g)
{
    if (width < 1 || height < 1) return "bad canvas size";
    if (g.columns < 1 || g.columns > kGridMaxSide || g.rows < 1 || g.rows > kGridMaxSide) return "columns and rows must be 1..256";
    if (g.tile_width < 1 || g.tile_height < 1) return "bad tile size";
    if ((int64_t)g.columns * g.tile_width < width || (int64_t)g.rows * g.tile_height < height) return "the tiles do not cover the canvas";
    if (xs && g.columns > 1 && (g.tile_width & 1)) return "an odd tile_width with subsampled columns and more than one column of tiles";
    if (ys && g.rows > 1 && (g.tile_height & 1)) return "an odd tile_height with subsampled rows and more than one row of tiles";
    return nullptr;
}

// the extent of a tile, in samples, in a luma-like (chroma == false) or a chroma plane
inline int grid_tile_w(const avifgpu_grid& g, bool chroma, int xs) { return chroma ? (g.tile_width + xs) >> xs : g.tile_width; }
inline int grid_tile_h(const avifgpu_grid& g, bool chroma, int ys) { return chroma ? (g.tile_height + ys) >> ys : g.tile_height; }

// a tile with no visible sample is never read
inline bool grid_tile_visible(const avifgpu_grid& g, int width, int height, int tile)
{
    const int c = tile % g.columns, r = tile / g.columns;
    return (int64_t)c * g.tile_width < width && (int64_t)r * g.tile_height < height;
}

// ---- the ImageGrid payload: version(8) = 0, flags(8), rows_minus_one(8), columns_minus_one(8), output_width, output_height as 16 bits each
// or, with flags & 1, 32 bits each; big-endian; trailing bytes ignored.  false: a null or short payload, a version other than 0, a zero
// size, a size above INT32_MAX.
inline bool grid_parse(const uint8_t* p, int64_t size, int32_t& rows, int32_t& columns, int32_t& out_w, int32_t& out_h)
{
    if (!p || size < 8 || p[0] != 0) return false;
    const bool wide = (p[1] & 1) != 0;
    if (wide && size < 12) return false;
    uint32_t w, h;
    if (wide) {
        w = (uint32_t)p[4] << 24 | (uint32_t)p[5] << 16 | (uint32_t)p[6] << 8 | p[7];
        h = (uint32_t)p[8] << 24 | (uint32_t)p[9] << 16 | (uint32_t)p[10] << 8 | p[11];
    } else {
        w = (uint32_t)p[4] << 8 | p[5];
        h = (uint32_t)p[6] << 8 | p[7];
    }
    if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) return false;
    rows = p[2] + 1; columns = p[3] + 1; out_w = (int32_t)w; out_h = (int32_t)h;
    return true;
}

// ---- pieces: rectangle [x0, x0 + w) x [y0, y0 + h) of an assembled plane whose tiles are tw x th samples of s bytes, `columns` to a row ----
// Piece = `rows` rows of `bytes` bytes: from byte src_x of row src_y of the tile's plane to byte dst_x of row dst_y of the rectangle.
// The caller has checked 0 <= x0, y0, 1 <= w, h and that the rectangle lies inside the plane, so every tile index is inside the table.
struct GridPiece { int tile; int64_t src_x; int src_y; int64_t dst_x; int dst_y; int64_t bytes; int rows; };

template <class F>
inline void grid_pieces(int columns, int tw, int th, int s, int x0, int y0, int w, int h, F&& each)
{
    for (int y = y0; y < y0 + h;) {
        const int tr = y / th, ty = y - tr * th;
        const int ny = (th - ty < y0 + h - y) ? th - ty : y0 + h - y;
        for (int x = x0; x < x0 + w;) {
            const int tc = x / tw, tx = x - tc * tw;
            const int nx = (tw - tx < x0 + w - x) ? tw - tx : x0 + w - x;
            const GridPiece p = { tr * columns + tc, (int64_t)tx * s, ty, (int64_t)(x - x0) * s, y - y0, (int64_t)nx * s, ny };
            each(p);
            x += nx;
        }
        y += ny;
    }
}

// ---- scratch of a MEM_DEVICE call (avifgpu_read_grid_scratch_bytes has the formula in words) ---------------------------------------------
// What is gathered for a source region of sw x sh samples is the cropped open's STAGED rectangle (crop_geometry.h): the region, the
// covering row / column or the bilinear halo, and up to 31 columns in front of it.  (sw + 38) x (sh + 6), cut to the canvas, bounds it.
constexpr int kGridStageColumns = 38, kGridStageRows = 6;
inline int grid_stage_bound(int n, int extra, int size) { return (int64_t)n + extra < size ? n + extra : size; }

} // namespace avifgpu
