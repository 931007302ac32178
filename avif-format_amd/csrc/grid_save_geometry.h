// grid_save_geometry.h -- the arithmetic of the grid save (include/avifgpu.h "grid save"): which grids a save takes, the
// band of plane rows a row range writes with its pad columns and pad rows, the PIECES -- one per intersecting tile -- that cover a band,
// the rule of avifgpu_grid_fit and the ImageGrid payload.  Plain integer arithmetic shared by csrc/grid_save_kernels.hip, csrc/pipeline.hip
// (the host path copies a band down piece by piece) and a stand-alone host program (tools/grid_save_geometry_check.cpp) that sweeps it
// under the sanitizers: no HIP type, no device call.
#pragma once
#include <stdint.h>

#include "grid_geometry.h"

namespace avifgpu {

// ---- legality: grid_illegal(), and every tile has a visible sample (the MINIMAL grid) ------------------------------------------------------
// Then every sample of every tile is written exactly once per save: an encoder is never handed a tile nobody wrote.
inline const char* grid_save_illegal(int width, int height, int xs, int ys, const avifgpu_grid& g)
{
    if (const char* why = grid_illegal(width, height, xs, ys, g)) return why;
    if ((int64_t)(g.columns - 1) * g.tile_width >= width) return "not minimal: the last column of tiles has no visible sample";
    if ((int64_t)(g.rows - 1) * g.tile_height >= height) return "not minimal: the last row of tiles has no visible sample";
    return nullptr;
}

// ---- the band of one plane that canvas rows [row0, row0 + nrows) write ---------------------------------------------------------------------
// The plane holds pw x ph pixels (ys: its row shift, 0 for luma-like planes), a tile of it tw_p x th_p, the padded plane
// (columns * tw_p) x (rows * th_p).  The band is plane rows [y0, y0 + rows); every band row has pad_cols pixels right of pw, each the
// row's pixel pw - 1; the band whose range ends at `height` also has pad_rows rows below it, each row y0 + rows - 1 (== ph - 1) again,
// pad columns included.  row0 is even where ys is 1 (avifgpu_write_rows' own rule), so the bands of a save tile the padded plane.
struct GridBand { int y0, rows, pad_cols, pad_rows; };
inline GridBand grid_save_band(const avifgpu_grid& g, int height, int row0, int nrows, int ys, int pw, int tw_p, int th_p)
{
    GridBand b;
    b.y0 = row0 >> ys;
    b.rows = (nrows + ys) >> ys;
    b.pad_cols = g.columns * tw_p - pw;
    b.pad_rows = (nrows > 0 && (int64_t)row0 + nrows == height) ? g.rows * th_p - ((height + ys) >> ys) : 0;
    return b;
}

// The pieces that cover a band and its pad rows: grid_pieces with source and destination swapped -- a piece's src_x / src_y are where it
// goes in ITS TILE's plane (bytes, row), dst_x / dst_y where it comes from in the band buffer (bytes from the row's start, row of the band).
template <class F>
inline void grid_save_pieces(const avifgpu_grid& g, const GridBand& b, int tw_p, int th_p, int pixel_bytes, F&& each)
{
    if (b.rows + b.pad_rows < 1) return;
    grid_pieces(g.columns, tw_p, th_p, pixel_bytes, 0, b.y0, g.columns * tw_p, b.rows + b.pad_rows, each);
}

// ---- avifgpu_grid_fit: one direction ---------------------------------------------------------------------------------------------------------
// count = the smallest number of tiles for which some multiple of `align` is at most max_tile and at least ceil(size / count); tile = the
// smallest such multiple.  align is raised to even where the direction is subsampled and count > 1.  false: no count in 1..256 has one.
// The result is minimal: were (count - 1) * tile >= size, tile -- a multiple of the align of count - 1 too -- would have qualified count - 1.
inline bool grid_fit_side(int size, int max_tile, int align, bool subsampled, int& count, int& tile)
{
    if (size < 1 || max_tile < 1 || align < 1) return false;
    for (int n = 1; n <= kGridMaxSide; ++n) {
        const int64_t a = (subsampled && n > 1 && (align & 1)) ? (int64_t)align * 2 : align;
        const int64_t need = ((int64_t)size + n - 1) / n;
        const int64_t t = (need + a - 1) / a * a;
        if (t <= max_tile) { count = n; tile = (int)t; return true; }
    }
    return false;
}

// ---- the ImageGrid payload: the inverse of grid_parse.  8 bytes, or 12 with flags bit 0 where a size exceeds 65 535; 0: it does not fit ----
inline int grid_payload(const avifgpu_grid& g, int32_t out_w, int32_t out_h, uint8_t* p, int64_t capacity)
{
    if (!p || out_w < 1 || out_h < 1 || g.rows < 1 || g.rows > kGridMaxSide || g.columns < 1 || g.columns > kGridMaxSide) return 0;
    const bool wide = out_w > 65535 || out_h > 65535;
    const int n = wide ? 12 : 8;
    if (capacity < n) return 0;
    p[0] = 0; p[1] = wide ? 1 : 0; p[2] = (uint8_t)(g.rows - 1); p[3] = (uint8_t)(g.columns - 1);
    const uint32_t w = (uint32_t)out_w, h = (uint32_t)out_h;
    if (wide) {
        p[4] = (uint8_t)(w >> 24); p[5] = (uint8_t)(w >> 16); p[6] = (uint8_t)(w >> 8); p[7] = (uint8_t)w;
        p[8] = (uint8_t)(h >> 24); p[9] = (uint8_t)(h >> 16); p[10] = (uint8_t)(h >> 8); p[11] = (uint8_t)h;
    } else {
        p[4] = (uint8_t)(w >> 8); p[5] = (uint8_t)w; p[6] = (uint8_t)(h >> 8); p[7] = (uint8_t)h;
    }
    return n;
}

// ---- the lane model of grid_scatter<B> (grid_save_kernels.hip), in host terms ----------------------------------------------------------------
// A padded plane row is columns * tw_p * B bytes; lane k owns bytes [16 k, 16 k + 16) of it.  Where those lie inside one tile AND inside the
// pw * B bytes a source row holds, the lane moves them as one 16-byte word; everywhere else -- a seam, the row's tail, the padding, a tile
// narrower than 16 bytes -- it places units of U bytes (U = 2 for the 16-bit pixel sizes 2, 6, 8, else 1), each from the source pixel
// min(pixel, pw - 1).  Source row = min(row, src_rows - 1) of the band buffer.
inline int grid_scatter_unit(int pixel_bytes) { return (pixel_bytes == 2 || pixel_bytes == 6 || pixel_bytes == 8) ? 2 : 1; }
inline bool grid_scatter_whole(int64_t off, int64_t tile_row_bytes, int64_t total, int64_t valid)
{
    const int64_t tx = off % tile_row_bytes;
    return off + 16 <= total && tx + 16 <= tile_row_bytes && off + 16 <= valid;
}
// the source byte of padded-row byte v
inline int64_t grid_scatter_source(int64_t v, int pixel_bytes, int pw)
{
    const int64_t pix = v / pixel_bytes, w = v - pix * pixel_bytes;
    return (pix < pw ? pix : pw - 1) * pixel_bytes + w;
}

} // namespace avifgpu
