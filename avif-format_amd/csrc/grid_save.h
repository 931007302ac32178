// grid_save.h -- what grid_save_kernels.hip offers pipeline.hip: the geometry of one plane of a grid save's band from the write
// descriptor, and the launch of the in-place padding kernel.  Internal; include/avifgpu.h "grid save" is the public surface.
#pragma once
#include "staging.h"
#include "grid_save_geometry.h"

namespace avifgpu {

// Plane pl of the band canvas rows [row0, row0 + nrows) write: pw valid pixels of b bytes a row, tiles of tw x th pixels, full_bytes =
// bytes of a padded row (columns * tw * b).
struct GridSavePlane { int pw, b, tw, th; GridBand band; int64_t full_bytes; };
void grid_save_plane(const avifgpu_write_desc* d, const WriteGeom& g, const avifgpu_grid& grid, int pl, int row0, int nrows, GridSavePlane& out);

// Every used plane of every tile of a HOST table: 0, or formatBadParameters with a message for a null table, a NULL pointer, a stride below
// tw_p * b, or 16-bit samples at an odd address or stride.  Whoever hands a GridDest to write_tile_enqueue / write_rows_host calls this first.
int check_grid_tiles(const avifgpu_write_desc* d, const WriteGeom& g, const avifgpu_grid& grid, const avifgpu_grid_tile* tiles, const char* who);

// Fill the pad columns and pad rows of the planes with base[pl] != nullptr in place (grid_pad), behind the launch_write() that wrote their
// band rows on `st`: a plane is band.rows + band.pad_rows rows of at least full_bytes at pitch[pl].
hipError_t launch_grid_pad(const GridSavePlane gp[4], uint8_t* const base[4], const int64_t pitch[4], hipStream_t st);

} // namespace avifgpu
