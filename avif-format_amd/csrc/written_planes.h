// written_planes.h -- what launch_thumbnail and launch_summary (thumbnail_kernels.hip, summary_kernels.hip) share on the host: the planes
// of a tile's written output, the rule that cuts their rows into bands, and the plane checks of the two probe entries.  Host code only.
#pragma once
#include <algorithm>

#include "staging.h"

namespace avifgpu {

inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// width / height of output channel c of the whole image, and the smallest over the channels
inline bool channel_extent(const avifgpu_write_desc* d, const WriteGeom& g, int c, int& pw, int& ph)      // true: a chroma plane
{
    const bool chroma = d->output == AVIFGPU_OUT_YCBCR && (c == 1 || c == 2);
    pw = chroma ? (d->width + g.xs) >> g.xs : d->width;
    ph = chroma ? (d->height + g.ys) >> g.ys : d->height;
    return chroma;
}
inline void smallest_plane(const avifgpu_write_desc* d, const WriteGeom& g, int& pw, int& ph)
{
    pw = d->width; ph = d->height;
    if (d->output == AVIFGPU_OUT_YCBCR) channel_extent(d, g, 1, pw, ph);
}

// One plane that the conversion of rows [row0, row0 + nrows) wrote: planes[plane] / stride[plane] as that kernel was given them (at the
// tile's first row), c0 = the channel of its first sample in the statistics (R,G,B[,A] | Y[,A] | Y,Cb,Cr[,A]), pw x ph = the WHOLE plane,
// prow0 / prows = the tile's plane rows, aligned = base and stride are multiples of 16.
struct WrittenPlane { int plane, c0, pw, ph, prow0, prows; bool aligned; };
// The interleaved reference is one plane of d->planes channels; gray and Y/Cb/Cr come one channel per plane, alpha last in plane 3.
inline int written_planes(const avifgpu_write_desc* d, const WriteGeom& g, int row0, int nrows, const uint8_t* const planes[4],
                          const int64_t stride[4], WrittenPlane out[4])
{
    int n = 0;
    auto add = [&](int plane, int c0) {
        WrittenPlane& t = out[n++];
        const bool chroma = channel_extent(d, g, c0, t.pw, t.ph);
        t.plane = plane; t.c0 = c0;
        t.prow0 = chroma ? row0 >> g.ys : row0;
        t.prows = chroma ? (nrows + g.ys) >> g.ys : nrows;
        t.aligned = ((reinterpret_cast<uintptr_t>(planes[plane]) | (uintptr_t)stride[plane]) & 15) == 0;
    };
    if (d->output == AVIFGPU_OUT_REFERENCE) { add(0, 0); if (!g.color && g.alpha) add(3, 1); }
    else { add(0, 0); add(1, 1); add(2, 2); if (g.alpha) add(3, 3); }
    return n;
}

// Plane rows per workgroup of a grid of gx column blocks x bands x nslots planes: about 8192 workgroups over all planes -- several rounds of
// what the chip holds at once, so that the last round's ragged end is a small part of the run -- but at least 8 rows each, so that a lane's
// loads stay in flight four deep, and no more bands than grid.y allows.
inline int64_t band_rows_for(int gx, int nslots, int max_rows)
{
    const int64_t bands_wanted = std::max<int64_t>(1, 8192 / ((int64_t)gx * nslots));
    const int64_t band_rows = std::max<int64_t>(8, ceil_div64(max_rows, bands_wanted));
    return std::max<int64_t>(band_rows, ceil_div64(max_rows, 65535));
}

// avifgpu_probe_thumbnail / avifgpu_probe_summary (`who`): every plane the descriptor writes is there and wide enough; pp = the planes as bytes
inline int check_probe_planes(const char* who, const avifgpu_write_desc* d, const WriteGeom& g, const void* const planes[4],
                              const int64_t stride[4], const uint8_t* pp[4])
{
    for (int pl = 0; pl < 4; ++pl) {
        pp[pl] = static_cast<const uint8_t*>(planes[pl]);
        if (!write_plane_used(d, g, pl)) continue;
        int rows; int64_t rb; write_plane_extent(d, g, pl, d->height, rows, rb);
        if (!pp[pl] || stride[pl] < rb) return fail(AVIFGPU_formatBadParameters, "%s: plane %d is null or its stride too small", who, pl);
    }
    return 0;
}

} // namespace avifgpu
