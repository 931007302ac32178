"""The definition of the grid save (include/avifgpu.h "grid save") as numpy: the padded plane Q is the canvas plane replicated at its
right and bottom edge, pixel by pixel, and the tiles are Q cut on the tile lattice.  Shared by the CPU and the GPU tests.

Planes are what harness.oracle_write / harness.gpu_write return: {plane: (rows, samples) array}; an interleaved AVIFGPU_OUT_REFERENCE
colour plane has `planes` samples to a pixel."""
import numpy as np

import harness

pkg = harness.pkg


def shifts(desc):
    """the chroma shifts of AVIFGPU_OUT_YCBCR output, (0, 0) otherwise"""
    return harness.chroma_shift(desc.chroma) if desc.output == pkg.OUT_YCBCR else (0, 0)


def geometry(desc, grid):
    """{plane: (pw, ph, tw_p, th_p, samples per pixel)} in pixels, for every plane the save writes"""
    cols, rows, tw, th = grid
    xs, ys = shifts(desc)
    out = {}
    for pl in harness.write_planes(desc):
        chroma = desc.output == pkg.OUT_YCBCR and pl in (1, 2)
        spp = desc.planes if (desc.output == pkg.OUT_REFERENCE and desc.planes >= 3) else 1
        if chroma:
            out[pl] = ((desc.width + xs) >> xs, (desc.height + ys) >> ys, (tw + xs) >> xs, (th + ys) >> ys, spp)
        else:
            out[pl] = (desc.width, desc.height, tw, th, spp)
    return out


def legal(desc, grid):
    """the legality rule of a save, restated: (ok, which rule fails)"""
    cols, rows, tw, th = grid
    xs, ys = shifts(desc)
    if not (1 <= cols <= 256 and 1 <= rows <= 256):
        return False, "1..256"
    if tw < 1 or th < 1:
        return False, "bad tile size"
    if cols * tw < desc.width or rows * th < desc.height:
        return False, "do not cover"
    if xs and cols > 1 and tw % 2:
        return False, "odd tile_width"
    if ys and rows > 1 and th % 2:
        return False, "odd tile_height"
    if (cols - 1) * tw >= desc.width or (rows - 1) * th >= desc.height:
        return False, "not minimal"
    return True, ""


def pad(planes, desc, grid):
    """{plane: Q_pl}: Q_pl[y, x] = P_pl[min(y, ph - 1), min(x, pw - 1)] over (rows * th_p) x (columns * tw_p) pixels"""
    cols, rows, _, _ = grid
    out = {}
    for pl, (pw, ph, twp, thp, spp) in geometry(desc, grid).items():
        P = np.asarray(planes[pl])[:ph, :pw * spp].reshape(ph, pw, spp)
        yy = np.minimum(np.arange(rows * thp), ph - 1)
        xx = np.minimum(np.arange(cols * twp), pw - 1)
        out[pl] = np.ascontiguousarray(P[yy][:, xx].reshape(rows * thp, cols * twp * spp))
    return out


def split(padded, desc, grid):
    """the tiles of padded planes: a row-major list of {plane: (th_p, tw_p * samples per pixel) array}"""
    cols, rows, _, _ = grid
    geo = geometry(desc, grid)
    tiles = []
    for k in range(cols * rows):
        c, r = k % cols, k // cols
        tiles.append({pl: np.ascontiguousarray(padded[pl][r * thp:(r + 1) * thp, c * twp * spp:(c + 1) * twp * spp])
                      for pl, (pw, ph, twp, thp, spp) in geo.items()})
    return tiles


def tiles_of(planes, desc, grid):
    return split(pad(planes, desc, grid), desc, grid)


def scratch_formula(desc, nrows):
    """avifgpu_write_grid_scratch_bytes as the header states it"""
    if nrows < 1:
        return 0
    ssz = 2 if desc.bit_depth > 8 else 1
    total = 256
    for pl, (w, xs, ys) in harness.write_planes(desc).items():
        total += harness.align(w * ssz, 256) * ((nrows + ys) >> ys)
    return total
