"""The definition of the grid open (include/avifgpu.h "grid open") as numpy: the assembled planes of a grid image are np.block of the
tiles' planes, cut to the canvas; everything behind that is the cropped open's own truth (tests/crop_truth.py).  Shared by the CPU and the
GPU tests."""
import numpy as np

import harness

pkg = harness.pkg


def shifts(desc):
    """the chroma shifts where they subsample planes (YCbCr), (0, 0) otherwise"""
    return harness.chroma_shift(desc.chroma) if desc.colorspace == pkg.COLORSPACE_YCBCR else (0, 0)


def plane_extents(desc, grid):
    """{plane: (canvas columns, canvas rows, tile columns, tile rows)} in samples, for every used plane"""
    cols, rows, tw, th = grid
    xs, ys = shifts(desc)
    out = {}
    for pl in harness.read_planes(desc):
        chroma = desc.colorspace == pkg.COLORSPACE_YCBCR and pl in (1, 2)
        if chroma:
            out[pl] = ((desc.width + xs) >> xs, (desc.height + ys) >> ys, (tw + xs) >> xs, (th + ys) >> ys)
        else:
            out[pl] = (desc.width, desc.height, tw, th)
    return out


def legal(desc, grid):
    """the legality rule, restated"""
    cols, rows, tw, th = grid
    xs, ys = shifts(desc)
    if not (1 <= cols <= 256 and 1 <= rows <= 256) or tw < 1 or th < 1 or desc.width < 1 or desc.height < 1:
        return False
    if cols * tw < desc.width or rows * th < desc.height:
        return False
    if xs and cols > 1 and tw % 2:
        return False
    if ys and rows > 1 and th % 2:
        return False
    return True


def visible(desc, grid, k):
    cols, rows, tw, th = grid
    return (k % cols) * tw < desc.width and (k // cols) * th < desc.height


def assemble(tiles, desc, grid):
    """{plane: (rows, columns) array}: np.block of the tiles' planes, cut to the canvas.  tiles[k][plane] is a (th_p, >= tw_p) array; a tile
    with no visible sample may be None."""
    cols, rows, _, _ = grid
    out = {}
    for pl, (cw, ch, twp, thp) in plane_extents(desc, grid).items():
        dt = next(t[pl].dtype for t in tiles if t is not None)
        blank = np.zeros((thp, twp), dtype=dt)
        block = [[tiles[r * cols + c][pl][:thp, :twp] if tiles[r * cols + c] is not None else blank for c in range(cols)] for r in range(rows)]
        out[pl] = np.ascontiguousarray(np.block(block)[:ch, :cw])
    return out


def split(planes, desc, grid, rng, base_offsets=(0, 1, 3), drop_invisible=True):
    """Cut assembled planes ({plane: (rows, >= columns) array}) into tiles: a list of {plane: (th_p, tw_p) VIEW} in row-major order, None
    for a tile with no visible sample (drop_invisible).  Every tile plane has a stride of its own and starts base_offsets[k % 3] samples into
    its buffer, so views are not contiguous and not aligned; the invisible part of edge tiles is random."""
    cols, rows, _, _ = grid
    ext = plane_extents(desc, grid)
    tiles = []
    for k in range(cols * rows):
        if drop_invisible and not visible(desc, grid, k):
            tiles.append(None)
            continue
        c, r = k % cols, k // cols
        t = {}
        for pl, (cw, ch, twp, thp) in ext.items():
            a = planes[pl]
            ssz = a.dtype.itemsize
            stride = (twp + 1 + (k * 5 + pl * 3) % 11) * ssz              # bytes; differs from tile to tile and plane to plane
            off = base_offsets[k % len(base_offsets)] * ssz                # off the 16-byte grid; samples stay naturally aligned
            raw = rng.integers(0, 256, size=(off + thp * stride + 16,), dtype=np.uint8)
            view = np.lib.stride_tricks.as_strided(raw[off:].view(a.dtype), shape=(thp, twp), strides=(stride, ssz))
            y0, x0 = r * thp, c * twp
            part = a[y0:min(y0 + thp, ch), x0:min(x0 + twp, cw)]
            view[:part.shape[0], :part.shape[1]] = part
            t[pl] = view
        tiles.append(t)
    return tiles


def tile_table(tiles, desc, grid, address=lambda a: a.ctypes.data):
    """A ctypes array of GridTile records for tiles as split() returns them; address(view) is the pointer to record for it."""
    table = (pkg.GridTile * len(tiles))()
    for k, t in enumerate(tiles):
        if t is None:
            continue
        for pl, a in t.items():
            table[k].plane[pl] = address(a)
            table[k].stride[pl] = a.strides[0]
    return table
