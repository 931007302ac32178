"""The grid open on the GPU (include/avifgpu.h "grid open", csrc/grid_kernels.hip).

The definition is exact: the grid open IS avifgpu_read_rows_cropped on the planes np.block assembles from the tiles (tests/grid_truth.py).
Every comparison is array_equal on bytes: the gather kernel alone against numpy; the entry against the GPU's own cropped open of the
assembled planes at every depth and, at depths 8 and 16, also against the oracle through the truths tests/test_gpu_crop.py uses.

Shapes are the smallest at which the code as built can go wrong: a lane of grid_gather owns 16 destination bytes, a wave 1 KiB, a
workgroup 4 KiB; a lane takes the one-load path only where its 16 bytes lie inside one tile, so tiles narrower than 16 bytes, seams off and
on the 16-byte grid, row tails below 16 bytes and more rows than grid.y holds are each a path of their own.

The file sorts behind every other test file, as the suite's other late additions do, so that no earlier test's place in the run moves."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import grid_truth
import harness
from fake_host import FakeHost
from test_gpu_crop import check, helper_tiles, open_cropped, refs, same
from upsample_truth import CENTER, LEFT, NEAREST

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
BAD = pkg.formatBadParameters


def root(view):
    """the buffer a tile plane of grid_truth.split() is a view into"""
    while view.base is not None:
        view = view.base
    return view


class DeviceTiles:
    """The tiles of grid_truth.split() in device memory -- one upload: every tile plane's buffer at a 256-byte slot, so its view keeps the
    offset from the 16-byte grid it has on the host -- and their table of device pointers, in device memory too."""

    def __init__(self, gpu, tiles, desc, grid):
        import torch
        dev = f"cuda:{gpu.device}"
        slots, at = {}, 0
        for t in tiles:
            for a in (t or {}).values():
                slots[id(a)] = at
                at += harness.align(root(a).size, 256)
        flat = np.zeros((max(at, 256),), dtype=np.uint8)
        for t in tiles:
            for a in (t or {}).values():
                flat[slots[id(a)]:slots[id(a)] + root(a).size] = root(a)
        self.data = torch.from_numpy(flat).to(dev)
        base = self.data.data_ptr()
        assert base % 256 == 0
        self.table = grid_truth.tile_table(tiles, desc, grid, address=lambda a: base + slots[id(a)] + a.ctypes.data - root(a).ctypes.data)
        self.dtable = torch.from_numpy(np.frombuffer(bytes(self.table), dtype=np.uint8).copy()).to(dev)
        self.ptr = self.dtable.data_ptr()


def cut_planes(desc, grid, seed, rng):
    """(planes as harness.make_read_source lays them out, their tiles): the assembled planes are the harness's own source, so that the
    existing entries and the oracle take them as they are"""
    planes = harness.make_read_source(desc, seed=seed)
    tiles = grid_truth.split(planes, desc, grid, rng)
    back = grid_truth.assemble(tiles, desc, grid)
    for pl, (w, _, ys) in harness.read_planes(desc).items():
        assert np.array_equal(back[pl], planes[pl][:(desc.height + ys) >> ys, :w])
    return planes, tiles


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("tw,th", [(2, 2), (6, 4), (18, 10), (64, 64), (130, 3)])
def test_gather_alone_against_numpy(gpu, S, tw, th):
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(tw * 7 + S)
    cols = min(256, (17 + 4200 // S) // tw + 2)                  # as wide as the probe's 256 columns allow, or a second workgroup and more
    rows = 3
    # a canvas whose last column and last row of tiles is only partly visible
    d = pkg.ReadDesc(width=cols * tw - tw // 2, height=rows * th - th // 2, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME,
                     bit_depth=8 if S == 1 else 12, depth=8 if S == 1 else 16, alpha_state=pkg.ALPHA_NONE)
    grid = (cols, rows, tw, th)
    planes, tiles = cut_planes(d, grid, 3, rng)
    P = planes[0][:, :d.width]
    dt = DeviceTiles(gpu, tiles, d, grid)
    assert len({t[0].strides[0] for t in tiles}) > 1 and any(t[0].ctypes.data % 16 for t in tiles)
    n = 0
    payloads = set()
    for x0, y0, pay in itertools.product((0, 1, tw - 1, tw, 17), (0, th - 1, th), (1, 15, 16, 17, 1024 + 5, 4096 + 40)):
        if x0 >= d.width:
            continue
        w = min(max(pay // S, 1), d.width - x0)
        h = min(d.height - y0, th + 2)
        rb = w * S
        payloads.add(rb)
        pitch = harness.align(rb, 16) + 32                       # destination row padding
        d_dst = torch.full(((h + 2) * pitch,), SENTINEL, dtype=torch.uint8, device=dev)      # a guard row above and one below
        gpu.probe_grid_gather(dt.ptr, cols, 0, tw, th, S, x0, y0, w, h, d_dst.data_ptr() + pitch, pitch, None)
        torch.cuda.synchronize(dev)
        got = d_dst.cpu().numpy().reshape(h + 2, pitch)
        what = (S, tw, th, x0, y0, w, h)
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (what, "guard rows")
        assert (got[1:-1, rb:] == SENTINEL).all(), (what, "bytes beyond the payload")
        want = np.ascontiguousarray(P[y0:y0 + h, x0:x0 + w]).view(np.uint8).reshape(h, rb)
        assert np.array_equal(got[1:-1, :rb], want), what
        n += 1
    assert n >= 60
    if tw >= 18:
        assert max(payloads) > 4096 and any(1024 < p <= 4096 for p in payloads), payloads


# ---- 2. more rows than grid.y holds -------------------------------------------------------------------------------------------------------------
def test_gather_row_wrap(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(257)
    th, nt, w, stride, rows = 257, 256, 8, 11, 65600
    raw = rng.integers(0, 256, size=(nt, th, stride), dtype=np.uint8)
    d_raw = torch.from_numpy(raw).to(dev)
    table = (pkg.GridTile * nt)()
    for k in range(nt):
        table[k].plane[0] = d_raw.data_ptr() + k * th * stride
        table[k].stride[0] = stride
    d_table = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    pitch = 16
    d_dst = torch.full(((rows + 2) * pitch,), SENTINEL, dtype=torch.uint8, device=dev)
    gpu.probe_grid_gather(d_table.data_ptr(), 1, 0, w, th, 1, 0, 0, w, rows, d_dst.data_ptr() + pitch, pitch, None)
    torch.cuda.synchronize(dev)
    got = d_dst.cpu().numpy().reshape(rows + 2, pitch)
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all() and (got[:, w:] == SENTINEL).all()
    assert np.array_equal(got[1:-1, :w], raw[:, :, :w].reshape(nt * th, w)[:rows])


# ---- 3 / 4. the entry ---------------------------------------------------------------------------------------------------------------------------
def _pq(**kw):
    return dict(transfer_characteristics=pkg.TC_PQ, color_primaries=pkg.PRIMARIES_BT2020, matrix_coefficients=pkg.MATRIX_BT2020_NCL, pq_peak_nits=1000, has_nclx=1, **kw)


FORMATS = [
    ("420-8", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT601)),
    ("422-10-16-alpha", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_422, bit_depth=10, depth=16, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT709)),
    ("444-12-32-pq", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_444, bit_depth=12, depth=32, alpha_state=pkg.ALPHA_NONE, **_pq())),
    ("gray-8", dict(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)),
    ("rgb-10-16-alpha", dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=10, depth=16, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_RGB_GBR)),
]
GRID = (3, 3, 32, 16)
CANVASES = ((70, 46), (67, 45))
RECTS = (None, (33, 17, 30, 20))                                 # whole; one that starts odd and spans seams


def open_grid(gpu, desc, grid, tiles, rect, mode=NEAREST, code=1, mem="device", max_rows=None, pinned=False, pad=16, guard_rows=1):
    """The grid open as (out_h, out_w, C), one call or the helper's tiles of max_rows.  Device: tiles is a DeviceTiles, every call gets
    exactly the scratch helper's bytes and a sentinel region behind them stays untouched.  Host: tiles is what grid_truth.split() returns.
    `pad` bytes beyond each destination row and guard rows above and below must come back untouched."""
    import torch
    r = rect or (0, 0, desc.width, desc.height)
    out_w, out_h = pkg.read_cropped_geometry(desc, r, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16) + pad
    flat = np.full(((out_h + 2 * guard_rows) * stride,), SENTINEL, dtype=np.uint8)
    cuts = list(helper_tiles(desc, r, mode, code, max_rows)) if max_rows else [(0, out_h)]
    if mem == "device":
        dev = f"cuda:{gpu.device}"
        d_out = torch.from_numpy(flat).to(dev)
        needs = [pkg.read_grid_scratch_bytes(desc, grid, rect, mode, code, n) for _, n in cuts]
        tail = 4096
        scratch = torch.full((max(needs) + tail,), 0x5A, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for (o, n), need in zip(cuts, needs):
            gpu.read_rows_grid(desc, grid, tiles.ptr, rect, mode, code, o, n, d_out.data_ptr() + (guard_rows + o) * stride, stride,
                               scratch.data_ptr(), need, mem=pkg.MEM_DEVICE, stream=stream)
        torch.cuda.synchronize(dev)
        assert bool((scratch[max(needs):] == 0x5A).all()), "bytes behind the scratch were touched"
        flat = d_out.cpu().numpy()
    else:
        keep = []
        if pinned:
            moved = []
            for t in tiles:
                if t is None:
                    moved.append(None)
                    continue
                m = {}
                for pl, a in t.items():
                    buf = torch.from_numpy(root(a).copy()).pin_memory()
                    keep.append(buf)
                    m[pl] = np.lib.stride_tricks.as_strided(buf.numpy()[a.ctypes.data - root(a).ctypes.data:].view(a.dtype), shape=a.shape, strides=a.strides)
                moved.append(m)
            tiles = moved
            out = torch.from_numpy(flat).pin_memory()
            keep.append(out)
            flat = out.numpy()
        table = grid_truth.tile_table(tiles, desc, grid)
        for o, n in cuts:
            gpu.read_rows_grid(desc, grid, table, rect, mode, code, o, n, flat.ctypes.data + (guard_rows + o) * stride, stride, mem=pkg.MEM_HOST)
        flat = flat.copy()
    buf = flat.reshape(out_h + 2 * guard_rows, stride)
    body = buf[guard_rows:guard_rows + out_h]
    assert (body[:, row_bytes:] == SENTINEL).all(), "bytes beyond out_w * bytes per pixel were touched"
    assert (buf[:guard_rows] == SENTINEL).all() and (buf[guard_rows + out_h:] == SENTINEL).all(), "rows outside the call were touched"
    return np.ascontiguousarray(body[:, :row_bytes]).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


def modes_of(desc):
    sub = desc.colorspace == pkg.COLORSPACE_YCBCR and desc.chroma in (pkg.CHROMA_420, pkg.CHROMA_422)
    return (NEAREST, CENTER, LEFT) if sub else (NEAREST, CENTER)    # a bilinear mode on anything else is the nearest open: once is enough


_expected = {}


def expected(gpu, desc, planes, rect, mode, code, key):
    """the GPU's own cropped open of the assembled planes, computed once per case and shared"""
    r = rect or (0, 0, desc.width, desc.height)
    k = (key, r, mode, code)
    if k not in _expected:
        want = open_cropped(gpu, desc, planes, r, mode, code)
        if desc.depth != 32:
            check(want, desc, refs(gpu, desc, planes, mode, ("grid",) + key), r, code, (k, "the cropped open against the oracle"))
        want.setflags(write=False)
        _expected[k] = want
    return _expected[k]


_sources = {}


def source(name, kw, size):
    key = (name, size)
    if key not in _sources:
        desc = pkg.ReadDesc(width=size[0], height=size[1], **kw)
        planes, tiles = cut_planes(desc, GRID, size[0] + len(name), np.random.default_rng(size[1]))
        _sources[key] = (desc, planes, tiles)
    return _sources[key] + (key,)


@pytest.mark.parametrize("name,kw", FORMATS, ids=[f[0] for f in FORMATS])
def test_entry_device(gpu, name, kw):
    for size in CANVASES:
        desc, planes, tiles, key = source(name, kw, size)
        dt = DeviceTiles(gpu, tiles, desc, GRID)
        codes = range(1, 9) if (name == "420-8" and size == CANVASES[1]) else (1, 4, 6)
        for rect, mode, code in itertools.product(RECTS, modes_of(desc), codes):
            want = expected(gpu, desc, planes, rect, mode, code, key)
            what = (name, size, rect, mode, code)
            assert same(open_grid(gpu, desc, GRID, dt, rect, mode, code), want), (what, "one call")
            assert same(open_grid(gpu, desc, GRID, dt, rect, mode, code, max_rows=5), want), (what, "tiles of 5 rows")


@pytest.mark.parametrize("name,kw", FORMATS, ids=[f[0] for f in FORMATS])
def test_entry_host(gpu, name, kw):
    size = CANVASES[1]
    desc, planes, tiles, key = source(name, kw, size)
    cases = [(None, NEAREST, 1, None), (RECTS[1], modes_of(desc)[-1], 6, 5), (RECTS[1], NEAREST, 4, None), (None, CENTER, 1, 5)]
    try:
        for nctx in (1, 2):
            g = pkg.AvifGpu(devices=[gpu.device] * nctx)
            for (rect, mode, code, max_rows), pinned in itertools.product(cases, (False, True)):
                want = expected(g, desc, planes, rect, mode, code, key)
                assert same(open_grid(g, desc, GRID, tiles, rect, mode, code, mem="host", max_rows=max_rows, pinned=pinned), want), (name, nctx, rect, mode, code, max_rows, pinned)
    finally:
        pkg.AvifGpu(gpu.device)                                  # the session's binding


def test_entry_one_tile_host_is_the_cropped_open(gpu):
    """A 1 x 1 grid -- the tile may be odd and larger than the canvas -- on host pointers is avifgpu_read_rows_cropped on tile 0; on device
    pointers it gathers, to the same bytes."""
    name, kw = FORMATS[0]
    desc = pkg.ReadDesc(width=37, height=21, **kw)
    grid = (1, 1, 39, 23)
    planes, tiles = cut_planes(desc, grid, 5, np.random.default_rng(5))
    for rect, mode, code in ((None, NEAREST, 1), ((3, 5, 30, 11), CENTER, 6), ((1, 1, 35, 19), NEAREST, 3)):
        want = expected(gpu, desc, planes, rect, mode, code, ("one", 37))
        assert same(open_grid(gpu, desc, grid, tiles, rect, mode, code, mem="host"), want), (rect, mode, code, "host")
        assert same(open_grid(gpu, desc, grid, DeviceTiles(gpu, tiles, desc, grid), rect, mode, code), want), (rect, mode, code, "device")


# ---- 5. the FormatRecord shim ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [FORMATS[0], FORMATS[1]], ids=[FORMATS[0][0], FORMATS[1][0]])
def test_shim_delivers_grid_tiles(gpu, name, kw):
    desc, planes, tiles, key = source(name, kw, CANVASES[1])
    nch = harness.read_channels(desc)
    imgs = (H.Image * len(tiles))()
    for k, t in enumerate(tiles):
        imgs[k].width, imgs[k].height, imgs[k].colorspace, imgs[k].chroma, imgs[k].bit_depth = GRID[2], GRID[3], desc.colorspace, desc.chroma, desc.bit_depth
        for pl, a in (t or {}).items():
            imgs[k].plane[pl] = a.ctypes.data
            imgs[k].stride[pl] = a.strides[0]
    assert desc.has_nclx
    nclx = H.Nclx(desc.color_primaries, desc.transfer_characteristics, desc.matrix_coefficients, desc.full_range_flag)
    g = pkg.Grid(*GRID)
    for rect, mode, code in ((None, NEAREST, 1), (RECTS[1], CENTER, 6)):
        r = rect or (0, 0, desc.width, desc.height)
        out_w, out_h = pkg.read_cropped_geometry(desc, r, code)
        row_bytes = out_w * nch * (desc.depth // 8)
        host = FakeHost(out_w, out_h, desc.depth, nch, max_data=row_bytes * (out_h // 6))
        cr = pkg.CropRect(*r)
        rc = gpu.lib.avifgpu_host_read_heif_image_grid(imgs, ctypes.byref(g), desc.width, desc.height, ctypes.byref(cr) if rect else None, code, mode, desc.alpha_state,
                                                       ctypes.byref(nclx), None, ctypes.byref(host.fr))
        assert rc == 0, gpu.lib.avifgpu_last_error()
        assert same(host.image.reshape(out_h, out_w, nch), expected(gpu, desc, planes, rect, mode, code, key)), (name, rect, mode, code)
        assert len(host.rects) >= 5 and host.rects[0][0] == 0 and host.rects[-1][2] == out_h
        assert all(a[2] == b[0] for a, b in zip(host.rects[:-1], host.rects[1:])) and host.polls == len(host.rects)
        assert [(q[0], q[2] - q[0]) for q in host.rects] == list(helper_tiles(desc, r, mode, code, out_h // 6))
    # a document of the wrong size and an illegal grid deliver nothing
    host = FakeHost(desc.width - 1, desc.height, desc.depth, nch)
    assert gpu.lib.avifgpu_host_read_heif_image_grid(imgs, ctypes.byref(g), desc.width, desc.height, None, 1, NEAREST, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(host.fr)) == BAD
    host = FakeHost(desc.width, desc.height, desc.depth, nch)
    g2 = pkg.Grid(2, 3, 32, 16)
    assert gpu.lib.avifgpu_host_read_heif_image_grid(imgs, ctypes.byref(g2), desc.width, desc.height, None, 1, NEAREST, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(host.fr)) == BAD
    assert not host.rects


# ---- 6. the CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_read_grid_crop_bilinear_orientation_6(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avif-format_amd", "avifgpu_cli")
    desc = pkg.ReadDesc(width=203, height=37, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8,
                        alpha_state=pkg.ALPHA_NONE, has_nclx=0, color_primaries=0, transfer_characteristics=0, matrix_coefficients=0)
    grid = (4, 3, 64, 16)
    planes, tiles = cut_planes(desc, grid, 8, np.random.default_rng(8))
    tiles = grid_truth.split(planes, desc, grid, np.random.default_rng(8), drop_invisible=False)      # the file holds every tile
    rect = (3, 1, 197, 35)
    want = expected(gpu, desc, planes, rect, CENTER, 6, ("cli",))
    with open(tmp_path / "in.planes", "wb") as f:
        for t in tiles:
            for pl in sorted(t):
                f.write(np.ascontiguousarray(t[pl]).tobytes())
    r = subprocess.run([cli, "read", "--width", "203", "--height", "37", "--depth", "8", "--bits", "8", "--colorspace", "ycbcr", "--chroma", "420",
                        "--grid", "4x3,64x16", "--crop", "3,1,197,35", "--orientation", "6", "--chroma-upsampling", "bilinear", "--maxdata", str(35 * 3 * 40),
                        str(tmp_path / "in.planes"), str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(197, 35, 3)
    assert same(got, want)


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_destination_untouched(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    name, kw = FORMATS[0]
    desc, planes, tiles, key = source(name, kw, CANVASES[0])
    dt = DeviceTiles(gpu, tiles, desc, GRID)
    rect = RECTS[1]
    need = pkg.read_grid_scratch_bytes(desc, GRID, rect, NEAREST, 1, 20)
    d_out = torch.full((64 * 256,), SENTINEL, dtype=torch.uint8, device=dev)
    scratch = torch.zeros((need + 256,), dtype=torch.uint8, device=dev)
    good = dict(grid=GRID, tiles=dt.ptr, rect=rect, mode=NEAREST, code=1, o=0, n=20, sb=need)
    bad = [dict(grid=(3, 3, 31, 16)),                            # odd tile_width for 4:2:0 with more than one column
           dict(grid=(2, 3, 32, 16)),                            # columns * tile_width < width
           dict(grid=(257, 3, 32, 16)), dict(tiles=None), dict(sb=need - 1), dict(mode=3), dict(code=0), dict(code=9)]
    for kw2 in [good] + bad:
        a = dict(good); a.update(kw2)
        try:
            gpu.read_rows_grid(desc, a["grid"], a["tiles"], a["rect"], a["mode"], a["code"], a["o"], a["n"], d_out.data_ptr(), 256, scratch.data_ptr(), a["sb"])
            ok = True
        except pkg.AvifGpuError as e:
            ok = False
            assert e.code == BAD, (kw2, e)
        torch.cuda.synchronize(dev)
        assert ok == (kw2 is good), kw2
        if not ok:
            assert bool((d_out == SENTINEL).all()), (kw2, "a rejected call wrote to dst")
        else:
            d_out.fill_(SENTINEL)
    # host pointers: a NULL plane of a visible tile
    table = grid_truth.tile_table(tiles, desc, GRID)
    table[4].plane[2] = None
    out = np.full((64 * 256,), SENTINEL, dtype=np.uint8)
    with pytest.raises(pkg.AvifGpuError) as e:
        gpu.read_rows_grid(desc, GRID, table, rect, NEAREST, 1, 0, 20, out.ctypes.data, 256, mem=pkg.MEM_HOST)
    assert e.value.code == BAD and (out == SENTINEL).all()
    # ... while the tiles nobody sees may be NULL: 4 x 4 tiles of 32 x 16 for the same canvas, its last column and row of tiles absent
    grid4 = (4, 4, 32, 16)
    tiles4 = grid_truth.split(planes, desc, grid4, np.random.default_rng(4))
    assert sum(t is None for t in tiles4) == 7
    want = expected(gpu, desc, planes, rect, NEAREST, 1, key)
    assert same(open_grid(gpu, desc, grid4, tiles4, rect, NEAREST, 1, mem="host"), want)
    assert same(open_grid(gpu, desc, grid4, DeviceTiles(gpu, tiles4, desc, grid4), rect, NEAREST, 1), want)
