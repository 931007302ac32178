"""Host-only half of the grid open (include/avifgpu.h "grid open"): the legality rule against a restatement, the ImageGrid payload parser, the
scratch formula as the header states it, the numpy truth's own round trip, the symbols and every rejection that returns before a device is
looked for.  No device is needed."""
import ctypes
import itertools
import struct

import numpy as np

import grid_truth
import harness

pkg = harness.pkg
BAD = pkg.formatBadParameters


def desc_for(width, height, chroma=pkg.CHROMA_444, **kw):
    base = dict(width=width, height=height, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    base.update(kw)
    return pkg.ReadDesc(**base)


def lib_check(desc, grid):
    return pkg.load().avifgpu_grid_check(ctypes.byref(desc), ctypes.byref(pkg.Grid(*grid)))


# ---- avifgpu_grid_check ------------------------------------------------------------------------------------------------------------------
def test_grid_check_against_restatement():
    kinds = [dict(chroma=pkg.CHROMA_420), dict(chroma=pkg.CHROMA_422), dict(chroma=pkg.CHROMA_444),
             dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_420),                    # the chroma field of a planar RGB image subsamples nothing
             dict(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME)]
    n = {True: 0, False: 0}
    for kw, (W, H), cols, rows, tw, th in itertools.product(kinds, ((1, 1), (7, 6), (8, 9), (12, 12)), (0, 1, 2, 3), (1, 2, 4), (1, 3, 4, 6, 7, 12), (2, 3, 5, 12)):
        d = desc_for(W, H, **kw)
        want = grid_truth.legal(d, (cols, rows, tw, th))
        assert (lib_check(d, (cols, rows, tw, th)) == 0) == want, (kw, W, H, cols, rows, tw, th)
        n[want] += 1
    assert n[True] > 300 and n[False] > 300
    d = desc_for(4096, 4096, pkg.CHROMA_420)
    assert lib_check(d, (256, 256, 16, 16)) == 0 and lib_check(d, (257, 256, 16, 16)) == BAD and lib_check(d, (256, 257, 16, 16)) == BAD
    assert lib_check(d, (256, 256, 15, 16)) == BAD and lib_check(d, (0, 1, 4096, 4096)) == BAD and lib_check(d, (1, 1, 4096, 4095)) == BAD
    assert lib_check(d, (1, 1, 4097, 4097)) == 0                                            # a single tile may be odd
    # the products are taken in 64 bits: 256 * (2^31 - 1) covers, and does not wrap to something small
    big = desc_for(2 ** 31 - 1, 16, pkg.CHROMA_444)
    assert lib_check(big, (2, 1, 2 ** 30, 16)) == 0 and lib_check(big, (2, 1, 2 ** 30 - 1, 16)) == BAD
    lib = pkg.load()
    assert lib.avifgpu_grid_check(None, ctypes.byref(pkg.Grid(1, 1, 4, 4))) == BAD
    assert lib.avifgpu_grid_check(ctypes.byref(d), None) == BAD
    assert lib_check(desc_for(16, 16, bit_depth=9), (1, 1, 16, 16)) == pkg.readErr           # the descriptor's own check


# ---- avifgpu_grid_parse ------------------------------------------------------------------------------------------------------------------
def lib_parse(payload):
    lib = pkg.load()
    r, c, w, h = (ctypes.c_int32(-7) for _ in range(4))
    buf = ctypes.create_string_buffer(bytes(payload), max(len(payload), 1))
    rc = lib.avifgpu_grid_parse(ctypes.addressof(buf), len(payload), ctypes.byref(r), ctypes.byref(c), ctypes.byref(w), ctypes.byref(h))
    assert rc in (0, BAD)
    if rc:
        assert (r.value, c.value, w.value, h.value) == (-7, -7, -7, -7)                      # nothing is written on a rejection
        return None
    return r.value, c.value, w.value, h.value


def test_grid_parse():
    short = struct.pack(">BBBBHH", 0, 0, 2, 15, 8192, 1536)
    wide = struct.pack(">BBBBII", 0, 1, 255, 0, 70000, 2 ** 31 - 1)
    assert lib_parse(short) == (3, 16, 8192, 1536)
    assert lib_parse(wide) == (256, 1, 70000, 2 ** 31 - 1)
    assert pkg.grid_parse(short) == (3, 16, 8192, 1536)
    assert lib_parse(short + b"\xff\xff\xff") == (3, 16, 8192, 1536)                         # trailing bytes are ignored
    assert lib_parse(struct.pack(">BBBBHH", 0, 0xFE, 0, 0, 1, 1)) == (1, 1, 1, 1)           # other flag bits do not select the field length
    for n in range(len(short)):
        assert lib_parse(short[:n]) is None, n
    for n in range(len(wide)):
        assert lib_parse(wide[:n]) is None, n
    assert lib_parse(struct.pack(">BBBBHH", 1, 0, 2, 15, 8192, 1536)) is None               # version
    assert lib_parse(struct.pack(">BBBBHH", 0, 0, 2, 15, 0, 1536)) is None and lib_parse(struct.pack(">BBBBHH", 0, 0, 2, 15, 8192, 0)) is None
    assert lib_parse(struct.pack(">BBBBII", 0, 1, 2, 15, 0, 7)) is None and lib_parse(struct.pack(">BBBBII", 0, 1, 2, 15, 7, 0)) is None
    assert lib_parse(struct.pack(">BBBBII", 0, 1, 2, 15, 2 ** 31, 7)) is None and lib_parse(struct.pack(">BBBBII", 0, 1, 2, 15, 7, 2 ** 32 - 1)) is None
    lib = pkg.load()
    v = ctypes.c_int32()
    buf = ctypes.create_string_buffer(short, 8)
    assert lib.avifgpu_grid_parse(None, 8, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == BAD
    assert lib.avifgpu_grid_parse(ctypes.addressof(buf), 8, None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == BAD
    assert lib.avifgpu_grid_parse(ctypes.addressof(buf), -1, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == BAD


# ---- avifgpu_read_grid_scratch_bytes -----------------------------------------------------------------------------------------------------
def align256(v):
    return (v + 255) // 256 * 256


def scratch_formula(d, rect, ups, code, onrows):
    """the formula as the header states it"""
    if onrows < 1:
        return 0
    xs, ys = grid_truth.shifts(d)
    s = 2 if d.bit_depth > 8 else 1
    b = harness.read_channels(d) * d.depth // 8
    turned = code >= 5
    sw, sh = (onrows, rect[3]) if turned else (rect[2], onrows)
    gw, gh = min(d.width, sw + 38), min(d.height, sh + 6)
    total = 256
    for pl in harness.read_planes(d):
        chroma = d.colorspace == pkg.COLORSPACE_YCBCR and pl in (1, 2)
        total += align256(((gw + xs) >> xs if chroma else gw) * s) * ((gh + ys) >> ys if chroma else gh)
    if ups != pkg.UPSAMPLE_NEAREST and xs:
        return total + 2 * align256(sw * s) * sh + (0 if code == 1 else align256(sw * b) * sh)
    px = 1 if xs and sw > 1 else 0
    py = 1 if ys and sh > 1 else 0
    if code == 1 and not px and not py:
        return total
    return total + align256((sw + px) * b) * (sh + py)


def test_scratch_bytes_formula():
    cases = [desc_for(137, 61, pkg.CHROMA_420), desc_for(138, 62, pkg.CHROMA_422), desc_for(137, 61, pkg.CHROMA_444),
             desc_for(137, 61, pkg.CHROMA_420, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_STRAIGHT),
             desc_for(137, 61, pkg.CHROMA_420, bit_depth=10, depth=32, has_nclx=1, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000),
             desc_for(137, 61, colorspace=pkg.COLORSPACE_RGB, alpha_state=pkg.ALPHA_STRAIGHT),
             desc_for(137, 61, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME)]
    grid = (5, 4, 32, 16)
    n = 0
    for d, rect, ups, code in itertools.product(cases, (None, (0, 0, 20, 10), (33, 17, 90, 40), (3, 3, 1, 1), (100, 50, 37, 11)),
                                                (pkg.UPSAMPLE_NEAREST, pkg.UPSAMPLE_BILINEAR_CENTER, pkg.UPSAMPLE_BILINEAR_LEFT), range(1, 9)):
        r = rect or (0, 0, d.width, d.height)
        out_h = r[2] if code >= 5 else r[3]
        for onrows in {0, 1, min(2, out_h), min(17, out_h), out_h}:
            got = pkg.read_grid_scratch_bytes(d, grid, rect, ups, code, onrows)
            assert got == scratch_formula(d, r, ups, code, onrows), (rect, ups, code, onrows)
            n += got > 0
    assert n > 1000
    lib = pkg.load()
    d = cases[0]
    g, r = pkg.Grid(*grid), pkg.CropRect(1, 1, 20, 10)
    def rc(desc=d, grid=g, rect=r, ups=0, code=1, onrows=5):
        return lib.avifgpu_read_grid_scratch_bytes(ctypes.byref(desc), ctypes.byref(grid) if grid else None, ctypes.byref(rect) if rect else None, ups, code, onrows)
    assert rc() > 0
    assert rc(onrows=11) == BAD and rc(code=6, onrows=21) == BAD and rc(onrows=-1) == BAD and rc(ups=3) == BAD and rc(code=0) == BAD and rc(code=9) == BAD
    assert rc(rect=pkg.CropRect(130, 1, 20, 10)) == BAD and rc(grid=None) == BAD and rc(grid=pkg.Grid(4, 4, 32, 16)) == BAD and rc(grid=pkg.Grid(5, 4, 31, 16)) == BAD


# ---- the numpy truth ---------------------------------------------------------------------------------------------------------------------
def test_split_then_assemble_is_the_identity():
    rng = np.random.default_rng(11)
    for kw, (W, H), grid in ((dict(chroma=pkg.CHROMA_420), (70, 46), (3, 3, 32, 16)), (dict(chroma=pkg.CHROMA_420), (67, 45), (3, 3, 32, 16)),
                             (dict(chroma=pkg.CHROMA_422, bit_depth=10, depth=16, alpha_state=pkg.ALPHA_STRAIGHT), (67, 45), (3, 3, 32, 16)),
                             (dict(chroma=pkg.CHROMA_420), (31, 13), (1, 1, 33, 15)),       # one odd tile
                             (dict(chroma=pkg.CHROMA_444), (20, 9), (4, 4, 7, 3)),          # a last column and a last row of tiles nobody sees
                             (dict(colorspace=pkg.COLORSPACE_RGB, bit_depth=10, depth=16), (11, 5), (6, 3, 2, 2))):
        d = desc_for(W, H, **kw)
        assert grid_truth.legal(d, grid)
        planes = harness.make_read_source(d, seed=W)
        tiles = grid_truth.split(planes, d, grid, rng)
        assert sum(t is None for t in tiles) == sum(not grid_truth.visible(d, grid, k) for k in range(grid[0] * grid[1]))
        got = grid_truth.assemble(tiles, d, grid)
        assert set(got) == set(planes)
        for pl, (w, _, ys) in harness.read_planes(d).items():
            assert np.array_equal(got[pl], planes[pl][:(H + ys) >> ys, :w]), (kw, pl)
        # strides differ from tile to tile, and some bases are off the 16-byte grid
        seen = [t for t in tiles if t is not None]
        if len(seen) > 2:
            assert len({t[0].strides[0] for t in seen}) > 1 and any(t[0].ctypes.data % 16 for t in seen)


# ---- symbols, and every rejection that returns before a device is looked for ----------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = pkg.load()
    for name in ("avifgpu_grid_parse", "avifgpu_grid_check", "avifgpu_read_grid_scratch_bytes", "avifgpu_read_rows_grid", "avifgpu_probe_grid_gather",
                 "avifgpu_host_read_heif_image_grid"):
        assert getattr(lib, name) is not None
    assert lib.avifgpu_abi_version() == 5
    assert ctypes.sizeof(pkg.GridTile) == 64 and ctypes.sizeof(pkg.Grid) == 16


def test_read_rows_grid_rejections_before_any_device():
    lib = pkg.load()
    buf = ctypes.create_string_buffer(1 << 16)
    d = desc_for(70, 46, pkg.CHROMA_420)
    grid = (3, 3, 32, 16)
    table = (pkg.GridTile * 9)()
    for k in range(9):
        for pl in range(3):
            table[k].plane[pl] = ctypes.addressof(buf)
            table[k].stride[pl] = 64

    def rc(desc=d, grid=grid, tiles=table, rect=(33, 17, 30, 20), ups=0, code=1, o=0, n=20, dst=buf, drb=96, scratch=None, sb=0, mem=pkg.MEM_HOST):
        return lib.avifgpu_read_rows_grid(ctypes.byref(desc), ctypes.byref(pkg.Grid(*grid)), ctypes.addressof(tiles) if tiles is not None else None,
                                          ctypes.byref(pkg.CropRect(*rect)) if rect else None, ups, code, o, n, dst, drb, scratch, sb, mem, None)

    def msg():
        return lib.avifgpu_last_error()

    null_plane = (pkg.GridTile * 9)(*table)
    null_plane[4].plane[1] = None
    thin = (pkg.GridTile * 9)(*table)
    thin[8].stride[0] = 31
    need = pkg.read_grid_scratch_bytes(d, grid, (33, 17, 30, 20), 0, 1, 20)
    for kw, text in ((dict(grid=(3, 3, 31, 16)), b"odd tile_width"), (dict(grid=(3, 3, 32, 17)), b"odd tile_height"), (dict(grid=(2, 3, 32, 16)), b"do not cover"),
                     (dict(grid=(3, 2, 32, 16)), b"do not cover"), (dict(grid=(257, 3, 32, 16)), b"1..256"), (dict(grid=(3, 0, 32, 16)), b"1..256"),
                     (dict(tiles=None), b"null buffer"), (dict(dst=None), b"null buffer"), (dict(tiles=null_plane), b"plane 1 of tile 4 is null"),
                     (dict(tiles=thin), b"stride"), (dict(rect=(33, 17, 38, 20)), b"not inside"), (dict(ups=3), b"upsampling"), (dict(ups=-1), b"upsampling"),
                     (dict(code=0), b"1..8"), (dict(code=9), b"1..8"), (dict(o=-1), b"outside"), (dict(o=5, n=16), b"outside"), (dict(code=6, n=31), b"outside"),
                     (dict(mem=7), b"mem_kind"), (dict(drb=89), b"dst_row_bytes"), (dict(code=6, drb=59), b"dst_row_bytes"),
                     (dict(mem=pkg.MEM_DEVICE), b"scratch"), (dict(mem=pkg.MEM_DEVICE, scratch=ctypes.addressof(buf), sb=need - 1), b"scratch")):
        assert rc(**kw) == BAD, kw
        assert text in msg(), (kw, msg())
    assert rc(desc=desc_for(70, 46, pkg.CHROMA_420, bit_depth=9)) == pkg.readErr
    # a tile nobody sees may be all NULL: 4 x 3 tiles of 32 x 16 cover 70 x 46 with a column to spare
    spare = (pkg.GridTile * 12)()
    for k in range(12):
        if k % 4 < 3:
            spare[k] = table[0]
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the missing device, and no further
        assert rc() == BAD and b"no CPU fallback" in msg()
        assert rc(rect=None, n=46, drb=210) == BAD and b"no CPU fallback" in msg()
        assert rc(grid=(4, 3, 32, 16), tiles=spare) == BAD and b"no CPU fallback" in msg()
        assert rc(mem=pkg.MEM_DEVICE, scratch=ctypes.addressof(buf), sb=need) == BAD and b"no CPU fallback" in msg()
    # the probe
    t = ctypes.addressof(table)
    def probe(tiles=t, columns=3, plane=0, tw=32, th=16, s=1, x0=0, y0=0, w=70, h=46, dst=ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, drb=96):
        return lib.avifgpu_probe_grid_gather(tiles, columns, plane, tw, th, s, x0, y0, w, h, dst, drb, None)
    for kw in (dict(tiles=None), dict(dst=None), dict(columns=0), dict(columns=257), dict(plane=4), dict(plane=-1), dict(tw=0), dict(th=0), dict(s=3), dict(s=0),
               dict(x0=-1), dict(y0=-1), dict(w=0), dict(h=0), dict(x0=27), dict(drb=64), dict(drb=100), dict(dst=probe.__defaults__[10] + 4)):
        assert probe(**kw) == BAD, kw
    if not torch.cuda.is_available():
        assert probe() == BAD and b"no CPU fallback" in msg()
