"""Host-only half of the grid save (include/avifgpu.h "grid save"): the numpy truth's own round trip, the legality rule of a save against a
restatement with the message of every rule, avifgpu_grid_fit, the ImageGrid payload against its parser, the scratch formula as the header
states it, every rejection of the entry that returns before a device is looked for, and the stand-alone sweep of
csrc/grid_save_geometry.h built with the sanitizers and run as a program.  No device is needed."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import grid_save_truth as truth
import grid_truth
import harness

pkg = harness.pkg
BAD = pkg.formatBadParameters
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wdesc(width, height, **kw):
    base = dict(width=width, height=height, depth=8, planes=3, bit_depth=8, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
                chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT709)
    base.update(kw)
    return pkg.WriteDesc(**base)


def msg():
    return pkg.load().avifgpu_last_error()


# ---- the truth of the truth ------------------------------------------------------------------------------------------------------------------
def test_pad_split_assemble_crop_is_the_identity():
    """pad, split, the grid open's own assemble, crop to the canvas: the oracle's planes again; every pad sample equals its edge sample"""
    rng = np.random.default_rng(5)
    d = wdesc(67, 45)
    grid = (3, 2, 32, 24)
    assert truth.legal(d, grid)[0]
    pkg.write_grid_check(d, grid)                                 # the library takes the grid the truth is cut on
    planes = harness.oracle_write(d, harness.make_write_source(d, seed=67))
    padded = truth.pad(planes, d, grid)
    tiles = truth.split(padded, d, grid)
    rd = pkg.ReadDesc(width=67, height=45, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    back = grid_truth.assemble(tiles, rd, grid)
    for pl, (pw, ph, twp, thp, spp) in truth.geometry(d, grid).items():
        assert padded[pl].shape == (grid[1] * thp, grid[0] * twp)
        assert np.array_equal(back[pl], planes[pl]), pl
        assert (padded[pl][:ph, pw:] == planes[pl][:, pw - 1:pw]).all() and (padded[pl][ph:, :pw] == planes[pl][ph - 1]).all()
        assert (padded[pl][ph:, pw:] == planes[pl][ph - 1, pw - 1]).all()
        assert all(t[pl].shape == (thp, twp) for t in tiles)
    # interleaved RGB: three samples to a pixel, padded pixel by pixel
    d = wdesc(21, 9, output=pkg.OUT_REFERENCE)
    grid = (2, 2, 16, 5)
    planes = harness.oracle_write(d, harness.make_write_source(d, seed=21))
    padded = truth.pad(planes, d, grid)
    assert padded[0].shape == (10, 32 * 3)
    P = planes[0].reshape(9, 21, 3)
    Q = padded[0].reshape(10, 32, 3)
    assert np.array_equal(Q[:9, :21], P) and (Q[:9, 21:] == P[:, 20:21]).all() and (Q[9:, :21] == P[8]).all() and (Q[9:, 21:] == P[8, 20]).all()
    tiles = truth.split(padded, d, grid)
    mono = pkg.ReadDesc(width=21 * 3, height=9, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    assert np.array_equal(grid_truth.assemble(tiles, mono, (2, 2, 48, 5))[0], planes[0])
    del rng


# ---- avifgpu_write_grid_check ------------------------------------------------------------------------------------------------------------------
def test_write_grid_check_against_restatement():
    lib = pkg.load()
    kinds = [dict(chroma=pkg.CHROMA_420), dict(chroma=pkg.CHROMA_422), dict(chroma=pkg.CHROMA_444),
             dict(output=pkg.OUT_REFERENCE, chroma=pkg.CHROMA_420),                        # the chroma field subsamples nothing in reference output
             dict(output=pkg.OUT_REFERENCE, planes=2, alpha_state=pkg.ALPHA_STRAIGHT)]
    seen = {}
    for kw, (W, H), cols, rows, tw, th in itertools.product(kinds, ((1, 1), (7, 6), (8, 9), (12, 12)), (0, 1, 2, 3), (1, 2, 4), (1, 3, 4, 6, 7, 12), (2, 3, 5, 12)):
        d = wdesc(W, H, **kw)
        ok, why = truth.legal(d, (cols, rows, tw, th))
        rc = lib.avifgpu_write_grid_check(ctypes.byref(d), ctypes.byref(pkg.Grid(cols, rows, tw, th)))
        assert (rc == 0) == ok and rc in (0, BAD), (kw, W, H, cols, rows, tw, th)
        if not ok:
            assert why.encode() in msg(), (why, msg())
        seen[why] = seen.get(why, 0) + 1
    assert seen[""] > 100 and all(seen.get(w, 0) > 5 for w in ("1..256", "do not cover", "odd tile_width", "odd tile_height", "not minimal")), seen
    d = wdesc(4096, 4096)
    def rc(*grid):
        return lib.avifgpu_write_grid_check(ctypes.byref(d), ctypes.byref(pkg.Grid(*grid)))
    assert rc(256, 256, 16, 16) == 0 and rc(257, 256, 16, 16) == BAD and b"1..256" in msg()
    assert rc(256, 128, 16, 34) == BAD and b"not minimal" in msg()           # 127 rows of 34 cover 4318 rows: the last row of tiles sees nothing
    assert rc(1, 1, 4097, 4097) == 0                                          # a single tile may be odd
    assert lib.avifgpu_write_grid_check(None, ctypes.byref(pkg.Grid(1, 1, 4, 4))) == BAD
    assert lib.avifgpu_write_grid_check(ctypes.byref(d), None) == BAD
    assert lib.avifgpu_write_grid_check(ctypes.byref(wdesc(16, 16, bit_depth=9)), ctypes.byref(pkg.Grid(1, 1, 16, 16))) == pkg.formatCannotRead


# ---- avifgpu_grid_fit ----------------------------------------------------------------------------------------------------------------------------
def qualifies(size, n, cap, align, sub):
    a = align * 2 if (sub and n > 1 and align % 2) else align
    need = -(-size // n)
    t = -(-need // a) * a
    return t if t <= cap else None


def test_grid_fit_is_legal_minimal_and_smallest():
    lib = pkg.load()
    n_ok = n_bad = 0
    for chroma, align in itertools.product((pkg.CHROMA_420, pkg.CHROMA_444), (1, 2, 16, 64)):
        xs, ys = harness.chroma_shift(chroma)
        for size in range(1, 301):
            other = 301 - size
            for cap_w, cap_h in ((64, 128), (16, 300), (7, 2)):
                d = wdesc(size, other, chroma=chroma)
                g = pkg.Grid()
                rc = lib.avifgpu_grid_fit(ctypes.byref(d), cap_w, cap_h, align, ctypes.byref(g))
                want_c = next((n for n in range(1, 257) if qualifies(size, n, cap_w, align, xs)), None)
                want_r = next((n for n in range(1, 257) if qualifies(other, n, cap_h, align, ys)), None)
                if want_c is None or want_r is None:
                    assert rc == BAD and b"avifgpu_grid_fit" in msg()
                    n_bad += 1
                    continue
                assert rc == 0, (size, other, cap_w, cap_h, align, msg())
                grid = (g.columns, g.rows, g.tile_width, g.tile_height)
                assert truth.legal(d, grid) == (True, ""), grid                  # legal and minimal
                assert g.tile_width <= cap_w and g.tile_height <= cap_h and g.tile_width % align == 0 and g.tile_height % align == 0
                assert g.columns == want_c and g.rows == want_r                 # no smaller count qualifies
                assert g.tile_width == qualifies(size, want_c, cap_w, align, xs) and g.tile_height == qualifies(other, want_r, cap_h, align, ys)
                assert pkg.load().avifgpu_write_grid_check(ctypes.byref(d), ctypes.byref(g)) == 0
                n_ok += 1
    assert n_ok > 1500 and n_bad > 100, (n_ok, n_bad)
    d = wdesc(20000, 9000, chroma=pkg.CHROMA_444)
    assert pkg.grid_fit(d, 8192, 4352, 64) == (3, 3, 6720, 3008)
    g = pkg.Grid()
    assert lib.avifgpu_grid_fit(ctypes.byref(d), 8192, 4352, 0, ctypes.byref(g)) == BAD and lib.avifgpu_grid_fit(ctypes.byref(d), 0, 4352, 1, ctypes.byref(g)) == BAD
    assert lib.avifgpu_grid_fit(ctypes.byref(d), 8192, 4352, 1, None) == BAD and lib.avifgpu_grid_fit(None, 8192, 4352, 1, ctypes.byref(g)) == BAD
    assert lib.avifgpu_grid_fit(ctypes.byref(d), 64, 4352, 1, ctypes.byref(g)) == BAD       # 313 columns


# ---- avifgpu_grid_payload ----------------------------------------------------------------------------------------------------------------------
def test_payload_round_trips_through_the_parser():
    lib = pkg.load()
    for cols, rows, w, h in ((16, 3, 8192, 1536), (1, 1, 1, 1), (256, 256, 65535, 65535), (2, 2, 65536, 7), (1, 256, 7, 70000), (3, 3, 2 ** 31 - 1, 2 ** 31 - 1)):
        wide = w > 65535 or h > 65535
        p = pkg.grid_payload((cols, rows, 64, 64), w, h)
        assert len(p) == (12 if wide else 8) and p[0] == 0 and (p[1] & 1) == int(wide)
        assert pkg.grid_parse(p) == (rows, cols, w, h)
        buf = ctypes.create_string_buffer(b"\xA5" * 16, 16)
        g = pkg.Grid(cols, rows, 64, 64)
        for cap in range(0, len(p)):
            assert lib.avifgpu_grid_payload(ctypes.byref(g), w, h, ctypes.addressof(buf), cap) == BAD, cap       # a short capacity is refused
            assert buf.raw == b"\xA5" * 16
        assert lib.avifgpu_grid_payload(ctypes.byref(g), w, h, ctypes.addressof(buf), len(p)) == len(p)
        assert buf.raw[:len(p)] == p and buf.raw[len(p):] == b"\xA5" * (16 - len(p))
    g = pkg.Grid(2, 2, 8, 8)
    buf = ctypes.create_string_buffer(16)
    assert lib.avifgpu_grid_payload(None, 8, 8, ctypes.addressof(buf), 16) == BAD and lib.avifgpu_grid_payload(ctypes.byref(g), 8, 8, None, 16) == BAD
    assert lib.avifgpu_grid_payload(ctypes.byref(g), 0, 8, ctypes.addressof(buf), 16) == BAD
    assert lib.avifgpu_grid_payload(ctypes.byref(pkg.Grid(257, 2, 8, 8)), 8, 8, ctypes.addressof(buf), 16) == BAD


# ---- avifgpu_write_grid_scratch_bytes ------------------------------------------------------------------------------------------------------------
def test_scratch_bytes_formula():
    cases = [wdesc(137, 61), wdesc(138, 62, chroma=pkg.CHROMA_422, depth=16, bit_depth=12), wdesc(137, 61, chroma=pkg.CHROMA_444, planes=4, alpha_state=pkg.ALPHA_STRAIGHT),
             wdesc(137, 61, output=pkg.OUT_REFERENCE), wdesc(137, 61, output=pkg.OUT_REFERENCE, depth=16, bit_depth=10, planes=4, alpha_state=pkg.ALPHA_STRAIGHT),
             wdesc(137, 61, output=pkg.OUT_REFERENCE, planes=2, alpha_state=pkg.ALPHA_STRAIGHT),
             wdesc(520, 33, depth=32, bit_depth=10, transfer=pkg.TRANSFER_PQ, chroma=pkg.CHROMA_444, matrix_coefficients=pkg.MATRIX_BT2020_NCL)]
    n = 0
    for d in cases:
        for nrows in (0, 1, 2, 17, d.height - 1, d.height):
            got = pkg.write_grid_scratch_bytes(d, nrows)
            assert got == truth.scratch_formula(d, nrows), (nrows, got)
            n += got > 0
    assert n == 5 * len(cases)
    lib = pkg.load()
    assert lib.avifgpu_write_grid_scratch_bytes(ctypes.byref(cases[0]), 62) == BAD and lib.avifgpu_write_grid_scratch_bytes(ctypes.byref(cases[0]), -1) == BAD
    assert lib.avifgpu_write_grid_scratch_bytes(None, 1) == BAD


# ---- symbols, and every rejection of the entry that returns before a device is looked for ------------------------------------------------------
def test_symbols_and_abi_version():
    lib = pkg.load()
    for name in ("avifgpu_write_grid_check", "avifgpu_write_grid_scratch_bytes", "avifgpu_grid_fit", "avifgpu_grid_payload", "avifgpu_write_rows_grid",
                 "avifgpu_probe_grid_scatter", "avifgpu_host_create_heif_image_grid"):
        assert getattr(lib, name) is not None
    assert lib.avifgpu_abi_version() == 5
    assert pkg.ICC_KIND_NONE == 0 and pkg.ICC_KIND_PIPELINE32 == 6


def test_write_rows_grid_rejections_before_any_device():
    lib = pkg.load()
    buf = ctypes.create_string_buffer(1 << 16)
    d = wdesc(37, 23)
    grid = (3, 2, 14, 12)
    table = (pkg.GridTile * 6)()
    for k in range(6):
        for pl in range(3):
            table[k].plane[pl] = ctypes.addressof(buf)
            table[k].stride[pl] = 16
    need = pkg.write_grid_scratch_bytes(d, 23)
    pipe = pkg.IccPipeline32()                                   # never proven: unstamped

    def rc(desc=d, kind=0, icc=None, grid=grid, tiles=table, row0=0, nrows=23, src=buf, srb=37 * 3, scratch=None, sb=0, mem=pkg.MEM_HOST):
        return lib.avifgpu_write_rows_grid(ctypes.byref(desc), kind, icc, ctypes.byref(pkg.Grid(*grid)) if grid else None,
                                           ctypes.addressof(tiles) if tiles is not None else None, row0, nrows, src, srb, scratch, sb, mem, None)

    null_plane = (pkg.GridTile * 6)(*table)
    null_plane[5].plane[2] = None
    thin = (pkg.GridTile * 6)(*table)
    thin[1].stride[0] = 13
    d16 = wdesc(37, 23, depth=16, bit_depth=10)                   # 16-bit samples: tile planes and strides are even
    table16 = (pkg.GridTile * 6)(*table)
    for k in range(6):
        for pl in range(3):
            table16[k].stride[pl] = 32
    odd_base = (pkg.GridTile * 6)(*table16)
    odd_base[3].plane[1] = ctypes.addressof(buf) + 1
    odd_stride = (pkg.GridTile * 6)(*table16)
    odd_stride[2].stride[0] = 33
    for kw, text in ((dict(grid=(3, 2, 13, 12)), b"odd tile_width"), (dict(grid=(3, 2, 14, 13)), b"odd tile_height"), (dict(grid=(2, 2, 14, 12)), b"do not cover"),
                     (dict(grid=(3, 1, 14, 12)), b"do not cover"), (dict(grid=(257, 2, 14, 12)), b"1..256"), (dict(grid=(3, 0, 14, 12)), b"1..256"),
                     (dict(grid=(4, 2, 14, 12)), b"not minimal"), (dict(grid=(3, 3, 14, 12)), b"not minimal"), (dict(grid=None), b"null grid"),
                     (dict(tiles=None), b"null buffer"), (dict(src=None), b"null buffer"), (dict(srb=110), b"src_row_bytes"),
                     (dict(tiles=null_plane), b"plane 2 of tile 5 is null"), (dict(tiles=thin), b"stride 13 of plane 0 of tile 1"),
                     (dict(desc=d16, srb=37 * 6, tiles=odd_base), b"plane 1 of tile 3 holds 16-bit samples at an odd address or stride"),
                     (dict(desc=d16, srb=37 * 6, tiles=odd_stride), b"plane 0 of tile 2 holds 16-bit samples at an odd address or stride"),
                     (dict(kind=7), b"icc_kind"), (dict(kind=-1), b"icc_kind"), (dict(kind=0, icc=ctypes.addressof(buf)), b"takes a NULL icc"), (dict(kind=3), b"NULL icc"),
                     (dict(kind=6, icc=ctypes.addressof(pipe)), b"not proven"),
                     (dict(row0=-2), b"outside"), (dict(row0=2, nrows=22), b"outside"), (dict(row0=1, nrows=2), b"even row"), (dict(row0=0, nrows=3), b"even height"),
                     (dict(mem=7), b"mem_kind"), (dict(mem=pkg.MEM_DEVICE), b"scratch"), (dict(mem=pkg.MEM_DEVICE, scratch=ctypes.addressof(buf), sb=need - 1), b"scratch")):
        assert rc(**kw) == BAD, kw
        assert text in msg(), (kw, msg())
        assert b"no CPU fallback" not in msg()
    assert rc(desc=wdesc(37, 23, bit_depth=9)) == pkg.formatCannotRead
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the missing device, and no further
        assert rc() == BAD and b"no CPU fallback" in msg()
        assert rc(row0=4, nrows=6) == BAD and b"no CPU fallback" in msg()
        assert rc(mem=pkg.MEM_DEVICE, scratch=ctypes.addressof(buf), sb=need) == BAD and b"no CPU fallback" in msg()
    # the probe
    t = ctypes.addressof(table)
    def probe(tiles=t, columns=3, plane=0, tw=14, th=12, b=1, pw=37, ph=23, y0=0, h=24, src=ctypes.addressof(buf), srb=37):
        return lib.avifgpu_probe_grid_scatter(tiles, columns, plane, tw, th, b, pw, ph, y0, h, src, srb, None)
    for kw in (dict(tiles=None), dict(src=None), dict(columns=0), dict(columns=257), dict(plane=4), dict(plane=-1), dict(tw=0), dict(th=0), dict(b=5), dict(b=0), dict(b=7),
               dict(pw=0), dict(ph=0), dict(pw=43), dict(y0=-1), dict(h=0), dict(y0=23), dict(srb=36), dict(b=3, srb=110),
               dict(b=2, srb=75), dict(b=6, srb=222, src=ctypes.addressof(buf) + 1), dict(b=8, srb=297)):        # 16-bit samples at an odd row distance / address
        assert probe(**kw) == BAD, kw
    if not torch.cuda.is_available():
        assert probe() == BAD and b"no CPU fallback" in msg()


# ---- the arithmetic under the sanitizers, as a program -----------------------------------------------------------------------------------------------
def test_geometry_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is part of the toolchain this project builds with"
    exe = tmp_path / "grid_save_geometry_check"
    # the sanitizer runtimes are linked into the program itself, so it runs as it is wherever it is started
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tools", "grid_save_geometry_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout
