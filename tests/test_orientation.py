"""Host-only half of the oriented open (include/avifgpu.h "oriented open"): composition of the eight EXIF codes, geometry, the tile
helper and every rejected argument.  No device is needed: everything here returns before anything would be launched."""
import ctypes
import itertools

import numpy as np
import pytest

import harness
from orientation_truth import orient

pkg = harness.pkg

CODES = range(1, 9)


def desc_for(width, height, chroma=pkg.CHROMA_444, **kw):
    base = dict(width=width, height=height, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    base.update(kw)
    return pkg.ReadDesc(**base)


def test_compose_all_pairs_against_numpy():
    label = np.arange(15).reshape(3, 5, 1)
    images = {c: orient(c, label) for c in CODES}
    assert len({(v.shape, v.tobytes()) for v in images.values()}) == 8           # the labelled array tells all eight apart
    for first, then in itertools.product(CODES, CODES):
        want = orient(then, orient(first, label))
        got = pkg.orientation_compose(first, then)
        assert 1 <= got <= 8
        assert images[got].shape == want.shape and np.array_equal(images[got], want), (first, then, got)


def test_compose_irot_imir_codes():
    # irot with angle a (anticlockwise quarter turns) is np.rot90(I, a): codes 1, 8, 3, 6; two quarter turns make a half turn
    assert pkg.orientation_compose(8, 8) == 3 and pkg.orientation_compose(8, 6) == 1 and pkg.orientation_compose(6, 6) == 3
    assert pkg.orientation_compose(2, 2) == 1 and pkg.orientation_compose(4, 4) == 1 and pkg.orientation_compose(2, 4) == 3


@pytest.mark.parametrize("bad", [(0, 1), (1, 0), (9, 1), (1, 9), (-1, 3)])
def test_compose_rejects(bad):
    lib = pkg.load()
    assert lib.avifgpu_orientation_compose(*bad) == pkg.formatBadParameters
    assert b"1..8" in lib.avifgpu_last_error()


def test_geometry():
    d = desc_for(67, 35)
    for code in CODES:
        assert pkg.read_oriented_geometry(d, code) == ((67, 35) if code <= 4 else (35, 67))
    lib = pkg.load()
    w, h = ctypes.c_int32(), ctypes.c_int32()
    for code in (0, 9, -3):
        assert lib.avifgpu_read_oriented_geometry(ctypes.byref(d), code, ctypes.byref(w), ctypes.byref(h)) == pkg.formatBadParameters
    assert lib.avifgpu_read_oriented_geometry(ctypes.byref(d), 6, None, ctypes.byref(h)) == pkg.formatBadParameters
    assert lib.avifgpu_read_oriented_geometry(None, 6, ctypes.byref(w), ctypes.byref(h)) == pkg.formatBadParameters
    assert lib.avifgpu_read_oriented_geometry(ctypes.byref(desc_for(0, 5)), 6, ctypes.byref(w), ctypes.byref(h)) == pkg.formatBadParameters


def source_start(d, code, orow0, n):
    """(first source row or column of the region, whether that direction is subsampled) -- restated from the definition."""
    xs, ys = harness.chroma_shift(d.chroma)
    turned = code >= 5
    size = d.width if turned else d.height                     # extent of the cut direction = rows of the oriented image
    flipped = code in ((7, 8) if turned else (3, 4))
    return (size - orow0 - n if flipped else orow0), bool(xs if turned else ys)


@pytest.mark.parametrize("chroma", [pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420])
def test_next_tile_partitions_on_even_source_starts(chroma):
    for code, w, h, max_rows in itertools.product(CODES, range(1, 10), range(1, 10), (1, 2, 3, 4, 7, 64)):
        d = desc_for(w, h, chroma)
        out_h = pkg.read_oriented_geometry(d, code)[1]
        o = 0
        while o < out_h:
            n = pkg.read_oriented_next_tile(d, code, o, max_rows)
            assert 0 < n <= max_rows and o + n <= out_h, (code, w, h, max_rows, o, n)
            start, sub = source_start(d, code, o, n)
            # a region of a subsampled direction starts on an even index; one of a single row / column is its own chroma sample
            assert not sub or start % 2 == 0 or n == 1, (code, w, h, max_rows, o, n, start)
            if sub and max_rows >= 2:
                assert start % 2 == 0, (code, w, h, max_rows, o, n, start)
            if not sub:
                assert n == min(max_rows, out_h - o)
            o += n
        assert o == out_h


def test_next_tile_first_tile_of_a_flipped_odd_direction_is_odd():
    d = desc_for(33, 31, pkg.CHROMA_420)
    assert pkg.read_oriented_next_tile(d, 4, 0, 8) == 7         # rows flipped, H = 31: source rows [24, 31)
    assert pkg.read_oriented_next_tile(d, 8, 0, 8) == 7         # columns flipped, W = 33: source columns [26, 33)
    assert pkg.read_oriented_next_tile(d, 6, 0, 8) == 8         # columns in order
    assert pkg.read_oriented_next_tile(d, 4, 7, 100) == 24      # the rest of the image


def test_next_tile_rejects():
    lib = pkg.load()
    d = desc_for(9, 7, pkg.CHROMA_420)
    for args in ((0, 0, 4), (9, 0, 4), (6, -1, 4), (6, 9, 4), (2, 7, 4), (6, 0, 0), (6, 0, -5)):
        assert lib.avifgpu_read_oriented_next_tile(ctypes.byref(d), *args) == pkg.formatBadParameters, args
    assert lib.avifgpu_read_oriented_next_tile(None, 6, 0, 4) == pkg.formatBadParameters


def test_scratch_bytes():
    d = desc_for(67, 35, alpha_state=pkg.ALPHA_STRAIGHT)        # 4 bytes per pixel
    assert pkg.read_oriented_scratch_bytes(d, 1, 35) == 0
    assert pkg.read_oriented_scratch_bytes(d, 3, 10) == 512 * 10            # 10 rows of 67 pixels, rows padded to 256 bytes
    assert pkg.read_oriented_scratch_bytes(d, 6, 10) == 256 * 35            # a band of 10 columns, all 35 rows
    lib = pkg.load()
    assert lib.avifgpu_read_oriented_scratch_bytes(ctypes.byref(d), 9, 10) == pkg.formatBadParameters
    assert lib.avifgpu_read_oriented_scratch_bytes(ctypes.byref(d), 6, 68) == pkg.formatBadParameters
    assert lib.avifgpu_read_oriented_scratch_bytes(ctypes.byref(d), 6, -1) == pkg.formatBadParameters


def test_read_rows_oriented_rejects_before_any_launch():
    """Every rejected argument comes back as formatBadParameters with its own message -- none of them is the "no device" message, so
    the checks run before a device is looked for."""
    lib = pkg.load()
    d = desc_for(9, 7, pkg.CHROMA_420)
    planes = harness.make_read_source(d)
    ptrs = pkg.planes4([planes[i].ctypes.data if i in planes else None for i in range(4)])
    strides = pkg.strides4([planes[i].strides[0] if i in planes else 0 for i in range(4)])
    dst = np.zeros((9, 64), np.uint8)

    def call(code, o, n, src=ptrs, st=strides, out=dst.ctypes.data, row_bytes=64, scratch=None, scratch_bytes=0, mem=pkg.MEM_HOST):
        rc = lib.avifgpu_read_rows_oriented(ctypes.byref(d), code, o, n, ctypes.byref(src) if src is not None else None,
                                            ctypes.byref(st) if st is not None else None, out, row_bytes, scratch, scratch_bytes, mem, None)
        return rc, lib.avifgpu_last_error()

    for code in (0, 9, -1):
        rc, msg = call(code, 0, 1)
        assert rc == pkg.formatBadParameters and b"1..8" in msg
    for code, o, n in ((2, 0, 8), (2, -1, 2), (6, 0, 10), (6, 8, 2), (3, 7, 1)):
        rc, msg = call(code, o, n)
        assert rc == pkg.formatBadParameters and b"outside" in msg, (code, o, n, msg)
    # illegal cuts: an odd source start of a subsampled direction, more than one row / column
    for code, o, n in ((2, 1, 2), (4, 0, 2), (6, 1, 4), (8, 0, 2), (1, 3, 2)):
        rc, msg = call(code, o, n)
        assert rc == pkg.formatBadParameters and b"odd source" in msg, (code, o, n, msg)
    rc, msg = call(6, 0, 4, row_bytes=7 * 3 - 1)
    assert rc == pkg.formatBadParameters and b"dst_row_bytes" in msg
    rc, msg = call(6, 0, 4, src=None)
    assert rc == pkg.formatBadParameters and b"null" in msg
    rc, msg = call(6, 0, 4, out=None)
    assert rc == pkg.formatBadParameters and b"null" in msg
    rc, msg = call(6, 0, 4, mem=7)
    assert rc == pkg.formatBadParameters and b"mem_kind" in msg
    need = pkg.read_oriented_scratch_bytes(d, 6, 4)
    for scratch, nbytes in ((None, need), (dst.ctypes.data, need - 1), (dst.ctypes.data, 0)):
        rc, msg = call(6, 0, 4, scratch=scratch, scratch_bytes=nbytes, mem=pkg.MEM_DEVICE)
        assert rc == pkg.formatBadParameters and b"scratch" in msg, (scratch, nbytes, msg)
    short = pkg.strides4([planes[0].strides[0], 3, planes[2].strides[0], 0])
    rc, msg = call(6, 0, 4, st=short)
    assert rc == pkg.formatBadParameters and b"src_stride" in msg


def test_probe_orient_rejects():
    lib = pkg.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    for args in ((1, 4, 8, 8, p, 32, p, 32), (9, 4, 8, 8, p, 32, p, 32), (6, 5, 8, 8, p, 40, p, 40), (6, 4, 0, 8, p, 32, p, 32),
                 (6, 4, 8, 8, None, 32, p, 32), (6, 4, 8, 4, p, 31, p, 16), (6, 4, 8, 4, p, 32, p, 15)):
        assert lib.avifgpu_probe_orient(*args, None) == pkg.formatBadParameters, args
        assert b"avifgpu_probe_orient" in lib.avifgpu_last_error()
