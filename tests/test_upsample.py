"""Host-only half of the upsampled open (include/avifgpu.h "upsampled open"): properties of the integer definition as
tests/upsample_truth.py states it, and everything of the library that returns before a device is looked for."""
import ctypes

import numpy as np

import harness
from upsample_truth import CENTER, LEFT, NEAREST, upsample_plane

pkg = harness.pkg


def desc_for(width, height, chroma=pkg.CHROMA_420, **kw):
    base = dict(width=width, height=height, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    base.update(kw)
    return pkg.ReadDesc(**base)


def _random_plane(rng, W, H, ys, dtype, top):
    return rng.integers(0, top + 1, size=((H + ys) >> ys, (W + 1) >> 1)).astype(dtype)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_constant_plane_stays_constant():
    for dtype, value in ((np.uint8, 0), (np.uint8, 255), (np.uint8, 77), (np.uint16, 4095), (np.uint16, 65535)):
        for W, H in ((1, 1), (2, 2), (7, 5), (16, 9)):
            for ys in (0, 1):
                for siting in (CENTER, LEFT):
                    C = np.full(((H + ys) >> ys, (W + 1) >> 1), value, dtype)
                    U = upsample_plane(C, W, H, ys, siting)
                    assert U.dtype == dtype and U.shape == (H, W) and (U == value).all(), (dtype, value, W, H, ys, siting)


def test_output_within_the_inputs_range():
    rng = np.random.default_rng(1)
    for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
        for W, H in ((9, 7), (10, 8), (1, 6), (6, 1)):
            for ys in (0, 1):
                for siting in (CENTER, LEFT):
                    C = _random_plane(rng, W, H, ys, dtype, top)
                    C[0, 0], C[-1, -1] = top, 0                                  # 16 * top must not wrap
                    U = upsample_plane(C, W, H, ys, siting)
                    assert U.min() >= C.min() and U.max() <= C.max()


def test_horizontal_ramp_tells_the_sitings_apart():
    """C[i] = 4 i: on interior pixels CENTER gives 2 x - 1, LEFT gives 2 x, both exact in integers."""
    W, H = 40, 6
    for ys in (0, 1):
        C = np.tile((4 * np.arange((W + 1) >> 1)).astype(np.uint16), ((H + ys) >> ys, 1))
        x = np.arange(1, W - 1)
        assert (upsample_plane(C, W, H, ys, CENTER)[:, 1:W - 1] == 2 * x - 1).all()
        assert (upsample_plane(C, W, H, ys, LEFT)[:, 1:W - 1] == 2 * x).all()


def test_422_leaves_rows_independent():
    rng = np.random.default_rng(2)
    W, H = 13, 6
    C = _random_plane(rng, W, H, 0, np.uint16, 4095)
    for siting in (CENTER, LEFT):
        U = upsample_plane(C, W, H, 0, siting)
        for y in range(H):
            assert np.array_equal(U[y], upsample_plane(C[y:y + 1], W, 1, 0, siting)[0]), (siting, y)
        D = C.copy()
        D[3] = 4095 - D[3]
        V = upsample_plane(D, W, H, 0, siting)
        assert np.array_equal(np.delete(U, 3, axis=0), np.delete(V, 3, axis=0))


def test_one_joint_rounding_not_one_per_direction():
    """C = [[0, 3], [0, 0]], CENTER, 4:2:0, W = H = 4: U[2, 1] = (1 * (3 * 0 + 1 * 3) + 3 * 0 + 8) >> 4 = 0.  (On this input a rounding
    per direction gives (3 + 2) >> 2 = 1 along x and then (1 + 2) >> 2 = 0 along y: the same 0, at every pixel -- so the two roundings
    are told apart on a second input, C = [[0, 2], [0, 0]] at U[1, 1]: jointly (3 * (3 * 0 + 2) + 0 + 8) >> 4 = 0, per direction
    (2 + 2) >> 2 = 1 and then (3 * 1 + 0 + 2) >> 2 = 1.)"""
    C = np.array([[0, 3], [0, 0]], np.uint8)
    assert upsample_plane(C, 4, 4, 1, CENTER)[2, 1] == 0
    D = np.array([[0, 2], [0, 0]], np.uint8)
    assert upsample_plane(D, 4, 4, 1, CENTER)[1, 1] == 0
    assert upsample_plane(D, 4, 4, 1, CENTER, separable=True)[1, 1] == 1
    rng = np.random.default_rng(3)
    R = _random_plane(rng, 32, 32, 1, np.uint8, 255)
    assert not np.array_equal(upsample_plane(R, 32, 32, 1, CENTER), upsample_plane(R, 32, 32, 1, CENTER, separable=True))


def test_taps_written_out_by_hand():
    """The table of the header on a 3 x 2 plane, W = 5, H = 4: every clamped edge once."""
    C = np.array([[16, 32, 64], [0, 160, 240]], np.uint16)
    U = upsample_plane(C, 5, 4, 1, CENTER)
    h0 = [16 * 4, 3 * 16 + 32, 16 + 3 * 32, 3 * 32 + 64, 32 + 3 * 64]
    h1 = [0, 160, 3 * 160, 3 * 160 + 240, 160 + 3 * 240]
    assert U[0].tolist() == [(4 * a + 8) >> 4 for a in h0]
    assert U[1].tolist() == [(3 * a + b + 8) >> 4 for a, b in zip(h0, h1)]
    assert U[2].tolist() == [(a + 3 * b + 8) >> 4 for a, b in zip(h0, h1)]
    assert U[3].tolist() == [(4 * b + 8) >> 4 for b in h1]
    L = upsample_plane(C, 5, 4, 0 + 1, LEFT)
    l0 = [4 * 16, 2 * 16 + 2 * 32, 4 * 32, 2 * 32 + 2 * 64, 4 * 64]
    assert L[0].tolist() == [(4 * a + 8) >> 4 for a in l0]


# ---- the library without a GPU -------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    lib = pkg.load()
    for name in ("avifgpu_read_upsampled_scratch_bytes", "avifgpu_read_rows_upsampled", "avifgpu_probe_upsample",
                 "avifgpu_host_read_heif_image_upsampled"):
        assert getattr(lib, name) is not None
    assert lib.avifgpu_abi_version() == 5
    assert (pkg.UPSAMPLE_NEAREST, pkg.UPSAMPLE_BILINEAR_CENTER, pkg.UPSAMPLE_BILINEAR_LEFT) == (NEAREST, CENTER, LEFT) == (0, 1, 2)


def test_scratch_bytes_zero_where_the_call_is_an_existing_entry_point():
    sub = desc_for(67, 35)
    for code in range(1, 9):
        assert pkg.read_upsampled_scratch_bytes(sub, NEAREST, code, 10) == 0
    others = [desc_for(67, 35, pkg.CHROMA_444),
              desc_for(67, 35, pkg.CHROMA_MONOCHROME, colorspace=pkg.COLORSPACE_MONOCHROME),
              desc_for(67, 35, pkg.CHROMA_444, colorspace=pkg.COLORSPACE_RGB, matrix_coefficients=pkg.MATRIX_RGB_GBR)]
    for d in others:
        for mode in (NEAREST, CENTER, LEFT):
            for code in (1, 3, 6):
                assert pkg.read_upsampled_scratch_bytes(d, mode, code, 10) == 0, (d.colorspace, d.chroma, mode, code)


def test_scratch_bytes_of_the_subsampled_cases():
    """2 * align256(sw * s) * sh for the two chroma rectangles, plus the oriented 4:4:4 open's align256(sw * b) * sh for codes 2-8."""
    for chroma in (pkg.CHROMA_420, pkg.CHROMA_422):
        d8 = desc_for(67, 35, chroma, alpha_state=pkg.ALPHA_STRAIGHT)                       # 1-byte samples, 4 bytes per pixel
        d16 = desc_for(300, 35, chroma, bit_depth=12, depth=16)                             # 2-byte samples, 6 bytes per pixel
        for mode in (CENTER, LEFT):
            assert pkg.read_upsampled_scratch_bytes(d8, mode, 1, 10) == 2 * 256 * 10
            assert pkg.read_upsampled_scratch_bytes(d8, mode, 3, 10) == 2 * 256 * 10 + 512 * 10
            assert pkg.read_upsampled_scratch_bytes(d8, mode, 6, 10) == 2 * 256 * 35 + 256 * 35      # a band of 10 columns, all 35 rows
            assert pkg.read_upsampled_scratch_bytes(d16, mode, 1, 4) == 2 * 768 * 4
            assert pkg.read_upsampled_scratch_bytes(d16, mode, 4, 4) == 2 * 768 * 4 + 2048 * 4
            assert pkg.read_upsampled_scratch_bytes(d16, mode, 8, 4) == 2 * 256 * 35 + 256 * 35
            assert pkg.read_upsampled_scratch_bytes(d8, mode, 2, 10) == \
                2 * 256 * 10 + pkg.read_oriented_scratch_bytes(desc_for(67, 35, pkg.CHROMA_444, alpha_state=pkg.ALPHA_STRAIGHT), 2, 10)


def test_scratch_bytes_rejects():
    lib = pkg.load()
    d = desc_for(67, 35)
    for mode, code, n in ((3, 1, 10), (-1, 1, 10), (99, 6, 10), (CENTER, 0, 10), (CENTER, 9, 10), (NEAREST, 9, 10), (CENTER, 6, 68), (LEFT, 1, -1)):
        assert lib.avifgpu_read_upsampled_scratch_bytes(ctypes.byref(d), mode, code, n) == pkg.formatBadParameters, (mode, code, n)
    assert lib.avifgpu_read_upsampled_scratch_bytes(None, CENTER, 1, 10) == pkg.formatBadParameters
    assert lib.avifgpu_read_upsampled_scratch_bytes(ctypes.byref(desc_for(0, 5)), CENTER, 1, 1) == pkg.formatBadParameters


def test_read_rows_upsampled_rejects_before_any_launch():
    """The error conventions of the oriented entry: formatBadParameters with the argument's own message, none of them "no device"."""
    lib = pkg.load()
    d = desc_for(9, 7)
    planes = harness.make_read_source(d)
    ptrs = pkg.planes4([planes[i].ctypes.data if i in planes else None for i in range(4)])
    strides = pkg.strides4([planes[i].strides[0] if i in planes else 0 for i in range(4)])
    dst = np.zeros((9, 64), np.uint8)

    def call(mode, code, o, n, src=ptrs, st=strides, out=dst.ctypes.data, row_bytes=64, scratch=None, scratch_bytes=0, mem=pkg.MEM_HOST):
        rc = lib.avifgpu_read_rows_upsampled(ctypes.byref(d), mode, code, o, n, ctypes.byref(src) if src is not None else None,
                                             ctypes.byref(st) if st is not None else None, out, row_bytes, scratch, scratch_bytes, mem, None)
        return rc, lib.avifgpu_last_error()

    for mode in (3, -1, 17):
        rc, msg = call(mode, 1, 0, 1)
        assert rc == pkg.formatBadParameters and b"AVIFGPU_UPSAMPLE" in msg
    for mode in (NEAREST, CENTER):
        for code in (0, 9, -1):
            rc, msg = call(mode, code, 0, 1)
            assert rc == pkg.formatBadParameters and b"1..8" in msg
    for mode in (NEAREST, CENTER, LEFT):
        for code, o, n in ((2, 0, 8), (2, -1, 2), (6, 0, 10), (6, 8, 2), (3, 7, 1)):
            rc, msg = call(mode, code, o, n)
            assert rc == pkg.formatBadParameters and b"outside" in msg, (mode, code, o, n, msg)
        for code, o, n in ((2, 1, 2), (4, 0, 2), (6, 1, 4), (8, 0, 2), (1, 3, 2)):
            rc, msg = call(mode, code, o, n)
            assert rc == pkg.formatBadParameters and b"odd source" in msg, (mode, code, o, n, msg)
        rc, msg = call(mode, 6, 0, 4, row_bytes=7 * 3 - 1)
        assert rc == pkg.formatBadParameters and b"dst_row_bytes" in msg
        rc, msg = call(mode, 6, 0, 4, src=None)
        assert rc == pkg.formatBadParameters and b"null" in msg
        rc, msg = call(mode, 6, 0, 4, out=None)
        assert rc == pkg.formatBadParameters and b"null" in msg
        rc, msg = call(mode, 6, 0, 4, mem=7)
        assert rc == pkg.formatBadParameters and b"mem_kind" in msg
        short = pkg.strides4([planes[0].strides[0], 3, planes[2].strides[0], 0])
        rc, msg = call(mode, 6, 0, 4, st=short)
        assert rc == pkg.formatBadParameters and b"src_stride" in msg
    for code in (1, 6):
        need = pkg.read_upsampled_scratch_bytes(d, CENTER, code, 4)
        assert need > 0
        for scratch, nbytes in ((None, need), (dst.ctypes.data, need - 1), (dst.ctypes.data, 0)):
            rc, msg = call(CENTER, code, 0, 4, scratch=scratch, scratch_bytes=nbytes, mem=pkg.MEM_DEVICE)
            assert rc == pkg.formatBadParameters and b"scratch" in msg, (code, scratch, nbytes, msg)


def test_probe_upsample_rejects():
    lib = pkg.load()
    buf = np.zeros(4096, np.uint8)
    p2 = (ctypes.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    s2 = (ctypes.c_int64 * 2)(32, 32)
    null2 = (ctypes.c_void_p * 2)(None, buf.ctypes.data)
    short2 = (ctypes.c_int64 * 2)(32, 3)
    ok = dict(bps=1, chroma=pkg.CHROMA_420, mode=CENTER, W=16, H=8, x0=0, y0=0, w=16, h=8, src=p2, st=s2, dst=p2, drb=32, twin=0)
    bad = [dict(bps=3), dict(bps=0), dict(chroma=pkg.CHROMA_444), dict(mode=NEAREST), dict(mode=3), dict(W=0), dict(w=0), dict(x0=-1),
           dict(x0=1), dict(y0=1), dict(h=9), dict(src=null2), dict(dst=null2), dict(st=short2), dict(drb=15),
           dict(twin=3), dict(twin=-1), dict(twin=1, mode=LEFT)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.avifgpu_probe_upsample(a["bps"], a["chroma"], a["mode"], a["W"], a["H"], a["x0"], a["y0"], a["w"], a["h"],
                                        ctypes.byref(a["src"]), ctypes.byref(a["st"]), ctypes.byref(a["dst"]), a["drb"], a["twin"], None)
        assert rc == pkg.formatBadParameters, change
        assert b"avifgpu_probe_upsample" in lib.avifgpu_last_error(), change
