"""The oriented open on the GPU (include/avifgpu.h "oriented open", csrc/orient_kernels.hip).

The truth is always: today's avifgpu_read_rows on the same planes, then the numpy expression of the header's table; the demand is
array_equal -- floats too, because the arithmetic of a pixel does not depend on where it sits.  Shapes are the smallest at which the
kernels can still go wrong: ragged tiles in both directions, more than one tile each way, whole tiles with and without a flipped
source start on a 16-byte boundary, single rows and columns, odd sizes of subsampled planes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harness
from fake_host import FakeHost
from orientation_truth import orient

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

CODES = range(2, 9)
SENTINEL = 0xA5


def fmt(channels, depth, width, height):
    """One of the 12 host formats: gray / gray+A / RGB / RGBA at 8 / 16 / 32 bit (colour as 4:4:4 YCbCr, float through PQ)."""
    kw = dict(width=width, height=height, depth=depth, bit_depth={8: 8, 16: 12, 32: 10}[depth],
              alpha_state=pkg.ALPHA_STRAIGHT if channels in (2, 4) else pkg.ALPHA_NONE)
    if channels <= 2:
        kw.update(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME)
    else:
        kw.update(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_444, matrix_coefficients=pkg.MATRIX_BT709)
    if depth == 32:
        kw.update(transfer_characteristics=pkg.TC_PQ, color_primaries=pkg.PRIMARIES_BT2020, pq_peak_nits=203)
        if channels > 2:
            kw.update(matrix_coefficients=pkg.MATRIX_BT2020_NCL)
    return pkg.ReadDesc(**kw)


FORMATS = [(c, d) for d in (8, 16, 32) for c in (1, 2, 3, 4)]

_truth_cache = {}


def truth(gpu, desc, planes, key):
    """I of the definition as (H, W, C): avifgpu_read_rows on the whole image, computed once per case and left unchanged."""
    if key not in _truth_cache:
        flat = harness.gpu_read(gpu, desc, planes, mem="device")
        a = flat.reshape(desc.height, desc.width, harness.read_channels(desc))
        a.setflags(write=False)
        _truth_cache[key] = a
    return _truth_cache[key]


def same(a, b):
    """array_equal on the bytes: bit for bit, so that a float NaN or a -0.0 cannot hide a difference."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def tiles(desc, code, max_rows):
    out_h = pkg.read_oriented_geometry(desc, code)[1]
    o = 0
    while o < out_h:
        n = pkg.read_oriented_next_tile(desc, code, o, max_rows)
        assert n > 0
        yield o, n
        o += n


def _ptrs(desc, planes, base_fn):
    ptrs, strides = [None] * 4, [0] * 4
    for pl in harness.read_planes(desc):
        ptrs[pl] = base_fn(pl)
        strides[pl] = planes[pl].strides[0]
    return ptrs, strides


def open_oriented(gpu, desc, planes, code, mem="device", max_rows=None, pad=0, guard_rows=0, pinned=False):
    """The oriented image as (out_h, out_w, C), opened tile by tile (max_rows=None: one call).  `pad` extra bytes per destination row and
    `guard_rows` rows above and below are pre-filled with a sentinel and must come back untouched."""
    import torch
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16) + pad
    buf = np.full((out_h + 2 * guard_rows, stride), SENTINEL, dtype=np.uint8)
    cuts = list(tiles(desc, code, max_rows)) if max_rows else [(0, out_h)]
    if mem == "device":
        dev = f"cuda:{gpu.device}"
        d_pl = {pl: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for pl, a in planes.items()}
        d_out = torch.from_numpy(buf.reshape(-1).copy()).to(dev)
        ptrs, strides = _ptrs(desc, planes, lambda pl: d_pl[pl].data_ptr())
        stream = torch.cuda.current_stream(dev).cuda_stream
        for o, n in cuts:
            need = pkg.read_oriented_scratch_bytes(desc, code, n)
            scratch = torch.full((max(need, 16),), 0x5A, dtype=torch.uint8, device=dev)
            gpu.read_rows_oriented(desc, code, o, n, ptrs, strides, d_out.data_ptr() + (guard_rows + o) * stride, stride,
                                   scratch.data_ptr(), need, mem=pkg.MEM_DEVICE, stream=stream)
        torch.cuda.synchronize(dev)
        buf = d_out.cpu().numpy().reshape(buf.shape)
    else:
        keep = []
        if pinned:
            host_planes = {}
            for pl, a in planes.items():
                t = torch.from_numpy(a.copy()).pin_memory()
                keep.append(t)
                host_planes[pl] = t.numpy()
            t = torch.from_numpy(buf).pin_memory()
            keep.append(t)
            buf = t.numpy()
        else:
            host_planes = planes
        ptrs, strides = _ptrs(desc, host_planes, lambda pl: host_planes[pl].ctypes.data)
        for o, n in cuts:
            gpu.read_rows_oriented(desc, code, o, n, ptrs, strides, buf.ctypes.data + (guard_rows + o) * stride, stride, mem=pkg.MEM_HOST)
        buf = buf.copy()
    body = buf[guard_rows:guard_rows + out_h]
    assert (body[:, row_bytes:] == SENTINEL).all(), "bytes beyond out_w * bytes per pixel were touched"
    if guard_rows:
        assert (buf[:guard_rows] == SENTINEL).all() and (buf[guard_rows + out_h:] == SENTINEL).all(), "rows outside the call were touched"
    return np.ascontiguousarray(body[:, :row_bytes]).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


# ---- every code x every host format: ragged tiles both ways, more than one tile each way, whole tiles ----------------------------
def test_every_code_every_format(gpu):
    """67 x 35: ragged tiles only; 130 x 66: whole and ragged tiles, a flipped source start off the 16-byte grid for most pixel sizes;
    128 x 96: whole tiles only, every path aligned.  One test for all 36 cases: each is a few milliseconds, the message says which."""
    for size in ((67, 35), (130, 66), (128, 96)):
        for channels, depth in FORMATS:
            desc = fmt(channels, depth, *size)
            planes = harness.make_read_source(desc, seed=channels * 100 + depth)
            I = truth(gpu, desc, planes, ("fmt", channels, depth, size))
            for code in CODES:
                got = open_oriented(gpu, desc, planes, code)
                assert same(got, orient(code, I)), (code, channels, depth, size)


def test_degenerate_sizes(gpu):
    for size in ((1, 1), (1, 70), (70, 1)):
        for channels, depth in ((1, 8), (3, 8), (4, 16), (3, 32)):
            desc = fmt(channels, depth, *size)
            planes = harness.make_read_source(desc, seed=7)
            I = truth(gpu, desc, planes, ("deg", channels, depth, size))
            for code in CODES:
                for mem in ("device", "host"):
                    assert same(open_oriented(gpu, desc, planes, code, mem=mem), orient(code, I)), (code, channels, depth, size, mem)


# ---- subsampled chroma: the pixel-domain definition at odd and even sizes, tile by tile ------------------------------------------
SUBSAMPLED = [
    dict(chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT601),
    dict(chroma=pkg.CHROMA_422, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT709),
    dict(chroma=pkg.CHROMA_420, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=pkg.MATRIX_BT2020_NCL, full_range_flag=0),
    dict(chroma=pkg.CHROMA_422, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT709),
    dict(chroma=pkg.CHROMA_420, bit_depth=12, depth=32, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
         color_primaries=pkg.PRIMARIES_BT2020, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000),
    dict(chroma=pkg.CHROMA_422, bit_depth=12, depth=32, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
         color_primaries=pkg.PRIMARIES_BT2020, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=203),
]


def test_subsampled_chroma_tile_invariance(gpu):
    """4:2:0 and 4:2:2 at 8 and 12 bit, straight and premultiplied alpha, PQ to f32, odd (33 x 31) and even (34 x 32) sizes: one whole
    call, and tiles cut by next_tile with max_rows 1, 7 and 64, all equal to the definition."""
    for size in ((33, 31), (34, 32)):
        for i, kw in enumerate(SUBSAMPLED):
            desc = pkg.ReadDesc(width=size[0], height=size[1], colorspace=pkg.COLORSPACE_YCBCR, **kw)
            planes = harness.make_read_source(desc, seed=size[0])
            I = truth(gpu, desc, planes, ("sub", i, size))
            for code in range(1, 9):
                want = orient(code, I)
                assert same(open_oriented(gpu, desc, planes, code), want), (size, i, code, "whole")
                for max_rows in (1, 7, 64):
                    assert same(open_oriented(gpu, desc, planes, code, max_rows=max_rows), want), (size, i, code, max_rows)
                assert same(open_oriented(gpu, desc, planes, code, mem="host", max_rows=7), want), (size, i, code, "host tiles")


RGB_AND_MONO = [
    dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=10, depth=16, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=pkg.MATRIX_RGB_GBR),
    dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_RGB_GBR),
    dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=12, depth=32, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_RGB_GBR,
         color_primaries=pkg.PRIMARIES_BT2020, transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=1),
    dict(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_STRAIGHT),
    dict(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_PREMULTIPLIED),
]


def test_planar_rgb_and_monochrome_with_alpha(gpu):
    for i, kw in enumerate(RGB_AND_MONO):
        desc = pkg.ReadDesc(width=67, height=35, **kw)
        planes = harness.make_read_source(desc, seed=11)
        I = truth(gpu, desc, planes, ("rgbmono", i))
        for code in CODES:
            assert same(open_oriented(gpu, desc, planes, code), orient(code, I)), (i, code)
            assert same(open_oriented(gpu, desc, planes, code, mem="host"), orient(code, I)), (i, code, "host")


# ---- buffers: padded destination rows, guard rows, source strides that are no multiple of 16 ------------------------------------
def test_padding_guard_rows_and_unaligned_strides(gpu):
    for channels, depth in ((1, 8), (3, 8), (4, 8), (3, 16), (3, 32), (4, 32)):
        desc = fmt(channels, depth, 130, 66)
        planes = harness.make_read_source(desc, seed=5, stride_pad=3)      # strides of 139 samples: no multiple of 16 bytes at either sample size
        assert all(a.strides[0] % 16 for a in planes.values())
        I = truth(gpu, desc, planes, ("pad", channels, depth))
        for code in CODES:
            want = orient(code, I)
            assert same(open_oriented(gpu, desc, planes, code, pad=48, guard_rows=2), want), (channels, depth, code)
            assert same(open_oriented(gpu, desc, planes, code, pad=48, guard_rows=2, max_rows=7), want), (channels, depth, code, "tiles")
            assert same(open_oriented(gpu, desc, planes, code, mem="host", pad=48, guard_rows=2), want), (channels, depth, code, "host")
            assert same(open_oriented(gpu, desc, planes, code, pad=4, guard_rows=1), want), (channels, depth, code, "destination stride no multiple of 16")


# ---- HOST path: equals DEVICE for every number of bound contexts, pinned and pageable -------------------------------------------
def test_host_equals_device_for_every_context_count(gpu):
    cases = [fmt(3, 8, 130, 66), fmt(4, 16, 67, 35), fmt(3, 32, 130, 66),
             pkg.ReadDesc(width=33, height=31, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[0])]
    sources = [harness.make_read_source(d, seed=21 + i) for i, d in enumerate(cases)]
    device = [{code: open_oriented(gpu, d, p, code) for code in range(1, 9)} for d, p in zip(cases, sources)]
    truths = [truth(gpu, d, p, ("ctx", i)) for i, (d, p) in enumerate(zip(cases, sources))]
    try:
        for n in (1, 2, 3):
            g = pkg.AvifGpu(devices=[gpu.device] * n)
            for i, (d, p) in enumerate(zip(cases, sources)):
                for code in range(1, 9):
                    for pinned in (False, True):
                        got = open_oriented(g, d, p, code, mem="host", pinned=pinned)
                        assert same(got, device[i][code]) and same(got, orient(code, truths[i])), (n, i, code, pinned)
    finally:
        pkg.AvifGpu(gpu.device)                                            # the session's binding


def test_host_stages_more_than_one_tile(gpu):
    """A whole-image HOST call on an image larger than one staged tile (32 MiB of output): both slots, several column bands."""
    desc = fmt(4, 32, 2048, 1100)                                          # 36 MB of output
    planes = harness.make_read_source(desc, seed=3)
    I = truth(gpu, desc, planes, ("hosttiles",))
    for code in (3, 6):
        assert same(open_oriented(gpu, desc, planes, code, mem="host"), orient(code, I)), code


def test_rgb_f32_2048x1024_per_transposing_code(gpu):
    desc = fmt(3, 32, 2048, 1024)
    planes = harness.make_read_source(desc, seed=2048)
    I = truth(gpu, desc, planes, ("big",))
    for code in (5, 6, 7, 8):
        assert same(open_oriented(gpu, desc, planes, code), orient(code, I)), code


def test_probe_orient_alone(gpu):
    """The kernels alone, every pixel size and code.  128 x 96: whole tiles; 2101 x 5 and 2100 x 70: rows long enough for whole spans of
    the row-mapped kernel's LDS strip (3-, 6- and 12-byte pixels: 1024, 512 and 256 pixels) and register path, with row lengths that are
    no multiple of 16 bytes -- a flipped x then reads every source chunk off the 16-byte grid -- and whole transposed tiles whose flipped
    source columns start off it.  Rows padded to 256 bytes (the aligned paths, as the library's own scratch), then tight (per pixel)."""
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(9)
    for w, h in ((128, 96), (2101, 5), (2100, 70)):
        for bpp in (1, 2, 3, 4, 6, 8, 12, 16):
            src = rng.integers(0, 256, size=(h, w, bpp), dtype=np.uint8)
            for padded in (True, False):
                sp = harness.align(w * bpp, 256) if padded else w * bpp
                wide = np.zeros((h, sp), np.uint8)
                wide[:, :w * bpp] = src.reshape(h, -1)
                d_src = torch.from_numpy(wide.reshape(-1)).to(dev)
                for code in CODES:
                    want = np.ascontiguousarray(orient(code, src))
                    oh, ow = want.shape[:2]
                    dp = harness.align(ow * bpp, 256) if padded else ow * bpp
                    d_dst = torch.full((oh * dp,), SENTINEL, dtype=torch.uint8, device=dev)
                    gpu.probe_orient(code, bpp, w, h, d_src.data_ptr(), sp, d_dst.data_ptr(), dp, None)
                    torch.cuda.synchronize(dev)
                    got = d_dst.cpu().numpy().reshape(oh, dp)
                    assert np.array_equal(got[:, :ow * bpp].reshape(want.shape), want), (w, h, bpp, code, padded)
                    assert (got[:, ow * bpp:] == SENTINEL).all(), (w, h, bpp, code, padded)


# ---- the FormatRecord shim ---------------------------------------------------------------------------------------------------
def _shim_open(gpu, desc, planes, code, max_data, abort_after=None):
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    host = FakeHost(out_w, out_h, desc.depth, nch, max_data=max_data, abort_after=abort_after)
    img = H.Image(width=desc.width, height=desc.height, colorspace=desc.colorspace, chroma=desc.chroma, bit_depth=desc.bit_depth)
    for pl, a in planes.items():
        img.plane[pl] = a.ctypes.data
        img.stride[pl] = a.strides[0]
    nclx = H.Nclx(desc.color_primaries, desc.transfer_characteristics, desc.matrix_coefficients, desc.full_range_flag)
    code = gpu.lib.avifgpu_host_read_heif_image_oriented(ctypes.byref(img), code, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(host.fr))
    return host, code


def test_shim_delivers_oriented_tiles(gpu):
    cases = [(fmt(3, 8, 67, 35), "rgb8"),
             (pkg.ReadDesc(width=34, height=31, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[0]), "420 odd H")]
    for desc, name in cases:
        planes = harness.make_read_source(desc, seed=17)
        I = truth(gpu, desc, planes, ("shim", name))
        nch = harness.read_channels(desc)
        for code in (3, 6, 8):
            out_w, out_h = pkg.read_oriented_geometry(desc, code)
            row_bytes = out_w * nch * (desc.depth // 8)
            max_data = row_bytes * (out_h // 6)                            # at least 6 tiles
            host, rc = _shim_open(gpu, desc, planes, code, max_data)
            assert rc == 0, gpu.lib.avifgpu_last_error()
            assert same(host.image.reshape(out_h, out_w, nch), orient(code, I)), (name, code)
            assert len(host.rects) >= 5 and host.rects[0][0] == 0 and host.rects[-1][2] == out_h
            assert all(a[2] == b[0] for a, b in zip(host.rects[:-1], host.rects[1:]))
            assert all(r[1] == 0 and r[3] == out_w and (r[2] - r[0]) * row_bytes <= max_data for r in host.rects)
            assert host.polls == len(host.rects) and host.fr.rowBytes == row_bytes
            # the tiles are avifgpu_read_oriented_next_tile's
            assert [(r[0], r[2] - r[0]) for r in host.rects] == list(tiles(desc, code, out_h // 6))


def test_shim_cancel_wrong_size_and_next_open_intact(gpu):
    desc = fmt(3, 8, 67, 35)
    planes = harness.make_read_source(desc, seed=17)
    I = truth(gpu, desc, planes, ("shim", "rgb8"))
    host, rc = _shim_open(gpu, desc, planes, 6, 35 * 3 * 8, abort_after=2)
    assert rc == pkg.userCanceledErr and len(host.rects) == 2              # tiles 0 and 1 were delivered, tile 2 was not started
    host, rc = _shim_open(gpu, desc, planes, 6, 35 * 3 * 8)
    assert rc == 0 and same(host.image.reshape(67, 35, 3), orient(6, I))
    # a document of the stored size for a quarter turn, and a code outside 1..8
    img = H.Image(width=67, height=35, colorspace=desc.colorspace, chroma=desc.chroma, bit_depth=8)
    for pl, a in planes.items():
        img.plane[pl] = a.ctypes.data
        img.stride[pl] = a.strides[0]
    nclx = H.Nclx(desc.color_primaries, desc.transfer_characteristics, desc.matrix_coefficients, desc.full_range_flag)
    wrong = FakeHost(67, 35, 8, 3)
    assert gpu.lib.avifgpu_host_read_heif_image_oriented(ctypes.byref(img), 6, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(wrong.fr)) == pkg.formatBadParameters
    assert gpu.lib.avifgpu_host_read_heif_image_oriented(ctypes.byref(img), 9, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(wrong.fr)) == pkg.formatBadParameters
    assert not wrong.rects
    # orientation 1 is the plain open
    assert gpu.lib.avifgpu_host_read_heif_image_oriented(ctypes.byref(img), 1, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(wrong.fr)) == 0
    assert same(wrong.image.reshape(35, 67, 3), I)


def test_cli_read_orientation_6(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avif-format_amd", "avifgpu_cli")
    desc = pkg.ReadDesc(width=203, height=37, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8,
                        alpha_state=pkg.ALPHA_NONE, has_nclx=0, color_primaries=0, transfer_characteristics=0, matrix_coefficients=0)
    planes = harness.make_read_source(desc, seed=8)
    want = open_oriented(gpu, desc, planes, 6)                             # the binding
    with open(tmp_path / "in.planes", "wb") as f:
        for pl, (w, xs, ys) in harness.read_planes(desc).items():
            f.write(np.ascontiguousarray(planes[pl][:, :w]).tobytes())
    r = subprocess.run([cli, "read", "--width", "203", "--height", "37", "--depth", "8", "--bits", "8", "--colorspace", "ycbcr", "--chroma", "420",
                        "--orientation", "6", "--maxdata", str(37 * 3 * 40), str(tmp_path / "in.planes"), str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(203, 37, 3)
    assert same(got, want)
    assert same(got, orient(6, truth(gpu, desc, planes, ("cli",))))
