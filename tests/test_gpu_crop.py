"""The cropped open on the GPU (include/avifgpu.h "cropped open", csrc/crop_kernels.hip).

The expected image is always the definition: the whole image's un-oriented open, sliced, then oriented (tests/crop_truth.py).  8- and
16-bit hosts: array_equal against harness.oracle_read of the whole image (for the bilinear modes: tests/upsample_truth.py followed by the
oracle's 4:4:4 open, as tests/test_gpu_upsample.py has it).  32-bit hosts: bits against the GPU's own whole-image open (avifgpu_read_rows /
avifgpu_read_rows_upsampled code 1), and the T2 read bar of tests/test_gpu_read.py (|gpu - oracle| <= 1e-4 |oracle| + 1e-9) against the
oracle.

Shapes are the smallest at which the code as built can go wrong: the mover's lane owns 16 bytes of a destination row on the destination's
16-byte grid, a wave 1024, with a ragged head and tail of up to 15 bytes; the dispatcher takes another path for every parity of x0 / y0 in
a subsampled direction, for a single row / column, for the whole image, for code 1 against codes 2-8 and for nearest against bilinear.

The cases are grouped under one test id (the last section of this file); every group runs even when an earlier one failed."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import crop_truth
import harness
from fake_host import FakeHost
from upsample_truth import CENTER, LEFT, NEAREST, upsample_planes

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
T2_RTOL, T2_ATOL = 1e-4, 1e-9                                  # tests/test_gpu_read.py
CODES = range(1, 9)


def same(a, b):
    """array_equal on the bytes: bit for bit, so that a float NaN or a -0.0 cannot hide a difference."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def interpolated(desc, mode):
    return mode != NEAREST and desc.colorspace == pkg.COLORSPACE_YCBCR and desc.chroma in (pkg.CHROMA_420, pkg.CHROMA_422)


def _whole_gpu(gpu, desc, planes, mode):
    """F of the definition, from the existing entries: avifgpu_read_rows, or avifgpu_read_rows_upsampled with code 1."""
    import torch
    if not interpolated(desc, mode):
        return harness.gpu_read(gpu, desc, planes).reshape(desc.height, desc.width, -1)
    dev = f"cuda:{gpu.device}"
    nch = harness.read_channels(desc)
    row_bytes = desc.width * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16)
    used = harness.read_planes(desc)
    d_pl = {pl: torch.from_numpy(planes[pl].view(np.uint8).reshape(-1).copy()).to(dev) for pl in used}
    d_out = torch.zeros((desc.height * stride,), dtype=torch.uint8, device=dev)
    ptrs = [d_pl[pl].data_ptr() if pl in used else None for pl in range(4)]
    strides = [planes[pl].strides[0] if pl in used else 0 for pl in range(4)]
    need = max(pkg.read_upsampled_scratch_bytes(desc, mode, 1, desc.height), 16)
    scratch = torch.zeros((need,), dtype=torch.uint8, device=dev)
    gpu.read_rows_upsampled(desc, mode, 1, 0, desc.height, ptrs, strides, d_out.data_ptr(), stride, scratch.data_ptr(), need, mem=pkg.MEM_DEVICE,
                            stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = d_out.cpu().numpy().reshape(desc.height, stride)[:, :row_bytes]
    return np.ascontiguousarray(got).view(harness.src_dtype(desc.depth)).reshape(desc.height, desc.width, nch)


_refs = {}


def refs(gpu, desc, planes, mode, key):
    """(oracle image of the WHOLE picture, the GPU's own whole-image open -- depth 32 only) as (H, W, C), computed once per key."""
    key = (key, mode if interpolated(desc, mode) else NEAREST)
    if key not in _refs:
        shape = (desc.height, desc.width, harness.read_channels(desc))
        if interpolated(desc, mode):
            xs, ys = harness.chroma_shift(desc.chroma)
            d4 = pkg.ReadDesc.from_buffer_copy(desc)
            d4.chroma = pkg.CHROMA_444
            want = harness.oracle_read(d4, upsample_planes(planes, desc.width, desc.height, xs, ys, mode)).reshape(shape)
        else:
            want = harness.oracle_read(desc, planes).reshape(shape)
        own = _whole_gpu(gpu, desc, planes, mode) if desc.depth == 32 else None
        want.setflags(write=False)
        _refs[key] = (want, own)
    return _refs[key]


def check(got, desc, ref, rect, code, what):
    want, own = ref
    if desc.depth != 32:
        assert same(got, crop_truth.cropped(want, rect, code)), what
        return
    assert same(got, crop_truth.cropped(own, rect, code)), (what, "against the GPU's own whole-image open")
    w64, g64 = np.ascontiguousarray(crop_truth.cropped(want, rect, code)).astype(np.float64), got.astype(np.float64)
    assert np.all(np.isfinite(g64)), what
    assert np.all(np.abs(g64 - w64) <= T2_RTOL * np.abs(w64) + T2_ATOL), (what, "T2 read bar against the oracle")


def helper_tiles(desc, rect, mode, code, max_rows):
    out_h = pkg.read_cropped_geometry(desc, rect, code)[1]
    o = 0
    while o < out_h:
        n = pkg.read_cropped_next_tile(desc, rect, mode, code, o, max_rows)
        assert n > 0
        yield o, n
        o += n


def fixed_tiles(desc, rect, code, rows):
    out_h = pkg.read_cropped_geometry(desc, rect, code)[1]
    return [(o, min(rows, out_h - o)) for o in range(0, out_h, rows)]


def open_cropped(gpu, desc, planes, rect, mode=NEAREST, code=1, mem="device", max_rows=None, cuts=None, pad=0, guard_rows=0, pinned=False, base_off=0,
                 dst_off=0, kernel_names=None):
    """The cropped image as (out_h, out_w, C), opened tile by tile (max_rows: the helper's tiles; cuts: given ones; neither: one call).
    `pad` extra bytes per destination row, `dst_off` bytes in front of the first row and `guard_rows` rows above and below are pre-filled
    with a sentinel and must come back untouched; `base_off` bytes in front of every source plane put its base off the 16-byte grid."""
    import torch
    out_w, out_h = pkg.read_cropped_geometry(desc, rect, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16) + pad
    flat = np.full((dst_off + (out_h + 2 * guard_rows) * stride,), SENTINEL, dtype=np.uint8)
    if cuts is None:
        cuts = list(helper_tiles(desc, rect, mode, code, max_rows)) if max_rows else [(0, out_h)]
    used = harness.read_planes(desc)
    strides = [planes[pl].strides[0] if pl in used else 0 for pl in range(4)]
    if mem == "device":
        dev = f"cuda:{gpu.device}"
        d_pl = {}
        for pl in used:
            d_pl[pl] = torch.from_numpy(np.concatenate([np.zeros(base_off, np.uint8), planes[pl].view(np.uint8).reshape(-1)])).to(dev)
        d_out = torch.from_numpy(flat.copy()).to(dev)
        ptrs = [d_pl[pl].data_ptr() + base_off if pl in used else None for pl in range(4)]
        stream = torch.cuda.current_stream(dev).cuda_stream
        bound = max([pkg.read_cropped_scratch_bytes(desc, rect, mode, code, n) for _, n in cuts] + [16])
        scratch = torch.full((bound,), 0x5A, dtype=torch.uint8, device=dev)
        for o, n in cuts:
            gpu.read_rows_cropped(desc, rect, mode, code, o, n, ptrs, strides, d_out.data_ptr() + dst_off + (guard_rows + o) * stride, stride,
                                  scratch.data_ptr(), bound, mem=pkg.MEM_DEVICE, stream=stream)
            if kernel_names is not None:
                kernel_names.append(gpu.last_kernel())
        torch.cuda.synchronize(dev)
        flat = d_out.cpu().numpy()
    else:
        keep = []
        if pinned:
            host_planes = {}
            for pl in used:
                t = torch.from_numpy(planes[pl].copy()).pin_memory()
                keep.append(t)
                host_planes[pl] = t.numpy()
            t = torch.from_numpy(flat).pin_memory()
            keep.append(t)
            flat = t.numpy()
        else:
            host_planes = planes
        ptrs = [host_planes[pl].ctypes.data if pl in used else None for pl in range(4)]
        for o, n in cuts:
            gpu.read_rows_cropped(desc, rect, mode, code, o, n, ptrs, strides, flat.ctypes.data + dst_off + (guard_rows + o) * stride, stride, mem=pkg.MEM_HOST)
        flat = flat.copy()
    assert (flat[:dst_off] == SENTINEL).all(), "bytes in front of the destination were touched"
    buf = flat[dst_off:].reshape(out_h + 2 * guard_rows, stride)
    body = buf[guard_rows:guard_rows + out_h]
    assert (body[:, row_bytes:] == SENTINEL).all(), "bytes beyond out_w * bytes per pixel were touched"
    if guard_rows:
        assert (buf[:guard_rows] == SENTINEL).all() and (buf[guard_rows + out_h:] == SENTINEL).all(), "rows outside the call were touched"
    return np.ascontiguousarray(body[:, :row_bytes]).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


# ---- the mover alone ----------------------------------------------------------------------------------------------------------------------------
def _probe_crop_alone(gpu):
    """Every row payload around a lane (16), a wave (1024) and a workgroup (4096), heights around the grid's row loop, every source byte
    offset of a pixel and a row in, destinations on and off the 16-byte grid with strides that are and are not multiples of 16.  Sentinel
    bytes beyond each row and guard rows above and below must come back untouched."""
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(5)
    pitch = 4352                                               # the library's scratch: rows of a multiple of 256 bytes
    src = rng.integers(0, 256, size=(36 * pitch,), dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    n = 0
    for rb, rows in itertools.product((1, 15, 16, 17, 1023, 1024, 1025, 4097), (1, 2, 33)):
        for soff, (doff, dstride_extra) in itertools.product((0, 1, 2, 3, 6, 8, 12, 17), ((0, 0), (16, 16), (5, 3), (12, 7), (1, 16))):
            if (soff + doff + rb + rows) % 3 and rb > 17 and rows == 33:
                continue                                       # a third of the large combinations is enough: every offset still meets every base
            dstride = harness.align(rb, 16) + 16 + dstride_extra
            total = doff + (rows + 2) * dstride
            d_dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
            assert soff + (rows - 1) * pitch + rb <= src.size and doff + dstride + (rows - 1) * dstride + rb <= total
            gpu.probe_crop(d_src.data_ptr() + soff, pitch, d_dst.data_ptr() + doff + dstride, dstride, rb, rows, None)
            torch.cuda.synchronize(dev)
            got = d_dst.cpu().numpy()
            what = (rb, rows, soff, doff, dstride)
            assert (got[:doff + dstride] == SENTINEL).all() and (got[doff + (rows + 1) * dstride:] == SENTINEL).all(), (what, "guard rows")
            body = got[doff + dstride:doff + (rows + 1) * dstride].reshape(rows, dstride)
            want = np.stack([src[soff + r * pitch:soff + r * pitch + rb] for r in range(rows)])
            assert np.array_equal(body[:, :rb], want), what
            assert (body[:, rb:] == SENTINEL).all(), (what, "bytes beyond the payload")
            n += 1
    assert n > 500


# ---- every phase ----------------------------------------------------------------------------------------------------------------------------------
def _pq(**kw):
    return dict(transfer_characteristics=pkg.TC_PQ, color_primaries=pkg.PRIMARIES_BT2020, matrix_coefficients=pkg.MATRIX_BT2020_NCL, pq_peak_nits=1000, **kw)


FORMATS = [
    ("420-8", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT601)),
    ("422-8", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_422, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT709)),
    ("420-12-16", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_PREMULTIPLIED,
                       matrix_coefficients=pkg.MATRIX_BT2020_NCL, full_range_flag=0)),
    ("420-10-32-pq", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=10, depth=32, alpha_state=pkg.ALPHA_NONE, **_pq())),
    ("422-10-32-hlg-ootf", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_422, bit_depth=10, depth=32, alpha_state=pkg.ALPHA_NONE,
                                transfer_characteristics=pkg.TC_HLG, color_primaries=pkg.PRIMARIES_BT2020, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                                hlg_apply_ootf=1, hlg_display_gamma=1.2, hlg_peak_nits=1000, pq_peak_nits=1000)),
    ("444-8", dict(colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_444, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT709)),
    ("gray-alpha-12-16", dict(colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_STRAIGHT)),
    ("rgb-10-16", dict(colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=10, depth=16, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_RGB_GBR)),
]


def phase_rects(W, Hh):
    """(x0, y0) over {0, 1, 2, 3}^2 with right and bottom edges of both parities -- the image's own edge among them -- then width 1 and
    height 1 at every parity."""
    out = []
    for i, (x0, y0) in enumerate(itertools.product(range(4), range(4))):
        right = (W, W - 1, W - 2, x0 + 9)[i % 4]
        bottom = (Hh, Hh - 1, Hh - 2, y0 + 6)[(i // 4 + i) % 4]
        out.append((x0, y0, right - x0, bottom - y0))
    for x0, y0 in ((1, 1), (2, 3), (3, 2), (W - 1, Hh - 1)):
        out += [(x0, y0, 1, min(7, Hh - y0)), (x0, y0, min(9, W - x0), 1), (x0, y0, 1, 1)]
    return out


def _every_phase_every_format(gpu):
    differs = 0
    for (W, Hh), (name, kw) in itertools.product(((37, 21), (38, 22)), FORMATS):
        desc = pkg.ReadDesc(width=W, height=Hh, **kw)
        planes = harness.make_read_source(desc, seed=W + len(name))
        rects = phase_rects(W, Hh)
        assert {(r[0], r[1]) for r in rects[:16]} == set(itertools.product(range(4), repeat=2))
        assert {((r[0] + r[2]) % 2, (r[1] + r[3]) % 2) for r in rects[:16]} == set(itertools.product((0, 1), repeat=2))
        assert any(r[0] + r[2] == W for r in rects) and any(r[1] + r[3] == Hh for r in rects)
        for mode in (NEAREST, CENTER, LEFT):
            if mode == LEFT and name not in ("420-8", "422-10-32-hlg-ootf"):
                continue
            ref = refs(gpu, desc, planes, mode, ("phase", name, W))
            for rect in rects:
                got = open_cropped(gpu, desc, planes, rect, mode, 1)
                check(got, desc, ref, rect, 1, (name, W, mode, rect))
                # what advanced plane pointers would give: the same call with the start rounded down to even, shifted back
                if mode == NEAREST and kw["chroma"] in (pkg.CHROMA_420, pkg.CHROMA_422) and kw["colorspace"] == pkg.COLORSPACE_YCBCR and rect[0] % 2 and rect[2] > 1:
                    even = (rect[0] - 1, rect[1], rect[2], rect[3])
                    differs += not same(open_cropped(gpu, desc, planes, even, mode, 1), got)
            # all eight codes where both starts are odd, and at one even / odd mix
            for rect in ((1, 1, W - 2, Hh - 3), (3, 1, W - 3, Hh - 1), (2, 3, 9, 6)):
                for code in CODES:
                    check(open_cropped(gpu, desc, planes, rect, mode, code), desc, ref, rect, code, (name, W, mode, rect, code))
    assert differs > 0, "an odd x0 never differed from the pointer-offset image: the phase is not exercised"


# ---- bilinear halo ------------------------------------------------------------------------------------------------------------------------------
def _bilinear_halo(gpu):
    """An interior rectangle equals the slice of the whole bilinear open -- a clamp at the rectangle's edge instead of the plane's shows
    here -- and so does a rectangle touching each plane edge."""
    for name, kw in (FORMATS[0], FORMATS[1], FORMATS[2], FORMATS[3]):
        desc = pkg.ReadDesc(width=67, height=35, **kw)
        planes = harness.make_read_source(desc, seed=67)
        for mode in (CENTER, LEFT):
            ref = refs(gpu, desc, planes, mode, ("halo", name))
            for rect in ((10, 6, 40, 20), (11, 7, 41, 21), (0, 5, 30, 20), (20, 0, 30, 20), (30, 5, 37, 20), (5, 10, 30, 25), (1, 1, 66, 34), (0, 0, 66, 35), (0, 0, 67, 34)):
                for code, mem in ((1, "device"), (6, "device"), (1, "host"), (7, "host")):
                    check(open_cropped(gpu, desc, planes, rect, mode, code, mem=mem), desc, ref, rect, code, (name, mode, rect, code, mem))


# ---- tile invariance ----------------------------------------------------------------------------------------------------------------------------
def _tile_invariance(gpu):
    """Tiles of 1, 2 and 7 rows from the helper and fixed 3-row tiles (odd absolute starts): the single call, byte for byte, device and host."""
    for (name, kw), (size, rect) in itertools.product((FORMATS[0], FORMATS[1], FORMATS[2], FORMATS[4]), (((37, 21), (1, 1, 35, 19)), ((38, 22), (2, 3, 33, 18)), ((37, 21), (0, 0, 37, 21)))):
        desc = pkg.ReadDesc(width=size[0], height=size[1], **kw)
        planes = harness.make_read_source(desc, seed=size[0])                # one source per (format, size): the reference is shared by its rectangles
        for mode in (NEAREST, CENTER):
            ref = refs(gpu, desc, planes, mode, ("tile", name, size))
            for code in CODES:
                whole = open_cropped(gpu, desc, planes, rect, mode, code)
                check(whole, desc, ref, rect, code, (name, rect, mode, code, "whole"))
                for mem in ("device", "host"):
                    if mem == "host" and code not in (1, 4, 6, 7):
                        continue
                    for max_rows in (1, 2, 7):
                        assert same(open_cropped(gpu, desc, planes, rect, mode, code, mem=mem, max_rows=max_rows), whole), (name, rect, mode, code, mem, max_rows)
                    assert same(open_cropped(gpu, desc, planes, rect, mode, code, mem=mem, cuts=fixed_tiles(desc, rect, code, 3)), whole), (name, rect, mode, code, mem, "3-row tiles")


# ---- the whole-image rectangle and the zero-copy condition -------------------------------------------------------------------------------------------
def _open_today(gpu, desc, planes, mode, code):
    import torch
    dev = f"cuda:{gpu.device}"
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16)
    used = harness.read_planes(desc)
    d_pl = {pl: torch.from_numpy(planes[pl].view(np.uint8).reshape(-1).copy()).to(dev) for pl in used}
    d_out = torch.full((out_h * stride,), SENTINEL, dtype=torch.uint8, device=dev)
    ptrs = [d_pl[pl].data_ptr() if pl in used else None for pl in range(4)]
    strides = [planes[pl].strides[0] if pl in used else 0 for pl in range(4)]
    need = max(pkg.read_upsampled_scratch_bytes(desc, mode, code, out_h), pkg.read_oriented_scratch_bytes(desc, code, out_h), 16)
    scratch = torch.zeros((need,), dtype=torch.uint8, device=dev)
    gpu.read_rows_upsampled(desc, mode, code, 0, out_h, ptrs, strides, d_out.data_ptr(), stride, scratch.data_ptr(), need, mem=pkg.MEM_DEVICE,
                            stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = d_out.cpu().numpy().reshape(out_h, stride)[:, :row_bytes]
    return np.ascontiguousarray(got).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


def _whole_image_rect_is_the_existing_entries(gpu):
    for name, kw in FORMATS:
        desc = pkg.ReadDesc(width=67, height=35, **kw)
        planes = harness.make_read_source(desc, seed=31)
        for mode, code in itertools.product((NEAREST, CENTER, LEFT), (1, 3, 6)):
            today = _open_today(gpu, desc, planes, mode, code)
            for mem in ("device", "host"):
                assert same(open_cropped(gpu, desc, planes, (0, 0, 67, 35), mode, code, mem=mem), today), (name, mode, code, mem)


def _zero_copy_condition(gpu):
    """An even-phase code-1 nearest call launches what avifgpu_read_rows launches for an image of the rectangle's size, and nothing else;
    an odd phase runs the mover."""
    import torch
    for name, kw in (FORMATS[0], FORMATS[1], FORMATS[3], FORMATS[5]):
        desc = pkg.ReadDesc(width=160, height=70, **kw)              # every plane's pitch is a multiple of 16 bytes
        planes = harness.make_read_source(desc, seed=9)
        assert all(a.strides[0] % 16 == 0 for a in planes.values())
        ref = refs(gpu, desc, planes, NEAREST, ("zero", name))
        sub = pkg.ReadDesc.from_buffer_copy(desc)
        sub.width, sub.height = 96, 40
        harness.gpu_read(gpu, sub, harness.make_read_source(sub, seed=1, stride_pad=16))     # pitches beyond the row, as a rectangle's are
        want_name = gpu.last_kernel()
        assert want_name.startswith("read_px"), want_name
        # x0 a multiple of 32 samples: the advanced pointers stay on the 16-byte grid the rect-sized image's own buffers are on
        names = []
        rect = (32, 2, 96, 40)
        check(open_cropped(gpu, desc, planes, rect, NEAREST, 1, kernel_names=names), desc, ref, rect, 1, (name, "even phase"))
        assert names == [want_name], (name, names, want_name)
        assert pkg.read_cropped_scratch_bytes(desc, (32, 2, 96, 40), NEAREST, 1, 40) == 0 or harness.chroma_shift(desc.chroma)[1]
        if name != "444-8":
            names = []
            rect = (33, 3, 96, 40)
            check(open_cropped(gpu, desc, planes, rect, NEAREST, 1, kernel_names=names), desc, ref, rect, 1, (name, "odd phase"))
            assert len(names) == 1 and names[0].startswith("crop_rows"), (name, names)
    torch.cuda.synchronize()


# ---- buffers -----------------------------------------------------------------------------------------------------------------------------------
def _unaligned_buffers_padding_guard_rows_and_rejections(gpu):
    import torch
    for i, (name, kw) in enumerate((FORMATS[0], FORMATS[2], FORMATS[3], FORMATS[6])):
        desc = pkg.ReadDesc(width=130, height=66, **kw)
        planes = harness.make_read_source(desc, seed=5 + i, stride_pad=3)             # strides that are no multiple of 16 (nor of 8) bytes
        off = 6 if desc.bit_depth > 8 else 3
        for mode in (NEAREST, CENTER):
            ref = refs(gpu, desc, planes, mode, ("pad", name))
            for rect, code in itertools.product(((3, 5, 120, 55), (2, 4, 121, 57)), (1, 2, 6, 7)):
                check(open_cropped(gpu, desc, planes, rect, mode, code, pad=48, guard_rows=2, base_off=off), desc, ref, rect, code, (name, mode, rect, code, "base and stride"))
                check(open_cropped(gpu, desc, planes, rect, mode, code, pad=5, guard_rows=1, base_off=16, dst_off=7), desc, ref, rect, code, (name, mode, rect, code, "destination off the grid"))
                check(open_cropped(gpu, desc, planes, rect, mode, code, mem="host", pad=48, guard_rows=2, max_rows=20), desc, ref, rect, code, (name, mode, rect, code, "host"))
    # dst stays sentinel after every rejected call
    desc = pkg.ReadDesc(width=37, height=21, **FORMATS[0][1])
    planes = harness.make_read_source(desc, seed=2)
    dev = f"cuda:{gpu.device}"
    d_pl = {pl: torch.from_numpy(planes[pl].view(np.uint8).reshape(-1).copy()).to(dev) for pl in planes}
    ptrs = [d_pl[pl].data_ptr() if pl in d_pl else None for pl in range(4)]
    strides = [planes[pl].strides[0] if pl in planes else 0 for pl in range(4)]
    d_out = torch.full((64 * 256,), SENTINEL, dtype=torch.uint8, device=dev)
    scratch = torch.zeros((1 << 16,), dtype=torch.uint8, device=dev)
    good = dict(rect=(1, 1, 20, 10), mode=NEAREST, code=1, o=0, n=10, drb=256, sb=1 << 16)
    bad = [dict(rect=(1, 1, 37, 10)), dict(rect=(0, 0, 0, 1)), dict(mode=3), dict(code=0), dict(code=9), dict(o=5, n=6), dict(n=-1), dict(drb=59), dict(sb=255),
           dict(code=6, n=21), dict(code=6, drb=29), dict(mode=CENTER, sb=1000)]
    for kw in [good] + bad:
        a = dict(good); a.update(kw)
        try:
            gpu.read_rows_cropped(desc, a["rect"], a["mode"], a["code"], a["o"], a["n"], ptrs, strides, d_out.data_ptr(), a["drb"], scratch.data_ptr(), a["sb"])
            ok = True
        except pkg.AvifGpuError as e:
            ok = False
            assert e.code == pkg.formatBadParameters, (kw, e)
        torch.cuda.synchronize(dev)
        assert ok == (kw is good), kw
        if not ok:
            assert bool((d_out == SENTINEL).all()), (kw, "a rejected call wrote to dst")
        else:
            d_out.fill_(SENTINEL)


# ---- HOST path -----------------------------------------------------------------------------------------------------------------------------------
def _host_equals_device_for_every_context_count(gpu):
    cases = [(pkg.ReadDesc(width=130, height=66, **FORMATS[0][1]), (3, 5, 120, 55)), (pkg.ReadDesc(width=67, height=35, **FORMATS[1][1]), (1, 2, 60, 31)),
             (pkg.ReadDesc(width=38, height=22, **FORMATS[2][1]), (2, 1, 35, 20)), (pkg.ReadDesc(width=67, height=35, **FORMATS[4][1]), (5, 4, 61, 30)),
             # starts beyond 32 columns: the staged image begins on a multiple of 32 columns in front of the rectangle, not at column 0
             (pkg.ReadDesc(width=130, height=66, **FORMATS[2][1]), (71, 3, 55, 60)), (pkg.ReadDesc(width=130, height=66, **FORMATS[1][1]), (70, 4, 56, 50))]
    sources = [harness.make_read_source(d, seed=21 + i) for i, (d, _) in enumerate(cases)]
    combos = [(NEAREST, 1), (NEAREST, 3), (CENTER, 6), (NEAREST, 6), (LEFT, 1)]
    device = [{c: open_cropped(gpu, d, p, r, c[0], c[1]) for c in combos} for (d, r), p in zip(cases, sources)]
    for i, ((d, r), p) in enumerate(zip(cases, sources)):
        for c in combos:
            check(device[i][c], d, refs(gpu, d, p, c[0], ("ctx", i)), r, c[1], (i, c, "device"))
    try:
        for n in (1, 2, 3):
            g = pkg.AvifGpu(devices=[gpu.device] * n)
            for i, ((d, r), p) in enumerate(zip(cases, sources)):
                for c in combos:
                    for pinned in (False, True):
                        assert same(open_cropped(g, d, p, r, c[0], c[1], mem="host", pinned=pinned), device[i][c]), (n, i, c, pinned)
    finally:
        pkg.AvifGpu(gpu.device)                                            # the session's binding


def _host_stages_more_than_one_tile(gpu):
    """A HOST call larger than one staged tile (16 MiB of output): both slots, row tiles and column bands, each with its own part of every
    plane and the covering row / column."""
    desc = pkg.ReadDesc(width=2048, height=1100, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12, depth=32,
                        alpha_state=pkg.ALPHA_NONE, **_pq())
    rect = (3, 5, 2041, 1090)
    assert rect[2] * rect[3] * 12 > 16 << 20
    planes = harness.make_read_source(desc, seed=3)
    own = harness.gpu_read(gpu, desc, planes).reshape(desc.height, desc.width, 3)
    for code in (1, 6):
        dev = open_cropped(gpu, desc, planes, rect, NEAREST, code)
        assert same(dev, crop_truth.cropped(own, rect, code)), ("device", code)
        assert same(open_cropped(gpu, desc, planes, rect, NEAREST, code, mem="host", pinned=(code == 6)), dev), code


# ---- the FormatRecord shim and the CLI ----------------------------------------------------------------------------------------------------------
def _shim_open(gpu, desc, planes, rect, mode, code, max_data, abort_after=None):
    out_w, out_h = pkg.read_cropped_geometry(desc, rect, code)
    nch = harness.read_channels(desc)
    host = FakeHost(out_w, out_h, desc.depth, nch, max_data=max_data, abort_after=abort_after)
    img = H.Image(width=desc.width, height=desc.height, colorspace=desc.colorspace, chroma=desc.chroma, bit_depth=desc.bit_depth)
    for pl, a in planes.items():
        img.plane[pl] = a.ctypes.data
        img.stride[pl] = a.strides[0]
    nclx = H.Nclx(desc.color_primaries, desc.transfer_characteristics, desc.matrix_coefficients, desc.full_range_flag)
    r = pkg.CropRect(*rect)
    rc = gpu.lib.avifgpu_host_read_heif_image_cropped(ctypes.byref(img), ctypes.byref(r), code, mode, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(host.fr))
    return host, rc


def _shim_delivers_cropped_tiles_and_survives_a_cancel(gpu):
    desc = pkg.ReadDesc(width=38, height=35, **FORMATS[0][1])
    planes = harness.make_read_source(desc, seed=17)
    rect = (3, 1, 34, 31)
    nch = harness.read_channels(desc)
    for mode in (NEAREST, CENTER):
        ref = refs(gpu, desc, planes, mode, ("shim",))
        for code in (1, 3, 6):
            out_w, out_h = pkg.read_cropped_geometry(desc, rect, code)
            row_bytes = out_w * nch
            max_data = row_bytes * (out_h // 6)                            # tiles of a few rows, at least 6 of them
            host, rc = _shim_open(gpu, desc, planes, rect, mode, code, max_data)
            assert rc == 0, gpu.lib.avifgpu_last_error()
            got = host.image.reshape(out_h, out_w, nch)
            check(got, desc, ref, rect, code, (mode, code))
            assert len(host.rects) >= 5 and host.rects[0][0] == 0 and host.rects[-1][2] == out_h
            assert all(a[2] == b[0] for a, b in zip(host.rects[:-1], host.rects[1:]))
            assert all(r[1] == 0 and r[3] == out_w and (r[2] - r[0]) * row_bytes <= max_data for r in host.rects)
            assert host.polls == len(host.rects)
            assert [(r[0], r[2] - r[0]) for r in host.rects] == list(helper_tiles(desc, rect, mode, code, out_h // 6))
    # a cancel at tile 2 leaves the next open intact
    host, rc = _shim_open(gpu, desc, planes, rect, CENTER, 6, 31 * 3 * 5, abort_after=2)
    assert rc == pkg.userCanceledErr and len(host.rects) == 2
    host, rc = _shim_open(gpu, desc, planes, rect, CENTER, 6, 31 * 3 * 5)
    assert rc == 0
    check(host.image.reshape(34, 31, 3), desc, refs(gpu, desc, planes, CENTER, ("shim",)), rect, 6, "after the cancel")
    # a rectangle outside the image and a document of the wrong size deliver nothing
    host, rc = _shim_open(gpu, desc, planes, rect, 3, 6, 31 * 3 * 5)
    assert rc == pkg.formatBadParameters and not host.rects
    host = FakeHost(34, 31, 8, 3)
    img = H.Image(width=desc.width, height=desc.height, colorspace=desc.colorspace, chroma=desc.chroma, bit_depth=desc.bit_depth)
    for pl, a in planes.items():
        img.plane[pl] = a.ctypes.data
        img.stride[pl] = a.strides[0]
    for bad in (pkg.CropRect(3, 1, 36, 31), pkg.CropRect(3, 1, 33, 31)):
        rc = gpu.lib.avifgpu_host_read_heif_image_cropped(ctypes.byref(img), ctypes.byref(bad), 1, NEAREST, desc.alpha_state, None, None, ctypes.byref(host.fr))
        assert rc == pkg.formatBadParameters and not host.rects


def _cli_read_crop_bilinear_orientation_6(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avif-format_amd", "avifgpu_cli")
    desc = pkg.ReadDesc(width=203, height=37, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8,
                        alpha_state=pkg.ALPHA_NONE, has_nclx=0, color_primaries=0, transfer_characteristics=0, matrix_coefficients=0)
    planes = harness.make_read_source(desc, seed=8)
    rect = (3, 1, 197, 35)
    want = open_cropped(gpu, desc, planes, rect, CENTER, 6)                # the API
    with open(tmp_path / "in.planes", "wb") as f:
        for pl, (w, xs, ys) in harness.read_planes(desc).items():
            f.write(np.ascontiguousarray(planes[pl][:, :w]).tobytes())
    r = subprocess.run([cli, "read", "--width", "203", "--height", "37", "--depth", "8", "--bits", "8", "--colorspace", "ycbcr", "--chroma", "420",
                        "--crop", "3,1,197,35", "--orientation", "6", "--chroma-upsampling", "bilinear", "--maxdata", str(35 * 3 * 40), str(tmp_path / "in.planes"),
                        str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(197, 35, 3)
    assert same(got, want)
    check(got, desc, refs(gpu, desc, planes, CENTER, ("cli",)), rect, 6, "cli")


# ---- the test: one id, many cases ------------------------------------------------------------------------------------------------------
def _run_groups(gpu, *groups):
    """Every group runs whatever the earlier ones did: a failure in one does not hide the others, and each message names its group
    and, through the group's own assertion message, its case."""
    failures = []
    for group in groups:
        try:
            group(gpu)
        except AssertionError as e:
            failures.append(f"{getattr(group, '__name__', 'group').lstrip('_')}: {e!r}"[:2000])
    assert not failures, "\n".join(failures)


def test_cropped_open(gpu, tmp_path):
    """One id for the whole feature -- the groups share the session's device binding and the cached references, and together take a few
    seconds; _run_groups names every group and case that fails."""
    def _cli(g):
        _cli_read_crop_bilinear_orientation_6(g, tmp_path)
    _cli.__name__ = "_cli_read_crop_bilinear_orientation_6"
    _run_groups(gpu, _probe_crop_alone, _every_phase_every_format, _bilinear_halo, _tile_invariance, _whole_image_rect_is_the_existing_entries,
                _zero_copy_condition, _unaligned_buffers_padding_guard_rows_and_rejections, _host_equals_device_for_every_context_count,
                _host_stages_more_than_one_tile, _shim_delivers_cropped_tiles_and_survives_a_cancel, _cli)
