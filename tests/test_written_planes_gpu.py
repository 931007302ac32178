"""The summary of a save's written planes on the GPU (avifgpu_summary_attach, include/avifgpu.h "summary of a save"): plane_summary
keeps, per output channel, the largest code and the largest 65535 - code of the planes the conversion kernel of the same rows has just
written, and the largest max(R,G,B) - min(R,G,B) of a pixel where R, G and B are there to be compared.

Truth is numpy (test_summary.counters_of: min / max / spread) of the planes THE SAME CALL returned.  Everything is exact integers:
no tolerances.
 * every output form, widths that cross the kernel's column block, heights of several bands, unaligned planes;
 * planted extremes: one pixel of a mid-grey frame at the corners, on either side of a block boundary, in the ragged tail;
 * independence of tiling (overlapping tiles too), HOST / DEVICE, pinned / pageable, several contexts;
 * no behaviour change with a summary armed; errors before anything is launched; the FormatRecord shim; the CLI; the measuring probe."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harness
from fake_host import FakeHost
from test_summary import GBR, HI, LO_INV, N, SPREAD, counters_of, spread_defined

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C444, C422, C420 = pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "avif-format_amd", "avifgpu_cli")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def desc_for(container, planes, output=REF, chroma=C444, width=61, height=7, depth=None, **kw):
    """container 8: 8-bit documents saved at 8 bits (u8 planes); 16: 16-bit documents saved at 10 bits (u16 planes)."""
    depth = depth or container
    bits = kw.pop("bits", 8 if container == 8 else 10)
    kw.setdefault("matrix_coefficients", pkg.MATRIX_BT2020_NCL)
    kw.setdefault("color_primaries", pkg.PRIMARIES_BT2020)
    return pkg.WriteDesc(width=width, height=height, depth=depth, planes=planes, bit_depth=bits,
                         transfer=pkg.TRANSFER_PQ if depth == 32 else pkg.TRANSFER_CLIP, peak_nits=1000,
                         alpha_state=pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE, output=output if planes >= 3 else REF,
                         chroma=chroma, **kw)


def write_summary(gpu, d, src, mem="device", cuts=None, arm=True, counters=None, stride_pad=0, return_raw=False, hist=None, thumb=None):
    """The frame through avifgpu_write_rows in the row tiles `cuts`, with fresh (or the given) summary counters armed around the calls
    (and a code histogram `hist` / thumbnail sums `thumb` = (sums, tw, th) with them).  Returns (planes, counters as numpy uint32)."""
    import torch
    cuts = cuts or [(0, d.height)]
    bufs = harness._alloc_write_out(d, d.height, stride_pad)
    geom = harness.write_planes(d)
    kind = pkg.MEM_HOST if mem == "host" else pkg.MEM_DEVICE
    dev = f"cuda:{gpu.device}"
    if mem == "host":
        acc = np.zeros(N, dtype=np.uint32) if counters is None else counters

        def go():
            for r0, nr in cuts:
                ptrs = [bufs[i][r0 >> geom[i][2]].ctypes.data if i in bufs else None for i in range(4)]
                strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
                gpu.write_rows(d, r0, nr, src[r0].ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)
    else:
        acc = torch.zeros(N, dtype=torch.int32, device=dev) if counters is None else counters
        d_src = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(src.shape[0], -1)).to(dev)
        d_out = {pl: torch.from_numpy(b.view(np.uint8).reshape(b.shape[0], -1).copy()).to(dev) for pl, b in bufs.items()}
        stream = torch.cuda.current_stream(dev).cuda_stream

        def go():
            for r0, nr in cuts:
                ptrs = [d_out[i][r0 >> geom[i][2]].data_ptr() if i in d_out else None for i in range(4)]
                strides = [d_out[i].stride(0) if i in d_out else 0 for i in range(4)]
                gpu.write_rows(d, r0, nr, d_src[r0].data_ptr(), d_src.stride(0), ptrs, strides, mem=pkg.MEM_DEVICE, stream=stream)
    with contextlib.ExitStack() as stack:
        if arm:
            stack.enter_context(pkg.plane_summary(acc, kind))
        if hist is not None:
            stack.enter_context(pkg.code_histogram(hist, d.bit_depth, kind))
        if thumb is not None:
            stack.enter_context(pkg.thumbnail_sums(thumb[0], thumb[1], thumb[2], kind))
        go()
    if mem == "host":
        out = acc.copy()
    else:
        torch.cuda.synchronize(dev)
        for pl in bufs:
            bufs[pl] = d_out[pl].cpu().numpy().view(bufs[pl].dtype).reshape(bufs[pl].shape)
        out = acc.cpu().numpy().view(np.uint32).copy()
    return (bufs if return_raw else harness._trim(d, bufs, d.height, harness.write_planes)), out


def same(got, want, what):
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())


_SRC = {}


def source(d, seed):
    """The random source of a descriptor, made once and shared; never modified."""
    key = (d.width, d.height, d.depth, d.planes, seed)
    if key not in _SRC:
        _SRC[key] = harness.make_write_source(d, seed=seed)
    return _SRC[key]


FORMS = [(1, REF, C444, {}), (2, REF, C444, {}), (3, REF, C444, {}), (4, REF, C444, {}),
         (3, YCC, C444, {}), (4, YCC, C444, {}), (3, YCC, C422, {}), (4, YCC, C422, {}), (3, YCC, C420, {}), (4, YCC, C420, {}),
         (3, YCC, C444, GBR), (4, YCC, C444, GBR)]


# ---- 1. every form, the widths and heights at which the kernel takes another path -----------------------------------------------------
@pytest.mark.parametrize("planes,output,chroma,kw", FORMS)
@pytest.mark.parametrize("container", (8, 16))
def test_every_form(gpu, container, planes, output, chroma, kw):
    d = desc_for(container, planes, output, chroma, **kw)
    src = source(d, seed=container + planes)
    for mem, pad in (("device", 0), ("host", 0), ("device", 3)):
        got, c = write_summary(gpu, d, src, mem=mem, stride_pad=pad)
        same(c, counters_of(d, got), (mem, pad))
        assert (c[SPREAD] > 0) == spread_defined(d) and not c[SPREAD + 1:].any()
        s = pkg.summary_read(d, c)                                      # and what the library reads out of them
        assert s.channels == planes and s.neutral == int(planes <= 2)


# a lane block is 4096 bytes of a planar or 4-channel row, 12288 bytes of a 3-channel row: 4099 u8 / 2051 u16 samples or pixels cross it
# with a ragged tail; 70 rows are nine bands of the launcher's eight rows
@pytest.mark.parametrize("container,width,height,planes,output,chroma,kw", [
    (8, 4099, 70, 1, REF, C444, {}), (8, 4099, 70, 3, REF, C444, {}), (8, 4099, 70, 4, REF, C444, {}), (8, 4099, 70, 4, YCC, C422, {}),
    (8, 4099, 70, 3, YCC, C444, GBR), (16, 2051, 70, 2, REF, C444, {}), (16, 2051, 70, 3, REF, C444, {}), (16, 2051, 70, 4, REF, C444, {}),
    (16, 2051, 70, 4, YCC, C444, GBR), (16, 2051, 9, 3, YCC, C420, {}), (8, 4099, 9, 4, YCC, C420, {}), (16, 4099, 71, 3, YCC, C420, {})])
def test_width_edges_and_bands(gpu, container, width, height, planes, output, chroma, kw):
    d = desc_for(container, planes, output, chroma, width=width, height=height, **kw)
    src = source(d, seed=7)
    for mem, pad in (("device", 0), ("host", 0), ("device", 5)):
        got, c = write_summary(gpu, d, src, mem=mem, stride_pad=pad)
        same(c, counters_of(d, got), (mem, pad))


def test_unaligned_planes(gpu):
    """Planes at an odd base with a stride that is no multiple of 16, handed to the kernel alone: only pw x prows is read (the rest holds
    values no plane has)."""
    import torch
    dev = f"cuda:{gpu.device}"
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(9)
    for container, planes, output, chroma, kw in ((8, 3, REF, C444, {}), (8, 4, YCC, C420, {}), (16, 4, REF, C444, {}), (16, 3, YCC, C444, GBR),
                                                  (16, 2, REF, C444, {})):
        d = desc_for(container, planes, output, chroma, width=1030, height=21, **kw)
        ssz = 2 if d.bit_depth > 8 else 1
        dt = np.uint16 if ssz == 2 else np.uint8
        maxcode = (1 << d.bit_depth) - 1
        want, keep, ptrs, strides = {}, [], [None] * 4, [0] * 4
        for pl, (w, xs, ys) in harness.write_planes(d).items():
            h = (d.height + ys) >> ys
            lead, stride = 1 + 2 * pl, w + 3                             # samples: an odd base (u8: an odd address) and an odd stride
            raw = np.full(lead + h * stride + 8, 0xA5A5 if ssz == 2 else 0xA5, dtype=dt)
            body = raw[lead:lead + h * stride].reshape(h, stride)
            body[:, :w] = rng.integers(maxcode // 4, maxcode // 2, size=(h, w))
            want[pl] = body[:, :w].copy()
            t = torch.from_numpy(raw).to(dev)
            keep.append(t)
            ptrs[pl], strides[pl] = t.data_ptr() + lead * ssz, stride * ssz
            assert ptrs[pl] % 16 and strides[pl] % 16
        c = torch.zeros(N, dtype=torch.int32, device=dev)
        rc = gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 0, ctypes.byref(pkg.planes4(ptrs)), ctypes.byref(pkg.strides4(strides)), c.data_ptr(), stream)
        assert rc == 0, gpu.lib.avifgpu_last_error()
        torch.cuda.synchronize(dev)
        same(c.cpu().numpy().view(np.uint32), counters_of(d, want), (container, planes))


# ---- 2. planted extremes --------------------------------------------------------------------------------------------------------------
def _planted_cases():
    out = []
    # (container, planes, output, chroma, kw, width, height, x of: last lane of the first block, first lane of the next, the ragged tail)
    for container, planes, output, chroma, kw, w, h, xs in (
            (8, 3, REF, C444, {}, 4099, 71, (4095, 4096, 4098)),                                            # 16 pixels per lane, 4096 per block
            (8, 3, YCC, C420, dict(chroma_downsampling=pkg.DOWNSAMPLE_NEAREST), 4099, 71, (4094, 4096, 4098)),   # even coordinates reach the chroma
            (16, 4, REF, C444, {}, 2051, 71, (511, 512, 2050)),                                             # 2 pixels per lane, 512 per block
            (16, 3, YCC, C444, GBR, 2051, 71, (2047, 2048, 2050))):                                         # 8 samples per lane, 2048 per block
        spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(x, 34) for x in xs]
        for k, (x, y) in enumerate(spots):
            out.append((container, planes, output, chroma, kw, w, h, x, y, k % 2 == 0))
    return out


@pytest.mark.parametrize("container,planes,output,chroma,kw,w,h,x,y,white", _planted_cases())
def test_planted_extremes(gpu, container, planes, output, chroma, kw, w, h, x, y, white):
    d = desc_for(container, planes, output, chroma, width=w, height=h, **kw)
    top = 255 if container == 8 else 32768
    src = np.full((h, w, planes), top // 2, dtype=harness.src_dtype(container))
    if planes == 4:
        src[..., 3] = top
    flat = counters_of(d, harness.oracle_write(d, np.ascontiguousarray(src.reshape(h, w * planes))))
    src[y, x, :3] = (top, 0, top) if white else (0, 0, 0)               # colour where the luma alone would not move far
    src = np.ascontiguousarray(src.reshape(h, w * planes))
    for mem in ("device", "host"):
        got, c = write_summary(gpu, d, src, mem=mem)
        want = counters_of(d, got)
        moved = (want[HI:HI + planes] != flat[HI:HI + planes]) | (want[LO_INV:LO_INV + planes] != flat[LO_INV:LO_INV + planes])
        assert moved.any(), "the planted pixel moved no channel's minimum or maximum"
        same(c, want, (mem, x, y))


def test_one_translucent_alpha_sample_in_the_last_corner(gpu):
    for container, planes, output, chroma, w in ((8, 4, REF, C444, 4099), (16, 4, YCC, C420, 2051), (8, 2, REF, C444, 4099)):
        d = desc_for(container, planes, output, chroma, width=w, height=23)
        top = 255 if container == 8 else 32768
        src = source(d, seed=31).reshape(d.height, w, planes).copy()
        src[..., -1] = top
        for plant in (False, True):
            if plant:
                src[-1, -1, -1] = top - (1 if container == 8 else 64)
            for mem in ("device", "host"):
                got, c = write_summary(gpu, d, np.ascontiguousarray(src.reshape(d.height, -1)), mem=mem)
                same(c, counters_of(d, got), (mem, plant))
                s = pkg.summary_read(d, c)
                assert s.alpha_opaque == int(not plant) and s.alpha_clear == 0, (container, planes, mem, plant)
                assert bool(s.advice & pkg.ADVICE_DROP_ALPHA) == (not plant)


# ---- 3. independence ------------------------------------------------------------------------------------------------------------------
def test_counters_do_not_depend_on_tiling_memory_or_contexts(gpu):
    import torch
    results = []
    try:
        for container, planes, output, chroma, cuts_list in (
                (16, 4, YCC, C444, ([(0, 70)], [(r, 1) for r in range(70)], [(r, 2) for r in range(0, 70, 2)], [(0, 7), (7, 33), (40, 29), (69, 1)],
                                    [(0, 40), (30, 40)], [(0, 70), (0, 70)])),                     # overlapping tiles, the frame fed twice
                (8, 3, YCC, C420, ([(0, 70)], [(r, 2) for r in range(0, 70, 2)], [(0, 22), (22, 48)], [(0, 40), (30, 40)])),
                (8, 3, REF, C444, ([(0, 70)], [(r, 1) for r in range(70)], [(0, 33), (33, 37)], [(10, 60), (0, 35)]))):
            d = desc_for(container, planes, output, chroma, width=2051, height=70)
            src = source(d, seed=41)
            ref = counters_of(d, harness.gpu_write(gpu, d, src))
            pinned = torch.from_numpy(src.copy()).pin_memory().numpy()
            for nctx in (1, 2, 3):
                g = pkg.AvifGpu(devices=[gpu.device] * nctx)
                for cuts in cuts_list[:1] + cuts_list[2:]:
                    for s in (src, pinned):
                        _, c = write_summary(g, d, s, mem="host", cuts=cuts)
                        results.append((planes, nctx, len(cuts), s is pinned, np.array_equal(c, ref)))
            for cuts in cuts_list:                                      # the device path, in one and in many launches
                _, c = write_summary(gpu, d, src, cuts=cuts)
                results.append((planes, 0, len(cuts), False, np.array_equal(c, ref)))
    finally:
        pkg.AvifGpu(int(os.environ.get("LOCAL_RANK", "0")))                        # the rest of the suite runs on one binding
    assert all(r[-1] for r in results), [r for r in results if not r[-1]]


def test_counters_are_running_maxima_and_never_cleared(gpu):
    import torch
    d = desc_for(8, 3, REF, width=97, height=41)
    src = source(d, seed=3)
    got, ref = write_summary(gpu, d, src)
    keep = np.zeros(N, dtype=np.uint32)
    keep[HI + 1], keep[LO_INV + 2], keep[SPREAD + 3] = 70000, 65535, 9     # above anything a feed gives: they stay
    want = np.maximum(ref, keep)
    for _ in range(2):
        write_summary(gpu, d, src, mem="host", counters=keep)
    same(keep, want, "host")
    dk = torch.from_numpy(np.where(want == ref, 0, want).astype(np.uint32).view(np.int32)).to(f"cuda:{gpu.device}")
    _, c = write_summary(gpu, d, src, counters=dk)
    same(c, want, "device")


# ---- 4. no behaviour change -----------------------------------------------------------------------------------------------------------
def test_armed_calls_write_the_same_bytes_and_disarmed_calls_leave_the_counters_alone(gpu):
    import torch
    for container, planes, output, chroma, depth in ((16, 3, YCC, C444, 32), (16, 4, YCC, C420, 16), (8, 3, REF, C444, 8), (8, 2, REF, C444, 8)):
        d = desc_for(container, planes, output, chroma, width=1030, height=31, depth=depth)
        src = source(d, seed=planes)
        for mem in ("device", "host"):
            plain, none = write_summary(gpu, d, src, mem=mem, arm=False, stride_pad=8, return_raw=True)
            assert not none.any()
            k_plain = gpu.last_kernel()
            armed, c = write_summary(gpu, d, src, mem=mem, stride_pad=8, return_raw=True)
            assert gpu.last_kernel() == k_plain                                     # the conversion's label, not the statistics kernel's
            for pl in plain:
                assert np.array_equal(plain[pl], armed[pl]), (planes, mem, pl)      # padding included
            same(c, counters_of(d, harness._trim(d, armed, d.height, harness.write_planes)), (planes, mem))
            keep = np.full(N, 1, dtype=np.uint32) if mem == "host" else torch.ones(N, dtype=torch.int32, device=f"cuda:{gpu.device}")
            _, after = write_summary(gpu, d, src, mem=mem, arm=False, counters=keep)
            assert (after == 1).all()                                               # disarmed again: the counters are left alone


def test_reads_do_not_touch_armed_counters(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    hc = np.zeros(N, dtype=np.uint32)
    dc = torch.zeros(N, dtype=torch.int32, device=dev)
    rd = pkg.ReadDesc(width=260, height=20, colorspace=pkg.COLORSPACE_YCBCR, chroma=C420, bit_depth=12, depth=32,
                      alpha_state=pkg.ALPHA_NONE, transfer_characteristics=pkg.TC_PQ, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                      color_primaries=pkg.PRIMARIES_BT2020)
    planes = harness.make_read_source(rd)
    want = harness.oracle_read(rd, planes)
    for mem, c, kind in (("host", hc, pkg.MEM_HOST), ("device", dc, pkg.MEM_DEVICE)):
        with pkg.plane_summary(c, kind):
            np.testing.assert_allclose(harness.gpu_read(gpu, rd, planes, mem=mem), want, rtol=1e-4, atol=1e-9)
    torch.cuda.synchronize(dev)
    assert not hc.any() and not bool(dc.any())


def test_histogram_thumbnail_and_summary_armed_together(gpu):
    import torch
    from test_thumbnail import box_sums
    d = desc_for(16, 3, YCC, C422, width=515, height=67, depth=32)
    src = source(d, seed=5)
    for mem in ("device", "host"):
        def zeros(n):
            return np.zeros(n, dtype=np.uint64) if mem == "host" else torch.zeros(n, dtype=torch.int64, device=f"cuda:{gpu.device}")
        _, alone = write_summary(gpu, d, src, mem=mem)
        bins, sums = zeros(1024), zeros(13 * 7 * 3)
        got, c = write_summary(gpu, d, src, mem=mem, hist=bins, thumb=(sums, 13, 7))
        b, s = (bins, sums) if mem == "host" else (bins.cpu().numpy(), sums.cpu().numpy())
        assert int(b.sum()) == d.width * d.height, mem
        assert np.array_equal(s.astype(np.int64).reshape(7, 13, 3), box_sums(got, d, 13, 7)), mem
        same(c, alone, mem)
        same(c, counters_of(d, got), mem)


def test_a_mem_kind_mismatch_fails_before_anything_is_launched(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    d8 = pkg.WriteDesc(width=64, height=4, depth=8, planes=3, bit_depth=8, output=REF)
    harness.gpu_write(gpu, d8, harness.make_write_source(d8))
    label = gpu.last_kernel()
    d = desc_for(8, 3, YCC, C420, width=97, height=41)
    src = source(d, seed=2)
    hc = np.zeros(N, dtype=np.uint32)
    dc = torch.zeros(N, dtype=torch.int32, device=dev)
    bufs = harness._alloc_write_out(d, d.height)
    ptrs = [bufs[i].ctypes.data if i in bufs else None for i in range(4)]
    strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
    d_out = {pl: torch.from_numpy(b.copy()).to(dev) for pl, b in bufs.items()}
    d_src = torch.from_numpy(src).to(dev)
    with pkg.plane_summary(dc, pkg.MEM_DEVICE):                         # device counters, host pointers
        with pytest.raises(pkg.AvifGpuError) as e:
            gpu.write_rows(d, 0, d.height, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)
    assert e.value.code == pkg.formatBadParameters and "armed summary" in e.value.message and "memory" in e.value.message
    with pkg.plane_summary(hc, pkg.MEM_HOST):                           # host counters, device pointers
        with pytest.raises(pkg.AvifGpuError) as e:
            gpu.write_rows(d, 0, d.height, d_src.data_ptr(), d_src.stride(0), [d_out[i].data_ptr() if i in d_out else None for i in range(4)],
                           [d_out[i].stride(0) if i in d_out else 0 for i in range(4)], mem=pkg.MEM_DEVICE)
    assert e.value.code == pkg.formatBadParameters and "armed summary" in e.value.message
    torch.cuda.synchronize(dev)
    assert gpu.last_kernel() == label
    for pl in bufs:
        assert (bufs[pl] == 0xA5).all() and bool((d_out[pl] == 0xA5).all()), pl
    assert not hc.any() and not bool(dc.any())
    # a host call that fails adds nothing, and leaves nothing behind for the next one
    with pkg.plane_summary(hc, pkg.MEM_HOST):
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height + 2, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)       # rows outside the image
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height, src.ctypes.data, src.strides[0], [ptrs[0], None, ptrs[2], None], strides, mem=pkg.MEM_HOST)
    assert not hc.any()
    got, c = write_summary(gpu, d, src, mem="host")
    same(c, counters_of(d, got), "after the failures")


# ---- 5. the shim, the CLI, the probe ----------------------------------------------------------------------------------------------------
def test_shim_save_over_several_tiles(gpu):
    """The shim's saves run on the caller's thread: every tile of a save folds into the counters armed around the call."""
    d = desc_for(8, 4, YCC, C420, width=2051, height=70, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST,
                 matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709)           # what default save options give
    src = source(d, seed=12).reshape(70, 2051, 4).copy()
    src[..., 3] = 255
    src[69, 2050, :3] = (255, 0, 255)                                   # the last tile's last pixel carries an extreme
    src = np.ascontiguousarray(src.reshape(70, -1))
    got, single = write_summary(gpu, d, src)                            # one launch on the device path
    same(single, counters_of(d, got), "device")
    host = FakeHost(d.width, d.height, d.depth, d.planes, max_data=src.strides[0] * 8, image=src)
    opts = H.SaveUIOptions(imageBitDepth=d.bit_depth, hdrTransferFunction=d.transfer, pq=H.PQOptions(d.peak_nits),
                           chromaSubsampling=d.chroma, lossless=0)
    img = H.Image()
    c = np.zeros(N, dtype=np.uint32)
    with pkg.plane_summary(c):
        code = gpu.lib.avifgpu_host_create_heif_image(ctypes.byref(host.fr), d.alpha_state, ctypes.byref(opts), d.output,
                                                      d.matrix_coefficients, d.color_primaries, ctypes.byref(img))
    assert code == 0, gpu.lib.avifgpu_last_error()
    gpu.lib.avifgpu_image_free(ctypes.byref(img))
    assert len(host.rects) >= 4, host.rects
    same(c, single, "shim")
    s = pkg.summary_read(d, c)
    assert s.alpha_opaque == 1 and s.neutral == 0 and s.advice == pkg.ADVICE_DROP_ALPHA


def test_cli_summary_line(tmp_path):
    d = pkg.WriteDesc(width=301, height=230, depth=8, planes=4, bit_depth=8, alpha_state=pkg.ALPHA_STRAIGHT, output=pkg.OUT_YCBCR,
                      chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709, full_range=1,
                      chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
    grey = np.repeat(np.random.default_rng(6).integers(0, 256, size=(230, 301, 1), dtype=np.uint8), 4, axis=2)
    grey[..., 3] = 255
    src = np.ascontiguousarray(grey.reshape(230, -1))
    want = harness.oracle_write(d, src)
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    args = [CLI, "write", "--width", "301", "--height", "230", "--depth", "8", "--planes", "4", "--bits", "8", "--alpha", "straight",
            "--ycbcr", "420", "--maxdata", str(src.strides[0] * 6)]
    r = subprocess.run(args + ["--summary", str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = pkg.summary_read(d, counters_of(d, want))                       # 8-bit saves are bit-exact with the oracle
    line = "summary " + " ".join("min%d %d max%d %d" % (c, s.min_code[c], c, s.max_code[c]) for c in range(4)) + \
           " spread -1 alpha_opaque 1 neutral 1 advice 3"
    assert r.stdout.splitlines() == [line], r.stdout
    assert int(r.stderr.split(" tiles")[0].split()[-1]) >= 24, r.stderr
    out = (tmp_path / "out.planes").read_bytes()
    assert out == b"".join(want[pl].tobytes() for pl in range(4))
    r = subprocess.run(args + [str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "" and (tmp_path / "out.planes").read_bytes() == out
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "[--summary]" in r.stderr


def test_probe_summary_is_the_kernel_of_an_armed_call(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    stream = torch.cuda.current_stream(dev).cuda_stream
    for container, planes, output, chroma, kw in ((16, 3, YCC, C422, {}), (8, 4, REF, C444, {}), (8, 2, REF, C444, {}), (16, 4, YCC, C444, GBR)):
        d = desc_for(container, planes, output, chroma, width=1030, height=37, **kw)
        src = source(d, seed=planes)
        got, armed = write_summary(gpu, d, src)
        d_pl = {pl: torch.from_numpy(a.copy()).to(dev) for pl, a in got.items()}
        ptrs = (ctypes.c_void_p * 4)(*[d_pl[i].data_ptr() if i in d_pl else None for i in range(4)])
        strides = (ctypes.c_int64 * 4)(*[d_pl[i].stride(0) * d_pl[i].element_size() if i in d_pl else 0 for i in range(4)])
        c = torch.zeros(N, dtype=torch.int32, device=dev)
        rc = gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 0, ctypes.byref(ptrs), ctypes.byref(strides), c.data_ptr(), stream)
        assert rc == 0, gpu.lib.avifgpu_last_error()
        torch.cuda.synchronize(dev)
        same(c.cpu().numpy().view(np.uint32), armed, planes)
        assert gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 0, ctypes.byref(ptrs), ctypes.byref(strides), None, stream) == pkg.formatBadParameters
        assert gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 2, ctypes.byref(ptrs), ctypes.byref(strides), c.data_ptr(), stream) == pkg.formatBadParameters
        short = (ctypes.c_int64 * 4)(*[max(s - 1, 0) for s in strides])
        assert gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 0, ctypes.byref(ptrs), ctypes.byref(short), c.data_ptr(), stream) == pkg.formatBadParameters
        # the atomics-free twin launches and leaves the counters alone
        before = c.clone()
        assert gpu.lib.avifgpu_probe_summary(ctypes.byref(d), 1, ctypes.byref(ptrs), ctypes.byref(strides), c.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        assert bool((c == before).all())
