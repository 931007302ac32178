"""The box-average thumbnail of a save on the GPU (avifgpu_thumbnail_attach, include/avifgpu.h "thumbnail of a save"): thumb_box_sums
sums the output codes of the planes the conversion kernel of the same rows has just written, per thumbnail cell and channel.

The reference is numpy (test_thumbnail.box_sums / thumb_codes: integer sums over planes with the cell rule, and the rounded mean).
 * integer documents: it is applied to the ORACLE's planes; GPU == oracle is bit-exact there, so sums and thumbnail codes are EQUAL;
 * depth 32: the sums equal box_sums of the planes the same GPU call wrote (the thumbnail describes what was written), and against
   the oracle's planes |dcode| <= 1 per thumbnail code -- every sample is within one code of the oracle's (the T2 bar), so is a mean of
   them, and the rounding of two means at most one apart keeps them at most one apart;
 * invariance (launches, row cuts inside cells, contexts, pinned / pageable, HOST / DEVICE): identical sums;
 * no behaviour change with a thumbnail armed; errors before anything is launched; the FormatRecord shim; the measuring probe."""
import ctypes
import os

import numpy as np
import pytest

import harness
from fake_host import FakeHost
from test_thumbnail import box_sums, cell_counts, channel_sizes, thumb_codes

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

PQ, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_CLIP
BT2020 = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C444, C422, C420 = pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def desc_for(depth, planes, bits, output=REF, chroma=C444, alpha=None, width=97, height=41, transfer=None, **kw):
    if alpha is None:
        alpha = pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE
    if transfer is None:
        transfer = PQ if depth == 32 else CLIP
    return pkg.WriteDesc(width=width, height=height, depth=depth, planes=planes, bit_depth=bits, transfer=transfer, peak_nits=1000,
                         alpha_state=alpha, output=output if planes >= 3 else REF, chroma=chroma, **BT2020, **kw)


def write_thumb(gpu, d, src, tw, th, mem="device", cuts=None, arm=True, sums=None, stride_pad=0, return_raw=False, hist=None):
    """The frame through avifgpu_write_rows in the row tiles `cuts`, with fresh (or the given) thumbnail sums armed around the calls
    (and a code histogram `hist` with them).  Returns (planes, sums as int64 numpy of shape (th, tw, planes))."""
    import contextlib
    import torch
    cuts = cuts or [(0, d.height)]
    n = tw * th * d.planes
    bufs = harness._alloc_write_out(d, d.height, stride_pad)
    geom = harness.write_planes(d)
    kind = pkg.MEM_HOST if mem == "host" else pkg.MEM_DEVICE
    dev = f"cuda:{gpu.device}"
    if mem == "host":
        acc = np.zeros(n, dtype=np.uint64) if sums is None else sums

        def go():
            for r0, nr in cuts:
                ptrs = [bufs[i][r0 >> geom[i][2]].ctypes.data if i in bufs else None for i in range(4)]
                strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
                gpu.write_rows(d, r0, nr, src[r0].ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)
    else:
        acc = torch.zeros(n, dtype=torch.int64, device=dev) if sums is None else sums
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
            stack.enter_context(pkg.thumbnail_sums(acc, tw, th, kind))
        if hist is not None:
            stack.enter_context(pkg.code_histogram(hist, d.bit_depth, kind))
        go()
    if mem == "host":
        out = acc.astype(np.int64)
    else:
        torch.cuda.synchronize(dev)
        for pl in bufs:
            bufs[pl] = d_out[pl].cpu().numpy().view(bufs[pl].dtype).reshape(bufs[pl].shape)
        out = acc.cpu().numpy().astype(np.int64)
    return (bufs if return_raw else harness._trim(d, bufs, d.height, harness.write_planes)), out[:n].reshape(th, tw, d.planes)


def smallest_plane(d):
    s = channel_sizes(d)
    return min(x[0] for x in s), min(x[1] for x in s)


_ORACLE = {}


def oracle_planes(d, seed):
    """(source, oracle planes) of a descriptor, computed once and shared; never modified."""
    key = (tuple(getattr(d, n) for n, _ in d._fields_ if isinstance(getattr(d, n), (int, float))), seed)
    if key not in _ORACLE:
        src = harness.make_write_source(d, seed=seed)
        _ORACLE[key] = (src, harness.oracle_write(d, src))
    return _ORACLE[key]


def check(d, got_planes, sums, want_planes, tw, th, what):
    """The bars of the module docstring for one save."""
    if d.depth != 32:
        want = box_sums(want_planes, d, tw, th)
        assert np.array_equal(sums, want), (what, int(np.abs(sums - want).max()))
        return
    own = box_sums(got_planes, d, tw, th)
    assert np.array_equal(sums, own), (what, int(np.abs(sums - own).max()))
    got_codes = thumb_codes(sums, d, tw, th)
    want_codes = thumb_codes(box_sums(want_planes, d, tw, th), d, tw, th)
    for pl in want_codes:
        delta = np.abs(got_codes[pl].astype(np.int64) - want_codes[pl].astype(np.int64)).max()
        assert delta <= 1, (what, pl, int(delta))


# ---- 1. sums and codes against the reference ----------------------------------------------------------------------------------------
def _cases():
    out = []
    for depth in (8, 16, 32):
        k = 0
        for planes in (1, 2, 3, 4):
            for alpha in ((pkg.ALPHA_NONE,) if planes in (1, 3) else (pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED)):
                outs = [(REF, C444)]
                if planes >= 3:
                    outs += [(YCC, c) for c in (C444, C422, C420)]
                for output, chroma in outs:
                    bits = ((10, 12) if depth == 32 else (8, 10, 12))[k % (2 if depth == 32 else 3)]     # every save bit depth at every depth
                    k += 1
                    out.append((depth, planes, alpha, output, chroma, bits))
    return out


@pytest.mark.parametrize("depth,planes,alpha,output,chroma,bits", _cases())
def test_sums_and_codes_equal_the_reference(gpu, depth, planes, alpha, output, chroma, bits):
    for (w, h) in ((97, 41), (260, 23)):                                   # odd and ragged; a width of whole lanes
        d = desc_for(depth, planes, bits, output, chroma, alpha, width=w, height=h)
        src, want = oracle_planes(d, seed=depth + planes)
        mw, mh = smallest_plane(d)
        # 13 x 7; the largest legal size (identity for 4:4:4 and REFERENCE, the chroma planes' own size for 4:2:x); 1 x 1
        for i, (tw, th) in enumerate(((13, 7), (mw, mh), (1, 1))):
            for j, mem in enumerate(("device", "host")):
                pad = 3 if (i + j) % 2 else 0
                got, sums = write_thumb(gpu, d, src, tw, th, mem=mem, stride_pad=pad)
                check(d, got, sums, want, tw, th, (w, h, tw, th, mem, pad))
                if (tw, th) == (w, h):                                     # identity: the sums ARE the codes that were written
                    codes = thumb_codes(sums, d, tw, th)
                    for pl in got:
                        assert np.array_equal(codes[pl], got[pl]), (w, h, mem, pl)
                if depth != 32:                                            # and the thumbnail the library makes of them is the reference's
                    lib_codes = pkg.thumbnail_from_sums(d, tw, th, np.ascontiguousarray(sums.reshape(-1)).astype(np.uint64))
                    ref_codes = thumb_codes(box_sums(want, d, tw, th), d, tw, th)
                    for pl in ref_codes:
                        assert np.array_equal(lib_codes[pl], ref_codes[pl]), (w, h, tw, th, mem, pl)


# cells wider than a wave's span with a boundary inside a wave (1030 -> 3: 344 / 343 / 343 samples), and a tall frame that many bands
# of workgroups share per thumbnail row (4099 rows -> 5)
@pytest.mark.parametrize("w,h,tw,th", [(1030, 70, 3, 2), (64, 4099, 1, 5)])
@pytest.mark.parametrize("depth,planes,output,chroma,bits", [(8, 1, REF, C444, 8), (8, 3, REF, C444, 8), (16, 4, REF, C444, 10), (16, 3, YCC, C420, 12),
                                                             (8, 4, YCC, C422, 8), (32, 3, YCC, C444, 10), (32, 2, REF, C444, 12)])
def test_wide_cells_and_tall_frames(gpu, w, h, tw, th, depth, planes, output, chroma, bits):
    d = desc_for(depth, planes, bits, output, chroma, width=w, height=h)
    src, want = oracle_planes(d, seed=7)
    for mem, pad in (("device", 0), ("host", 0), ("device", 3)):
        got, sums = write_thumb(gpu, d, src, tw, th, mem=mem, stride_pad=pad)
        check(d, got, sums, want, tw, th, (mem, pad))


# ---- 2. invariance ----------------------------------------------------------------------------------------------------------------------
def test_sums_do_not_depend_on_launches_cuts_contexts_or_pinning(gpu):
    import torch
    results = []
    try:
        for (w, h, tw, th), chroma, cuts_list in (
                ((97, 41, 13, 7), C444, ([(0, 41)], [(0, 2), (2, 20), (22, 19)], [(0, 1), (1, 39), (40, 1)])),       # cuts inside cells
                ((97, 41, 13, 7), C420, ([(0, 41)], [(0, 2), (2, 20), (22, 19)])),
                ((64, 4099, 1, 5), C444, ([(0, 4099)], [(0, 819), (819, 2000), (2819, 1280)])),
                ((64, 4099, 1, 5), C420, ([(0, 4099)], [(0, 820), (820, 2000), (2820, 1279)]))):
            d = desc_for(16, 3, 10, YCC, chroma, width=w, height=h)
            src, want = oracle_planes(d, seed=41)
            ref = box_sums(want, d, tw, th)
            pinned = torch.from_numpy(src.copy()).pin_memory().numpy()
            for nctx in (1, 2, 3):
                g = pkg.AvifGpu(devices=[gpu.device] * nctx)
                for cuts in cuts_list:
                    for s in (src, pinned):
                        _, sums = write_thumb(g, d, s, tw, th, mem="host", cuts=cuts)
                        results.append((w, chroma, nctx, cuts, s is pinned, np.array_equal(sums, ref)))
            for cuts in cuts_list:
                _, sums = write_thumb(gpu, d, src, tw, th, cuts=cuts)         # device path, in one and in several launches
                results.append((w, chroma, 0, cuts, False, np.array_equal(sums, ref)))
    finally:
        pkg.AvifGpu(int(os.environ.get("LOCAL_RANK", "0")))                        # the rest of the suite runs on one binding
    assert all(r[-1] for r in results), [r for r in results if not r[-1]]


def test_sums_accumulate_and_are_never_zeroed(gpu):
    d = desc_for(8, 3, 8, width=97, height=41)
    src, want = oracle_planes(d, seed=3)
    ref = box_sums(want, d, 13, 7)
    keep = np.full(13 * 7 * 3, 5, dtype=np.uint64)
    for _ in range(2):
        write_thumb(gpu, d, src, 13, 7, mem="host", sums=keep)
    assert np.array_equal(keep.astype(np.int64).reshape(7, 13, 3), 2 * ref + 5)


# ---- 3. no behaviour change -----------------------------------------------------------------------------------------------------------------
def test_armed_calls_write_the_same_bytes_and_disarmed_calls_leave_the_sums_alone(gpu):
    import torch
    for depth, planes, output, chroma, bits in ((32, 3, YCC, C444, 10), (16, 4, YCC, C420, 12), (8, 3, REF, C444, 8), (8, 2, REF, C444, 8)):
        d = desc_for(depth, planes, bits, output, chroma, width=1030, height=31)
        src = harness.make_write_source(d, seed=planes)
        for mem in ("device", "host"):
            plain, _ = write_thumb(gpu, d, src, 13, 7, mem=mem, arm=False, stride_pad=8, return_raw=True)
            k_plain = gpu.last_kernel()
            armed, sums = write_thumb(gpu, d, src, 13, 7, mem=mem, stride_pad=8, return_raw=True)
            assert gpu.last_kernel() == k_plain                                     # the conversion's label, not the statistics kernel's
            for pl in plain:
                assert np.array_equal(plain[pl], armed[pl]), (planes, mem, pl)      # padding included
            assert sums.any()
            flat = np.ascontiguousarray(sums.reshape(-1))
            keep = flat.astype(np.uint64) if mem == "host" else torch.from_numpy(flat.copy()).to(f"cuda:{gpu.device}")
            _, after = write_thumb(gpu, d, src, 13, 7, mem=mem, arm=False, sums=keep)
            assert np.array_equal(after, sums)                                      # disarmed again: the former sums are left alone


def test_histogram_and_thumbnail_armed_together(gpu):
    import torch
    d = desc_for(32, 3, 10, YCC, C422, width=515, height=67)
    src = harness.make_write_source(d, seed=5)
    for mem in ("device", "host"):
        def bins():
            return np.zeros(1024, dtype=np.uint64) if mem == "host" else torch.zeros(1024, dtype=torch.int64, device=f"cuda:{gpu.device}")
        alone = bins()
        write_thumb(gpu, d, src, 13, 7, mem=mem, arm=False, hist=alone)
        both = bins()
        got, sums = write_thumb(gpu, d, src, 13, 7, mem=mem, hist=both)
        a, b = (alone, both) if mem == "host" else (alone.cpu().numpy(), both.cpu().numpy())
        assert int(a.sum()) == d.width * d.height and np.array_equal(a, b), mem
        assert np.array_equal(sums, box_sums(got, d, 13, 7)), mem


def test_reads_do_not_touch_armed_sums(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    hs = np.zeros(13 * 7 * 4, dtype=np.uint64)
    ds = torch.zeros(13 * 7 * 4, dtype=torch.int64, device=dev)
    rd = pkg.ReadDesc(width=260, height=20, colorspace=pkg.COLORSPACE_YCBCR, chroma=C420, bit_depth=12, depth=32,
                      alpha_state=pkg.ALPHA_NONE, transfer_characteristics=pkg.TC_PQ, **BT2020)
    planes = harness.make_read_source(rd)
    want = harness.oracle_read(rd, planes)
    for mem, sums, kind in (("host", hs, pkg.MEM_HOST), ("device", ds, pkg.MEM_DEVICE)):
        with pkg.thumbnail_sums(sums, 13, 7, kind):
            np.testing.assert_allclose(harness.gpu_read(gpu, rd, planes, mem=mem), want, rtol=1e-4, atol=1e-9)
    torch.cuda.synchronize(dev)
    assert not hs.any() and not bool(ds.any())


# ---- 4. magnitude -----------------------------------------------------------------------------------------------------------------------
def test_sums_pass_two_to_the_32(gpu):
    """4096 x 2048 samples of code 4095 in ONE cell: 4095 * 2^23 = 3.4e10 per channel."""
    d = desc_for(16, 3, 12, REF, width=4096, height=2048)
    src = np.full((2048, 4096 * 3), 32768, dtype=np.uint16)
    for mem in ("device", "host"):
        got, sums = write_thumb(gpu, d, src, 1, 1, mem=mem)
        assert int(got[0].min()) == 4095
        assert sums.reshape(-1).tolist() == [4095 << 23] * 3, mem
    assert int(pkg.thumbnail_from_sums(d, 1, 1, sums.reshape(-1).astype(np.uint64))[0].max()) == 4095


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------------
def test_a_mismatch_fails_before_anything_is_launched(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    d8 = pkg.WriteDesc(width=64, height=4, depth=8, planes=3, bit_depth=8, output=REF)
    harness.gpu_write(gpu, d8, harness.make_write_source(d8))
    label = gpu.last_kernel()
    d = desc_for(8, 3, 8, YCC, C420, width=97, height=41)
    src, want = oracle_planes(d, seed=2)
    hs = np.zeros(64 * 64 * 3, dtype=np.uint64)
    ds = torch.zeros(64 * 64 * 3, dtype=torch.int64, device=dev)
    for sums, tw, th, kind, mem, text in ((hs, 13, 7, pkg.MEM_HOST, "device", "memory"), (ds, 13, 7, pkg.MEM_DEVICE, "host", "memory"),   # memory kind differs
                                          (hs, 50, 7, pkg.MEM_HOST, "host", "smallest plane"), (ds, 50, 7, pkg.MEM_DEVICE, "device", "smallest plane"),   # chroma is 49 wide
                                          (hs, 13, 22, pkg.MEM_HOST, "host", "smallest plane"), (ds, 13, 22, pkg.MEM_DEVICE, "device", "smallest plane")):  # and 21 high
        raw = {}
        with pkg.thumbnail_sums(sums, tw, th, kind):
            with pytest.raises(pkg.AvifGpuError) as e:
                raw = harness.gpu_write(gpu, d, src, mem=mem, return_raw=True)
        assert e.value.code == pkg.formatBadParameters and "armed thumbnail" in e.value.message and text in e.value.message, e.value.message
        assert gpu.last_kernel() == label
        assert raw == {}
    # the output planes keep their fill: the same calls on buffers this test can look at afterwards
    bufs = harness._alloc_write_out(d, d.height)
    ptrs = [bufs[i].ctypes.data if i in bufs else None for i in range(4)]
    strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
    with pkg.thumbnail_sums(hs, 50, 7, pkg.MEM_HOST):
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)
    d_out = {pl: torch.from_numpy(b.copy()).to(dev) for pl, b in bufs.items()}
    d_src = torch.from_numpy(src).to(dev)
    with pkg.thumbnail_sums(hs, 13, 7, pkg.MEM_HOST):
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height, d_src.data_ptr(), d_src.stride(0), [d_out[i].data_ptr() if i in d_out else None for i in range(4)],
                           [d_out[i].stride(0) if i in d_out else 0 for i in range(4)], mem=pkg.MEM_DEVICE)
    torch.cuda.synchronize(dev)
    for pl in bufs:
        assert (bufs[pl] == 0xA5).all() and bool((d_out[pl] == 0xA5).all()), pl
    assert not hs.any() and not bool(ds.any())
    # a host call that fails adds nothing, and leaves nothing behind for the next one
    with pkg.thumbnail_sums(hs, 13, 7, pkg.MEM_HOST):
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height + 2, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)       # rows outside the image
        with pytest.raises(pkg.AvifGpuError):
            gpu.write_rows(d, 0, d.height, src.ctypes.data, src.strides[0], [ptrs[0], None, ptrs[2], None], strides, mem=pkg.MEM_HOST)
    assert not hs.any()
    _, sums = write_thumb(gpu, d, src, 13, 7, mem="host")
    assert np.array_equal(sums, box_sums(want, d, 13, 7))
    got = harness.gpu_write(gpu, d, src)                                             # disarmed: the call works as ever
    for pl in want:
        assert np.array_equal(got[pl], want[pl])


# ---- 6. through the shim ----------------------------------------------------------------------------------------------------------------
def _shim_save(gpu, d, src, max_data, sums, tw, th, expect=0, **host_kw):
    host = FakeHost(d.width, d.height, d.depth, d.planes, max_data=max_data, image=src, **host_kw)
    opts = H.SaveUIOptions(imageBitDepth=d.bit_depth, hdrTransferFunction=d.transfer, pq=H.PQOptions(d.peak_nits),
                           chromaSubsampling=d.chroma, lossless=0)
    img = H.Image()
    with pkg.thumbnail_sums(sums, tw, th, pkg.MEM_HOST):
        code = gpu.lib.avifgpu_host_create_heif_image(ctypes.byref(host.fr), d.alpha_state, ctypes.byref(opts), d.output,
                                                      d.matrix_coefficients, d.color_primaries, ctypes.byref(img))
    if expect != 0:
        assert code != 0
        return len(host.rects)
    assert code == 0, gpu.lib.avifgpu_last_error()
    gpu.lib.avifgpu_image_free(ctypes.byref(img))
    return len(host.rects)


def test_shim_save_sums_every_tile(gpu):
    d = desc_for(8, 3, 8, YCC, C420, width=2048, height=1024, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)    # what default save options give
    src, want = oracle_planes(d, seed=12)
    tw, th = pkg.thumbnail_fit(d, 256)
    assert (tw, th) == (256, 128)
    _, single = write_thumb(gpu, d, src, tw, th)                                    # one launch on the device path
    assert np.array_equal(single, box_sums(want, d, tw, th))
    sums = np.zeros(tw * th * 3, dtype=np.uint64)
    tiles = _shim_save(gpu, d, src, src.strides[0] * 100, sums, tw, th)
    assert tiles >= 8, tiles
    assert np.array_equal(sums.astype(np.int64).reshape(th, tw, 3), single)
    # a save the host fails half way: whatever it leaves in the caller's sums, the contexts keep nothing for the next save
    scratch = np.zeros(tw * th * 3, dtype=np.uint64)
    _shim_save(gpu, d, src, src.strides[0] * 100, scratch, tw, th, expect=1, fail_at_row=600)
    again = np.zeros(tw * th * 3, dtype=np.uint64)
    _shim_save(gpu, d, src, src.strides[0] * 100, again, tw, th)
    assert np.array_equal(again, sums)


# ---- 7. the measuring aid ---------------------------------------------------------------------------------------------------------------
def test_probe_thumbnail_is_the_kernel_of_an_armed_call(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    stream = torch.cuda.current_stream(dev).cuda_stream
    for depth, planes, output, chroma, bits in ((16, 3, YCC, C422, 10), (8, 4, REF, C444, 8), (8, 2, REF, C444, 8)):
        d = desc_for(depth, planes, bits, output, chroma, width=1030, height=37)
        src, want = oracle_planes(d, seed=planes)
        d_pl = {pl: torch.from_numpy(a.copy()).to(dev) for pl, a in want.items()}
        ptrs = (ctypes.c_void_p * 4)(*[d_pl[i].data_ptr() if i in d_pl else None for i in range(4)])
        strides = (ctypes.c_int64 * 4)(*[d_pl[i].stride(0) * d_pl[i].element_size() if i in d_pl else 0 for i in range(4)])
        sums = torch.zeros(13 * 7 * planes, dtype=torch.int64, device=dev)
        rc = gpu.lib.avifgpu_probe_thumbnail(ctypes.byref(d), 0, 13, 7, ctypes.byref(ptrs), ctypes.byref(strides), sums.data_ptr(), stream)
        assert rc == 0, gpu.lib.avifgpu_last_error()
        torch.cuda.synchronize(dev)
        assert np.array_equal(sums.cpu().numpy().reshape(7, 13, planes), box_sums(want, d, 13, 7)), planes
        assert gpu.lib.avifgpu_probe_thumbnail(ctypes.byref(d), 0, 2000, 7, ctypes.byref(ptrs), ctypes.byref(strides), sums.data_ptr(), stream) == pkg.formatBadParameters
        assert gpu.lib.avifgpu_probe_thumbnail(ctypes.byref(d), 0, 13, 7, ctypes.byref(ptrs), ctypes.byref(strides), None, stream) == pkg.formatBadParameters
        assert gpu.lib.avifgpu_probe_thumbnail(ctypes.byref(d), 2, 13, 7, ctypes.byref(ptrs), ctypes.byref(strides), sums.data_ptr(), stream) == pkg.formatBadParameters
        # the atomics-free twin launches and leaves the sums alone
        before = sums.clone()
        assert gpu.lib.avifgpu_probe_thumbnail(ctypes.byref(d), 1, 13, 7, ctypes.byref(ptrs), ctypes.byref(strides), sums.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        assert bool((sums == before).all())
