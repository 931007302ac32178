"""The code histogram of a 32-bit save (avifgpu_histogram_attach; content light level, include/avifgpu.h) on the GPU:
count[max(code R, code G, code B)] per pixel, taken by write_hist_px behind the conversion of the same rows.

 * truth: on determined sources (tests/truth64.py) the bins EQUAL the bincount of the float64 codes;
 * arbitrary sources against the oracle: sum |count_gpu - count_oracle| <= 2 u, u = pixels with an undetermined colour sample;
 * it describes what was written: the bins equal the bincount of the planes the same call wrote in OUT_REFERENCE form -- for every
   pq_evaluation and hot-variant word; behind an ICC transform, where streaming and generic kernels agree within one code, the
   cumulative counts interlock, and with the generic kernel writing they are equal;
 * invariance (contexts, row cuts, pinned / pageable), no behaviour change with a histogram armed, and the FormatRecord shim."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import harness
import truth64
from fake_host import FakeHost

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP
BT2020 = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "avif-format_amd", "avifgpu_cli")
ICC_LIB = os.path.join(ROOT, "oracle", "liboracle_icc.so")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def max_code_bincount(desc, planes_out):
    """bincount of max(R, G, B) (gray: Y) of OUT_REFERENCE planes: interleaved RGB(A), or planar Y (+ A)."""
    p0 = planes_out[0].astype(np.int64)
    m = p0.reshape(p0.shape[0], desc.width, desc.planes)[..., :3].max(axis=2) if desc.planes >= 3 else p0
    return np.bincount(m.reshape(-1), minlength=1 << desc.bit_depth)


def as_reference(d):
    kw = {name: getattr(d, name) for name, _ in d._fields_}
    kw.update(output=pkg.OUT_REFERENCE)
    return pkg.WriteDesc(**kw)


def write_hist(gpu, d, src, mem="device", icc=None, cuts=None, arm=True, bins=None, stride_pad=0, return_raw=False):
    """The frame through avifgpu_write_rows* in the row tiles `cuts`, with a fresh (or the given) histogram armed around the calls.
    Returns (planes, bins as int64 numpy)."""
    import torch
    cuts = cuts or [(0, d.height)]
    nb = 1 << d.bit_depth
    bufs = harness._alloc_write_out(d, d.height, stride_pad)
    geom = harness.write_planes(d)
    if mem == "host":
        hb = np.zeros(nb, dtype=np.uint64) if bins is None else bins

        def go():
            for r0, n in cuts:
                ptrs = [bufs[i][r0 >> geom[i][2]].ctypes.data if i in bufs else None for i in range(4)]
                strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
                gpu.write_rows(d, r0, n, src[r0].ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST, icc=icc)
        if arm:
            with pkg.code_histogram(hb, d.bit_depth, pkg.MEM_HOST):
                go()
        else:
            go()
        out = hb.astype(np.int64)
    else:
        dev = f"cuda:{gpu.device}"
        db = torch.zeros(nb, dtype=torch.int64, device=dev) if bins is None else bins
        d_src = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(src.shape[0], -1)).to(dev)
        d_out = {pl: torch.from_numpy(b.view(np.uint8).reshape(b.shape[0], -1).copy()).to(dev) for pl, b in bufs.items()}
        stream = torch.cuda.current_stream(dev).cuda_stream

        def go():
            for r0, n in cuts:
                ptrs = [d_out[i][r0 >> geom[i][2]].data_ptr() if i in d_out else None for i in range(4)]
                strides = [d_out[i].stride(0) if i in d_out else 0 for i in range(4)]
                gpu.write_rows(d, r0, n, d_src[r0].data_ptr(), d_src.stride(0), ptrs, strides, mem=pkg.MEM_DEVICE, stream=stream, icc=icc)
        if arm:
            with pkg.code_histogram(db, d.bit_depth, pkg.MEM_DEVICE):
                go()
        else:
            go()
        torch.cuda.synchronize(dev)
        for pl in bufs:
            bufs[pl] = d_out[pl].cpu().numpy().view(bufs[pl].dtype).reshape(bufs[pl].shape)
        out = db.cpu().numpy().astype(np.int64)
    return (bufs if return_raw else harness._trim(d, bufs, d.height, harness.write_planes)), out


def desc_for(planes, bits, tr, output, chroma=pkg.CHROMA_444, alpha=None, width=97, height=41, peak=1000, **kw):
    if alpha is None:
        alpha = pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE
    return pkg.WriteDesc(width=width, height=height, depth=32, planes=planes, bit_depth=bits, transfer=tr, peak_nits=peak, alpha_state=alpha,
                         output=output if planes >= 3 else pkg.OUT_REFERENCE, chroma=chroma, **BT2020, **kw)


# ---- 5. truth ---------------------------------------------------------------------------------------------------------------------
def _truth_cases():
    out = []
    for planes in (1, 2, 3, 4):
        for bits in (10, 12):
            for tr in ((PQ,) if planes <= 2 else (PQ, HLG, S428)):                 # gray saves take PQ or Clip only (check_write)
                alphas = (pkg.ALPHA_NONE,) if planes in (1, 3) else (pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED)
                for alpha in alphas:
                    outs = [(pkg.OUT_REFERENCE, pkg.CHROMA_444)]
                    if planes >= 3:
                        outs += [(pkg.OUT_YCBCR, c) for c in (pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420)]
                    for output, chroma in outs:
                        out.append((planes, bits, tr, alpha, output, chroma))
    return out


@pytest.mark.parametrize("planes,bits,tr,alpha,output,chroma", _truth_cases())
def test_bins_equal_the_float64_codes_on_determined_sources(gpu, planes, bits, tr, alpha, output, chroma):
    for (w, h), mem in (((97, 41), "device"), ((97, 41), "host"), ((260, 23), "device"), ((260, 23), "host")):   # odd widths and heights; a width of whole lanes
        d = desc_for(planes, bits, tr, output, chroma, alpha, width=w, height=h, peak=(80, 1000, 10000)[(planes + bits) % 3])
        src, _ = truth64.make_determined_source(d, seed=planes * 100 + bits)
        codes, mask = truth64.determined_codes(d, src)
        assert mask.all()
        want = np.bincount(codes.max(axis=2).reshape(-1), minlength=1 << bits)
        _, bins = write_hist(gpu, d, src, mem=mem)
        assert bins.sum() == w * h, (mem, int(bins.sum()))
        assert np.array_equal(bins, want), (mem, int(np.abs(bins - want).sum()))


@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("bits", [10, 12])
def test_clip_bins_equal_the_oracle(gpu, planes, bits):
    """Clip has no curve, only the clamp and the truncation, which the parity tests hold exact: arbitrary sources, equality."""
    for alpha in ((pkg.ALPHA_NONE,) if planes in (1, 3) else (pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED)):
        for output, chroma in ((pkg.OUT_REFERENCE, pkg.CHROMA_444), (pkg.OUT_YCBCR, pkg.CHROMA_420)):
            d = desc_for(planes, bits, CLIP, output, chroma, alpha, width=131, height=37)
            src = harness.make_write_source(d, seed=bits + planes)
            want = max_code_bincount(d, harness.oracle_write(as_reference(d), src))
            for mem in ("device", "host"):
                _, bins = write_hist(gpu, d, src, mem=mem)
                assert np.array_equal(bins, want), (alpha, output, mem)


# ---- 6. arbitrary sources against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes,bits,tr,alpha", [(3, 10, PQ, 0), (3, 12, PQ, 0), (4, 12, PQ, pkg.ALPHA_STRAIGHT), (4, 10, PQ, pkg.ALPHA_PREMULTIPLIED),
                                                  (1, 10, PQ, 0), (2, 12, PQ, pkg.ALPHA_PREMULTIPLIED), (3, 12, HLG, 0), (3, 10, HLG, 0),
                                                  (3, 12, S428, 0), (4, 12, S428, pkg.ALPHA_STRAIGHT)])
def test_arbitrary_sources_differ_from_the_oracle_only_by_undetermined_pixels(gpu, planes, bits, tr, alpha):
    d = desc_for(planes, bits, tr, pkg.OUT_REFERENCE, alpha=alpha, width=515, height=203, peak=203)
    src = harness.make_write_source(d, seed=bits * planes)
    _, mask = truth64.determined_codes(d, src)
    u = int((~mask.all(axis=2)).sum())
    want = max_code_bincount(d, harness.oracle_write(d, src))
    _, bins = write_hist(gpu, d, src)
    dist = int(np.abs(bins - want).sum())
    print(f"planes {planes} {bits}-bit transfer {tr}: {d.width * d.height} pixels, {u} undetermined, sum |dcount| = {dist}")
    assert bins.sum() == d.width * d.height
    assert dist <= 2 * u, (dist, u)


# ---- 7. it describes what was written -------------------------------------------------------------------------------------------------
# every word tests/test_gpu_kernel_equivalence.py uses: streaming kernels off; the default; the size-gated ones at any size (bit 3); and both
# with flat launches off (bit 4: the conversion is launched row by row while the histogram still walks the contiguous tile as one row)
HOT_WORDS = (0, 1 | 2 | 4, 1 | 2 | 4 | 8, 1 | 2 | 4 | 8 | 16, 1 | 2 | 4 | 16)


@pytest.mark.parametrize("planes,bits,tr", [(3, 10, PQ), (3, 12, PQ), (4, 12, PQ), (1, 10, PQ), (2, 12, PQ), (3, 10, HLG), (3, 12, S428), (4, 10, CLIP)])
def test_bins_equal_the_written_codes_for_every_evaluation_and_kernel(gpu, planes, bits, tr):
    for ev in ((0, 1, 2) if tr == PQ else (0,)):
        d = desc_for(planes, bits, tr, pkg.OUT_REFERENCE, width=1028, height=19, peak=1000, pq_evaluation=ev)
        src = harness.make_write_source(d, seed=ev + planes)
        try:
            for word in HOT_WORDS:
                gpu.lib.avifgpu_set_hot_variant(word)
                for mem in ("device", "host"):
                    got, bins = write_hist(gpu, d, src, mem=mem)
                    assert np.array_equal(bins, max_code_bincount(d, got)), (ev, word, mem, gpu.last_kernel())
                    # which kernel wrote: the generic one with word 0, a streaming kernel with bit 3, none of them flat with bit 4
                    if word == 0:
                        assert "write_px" in gpu.last_kernel(), (word, mem, gpu.last_kernel())
                    if word & 8:
                        assert "write_px" not in gpu.last_kernel(), (word, mem, gpu.last_kernel())
                    if word & 16:
                        assert "flat" not in gpu.last_kernel(), (word, mem, gpu.last_kernel())
        finally:
            gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4)


@pytest.fixture(scope="module")
def lcms():
    if not os.path.exists(ICC_LIB):
        pytest.skip("oracle/liboracle_icc.so not built (lcms2 absent)")
    L = ctypes.CDLL(ICC_LIB)
    L.oracle_icc_make_profile.restype = ctypes.c_int32
    L.oracle_icc_make_profile.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32]
    L.oracle_icc_make_a2b_profile.restype = ctypes.c_int32
    L.oracle_icc_make_a2b_profile.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]
    return L


def _profile(L, kind, trc, g):
    buf = ctypes.create_string_buffer(1 << 16)
    n = L.oracle_icc_make_profile(kind, trc, g, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


def _interlocked(bins, written):
    """C_h(c - 1) <= C_w(c) <= C_h(c + 1) for every code c: what |dcode| <= 1 per sample leaves of equality."""
    ch, cw = np.cumsum(bins), np.cumsum(written)
    lo = np.concatenate([[0], ch[:-1]])
    hi = np.concatenate([ch[1:], [ch[-1]]])
    return bool(np.all(lo <= cw) and np.all(cw <= hi))


def _check_icc(gpu, d, src, xf, what):
    """Default word: streaming kernels (single-precision matrix) write, the histogram runs the generic stage_a -- within one code of
    each other (the project's bar, asserted on the OUT_REFERENCE planes first), so the cumulative counts interlock.  Word 0: the
    generic kernel writes, both sides run the same stage_a: equality."""
    try:
        gpu.lib.avifgpu_set_hot_variant(0)
        slow, bins0 = write_hist(gpu, d, src, icc=xf)
        assert "write_px" in gpu.last_kernel(), gpu.last_kernel()
        assert np.array_equal(bins0, max_code_bincount(d, slow)), what
        _, bins0h = write_hist(gpu, d, src, icc=xf, mem="host")
        assert np.array_equal(bins0h, bins0), what
        gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4)
        fast, bins1 = write_hist(gpu, d, src, icc=xf)
        st = harness.compare_write(d, slow, fast)
        assert st["max_abs"] <= 1, (what, st)
        assert np.array_equal(bins1, bins0), what                                   # the histogram does not depend on which kernel wrote
        assert _interlocked(bins1, max_code_bincount(d, fast)), what
    finally:
        gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4)


@pytest.mark.parametrize("name,kind,trc,g", [("p3-linear", 1, 0, 1.0), ("adobergb-gamma2.2", 3, 0, 2.19921875), ("srgb-parametric", 0, 1, 0.0)])
@pytest.mark.parametrize("planes", [3, 4])
def test_bins_behind_a_matrix_trc_profile(gpu, lcms, name, kind, trc, g, planes):
    icc = _profile(lcms, kind, trc, g)
    for target, tr, bits in ((pkg.ICC_TARGET_REC2020_LINEAR, PQ, 10), (pkg.ICC_TARGET_SRGB_FLOAT, CLIP, 12)):
        xf = gpu.icc_prepare(icc, target)
        d = desc_for(planes, bits, tr, pkg.OUT_REFERENCE, width=1024, height=12, peak=80)
        src = np.abs(harness.make_write_source(d, seed=5))
        _check_icc(gpu, d, src, xf, (name, planes, target))


@pytest.mark.parametrize("name,kind,trc,n", [("p3-sampled-srgb-1024", 1, 3, 1024), ("prophoto-sampled-per-channel-33", 2, 4, 33)])
def test_bins_behind_a_sampled_curve_profile(gpu, lcms, name, kind, trc, n):
    icc = _profile(lcms, kind, trc, float(n))
    for target, tr, bits in ((pkg.ICC_TARGET_REC2020_LINEAR, PQ, 12), (pkg.ICC_TARGET_SRGB_FLOAT, CLIP, 10)):
        xf = gpu.icc_prepare_sampled(icc, target)
        for planes in (3, 4):
            d = desc_for(planes, bits, tr, pkg.OUT_REFERENCE, width=516, height=14, peak=1000)
            src = np.abs(harness.make_write_source(d, seed=9))
            _check_icc(gpu, d, src, xf, (name, planes, target))


@pytest.mark.parametrize("variant", [0, 1])
def test_bins_behind_a_lut_based_profile(gpu, lcms, variant):
    if pkg.lcms_bridge() is None:
        pytest.skip("libavifgpu_lcms_bridge.so not built (lcms2 absent)")
    buf = ctypes.create_string_buffer(1 << 20)
    n = lcms.oracle_icc_make_a2b_profile(variant, buf, len(buf))
    assert n > 0
    icc = buf.raw[:n]
    for target, tr, bits in ((pkg.ICC_TARGET_REC2020_LINEAR, PQ, 10), (pkg.ICC_TARGET_SRGB_FLOAT, CLIP, 12)):
        for planes in (3, 4):
            rc, prog = pkg.icc_pipeline32_from_profile(icc, target, planes == 4)
            assert rc == 0, pkg.load().avifgpu_last_error()
            d = desc_for(planes, bits, tr, pkg.OUT_REFERENCE, width=260, height=9, peak=1000)
            src = np.abs(harness.make_write_source(d, seed=3))
            _check_icc(gpu, d, src, prog, (variant, planes, target))


# ---- 8. invariance ----------------------------------------------------------------------------------------------------------------------
def test_host_bins_do_not_depend_on_contexts_cuts_or_pinning(gpu):
    import torch
    results = []
    try:
        for chroma, cuts_list in ((pkg.CHROMA_444, ([(0, 203)], [(0, 64), (64, 63), (127, 76)], [(0, 1), (1, 201), (202, 1)])),
                                  (pkg.CHROMA_420, ([(0, 203)], [(0, 64), (64, 100), (164, 39)]))):
            d = desc_for(3, 10, PQ, pkg.OUT_YCBCR, chroma, width=1030, height=203, peak=1000)
            src = harness.make_write_source(d, seed=41)
            pinned = torch.from_numpy(src.copy()).pin_memory().numpy()
            _, ref = write_hist(gpu, d, src)                                         # device path, one call
            for nctx in (1, 2, 3):
                g = pkg.AvifGpu(devices=[gpu.device] * nctx)
                for cuts in cuts_list:
                    for s in (src, pinned):
                        _, bins = write_hist(g, d, s, mem="host", cuts=cuts)
                        results.append((chroma, nctx, cuts, s is pinned, np.array_equal(bins, ref)))
            for cuts in cuts_list[1:]:
                _, bins = write_hist(gpu, d, src, cuts=cuts)                          # device path in several calls
                results.append((chroma, 0, cuts, False, np.array_equal(bins, ref)))
    finally:
        pkg.AvifGpu(int(os.environ.get("LOCAL_RANK", "0")))                        # the rest of the suite runs on one binding
    assert all(r[-1] for r in results), [r for r in results if not r[-1]]


def test_two_threads_keep_their_own_histograms(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    out, errs = {}, []

    def work(k, mem):
        try:
            torch.cuda.set_device(dev)
            d = desc_for(3, 10 if k == 0 else 12, PQ, pkg.OUT_REFERENCE, width=300 + 37 * k, height=50 + k, peak=1000)
            src = harness.make_write_source(d, seed=90 + k)
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                for rep in range(3):
                    got, bins = write_hist(gpu, d, src, mem=mem)
                    out[(k, mem, rep)] = np.array_equal(bins, max_code_bincount(d, got))
        except Exception as e:                                                      # noqa: BLE001 -- reported by the assertion below
            errs.append(repr(e))
    for mem in ("device", "host"):
        ts = [threading.Thread(target=work, args=(k, mem)) for k in (0, 1)]
        [t.start() for t in ts]
        [t.join() for t in ts]
    assert not errs, errs
    assert len(out) == 12 and all(out.values()), out


# ---- 9. no behaviour change ---------------------------------------------------------------------------------------------------------------
def test_armed_calls_write_the_same_bytes_and_disarmed_calls_leave_the_bins_alone(gpu):
    for planes, output, chroma in ((3, pkg.OUT_YCBCR, pkg.CHROMA_444), (4, pkg.OUT_YCBCR, pkg.CHROMA_420), (3, pkg.OUT_REFERENCE, pkg.CHROMA_444), (2, 0, 3)):
        d = desc_for(planes, 12, PQ, output, chroma, width=1030, height=31)
        src = harness.make_write_source(d, seed=7)
        for mem in ("device", "host"):
            plain, _ = write_hist(gpu, d, src, mem=mem, arm=False, stride_pad=8, return_raw=True)
            k_plain = gpu.last_kernel()
            armed, bins = write_hist(gpu, d, src, mem=mem, stride_pad=8, return_raw=True)
            assert gpu.last_kernel() == k_plain                                     # the conversion's label, not the statistics kernel's
            for pl in plain:
                assert np.array_equal(plain[pl], armed[pl]), (planes, mem, pl)      # padding included
            assert bins.sum() == d.width * d.height
            # disarmed again: the former bins are left alone
            if mem == "host":
                keep = bins.astype(np.uint64)
                write_hist(gpu, d, src, mem=mem, arm=False, bins=keep)
                assert np.array_equal(keep.astype(np.int64), bins)
            else:
                import torch
                keep = torch.from_numpy(bins.copy()).to(f"cuda:{gpu.device}")
                _, after = write_hist(gpu, d, src, mem=mem, arm=False, bins=keep)
                assert np.array_equal(after, bins)


def test_other_depths_and_reads_do_not_touch_an_armed_histogram(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    hb = np.zeros(4096, dtype=np.uint64)
    db = torch.zeros(4096, dtype=torch.int64, device=dev)
    for mem, bins, kind in (("host", hb, pkg.MEM_HOST), ("device", db, pkg.MEM_DEVICE)):
        with pkg.code_histogram(bins, 12, kind):
            for depth, bits in ((8, 8), (8, 12), (16, 12), (16, 10)):
                d = pkg.WriteDesc(width=260, height=20, depth=depth, planes=3, bit_depth=bits, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT2020)
                src = harness.make_write_source(d, seed=depth)
                want = harness.oracle_write(d, src)
                got = harness.gpu_write(gpu, d, src, mem=mem)
                for pl in want:
                    assert np.array_equal(got[pl], want[pl]), (depth, bits, mem, pl)
            rd = pkg.ReadDesc(width=260, height=20, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12, depth=32,
                              alpha_state=pkg.ALPHA_NONE, transfer_characteristics=pkg.TC_PQ, **BT2020)
            planes = harness.make_read_source(rd)
            got = harness.gpu_read(gpu, rd, planes, mem=mem)
            np.testing.assert_allclose(got, harness.oracle_read(rd, planes), rtol=1e-4, atol=1e-9)
    torch.cuda.synchronize(dev)
    assert not hb.any() and not bool(db.any())


def test_a_mismatch_fails_before_anything_is_launched(gpu):
    import torch
    dev = f"cuda:{gpu.device}"
    d8 = pkg.WriteDesc(width=64, height=4, depth=8, planes=3, bit_depth=8, output=pkg.OUT_REFERENCE)
    harness.gpu_write(gpu, d8, harness.make_write_source(d8))
    label = gpu.last_kernel()
    d = desc_for(3, 10, PQ, pkg.OUT_YCBCR, width=64, height=8)
    src = harness.make_write_source(d)
    hb = np.zeros(4096, dtype=np.uint64)
    db = torch.zeros(4096, dtype=torch.int64, device=dev)
    for bins, bits, kind, mem in ((hb, 12, pkg.MEM_HOST, "host"), (db, 12, pkg.MEM_DEVICE, "device"),       # bit depth differs
                                  (hb, 10, pkg.MEM_HOST, "device"), (db, 10, pkg.MEM_DEVICE, "host")):      # memory kind differs
        with pkg.code_histogram(bins, bits, kind):
            with pytest.raises(pkg.AvifGpuError) as e:
                harness.gpu_write(gpu, d, src, mem=mem)
        assert e.value.code == pkg.formatBadParameters and "armed code histogram" in e.value.message
        assert gpu.last_kernel() == label
    torch.cuda.synchronize(dev)
    assert not hb.any() and not bool(db.any())
    got = harness.gpu_write(gpu, d, src)                                             # disarmed: the call works as ever
    assert harness.compare_write(d, harness.oracle_write(d, src), got)["max_abs"] <= 1


def test_probe_histogram_is_the_kernel_of_an_armed_call(gpu):
    """avifgpu_probe_histogram (the measuring aid of tools/bench_light_level.py): twin 0 counts what an armed call counts; the timing
    twins launch for aligned RGB PQ rows only and are refused elsewhere."""
    import torch
    dev = f"cuda:{gpu.device}"
    stream = torch.cuda.current_stream(dev).cuda_stream
    for planes, bits in ((3, 10), (4, 12), (1, 10)):
        d = desc_for(planes, bits, PQ, pkg.OUT_REFERENCE, width=1028, height=21)
        src = harness.make_write_source(d, seed=planes)
        _, want = write_hist(gpu, d, src)
        d_src = torch.from_numpy(src).to(dev)
        bins = torch.zeros(1 << bits, dtype=torch.int64, device=dev)
        assert gpu.lib.avifgpu_probe_histogram(ctypes.byref(d), 0, d_src.data_ptr(), d_src.stride(0) * 4, bins.data_ptr(), stream) == 0
        torch.cuda.synchronize(dev)
        assert np.array_equal(bins.cpu().numpy(), want), planes
        for twin in (1, 2):
            rc = gpu.lib.avifgpu_probe_histogram(ctypes.byref(d), twin, d_src.data_ptr(), d_src.stride(0) * 4, bins.data_ptr(), stream)
            assert rc == (0 if planes == 3 else pkg.formatBadParameters), (planes, twin)
        torch.cuda.synchronize(dev)
        assert gpu.lib.avifgpu_probe_histogram(ctypes.byref(d), 3, d_src.data_ptr(), d_src.stride(0) * 4, bins.data_ptr(), stream) == pkg.formatBadParameters
    d16 = pkg.WriteDesc(width=64, height=4, depth=16, planes=3, bit_depth=10, output=pkg.OUT_REFERENCE)
    assert gpu.lib.avifgpu_probe_histogram(ctypes.byref(d16), 0, d_src.data_ptr(), 64 * 6, bins.data_ptr(), stream) == pkg.formatBadParameters


# ---- 10. through the shim ---------------------------------------------------------------------------------------------------------------
def _shim_save(gpu, d, src, max_data, bins, icc=None, to_rec2020=0):
    host = FakeHost(d.width, d.height, d.depth, d.planes, max_data=max_data, image=src)
    keep = None
    if icc is not None:
        keep = ctypes.create_string_buffer(icc, len(icc))
        host.fr.iCCprofileData = ctypes.cast(keep, ctypes.c_void_p)
        host.fr.iCCprofileSize = len(icc)
    opts = H.SaveUIOptions(imageBitDepth=d.bit_depth, hdrTransferFunction=d.transfer, pq=H.PQOptions(d.peak_nits),
                           chromaSubsampling=d.chroma, lossless=0, convertToRec2020=to_rec2020)
    assert gpu.lib.avifgpu_host_save_wants_light_level(ctypes.byref(host.fr), ctypes.byref(opts)) == 1
    img = H.Image()
    with pkg.code_histogram(bins, d.bit_depth, pkg.MEM_HOST):
        code = gpu.lib.avifgpu_host_create_heif_image(ctypes.byref(host.fr), d.alpha_state, ctypes.byref(opts), d.output,
                                                      d.matrix_coefficients, d.color_primaries, ctypes.byref(img))
    assert code == 0, gpu.lib.avifgpu_last_error()
    got = {}
    for pl, (w, xs, ys) in harness.write_planes(d).items():
        h = (d.height + ys) >> ys
        raw = (ctypes.c_uint8 * (img.stride[pl] * h)).from_address(img.plane[pl])
        got[pl] = np.frombuffer(raw, dtype=np.uint8).reshape(h, img.stride[pl])[:, :w * 2].view(np.uint16).copy()
    gpu.lib.avifgpu_image_free(ctypes.byref(img))
    return got, len(host.rects)


def test_shim_save_counts_every_tile(gpu, tmp_path):
    d = desc_for(3, 10, PQ, pkg.OUT_REFERENCE, width=301, height=230, peak=1000)
    src = harness.make_write_source(d, seed=12)
    bins = np.zeros(1024, dtype=np.uint64)
    got, tiles = _shim_save(gpu, d, src, src.strides[0] * 6, bins)
    assert tiles >= 24, tiles
    assert np.array_equal(bins.astype(np.int64), max_code_bincount(d, got))
    # the fused output of the same save: stage A is shared, the bins are the same
    dy = desc_for(3, 10, PQ, pkg.OUT_YCBCR, pkg.CHROMA_422, width=301, height=230, peak=1000, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
    bins_y = np.zeros(1024, dtype=np.uint64)
    _, tiles = _shim_save(gpu, dy, src, src.strides[0] * 6, bins_y)
    assert tiles >= 24 and np.array_equal(bins_y, bins)
    # the CLI's line is avifgpu_light_level_from_histogram of them
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    for extra, p in (([], 1.0), (["--percentile", "0.999"], 0.999)):
        r = subprocess.run([CLI, "write", "--width", str(d.width), "--height", str(d.height), "--depth", "32", "--planes", "3", "--bits", "10",
                            "--transfer", "pq", "--peak", "1000", "--maxdata", str(src.strides[0] * 6), "--light-level", *extra,
                            str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        ll = pkg.light_level_from_histogram(bins, 10, PQ, p)
        line = f"light-level: MaxCLL {ll.max_cll} MaxFALL {ll.max_fall} code {ll.max_code} pixels {ll.pixels}"
        assert line in r.stderr.splitlines(), (line, r.stderr)
    # without the flag: nothing new
    r = subprocess.run([CLI, "write", "--width", str(d.width), "--height", str(d.height), "--depth", "32", "--planes", "3", "--bits", "10",
                        "--transfer", "pq", "--peak", "1000", str(tmp_path / "in.raw"), str(tmp_path / "out.planes")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "light-level" not in r.stderr and len(r.stderr.splitlines()) == 1, r.stderr
    # a save that carries no light level refuses the flag
    r = subprocess.run([CLI, "write", "--width", "8", "--height", "8", "--depth", "32", "--planes", "3", "--bits", "12", "--transfer", "clip",
                        "--light-level", str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "32-bit PQ saves only" in r.stderr


def test_shim_save_behind_a_document_profile(gpu, lcms):
    icc = _profile(lcms, 1, 0, 1.0)                                                 # Display-P3 primaries, linear: a typical 32-bit document
    d = desc_for(3, 12, PQ, pkg.OUT_REFERENCE, width=300, height=120, peak=1000)
    src = harness.make_write_source(d, seed=11)
    xf = gpu.icc_prepare(icc)
    try:
        gpu.lib.avifgpu_set_hot_variant(0)                                          # the generic kernel writes: equality
        bins0 = np.zeros(4096, dtype=np.uint64)
        got, tiles = _shim_save(gpu, d, src, src.strides[0] * 5, bins0, icc=icc, to_rec2020=1)
        assert tiles >= 24 and np.array_equal(bins0.astype(np.int64), max_code_bincount(d, got))
        _, direct = write_hist(gpu, d, src, icc=xf)
        assert np.array_equal(direct, bins0.astype(np.int64))                       # the same bins as the C-ABI call with the prepared transform
        gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4)                                  # the streaming kernels write: within one code, interlocked
        bins1 = np.zeros(4096, dtype=np.uint64)
        got, _ = _shim_save(gpu, d, src, src.strides[0] * 5, bins1, icc=icc, to_rec2020=1)
        assert np.array_equal(bins1, bins0)
        assert _interlocked(bins1.astype(np.int64), max_code_bincount(d, got))
    finally:
        gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4)
