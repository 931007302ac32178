"""Content light level (clli: MaxCLL / MaxFALL) of an HDR save, the host side: avifgpu_light_level_from_histogram against a float64
restatement of its definition (include/avifgpu.h), every refusal, arming and disarming without a device, the shim's decision helper,
and the oracle side of the GPU tests' bars -- the yardstick meets them alone.  CPU only: none of these calls touches a device."""
import ctypes
import math

import numpy as np
import pytest

import harness
import truth64

pkg = harness.pkg
H = pkg.host

PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP


# ---- restatement: SMPTE ST 2084 EOTF with its exact rational constants, float64 ----------------------------------------------
def pq_nits(code, bits):
    m1, m2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
    c1, c2, c3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
    e = np.asarray(code, dtype=np.float64) / float((1 << bits) - 1)
    ep = np.power(e, 1.0 / m2)
    return 10000.0 * np.power(np.maximum(ep - c1, 0.0) / (c2 - c3 * ep), 1.0 / m1)


def light_level(bins, bits, p):
    bins = np.asarray(bins, dtype=np.uint64)
    n = int(bins.astype(object).sum())
    need = math.ceil(p * float(n))
    cum, cp = 0, None
    for c in range(1 << bits):
        cum += int(bins[c])
        if cum >= need:
            cp = c
            break
    L = pq_nits(np.arange(1 << bits), bits)
    fall = 0.0
    for c in range(1 << bits):                     # ascending code order
        if bins[c]:
            fall += float(bins[c]) * float(L[c])
    fall /= float(n)
    cll = float(L[cp])
    return dict(max_code=cp, pixels=n, max_cll_nits=cll, max_fall_nits=fall,
                max_cll=min(65535, math.floor(cll + 0.5)), max_fall=min(65535, math.floor(fall + 0.5)))


def check(bins, bits, p):
    got = pkg.light_level_from_histogram(bins, bits, PQ, p)
    want = light_level(bins, bits, p)
    assert got.max_code == want["max_code"] and got.pixels == want["pixels"], (bits, p, got.max_code, want)
    assert got.max_cll == want["max_cll"] and got.max_fall == want["max_fall"], (bits, p, got.max_cll, got.max_fall, want)
    for g, w in ((got.max_cll_nits, want["max_cll_nits"]), (got.max_fall_nits, want["max_fall_nits"])):
        assert abs(g - w) <= 1e-12 * abs(w), (bits, p, g, w)
    return got


@pytest.mark.parametrize("bits", [10, 12])
def test_every_single_bin_histogram(bits):
    """Every L(c): a histogram with one non-empty bin has MaxCLL = MaxFALL = L(c) at every percentile."""
    L = pq_nits(np.arange(1 << bits), bits)
    for c in range(1 << bits):
        bins = np.zeros(1 << bits, dtype=np.uint64)
        bins[c] = 1 + (c % 7)
        got = pkg.light_level_from_histogram(bins, bits, PQ, 1.0 if c % 2 else 0.5)
        assert got.max_code == c and got.pixels == 1 + (c % 7)
        assert abs(got.max_cll_nits - L[c]) <= 1e-12 * L[c] and abs(got.max_fall_nits - L[c]) <= 1e-12 * L[c], (c, got.max_cll_nits, L[c])
        want = min(65535, math.floor(float(L[c]) + 0.5))
        assert got.max_cll == want and got.max_fall == want, (c, got.max_cll, want)


@pytest.mark.parametrize("bits", [10, 12])
@pytest.mark.parametrize("p", [1.0, 0.9999, 0.5])
def test_random_histograms(bits, p):
    rng = np.random.default_rng(harness.SEED + bits)
    for trial in range(12):
        bins = rng.integers(0, 1 << (4 + 4 * (trial % 10)), size=1 << bits, dtype=np.uint64)
        if trial % 3 == 0:
            bins[rng.random(1 << bits) < 0.9] = 0                  # sparse
        if trial % 4 == 1:
            bins[(1 << bits) * 3 // 4:] = 0                        # nothing bright
        if int(bins.sum()) == 0:
            bins[5] = 1
        check(bins, bits, p)


def test_anchors():
    # the top code is 10 000 cd/m2, exactly
    for bits in (10, 12):
        bins = np.zeros(1 << bits, dtype=np.uint64)
        bins[-1] = 3
        got = check(bins, bits, 1.0)
        assert got.max_cll == 10000 and got.max_fall == 10000 and got.max_cll_nits == 10000.0
    # a gray PQ save at peak_nits = 203 of a source clamped at 1.0 peaks at code 594 of 1023: MaxCLL 203 (the oracle's codes)
    d = pkg.WriteDesc(width=64, height=4, depth=32, planes=1, bit_depth=10, transfer=PQ, peak_nits=203, alpha_state=pkg.ALPHA_NONE,
                      output=pkg.OUT_REFERENCE)
    src = np.linspace(0.0, 3.0, 256, dtype=np.float32).reshape(4, 64)
    codes = harness.oracle_write(d, src)[0]
    assert int(codes.max()) == 594
    bins = np.bincount(codes.reshape(-1), minlength=1024).astype(np.uint64)
    got = check(bins, 10, 1.0)
    assert got.max_code == 594 and got.max_cll == 203


def test_percentile_picks_the_smallest_code_that_covers_it():
    bins = np.zeros(1024, dtype=np.uint64)
    bins[100], bins[500], bins[900] = 9990, 9, 1                   # n = 10 000
    assert check(bins, 10, 1.0).max_code == 900
    assert check(bins, 10, 0.9999).max_code == 500
    assert check(bins, 10, 0.999).max_code == 100
    assert check(bins, 10, 0.5).max_code == 100


def test_code_zero_is_zero_nits():
    # (no PQ code exceeds 10 000 cd/m2, so the 65535 cap of the fields is unreachable from a histogram)
    bins = np.zeros(1024, dtype=np.uint64)
    bins[0] = 1
    got = check(bins, 10, 1.0)
    assert got.max_cll == 0 and got.max_fall == 0 and got.max_cll_nits == 0.0


def test_refusals():
    lib = pkg.load()
    bins = np.ones(4096, dtype=np.uint64)
    out = pkg.ContentLightLevel()

    def code(b, bits, tr, p, o=out):
        return lib.avifgpu_light_level_from_histogram(b.ctypes.data if b is not None else None, bits, tr, p, ctypes.byref(o) if o is not None else None)
    assert code(bins, 10, PQ, 1.0) == 0
    for tr in (HLG, S428, CLIP, 7, -1):
        assert code(bins, 10, tr, 1.0) == pkg.formatBadParameters and b"PQ" in lib.avifgpu_last_error()
    for bits in (8, 9, 11, 16, 0, -10):
        assert code(bins, bits, PQ, 1.0) == pkg.formatBadParameters and b"bit depth" in lib.avifgpu_last_error()
    for p in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        assert code(bins, 10, PQ, p) == pkg.formatBadParameters and b"percentile" in lib.avifgpu_last_error()
    assert code(np.zeros(1024, dtype=np.uint64), 10, PQ, 1.0) == pkg.formatBadParameters and b"empty" in lib.avifgpu_last_error()
    assert code(None, 10, PQ, 1.0) == pkg.formatBadParameters
    assert lib.avifgpu_light_level_from_histogram(bins.ctypes.data, 10, PQ, 1.0, None) == pkg.formatBadParameters
    with pytest.raises(pkg.AvifGpuError):
        pkg.light_level_from_histogram(bins, 10, HLG, 1.0)


def test_arming_and_disarming_need_no_device():
    lib = pkg.load()
    bins = np.zeros(4096, dtype=np.uint64)
    try:
        for bits in (10, 12):
            for mem in (pkg.MEM_HOST, pkg.MEM_DEVICE):
                assert lib.avifgpu_histogram_attach(bins.ctypes.data, bits, mem) == 0
        for bits in (8, 9, 11, 16, 0):
            assert lib.avifgpu_histogram_attach(bins.ctypes.data, bits, pkg.MEM_HOST) == pkg.formatBadParameters
            assert b"bit depth" in lib.avifgpu_last_error()
        assert lib.avifgpu_histogram_attach(bins.ctypes.data, 10, 2) == pkg.formatBadParameters and b"mem_kind" in lib.avifgpu_last_error()
        assert lib.avifgpu_histogram_attach(None, 0, pkg.MEM_HOST) == 0            # disarm: the other arguments are not looked at
        assert lib.avifgpu_histogram_attach(None, 99, 99) == 0
        with pkg.code_histogram(bins, 12):
            pass
        with pytest.raises(pkg.AvifGpuError):
            with pkg.code_histogram(bins, 8):
                pass
        with pytest.raises(ValueError):
            with pkg.code_histogram(np.zeros(1024, dtype=np.uint64), 12):
                pass
        import torch
        for bad in (np.zeros(4096, dtype=np.uint32), torch.zeros(4096, dtype=torch.int32), torch.zeros(8192, dtype=torch.int64)[::2]):
            with pytest.raises(ValueError):
                with pkg.code_histogram(bad, 12):
                    pass
        for bad in (np.ones(4096, dtype=np.uint32), np.ones(1024, dtype=np.uint64)):
            with pytest.raises(ValueError):
                pkg.light_level_from_histogram(bad, 12)
    finally:
        lib.avifgpu_histogram_attach(None, 0, pkg.MEM_HOST)
    assert not bins.any()                                                           # bookkeeping only: nothing wrote


def test_armed_calls_without_a_bound_device_end_where_unarmed_calls_end():
    """With a histogram armed and no device bound (the case on a CPU-only box), a write call returns what it returns unarmed: the descriptor's own error first, then the
    no-device error (write_rows_any looks for a bound device before it looks at the arming; the mismatch refusals themselves are
    tests/test_gpu_light_level.py::test_a_mismatch_fails_before_anything_is_launched).  Nothing is counted."""
    lib = pkg.load()
    bound = lib.avifgpu_device_count() > 0                                          # an earlier test of the session may have bound one
    P4, S4 = ctypes.c_void_p * 4, ctypes.c_int64 * 4
    buf = ctypes.create_string_buffer(8192)
    ptrs, strides = P4(*[ctypes.addressof(buf)] * 4), S4(256, 256, 256, 256)

    def wcode(mem=pkg.MEM_HOST, **kw):
        base = dict(width=4, height=4, depth=32, planes=3, bit_depth=10, transfer=PQ, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
        base.update(kw)
        d = pkg.WriteDesc(**base)
        return lib.avifgpu_write_rows(ctypes.byref(d), 0, 4, buf, 256, ctypes.byref(ptrs), ctypes.byref(strides), mem, None)
    bins = np.zeros(4096, dtype=np.uint64)
    with pkg.code_histogram(bins, 12):
        assert wcode(bit_depth=9) == pkg.formatCannotRead
        assert wcode(bit_depth=10) == pkg.formatBadParameters
        assert (b"armed code histogram" if bound else b"no CPU fallback") in lib.avifgpu_last_error()
    assert not bins.any()


def test_probe_histogram_validates_before_it_looks_for_a_device():
    lib = pkg.load()
    buf = ctypes.create_string_buffer(4096)
    d = pkg.WriteDesc(width=4, height=4, depth=32, planes=3, bit_depth=10, transfer=PQ, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    assert lib.avifgpu_probe_histogram(ctypes.byref(d), 5, buf, 48, buf, None) == pkg.formatBadParameters
    assert lib.avifgpu_probe_histogram(ctypes.byref(d), 0, None, 48, buf, None) == pkg.formatBadParameters
    assert lib.avifgpu_probe_histogram(ctypes.byref(d), 0, buf, 47, buf, None) == pkg.formatBadParameters
    d.depth, d.bit_depth = 8, 8
    assert lib.avifgpu_probe_histogram(ctypes.byref(d), 0, buf, 48, buf, None) == pkg.formatBadParameters


# ---- the oracle side of the GPU bars --------------------------------------------------------------------------------------------
def max_code_bincount(desc, planes_out):
    """bincount of max(R, G, B) (gray: Y) of OUT_REFERENCE planes: interleaved RGB(A), or planar Y (+ A)."""
    p0 = planes_out[0].astype(np.int64)
    if desc.planes >= 3:
        m = p0.reshape(p0.shape[0], desc.width, desc.planes)[..., :3].max(axis=2)
    else:
        m = p0
    return np.bincount(m.reshape(-1), minlength=1 << desc.bit_depth)


@pytest.mark.parametrize("planes,bits,peak,alpha", [(3, 10, 1000, pkg.ALPHA_NONE), (4, 12, 1000, pkg.ALPHA_STRAIGHT), (1, 10, 203, pkg.ALPHA_NONE),
                                                    (3, 12, 80, pkg.ALPHA_NONE), (3, 12, 203, pkg.ALPHA_NONE), (3, 12, 4000, pkg.ALPHA_NONE),
                                                    (3, 12, 10000, pkg.ALPHA_NONE), (4, 10, 1000, pkg.ALPHA_PREMULTIPLIED), (2, 12, 1000, pkg.ALPHA_STRAIGHT)])
def test_oracle_codes_of_determined_sources_are_the_float64_codes(planes, bits, peak, alpha):
    """What the GPU truth test demands of the kernel, the oracle meets alone: on a determined source the histogram of its codes
    equals the histogram of the float64 codes."""
    tr = PQ
    d = pkg.WriteDesc(width=97, height=41, depth=32, planes=planes, bit_depth=bits, transfer=tr, peak_nits=peak, alpha_state=alpha,
                      output=pkg.OUT_REFERENCE)
    src, _ = truth64.make_determined_source(d)
    codes, mask = truth64.determined_codes(d, src)
    assert mask.all()
    want = np.bincount(codes.max(axis=2).reshape(-1), minlength=1 << bits)
    assert np.array_equal(max_code_bincount(d, harness.oracle_write(d, src)), want)


@pytest.mark.parametrize("tr", [HLG, S428])
def test_oracle_codes_of_determined_sources_other_curves(tr):
    d = pkg.WriteDesc(width=97, height=41, depth=32, planes=3, bit_depth=12, transfer=tr, peak_nits=1000, alpha_state=pkg.ALPHA_NONE,
                      output=pkg.OUT_REFERENCE)
    src, _ = truth64.make_determined_source(d)
    codes, mask = truth64.determined_codes(d, src)
    assert mask.all()
    assert np.array_equal(max_code_bincount(d, harness.oracle_write(d, src)), np.bincount(codes.max(axis=2).reshape(-1), minlength=4096))


# ---- the shim's decision ---------------------------------------------------------------------------------------------------------
def test_save_wants_light_level_over_every_mode_depth_and_transfer():
    lib = pkg.load()
    modes = {(False, 8): H.plugInModeRGBColor, (False, 16): H.plugInModeRGB48, (False, 32): H.plugInModeRGB96,
             (True, 8): H.plugInModeGrayScale, (True, 16): H.plugInModeGray16, (True, 32): H.plugInModeGray32}
    for (mono, depth), mode in modes.items():
        for tr in (PQ, HLG, S428, CLIP):
            for bits in (8, 10, 12):
                for premul in (0, 1):
                    fr = H.FormatRecord()
                    fr.depth, fr.imageMode, fr.planes = depth, mode, (1 if mono else 3)
                    o = H.SaveUIOptions()
                    o.imageBitDepth, o.hdrTransferFunction, o.premultipliedAlpha = bits, tr, premul
                    n = H.SaveUIOptions()
                    n.imageBitDepth, n.hdrTransferFunction, n.premultipliedAlpha = bits, tr, premul
                    assert lib.avifgpu_host_normalize_save_options(ctypes.byref(fr), ctypes.byref(n)) == 0
                    want = 1 if (depth == 32 and n.hdrTransferFunction == PQ) else 0
                    assert want == (1 if (depth == 32 and not mono and tr == PQ) else 0)     # 32-bit mono is saved as Clip (Write.cpp:235-240)
                    assert lib.avifgpu_host_save_wants_light_level(ctypes.byref(fr), ctypes.byref(o)) == want, (mono, depth, tr, bits)
                    assert (o.imageBitDepth, o.hdrTransferFunction, o.premultipliedAlpha) == (bits, tr, premul)   # the options are not modified
    assert lib.avifgpu_host_save_wants_light_level(None, None) == pkg.formatBadParameters
