"""32-bit saves behind a document profile held EXACTLY on determined sources (tests/truth64.py, "Behind a document profile").

The rate bars of tests/test_gpu_icc.py pool every plane at 99.5 %: a matrix coefficient rounded the wrong way, a matrix row applied
to the wrong channel in a tail path, channel 0's curve parameters used for channel 2, or a premultiply in front of the transform
all pass them.  Here the source is drawn so that every colour code is determined -- the float64 value of the ICC stage, widened by
the band of both judged evaluations and then by the curve's, does not straddle a code boundary -- and every output sample of every
plane, padding included, must equal the oracle's on float32(truth) rows bit for bit (and on lcms2's rows, where lcms2 is built):
icc = 1 / 2 / 4 / 6, both targets, every streaming kernel that takes an ICC stage and the generic one, at the shapes where their
edge paths run, under the three tuning words, device memory and padded host memory, an inner row tile, a continued save, and the
content light level histogram.  The last test measures how much of the band the kernels use (profiles/icc_truth/band_usage.txt)."""
import numpy as np
import pytest

import harness
import icc_profiles as ip
import truth64
from test_gpu_light_level import max_code_bincount, write_hist

pkg = harness.pkg
pytestmark = pytest.mark.gpu

DEFAULT_WORD = 1 | 2 | 4                 # the library's default tuning word
WORDS = {"default": DEFAULT_WORD, "stream": 1 | 2 | 4 | 8, "generic": 0}
MEMORY_WORD = 1 | 2 | 4 | 64             # icc = 6 with its curves looked up in memory instead of LDS
HDR = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
SDR = dict(matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709)
CURVES = [("pq80", dict(transfer=pkg.TRANSFER_PQ, peak_nits=80)), ("pq1000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=1000)),
          ("hlg", dict(transfer=pkg.TRANSFER_HLG)), ("pq10000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=10000)),
          ("smpte428", dict(transfer=pkg.TRANSFER_SMPTE428))]
CLIP = ("clip", dict(transfer=pkg.TRANSFER_CLIP))
REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C444, C422, C420 = pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420
BOX, NEAREST = pkg.DOWNSAMPLE_AVERAGE, pkg.DOWNSAMPLE_NEAREST
NONE, STRAIGHT, PREMUL = pkg.ALPHA_NONE, pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED


def _kw(w, h, planes, alpha, output, chroma, ds, target, curve, bits):
    """The save a target goes with: Rec.2020 -> an HDR curve and BT.2020, sRGB -> Clip and BT.601 with 709 primaries."""
    return dict(width=w, height=h, depth=32, planes=planes, bit_depth=bits, alpha_state=alpha, output=output, chroma=chroma,
                chroma_downsampling=ds, **curve[1], **(SDR if target == ip.SRGB else HDR))


def _icc_number(name, target):
    if name in ip.TABLES:
        return 6
    if target == ip.SRGB:
        return 4
    return 1 if name in ip.LINEAR else 2


def _streaming_kernel(name, target, kw):
    """The streaming kernel a device-memory save takes under the default word (launch_write_impl in csrc/write_kernels.hip), or None
    where the generic kernel runs: sampled curves (icc = 6), a different curve per channel, a non-linear profile to sRGB, RGBA with
    subsampled chroma or as interleaved codes."""
    if name in ip.TABLES or name == ip.PER_CHANNEL or (target == ip.SRGB and name not in ip.LINEAR):
        return None
    if kw["output"] == REF:
        return "write_rgb32_icc1_ycbcr444_hot" if kw["planes"] == 3 else None
    if kw["planes"] == 4:
        return "write_rgba32_ycbcra444_hot" if kw["chroma"] == C444 else None
    return "write_rgb32_icc1_ycbcr444_hot" if kw["chroma"] == C444 else "write_rgb32_ycbcr_sub_hot"


def _check_kernel(kernel, name, target, kw, word, mem):
    assert f"icc={_icc_number(name, target)}" in kernel, kernel
    if name in ip.TABLES:                                          # LDS where every table fits (<= 4096 entries: all of these) and bit 6 is clear
        assert (" lds" in kernel) == (not word & 64), kernel
    if word == 0:
        assert "write_px" in kernel, kernel
    elif mem == "device":
        want = _streaming_kernel(name, target, kw)
        assert (want or "write_px") in kernel, (kernel, want)
        if want and kw["output"] == REF and (kw["width"] * 6) % 16 == 0:
            assert "out=ref" in kernel, kernel


def _sources(d, name, target, seed):
    xf = ip.prepared(name, target)
    src, _ = truth64.make_determined_source_icc(d, xf, seed=seed)
    rows = truth64.icc_truth_rows(d, xf, src)
    if ip.lcms() is not None and name != ip.PER_CHANNEL:           # the live library hands the pixel loop rows that give the same planes
        live = ip.lcms_rows(name, target, src, d.width, d.planes)
        a, b = harness.oracle_write(d, rows), harness.oracle_write(d, live)
        assert all(np.array_equal(a[pl], b[pl]) for pl in a), name
    return xf, src, rows


def _assert_equal(got, want, what):
    assert sorted(got) == sorted(want)
    for pl in want:
        bad = np.argwhere(got[pl] != want[pl])
        assert bad.shape[0] == 0, (what, pl, bad.shape[0], bad[:8].tolist(), got[pl][tuple(bad[0])], want[pl][tuple(bad[0])])


def _run(gpu, name, target, kw, word=DEFAULT_WORD, mem="device", row0=0, nrows=None, seed=harness.SEED):
    d = pkg.WriteDesc(**kw)
    xf, src, rows = _sources(d, name, target, seed)
    pad = 24 if mem == "host" else 0
    want = harness.oracle_write(d, rows, row0=row0, nrows=nrows, stride_pad=pad, return_raw=True)
    try:
        gpu.lib.avifgpu_set_hot_variant(word)
        got = harness.gpu_write(gpu, d, src, row0=row0, nrows=nrows, mem=mem, stride_pad=pad, return_raw=True, icc=xf)
        kernel = gpu.last_kernel()
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
    _assert_equal(got, want, (kernel, name, target))
    _check_kernel(kernel, name, target, kw, word, mem)
    return kernel


# ---- every profile, both targets, every output form, at 67 x 21 ----------------------------------------------------------------------
OUTPUTS = [(3, NONE, REF, C444, BOX), (4, STRAIGHT, REF, C444, BOX), (4, PREMUL, REF, C444, BOX), (3, NONE, YCC, C444, BOX),
           (4, PREMUL, YCC, C444, BOX), (4, STRAIGHT, YCC, C444, BOX), (3, NONE, YCC, C422, BOX), (3, NONE, YCC, C420, NEAREST),
           (4, STRAIGHT, YCC, C420, BOX), (4, PREMUL, YCC, C422, NEAREST)]


def _basic_cases():
    out, i = [], 0
    for name in ip.ALL:
        for target in (ip.REC2020, ip.SRGB):
            for planes, a, output, chroma, ds in OUTPUTS:
                curve = CLIP if target == ip.SRGB else CURVES[i % len(CURVES)]
                bits = (10, 12)[(i // len(CURVES)) % 2]
                i += 1
                out.append((f"{name}-t{target}-p{planes}-a{a}-o{output}-c{chroma}-ds{ds}-{curve[0]}-b{bits}", name, target,
                            _kw(67, 21, planes, a, output, chroma, ds, target, curve, bits)))
    return out


# ---- what each kernel takes, at the shapes where its edge paths run (tests/test_gpu_t2_determined.py) ---------------------------------
# (label, profiles to rotate over, target, planes, alpha, output, chroma, downsampling)
KERNEL_CONFIGS = [
    ("icc1_444", ip.LINEAR, ip.REC2020, 3, NONE, YCC, C444, BOX), ("icc2_444", ip.CURVED, ip.REC2020, 3, NONE, YCC, C444, BOX),
    ("icc4_444", ip.LINEAR, ip.SRGB, 3, NONE, YCC, C444, BOX),
    ("icc1_ref", ip.LINEAR, ip.REC2020, 3, NONE, REF, C444, BOX), ("icc2_ref", ip.CURVED, ip.REC2020, 3, NONE, REF, C444, BOX),
    ("icc4_ref", ip.LINEAR, ip.SRGB, 3, NONE, REF, C444, BOX),
    ("icc1_420_box", ip.LINEAR, ip.REC2020, 3, NONE, YCC, C420, BOX), ("icc1_422_nearest", ip.LINEAR, ip.REC2020, 3, NONE, YCC, C422, NEAREST),
    ("icc2_422_box", ip.CURVED, ip.REC2020, 3, NONE, YCC, C422, BOX), ("icc2_420_nearest", ip.CURVED, ip.REC2020, 3, NONE, YCC, C420, NEAREST),
    ("icc4_420_box", ip.LINEAR, ip.SRGB, 3, NONE, YCC, C420, BOX), ("icc4_422_nearest", ip.LINEAR, ip.SRGB, 3, NONE, YCC, C422, NEAREST),
    ("icc1_rgba_straight", ip.LINEAR, ip.REC2020, 4, STRAIGHT, YCC, C444, BOX), ("icc1_rgba_premul", ip.LINEAR, ip.REC2020, 4, PREMUL, YCC, C444, BOX),
    ("icc4_rgba_straight", ip.LINEAR, ip.SRGB, 4, STRAIGHT, YCC, C444, BOX), ("icc4_rgba_premul", ip.LINEAR, ip.SRGB, 4, PREMUL, YCC, C444, BOX),
    ("icc2_rgba_premul", ip.CURVED, ip.REC2020, 4, PREMUL, YCC, C444, BOX),
    ("icc4_curved_444", ip.CURVED, ip.SRGB, 3, NONE, YCC, C444, BOX), ("icc2_rgba_ref_premul", ip.CURVED, ip.REC2020, 4, PREMUL, REF, C444, BOX),
    ("icc2_per_channel_422_box", [ip.PER_CHANNEL], ip.REC2020, 3, NONE, YCC, C422, BOX),
    ("icc4_per_channel_rgba_premul", [ip.PER_CHANNEL], ip.SRGB, 4, PREMUL, YCC, C444, BOX),
    ("icc6_420_box", ip.TABLES, ip.REC2020, 3, NONE, YCC, C420, BOX), ("icc6_rgba_ref_premul", ip.TABLES, ip.SRGB, 4, PREMUL, REF, C444, BOX),
    ("icc6_rgba_444_straight", ip.TABLES, ip.REC2020, 4, STRAIGHT, YCC, C444, BOX), ("icc6_422_nearest", ip.TABLES, ip.SRGB, 3, NONE, YCC, C422, NEAREST),
]
SHAPES = [(67, 21), (1003, 7), (1004, 7), (515, 5), (259, 5), (513, 3), (1, 3), (6, 2), (1024, 6),
          (520, 5), (8, 3)]                                        # the last two: rows of 16-byte multiples, the out=ref hand-off


def _kernel_cases():
    """Every configuration at every shape under the default word; all streaming kernels off on every second case, the size-gated
    ones forced on on every fourth (no ICC kernel is size-gated: that word must change nothing)."""
    out, i = [], 0
    for w, h in SHAPES:
        for label, names, target, planes, a, output, chroma, ds in KERNEL_CONFIGS:
            name = names[i % len(names)]
            curve = CLIP if target == ip.SRGB else CURVES[i % len(CURVES)]
            bits = (12, 10)[i % 2]
            kw = _kw(w, h, planes, a, output, chroma, ds, target, curve, bits)
            for word in ("default",) + (("generic",) if i % 2 == 0 else ()) + (("stream",) if i % 4 == 1 else ()):
                out.append((f"{label}-{w}x{h}-{name}-{curve[0]}-b{bits}-{word}", name, target, kw, word))
            i += 1
    return out


# One test per profile and target, per kernel configuration, per profile: each loops over its cases (a failure names kernel, profile,
# shape, plane and indices), so that the suite pays the per-test cost a hundred times and not a thousand.
@pytest.mark.parametrize("name,target", [(n, t) for n in ip.ALL for t in (ip.REC2020, ip.SRGB)])
def test_determined_icc_write_is_exact(gpu, name, target):
    cases = [c for c in _basic_cases() if c[1] == name and c[2] == target]
    assert len(cases) == len(OUTPUTS)
    for cid, _, _, kw in cases:
        _run(gpu, name, target, kw)


@pytest.mark.parametrize("label", [c[0] for c in KERNEL_CONFIGS])
def test_determined_icc_write_is_exact_on_every_kernel(gpu, label):
    cases = [c for c in _kernel_cases() if c[0].startswith(label + "-")]
    assert len(cases) >= len(SHAPES)
    for cid, name, target, kw, word in cases:
        _run(gpu, name, target, kw, word=WORDS[word], seed=harness.SEED + len(cid))


def test_every_icc_kernel_is_among_the_cases():
    """The cases above reach what they are meant to reach (each _run asserts its own kernel): every streaming kernel with every icc
    number it takes, the generic kernel with all four, and every parametric_mask of the mixed profiles."""
    seen = set()
    for _, name, target, kw, word in _kernel_cases():
        k = "write_px" if word == "generic" else (_streaming_kernel(name, target, kw) or "write_px")
        seen.add((k, _icc_number(name, target), "ref" if kw["output"] == REF else kw["chroma"], kw["chroma_downsampling"], kw["alpha_state"]))
    for icc in (1, 2, 4):
        assert ("write_rgb32_icc1_ycbcr444_hot", icc, C444, BOX, NONE) in seen and ("write_rgb32_icc1_ycbcr444_hot", icc, "ref", BOX, NONE) in seen
        assert {c for k, n, c, _, _ in seen if k == "write_rgb32_ycbcr_sub_hot" and n == icc} == {C420, C422}
        assert {ds for k, n, _, ds, _ in seen if k == "write_rgb32_ycbcr_sub_hot" and n == icc} == {BOX, NEAREST}
    for icc in (1, 4):
        assert {a for k, n, _, _, a in seen if k == "write_rgba32_ycbcra444_hot" and n == icc} == {STRAIGHT, PREMUL}
    assert {n for k, n, _, _, _ in seen if k == "write_px"} == {1, 2, 4, 6}
    masks = {ip.prepared(name, target).parametric_mask for _, name, target, _, _ in _kernel_cases() if name in ip.TABLES}
    assert masks == {0} | set(ip.MIXED_MASKS.values())


HOST_CASES = [c[:4] for c in (_basic_cases() + _kernel_cases())[::4]]          # padded strides in host memory: a quarter of the cases


@pytest.mark.parametrize("name", ip.ALL)
def test_determined_icc_write_is_exact_host_padded(gpu, name):
    cases = [c for c in HOST_CASES if c[1] == name]
    assert cases
    for cid, _, target, kw in cases:
        _run(gpu, name, target, kw, mem="host", seed=77)


ALL_WORDS = dict(WORDS, memory=MEMORY_WORD)
TILE_PROFILES = [("p3-linear", ip.REC2020, 3, NONE), ("srgb-parametric", ip.REC2020, 4, PREMUL), ("prophoto-linear-d50", ip.SRGB, 3, NONE),
                 ("p3-R-sampled-G-srgb-para-B-gamma2.2", ip.REC2020, 4, PREMUL)]


@pytest.mark.parametrize("name,target,planes,a", TILE_PROFILES)
def test_determined_icc_write_is_exact_on_an_inner_tile(gpu, name, target, planes, a):
    """An even-row tile with row0 > 0 that ends before the image does (what the multi-GPU sharding hands each device), 4:2:0 /
    4:2:2 / 4:4:4, every tuning word; bit 6 selects between the two forms of icc = 6 only, so that word goes with the sampled profile."""
    curve = CLIP if target == ip.SRGB else CURVES[1]
    for chroma, ds in ((C420, BOX), (C422, NEAREST), (C444, BOX)):
        for word in ALL_WORDS:
            if word != "memory" or name in ip.TABLES:
                _run(gpu, name, target, _kw(1003, 11, planes, a, YCC, chroma, ds, target, curve, 12), word=ALL_WORDS[word], row0=4, nrows=4)


@pytest.mark.parametrize("name", ip.TABLES)
def test_continued_icc6_save_equals_the_one_call_save(gpu, name):
    """One save issued as three calls that continue one another, rows [0, 4), [4, 8), [8, 11): the "continued save" of the table
    lifetime contract (include/avifgpu.h) reuses the curves uploaded by the first call.  Same planes as one call, and as the truth."""
    for word, (target, planes, a, output, chroma) in [(w, c) for w in ("default", "memory", "generic") for c in (
            (ip.REC2020, 3, NONE, REF, C444), (ip.SRGB, 4, PREMUL, YCC, C420), (ip.REC2020, 4, STRAIGHT, YCC, C444))]:
        curve = CLIP if target == ip.SRGB else CURVES[(planes + len(name)) % len(CURVES)]
        kw = _kw(259, 11, planes, a, output, chroma, BOX, target, curve, 12)
        d = pkg.WriteDesc(**kw)
        xf, src, rows = _sources(d, name, target, harness.SEED + planes)
        want = harness.oracle_write(d, rows, return_raw=True)
        w = ALL_WORDS[word]
        try:
            gpu.lib.avifgpu_set_hot_variant(w)
            one, _ = write_hist(gpu, d, src, icc=xf, arm=False, return_raw=True)
            three, _ = write_hist(gpu, d, src, icc=xf, arm=False, cuts=[(0, 4), (4, 4), (8, 3)], return_raw=True)
            kernel = gpu.last_kernel()
        finally:
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
        _check_kernel(kernel, name, target, kw, w, "device")
        _assert_equal(one, want, (kernel, name, "one call"))
        _assert_equal(three, want, (kernel, name, "three calls"))


@pytest.mark.parametrize("name", ["p3-linear", "adobergb-gamma2.2", "srgb-parametric", "p3-sampled-srgb-1024", "adobergb-R-linear-GB-sampled-256"])
def test_light_level_bins_equal_the_written_codes_behind_a_profile(gpu, name):
    """avifgpu_histogram_attach armed around a PQ save behind icc = 1, 2 and 6: on a determined source the bins EQUAL the bincount
    of max(R, G, B) of the planes the streaming kernel wrote, of the generic kernel's, and of the truth -- where an arbitrary source
    leaves tests/test_gpu_light_level.py only the interlocking of the cumulative counts."""
    for planes, a, bits, peak in [(p, al, b, pk) for p, al in ((3, NONE), (4, STRAIGHT), (4, PREMUL)) for b, pk in ((10, 80), (12, 1000))]:
        kw = _kw(1024, 12, planes, a, REF, C444, BOX, ip.REC2020, ("pq", dict(transfer=pkg.TRANSFER_PQ, peak_nits=peak)), bits)
        d = pkg.WriteDesc(**kw)
        xf, src, rows = _sources(d, name, ip.REC2020, harness.SEED + bits)
        want = harness.oracle_write(d, rows)
        truth = max_code_bincount(d, want)
        try:
            for word in (DEFAULT_WORD, 0):
                gpu.lib.avifgpu_set_hot_variant(word)
                for mem in ("device", "host"):
                    got, bins = write_hist(gpu, d, src, mem=mem, icc=xf)
                    kernel = gpu.last_kernel()
                    if mem == "device":
                        _check_kernel(kernel, name, ip.REC2020, kw, word, mem)
                    _assert_equal(got, want, (kernel, name, mem))
                    assert bins.sum() == d.width * d.height
                    assert np.array_equal(bins, max_code_bincount(d, got)), (kernel, mem, int(np.abs(bins - max_code_bincount(d, got)).sum()))
                    assert np.array_equal(bins, truth), (kernel, mem)
        finally:
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)


# ---- the kernels' half of the band, measured ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ip.ALL)
def test_icc_write_mismatches_use_at_most_the_band(gpu, name):
    """An UNDRAWN source (harness.make_write_source, 1024 x 64, 12-bit OUT_REFERENCE), default word and word 0: every sample whose
    GPU code differs from floor(truth code) sits next to a code boundary, and the float64 distance of the truth from the boundary
    that was crossed is at most that sample's band on that side -- the ICC stage's dv carried through premultiply and curve, plus
    the curve's band.  That is the band's claim, judged against the float64 truth.  The worst fraction per kernel is printed, and
    next to it the worst among the samples whose band is mostly dv (at least half of it): those judge the derivation of dv.
    profiles/icc_truth/band_usage.txt records a run.  Measured: behind the PQ curve at most 0.64 of the band, on icc = 1 with its
    exact matrix as on the others -- that is the PQ band's own use (1.3e-5 of its 2e-5, tests/truth64.py), dv is a hundredth of the
    band there; behind HLG 0.04 and SMPTE 428 0.06; behind Clip (sRGB target), where dv is about 0.7 of the band, at most 0.15."""
    for curve in (CURVES[1], CURVES[2], CURVES[4], CLIP):
        _band_usage(gpu, name, curve)


def _band_usage(gpu, name, curve):
    target = ip.SRGB if curve is CLIP else ip.REC2020
    xf = ip.prepared(name, target)
    kw = _kw(1024, 64, 3, NONE, REF, C444, BOX, target, curve, 12)
    d = pkg.WriteDesc(**kw)
    src = harness.make_write_source(d, seed=31)
    if truth64.icc_has_nonlinear_parametric(xf):
        src = np.abs(src)
    t, lo, hi, lo_dv, hi_dv = truth64.icc_code_interval(d, xf, src.reshape(d.height, d.width, 3), parts=True)
    maxv = float((1 << d.bit_depth) - 1)
    code = np.floor(np.clip(t, 0.0, maxv))
    for word in (DEFAULT_WORD, 0):
        try:
            gpu.lib.avifgpu_set_hot_variant(word)
            got = harness.gpu_write(gpu, d, src, icc=xf)[0].reshape(d.height, d.width, 3).astype(np.float64)
            kernel = gpu.last_kernel()
        finally:
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
        _check_kernel(kernel, name, target, kw, word, "device")
        up, down = got > code, got < code
        frac, share = np.zeros_like(t), np.zeros_like(t)
        frac[up] = (got[up] - t[up]) / (hi[up] - t[up])           # the boundary crossed upwards is the code that was written
        share[up] = (hi_dv[up] - t[up]) / (hi[up] - t[up])
        frac[down] = (t[down] - (got[down] + 1.0)) / (t[down] - lo[down])
        share[down] = (t[down] - lo_dv[down]) / (t[down] - lo[down])
        worst = float(frac.max())
        mostly_dv = frac[share >= 0.5]
        print(f"band usage: {name} target {target} {curve[0]} word {word}: {int(up.sum() + down.sum())} of {t.size} samples differ from "
              f"floor(truth), worst fraction of the band {worst:.3f} (dv is {float(share.flat[frac.argmax()]):.2f} of the band there), "
              f"where dv is most of the band {float(mostly_dv.max()) if mostly_dv.size else 0.0:.3f} ({int((mostly_dv > 0).sum())} samples)  "
              f"[{kernel.split('<')[0]} icc={_icc_number(name, target)}]")
        assert worst <= 1.0, (kernel, worst, np.argwhere(frac > 1.0)[:8].tolist())
