"""CPU pins of the ICC half of tests/truth64.py (no GPU): the float64 truth and the band that tests/test_gpu_icc_determined.py judges
the kernels by are first held against the real lcms2 and the oracle.

 * On determined sources -- every profile of tests/test_gpu_icc.py (PROFILES, SAMPLED, MIXED), both targets, 10 and 12 bit, PQ 80 /
   1000 / 10000, HLG, SMPTE 428 (Rec.2020 target) and Clip (sRGB target), 3 planes, 4 planes straight and premultiplied -- lcms2's
   row conversion followed by the oracle's pixel loop equals truth64.determined_codes_icc sample for sample, alpha included; and
   the oracle fed with float32(truth) rows gives the same planes, which is what lets the GPU half run where lcms2 is absent.
 * The lcms2 half of the band is measured on 400 000 pixels per profile and target: at most 2 of the 4 units allowed.
 * The redraw replaces at most 0.6 of a case's pixels (counted with repeats) and keeps the distribution.
 * The same functions on torch tensors give the same codes and masks.
Profiles come from the live lcms2 where oracle/liboracle_icc.so is built, else from tests/golden/icc_truth_profiles.npz; the checks
that need lcms2's arithmetic skip without it."""
import numpy as np
import pytest

import harness
import icc_profiles as ip
import truth64

pkg = harness.pkg

W, H = 67, 21
HDR_CURVES = [("pq80", dict(transfer=pkg.TRANSFER_PQ, peak_nits=80)), ("pq1000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=1000)),
              ("pq10000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=10000)), ("hlg", dict(transfer=pkg.TRANSFER_HLG)),
              ("smpte428", dict(transfer=pkg.TRANSFER_SMPTE428))]
CLIP = ("clip", dict(transfer=pkg.TRANSFER_CLIP))
PLANE_ALPHAS = [(3, pkg.ALPHA_NONE), (4, pkg.ALPHA_STRAIGHT), (4, pkg.ALPHA_PREMULTIPLIED)]
CASES = [(name, ip.REC2020, c) for name in ip.SPECS for c in HDR_CURVES] + [(name, ip.SRGB, CLIP) for name in ip.SPECS]
IDS = [f"{name}-{c[0]}" for name, _, c in CASES]
# ... and the transform with a different parametric curve per channel (icc_profiles.PER_CHANNEL): no profile, so no lcms2 run
TRUTH_CASES = CASES + [(ip.PER_CHANNEL, ip.REC2020, c) for c in HDR_CURVES] + [(ip.PER_CHANNEL, ip.SRGB, CLIP)]
TRUTH_IDS = [f"{name}-{c[0]}" for name, _, c in TRUTH_CASES]


def _descs(ckw):
    for bits in (10, 12):
        for planes, a in PLANE_ALPHAS:
            yield pkg.WriteDesc(width=W, height=H, depth=32, planes=planes, bit_depth=bits, alpha_state=a, output=pkg.OUT_REFERENCE, **ckw)


def _split(d, planes_out):
    got = planes_out[0].reshape(H, W, d.planes).astype(np.int64)
    return got[..., :3], (got[..., 3] if d.planes == 4 else None)


def _determined(d, name, target):
    xf = ip.prepared(name, target)
    src, replaced = truth64.make_determined_source_icc(d, xf)
    print(f"{name} target {target} transfer {d.transfer} peak {d.peak_nits} {d.bit_depth}-bit planes {d.planes} alpha {d.alpha_state}: "
          f"{replaced} of {H * W} pixels drawn again")
    assert replaced <= 0.6 * H * W, replaced                      # redraws of whole pixels, counted with repeats
    codes, mask = truth64.determined_codes_icc(d, xf, src)
    assert mask.all()                                              # every sample is judged: nothing is masked out below
    return xf, src, codes


@pytest.mark.parametrize("name,target,curve", TRUTH_CASES, ids=TRUTH_IDS)
def test_oracle_on_truth_rows_equals_determined_codes(name, target, curve):
    """float32(truth) rows through the oracle's pixel loop: the codes of determined_codes_icc, alpha included."""
    for d in _descs(curve[1]):
        xf, src, codes = _determined(d, name, target)
        col, alpha = _split(d, harness.oracle_write(d, truth64.icc_truth_rows(d, xf, src)))
        assert np.array_equal(col, codes), (name, d.bit_depth, d.planes, d.alpha_state, int(np.sum(col != codes)))
        if alpha is not None:
            assert np.array_equal(alpha, truth64.alpha_codes(d, src))


@pytest.mark.parametrize("name,target,curve", CASES, ids=IDS)
def test_lcms2_then_oracle_equals_determined_codes(name, target, curve):
    """The reference's flow -- lcms2 converts the row in place, the pixel loop runs on the converted row -- gives the codes of
    determined_codes_icc sample for sample, and the very planes the oracle gives on float32(truth) rows."""
    if ip.lcms() is None:
        pytest.skip(ip.NO_LCMS)
    for d in _descs(curve[1]):
        xf, src, codes = _determined(d, name, target)
        want = harness.oracle_write(d, ip.lcms_rows(name, target, src, d.width, d.planes), return_raw=True)
        col, alpha = _split(d, harness._trim(d, want, d.height, harness.write_planes))
        assert np.array_equal(col, codes), (name, d.bit_depth, d.planes, d.alpha_state, int(np.sum(col != codes)))
        if alpha is not None:
            assert np.array_equal(alpha, truth64.alpha_codes(d, src))
        mine = harness.oracle_write(d, truth64.icc_truth_rows(d, xf, src), return_raw=True)
        assert np.array_equal(mine[0], want[0])


@pytest.mark.parametrize("target", [ip.REC2020, ip.SRGB])
@pytest.mark.parametrize("name", list(ip.SPECS))
def test_lcms2_half_of_the_band_is_measured(name, target):
    """lcms2's float output against the float64 truth on a dense draw, in units of 2^-24 * sum |m||t| (Rec.2020 target) and of
    2^-24 * (slope * sum |m||t| + |w|) (sRGB target): measured at most 1.96 and 1.29.  The band allows 4; at most half may be used."""
    if ip.lcms() is None:
        pytest.skip(ip.NO_LCMS)
    n = 400000
    xf = ip.prepared(name, target)
    col = truth64._draw_colour(np.random.default_rng(7), n * 3).reshape(1, n * 3)
    if truth64.icc_has_nonlinear_parametric(xf):
        col = np.abs(col)
    got = ip.lcms_rows(name, target, col, n, 3).reshape(n, 3).astype(np.float64)
    px = col.reshape(n, 3)
    dev = np.abs(got - truth64.icc_stage64(xf, px)[0])
    unit = truth64.icc_lcms_unit(xf, px)
    assert np.all(dev[unit == 0] == 0)                             # nothing in, nothing out
    worst = float(np.max(dev[unit > 0] / unit[unit > 0]))
    print(f"{name} target {target}: lcms2 deviates by at most {worst:.3f} units")
    assert worst <= 0.5 * truth64.ICC_LCMS_UNITS, worst
    assert np.all(dev <= truth64.icc_band(xf, px))                 # ... and sits inside the band, every sample


@pytest.mark.parametrize("name", ip.ALL)
def test_determined_icc_source_keeps_the_distribution(name):
    for target, ckw in ((ip.REC2020, dict(transfer=pkg.TRANSFER_PQ, peak_nits=80)), (ip.SRGB, dict(transfer=pkg.TRANSFER_CLIP))):
        d = pkg.WriteDesc(width=W, height=H, depth=32, planes=4, bit_depth=12, alpha_state=pkg.ALPHA_PREMULTIPLIED,
                          output=pkg.OUT_REFERENCE, **ckw)
        xf = ip.prepared(name, target)
        src, _ = truth64.make_determined_source_icc(d, xf)
        px = src.reshape(H, W, 4)
        col, a = px[..., :3], px[..., 3]
        assert 0.05 < np.mean(col > 1.0) < 0.15                    # highlights up to 12.5
        assert col.max() <= 125.0
        if not truth64.icc_has_nonlinear_parametric(xf):           # linear and sampled profiles keep their negatives
            assert np.any(col < 0)
        else:
            assert not np.any(col < 0)
        assert np.any(a == 0) and np.any(a == 1) and np.any(a > 1) and np.any(a < 0)


def test_word_restatement_equals_the_tabulated_curve_ends_and_steps():
    """quick_saturate_word64 at the places where the magic-number floor and the saturation tests decide: the word steps at
    (k + 0.5) / 65535 rounded to 2^-16 of the scaled value, saturates at both ends, and takes negatives to 0."""
    v = np.array([-1.0, -1e-9, 0.0, 7e-6, 7.7e-6, 1.0 / 65535.0, 0.5, 1.0 - 2.0 ** -24, 1.0, 12.5], np.float32)
    d = v.astype(np.float64) * 65535.0 + 0.5
    want = np.where(d <= 0, 0, np.where(d >= 65535.0, 65535, np.floor(np.round((np.clip(d, 0, 65535) - 32767.0) * 65536.0) / 65536.0) + 32767))
    assert np.array_equal(truth64.quick_saturate_word64(v), want)
    assert list(truth64.quick_saturate_word64(v)[[0, 1, 2, 8, 9]]) == [0, 0, 0, 65535, 65535]


@pytest.mark.parametrize("name,target,ckw", [("p3-linear", ip.REC2020, dict(transfer=pkg.TRANSFER_PQ, peak_nits=1000)),
                                             ("adobergb-gamma2.2", ip.REC2020, dict(transfer=pkg.TRANSFER_HLG)),
                                             ("srgb-parametric", ip.SRGB, dict(transfer=pkg.TRANSFER_CLIP)),
                                             ("prophoto-sampled-per-channel-33", ip.REC2020, dict(transfer=pkg.TRANSFER_SMPTE428)),
                                             ("p3-R-sampled-G-srgb-para-B-gamma2.2", ip.SRGB, dict(transfer=pkg.TRANSFER_CLIP)),
                                             (ip.PER_CHANNEL, ip.REC2020, dict(transfer=pkg.TRANSFER_PQ, peak_nits=80))])
def test_torch_icc_codes_and_masks_equal_numpy(name, target, ckw):
    """One case per kind of curve stage (linear, gamma, parametric type 4, sampled, mixed, a parametric curve per channel): the functions on torch tensors (here on
    the CPU) give the codes, masks and bands they give on numpy arrays."""
    import torch
    d = pkg.WriteDesc(width=W, height=H, depth=32, planes=4, bit_depth=12, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_REFERENCE, **ckw)
    xf = ip.prepared(name, target)
    src = harness.make_write_source(d, seed=5)
    if truth64.icc_has_nonlinear_parametric(xf):
        src = np.abs(src)
    codes, mask = truth64.determined_codes_icc(d, xf, src)
    tc, tm = truth64.determined_codes_icc(d, xf, torch.from_numpy(src))
    assert np.array_equal(tc.numpy().astype(np.int64), codes) and np.array_equal(tm.numpy(), mask)
    assert 0 < mask.mean() < 1                                     # an undrawn source: both answers occur
    px = src.reshape(H, W, 4)[..., :3]
    assert np.allclose(truth64.icc_band(xf, torch.from_numpy(px)).numpy(), truth64.icc_band(xf, px), rtol=1e-9, atol=0)
