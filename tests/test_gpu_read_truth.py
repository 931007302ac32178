"""Float-tier opens (32-bit documents) against float64 truth of the WHOLE chain, sample by sample (avif_oracle.c:750-790,
YuvDecode.cpp:281-696, ReadHeifImage.cpp:1027-1176).

tests/test_gpu_read.py holds every 32-bit open to 1e-4 relative of the oracle, and tests/test_gpu_t2_truth.py holds the EOTF alone
to 1e-5 (PQ) / 2e-6 (HLG, SMPTE 428) on planar RGB.  A kernel whose YCbCr -> RGB step, chroma index, limited-range table, float
unpremultiply or HLG OOTF is a few ulps off fits under 1e-4.  Here the truth is computed in float64 from the float32 tables as the
reference builds them and the float32 kr, kb:

    R = Y + 2(1 - kr) Cr,  B = Y + 2(1 - kb) Cb,  G = Y - 2(kr(1 - kr) Cr + kb(1 - kb) Cb) / kg   (kg = 1 - kr - kb), clamped;
    unpremultiply min(c / A, 1); EOTF; HLG OOTF

and every colour sample must satisfy |k - T| <= eps |T| + dT(dV) + 1e-12, where
 * eps is the EOTF bar (KERNEL_EOTF_EPS for the kernels; ORACLE_EOTF_EPS for the oracle, whose float32 PQ formula cancels),
   widened by the OOTF's own float32 evaluation where one is applied;
 * dV bounds the float32 roundings of the YCbCr -> RGB step: N * 2^-24 * (|Y| + |coef * C|) with N = 3 for R and B (1 - kr, the
   product, the sum) and N = 9 for G (1 - kr, kr(1 - kr), the product, twice; the sum; kg = 1 - kr - kb rounded twice in float32;
   the quotient; the difference), then / A plus one rounding of the quotient where the colour is unpremultiplied;
 * dT(dV) is the largest excursion of the float64 chain (curve and OOTF) when each channel's V moves by its dV, summed over the
   channels (for each channel the chain is monotone in V, so this is |dT/dV| * dV taken at its worst point).
Alpha is table lookup only and must be bit-exact.  Mono and planar RGB carry no float32 step in front of the curve (dV = 0).

A second, tighter bar takes the YCbCr -> RGB step, clamp and unpremultiply in float32 exactly as the reference orders them (the
kernels claim those bits: the integer tiers hold them bit-exact) and only the curve in float64: |k - T32| <= eps |T32| + 1e-12.
That is the bar a kr / kg / kb a few ulps off, or a reordered sum, fails where the float64 bound's rounding budget would hide it.

The CPU half checks both bounds against the oracle, so they are shown sound before they judge a kernel.
The truth and the bars themselves live in tests/read_truth64.py, which the whole-domain files share."""
import numpy as np
import pytest

import cases
import harness
import oracle_binding
import truth64

from read_truth64 import N_G, N_RB, OOTF_EPS, _chain, _check, _full, _split, _transfer, _ycc_float32, truth_and_bound   # noqa: F401 (the truth lives there)

pkg = harness.pkg


def _read_truth_cases():
    out = [(cid, kw) for cid, kw in cases.read_cases() if cases.is_float_tier_read(kw)]
    for tc in (pkg.TC_PQ, pkg.TC_HLG, pkg.TC_SMPTE428):              # limited range, every chroma format
        for chroma, a in ((pkg.CHROMA_420, pkg.ALPHA_PREMULTIPLIED), (pkg.CHROMA_422, pkg.ALPHA_STRAIGHT), (pkg.CHROMA_444, pkg.ALPHA_NONE)):
            for bits in (10, 12):
                out.append((f"f32-limited-tc{tc}-c{chroma}-a{a}-b{bits}",
                            dict(width=67, height=21, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=bits, depth=32, alpha_state=a,
                                 matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709, full_range_flag=0,
                                 transfer_characteristics=tc, pq_peak_nits=1000)))
    for m, pr in ((pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT709, pkg.PRIMARIES_BT709)):   # the other kg
        out.append((f"f32-m{m}-420-premul", dict(width=67, height=21, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12,
                                                 depth=32, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=m, color_primaries=pr,
                                                 transfer_characteristics=pkg.TC_PQ, pq_peak_nits=80)))
    return out


OVER_RANGE = [cid for cid, kw in _read_truth_cases() if kw["colorspace"] != pkg.COLORSPACE_RGB][::3]


def make_source(d, cid, seed=harness.SEED):
    """harness.make_read_source, plus (for a third of the YCbCr / mono cases) 3 % of every plane at maxc + 1 ... maxc + 7."""
    planes = harness.make_read_source(d, seed=seed)
    if cid in OVER_RANGE:
        rng = np.random.default_rng(seed + 7)
        maxc = (1 << d.bit_depth) - 1
        for pl, arr in planes.items():
            w = harness.read_planes(d)[pl][0]
            m = rng.random(arr[:, :w].shape) < 0.03
            arr[:, :w][m] = maxc + rng.integers(1, 8, size=int(m.sum()))
    return planes


@pytest.mark.parametrize("cid,kw", _read_truth_cases())
def test_oracle_open_within_float64_bound(cid, kw):
    """CPU: the oracle itself meets the bound with its own EOTF error (PQ: 5.9e-5 measured, bar 7e-5)."""
    d = pkg.ReadDesc(**kw)
    planes = make_source(d, cid)
    eps = truth64.ORACLE_EOTF_EPS[_transfer(d.transfer_characteristics)]
    _check(cid, d, harness.oracle_read(d, planes), eps, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,kw", _read_truth_cases())
def test_kernel_open_within_float64_bound(gpu, cid, kw):
    d = pkg.ReadDesc(**kw)
    planes = make_source(d, cid)
    eps = truth64.KERNEL_EOTF_EPS[_transfer(d.transfer_characteristics)]
    got = harness.gpu_read(gpu, d, planes, mem="device")
    assert "read" in gpu.last_kernel()
    r = _check(cid, d, got, eps, planes)
    print(f"{cid}: worst error / bound {r[0]:.3f} (float64 chain), {r[1]:.3f} (float32 step, float64 curve)")
