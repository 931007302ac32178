"""CPU half of the whole-code-domain float opens (tests/test_zz_gpu_whole_float_opens.py is the GPU half).

 * The oracle inside its OWN bar (truth64.ORACLE_EOTF_EPS) on the very inputs the kernels are judged on: every 10-bit case of section A
   under both bars of tests/read_truth64.py, one band of every 12-bit family of section B under the float32-step bar.  So the bars are
   shown sound on these inputs before they judge a kernel.
 * The inputs hold what the GPU file's docstring claims, each claim counted.
 * read_truth64.unpremultiply_codes, the vectorised restatement of the reference's integer UnpremultiplyColor, equals the oracle's
   oracle_unpremultiply_u16 on every (code, alpha >= 1) pair at 10 bit and on every pair of every 16th alpha row at 12 bit.
"""
import numpy as np
import pytest

import float_open_cases as fc
import harness
import oracle_binding
import read_truth64 as rt
import truth64

pkg = harness.pkg
f32 = np.float32


def _oracle_inside_its_bar(cid, d, planes, chain_bar):
    eps = truth64.ORACLE_EOTF_EPS[rt._transfer(d.transfer_characteristics)]
    used = rt._check(cid, d, harness.oracle_read(d, planes), eps, planes, chain_bar=chain_bar)
    print(f"{cid}: the oracle's worst error / bound {used[0] if used[0] is None else round(used[0], 3)} (float64 chain), {used[1]:.3f} (float32 step)")


CASES_A = fc.cases_a()


@pytest.mark.parametrize("curve,chroma,fr,alpha,matrix", CASES_A, ids=[fc.case_id(*c) for c in CASES_A])
def test_oracle_inside_its_bar_on_the_10bit_square(curve, chroma, fr, alpha, matrix):
    planes = fc.ycc_planes(10, chroma, alpha)
    _oracle_inside_its_bar(fc.case_id(curve, chroma, fr, alpha, matrix), fc.ycc_desc(planes, 10, curve, chroma, fr, alpha, matrix), planes, True)


@pytest.mark.parametrize("family", list(fc.FAMILIES_B))
def test_oracle_inside_its_bar_on_one_12bit_band(family):
    chroma, fr, alpha, rows = fc.FAMILIES_B[family]
    band = (2048, rows)                                          # the band that begins at the neutral chroma row
    assert band in fc.bands_b(family)
    planes = fc.ycc_planes(fc.BITS_B, chroma, alpha, band=band)
    _oracle_inside_its_bar(f"{family}-rows2048", fc.ycc_desc(planes, fc.BITS_B, fc.CURVE_B, chroma, fr, alpha), planes, False)


# ---- the inputs hold what is claimed ------------------------------------------------------------------------------------------------------
def _v32_of_square(bits, fr, alpha=fc.NONE, curve="pq80"):
    """V32 of the BT.2020-NCL 4:4:4 square, band by band at 12 bit (a band is an image)."""
    bands = [None] if bits == 10 else fc.bands_b("444-full-opaque")
    for band in bands:
        planes = fc.ycc_planes(bits, "444", alpha, band=band)
        yield rt.ycc_v32(fc.ycc_desc(planes, bits, curve, "444", fr, alpha), planes)


@pytest.mark.parametrize("bits,least", [(10, 1000), (12, 4000)])
def test_square_holds_curve_arguments_below_the_first_code(bits, least):
    """BT.2020-NCL full range 4:4:4: colour samples with 0 < V32 < 1 / max, arguments no table-built test gives a curve (1 467 at
    10 bit, the smallest 5.2e-8; 5 859 at 12 bit, the smallest 2.2e-8)."""
    count, smallest = 0, 1.0
    for V in _v32_of_square(bits, 1):
        w = fc.small_window(V, bits)
        count += int(w.sum())
        smallest = min(smallest, float(V[w].min()) if w.any() else 1.0)
    print(f"{bits} bit: {count} samples with 0 < V32 < 1/max, the smallest {smallest:.3g}")
    assert count >= least and smallest < 1e-6


@pytest.mark.parametrize("fr", [1, 0], ids=["full", "limited"])
@pytest.mark.parametrize("alpha", [fc.NONE, fc.PREMUL], ids=["opaque", "premul"])
def test_square_clamps_at_both_ends_in_every_channel(fr, alpha):
    V, = _v32_of_square(10, fr, alpha)
    zeros, ones = (V == 0).sum((0, 1)), (V == 1).sum((0, 1))
    print(f"clamped at 0 per channel {zeros}, at 1 {ones}")
    assert np.all(zeros > 1000) and np.all(ones > 1000)


def test_inputs_hold_samples_on_both_sides_of_the_hlg_select():
    """Within two float32 steps of 0.5: the premultiplied full-range 4:4:4 square holds a sample above it, select_planes() samples
    below it.  None equals 0.5: none was found in any 10-bit input searched (fc.HLG_SELECT)."""
    V, = _v32_of_square(10, 1, fc.PREMUL, "hlg")
    planes = fc.select_planes()
    S = rt.ycc_v32(fc.ycc_desc(planes, 10, "hlg", "444", 1, fc.PREMUL), planes)
    print(f"(below, at, above) 0.5 within 2 steps: the square {fc.near_half(V)}, the select image {fc.near_half(S)}")
    assert fc.near_half(V)[2] >= 1 and fc.near_half(S)[0] >= 3


@pytest.mark.parametrize("curve", ["hlg", "hlg-ootf"])
def test_oracle_inside_its_bar_around_the_hlg_select(curve):
    planes = fc.select_planes()
    _oracle_inside_its_bar(f"{curve}-select", fc.ycc_desc(planes, 10, curve, "444", 1, fc.PREMUL), planes, True)


@pytest.mark.parametrize("bits,chroma", [(10, "444"), (10, "422"), (10, "420"), (12, "420")])
def test_alpha_0_and_opaque_meet_every_luma_column(bits, chroma):
    planes = fc.ycc_planes(bits, chroma, fc.PREMUL)
    n = 1 << bits
    a, y = planes[3], planes[0]
    assert a.shape == y.shape
    for code in (0, n - 1):
        assert np.all((a == code).any(axis=0)), code                      # every column of the image
        assert np.array_equal(np.unique(y[a == code]), np.arange(n))       # and under it every Y code


def test_12bit_square_gives_the_packed_curve_1000_code_values():
    """For the comparison of the packed with the scalar PQ: distinct code values i / 4095, 0 < i < 4095, that some V32 of the
    full-range 4:4:4 square equals exactly (1 008 - 1 700 per channel)."""
    n = 1 << 12
    cv = (np.arange(n, dtype=f32) / f32(n - 1)).view(np.uint32)
    seen = np.zeros((3, n), dtype=bool)
    for V in _v32_of_square(12, 1):
        bits = np.ascontiguousarray(V.astype(f32)).view(np.uint32)
        for ch in range(3):
            b = np.unique(bits[..., ch])
            i = np.minimum(np.searchsorted(cv, b), n - 1)
            seen[ch, i[cv[i] == b]] = True
    seen[:, [0, n - 1]] = False
    print(f"distinct code values met per channel {seen.sum(1)}, in any channel {int(seen.any(0).sum())}")
    assert np.all(seen.sum(1) >= 1000)


# ---- the integer unpremultiply, restated ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,step", [(10, 1), (12, 16)])
def test_unpremultiply_restatement_equals_the_oracle(bits, step):
    L = oracle_binding.load()
    maxc = (1 << bits) - 1
    code = np.arange(maxc + 1)
    fn = L.oracle_unpremultiply_u16
    for a in range(1, maxc + 1, step):
        want = np.fromiter((fn(int(c), a, maxc) for c in code), dtype=np.int64, count=code.size)
        got = rt.unpremultiply_codes(code, np.full_like(code, a), maxc)
        assert np.array_equal(got, want), (bits, a, np.flatnonzero(got != want)[:4])
    # alpha max is the identity, whatever the code
    assert np.array_equal(rt.unpremultiply_codes(code, np.full_like(code, maxc), maxc), code)
