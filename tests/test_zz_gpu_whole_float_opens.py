"""Float-tier (32-bit host) opens held to float64 truth on WHOLE code domains, every sample of every opened image under a bar.

The integer opens run on every code combination (tests/test_zz_gpu_whole_domain_read.py) and the float-tier saves on every float32
(tests/test_zz_gpu_whole_float_domain.py); a 32-bit open was judged on 67 x 21 random frames and on the n codes of an opaque
planar-RGB open.  Here the product's own kernels run over

  A  YCbCr at 10 bit on the Latin square -- every (Y, Cb), (Y, Cr), (Cb, Cr) pair: PQ 80 nits in all 18 combinations of chroma format,
     range and alpha; PQ 10 000 nits, HLG, HLG + OOTF and SMPTE 428 on six forms each; HLG + OOTF at gamma 1.0; three more divisors kg;
     and every (Y, alpha) pair under the chroma fc.HLG_SELECT, which holds samples one and two floats below the HLG select at 0.5 (the
     squares hold one sample next to it, above)
  B  YCbCr at 12 bit, PQ, the same square in row bands (a band is itself an image; the bands together are the square)
  C  planar RGB and gray with alpha on every (code, alpha) pair, 10 bit (12 bit: PQ premultiplied, in bands)
  D  one curve, one value: PQ, HLG and SMPTE 428 are functions of one float, so every open of A must map a float32 argument V32 to the
     SAME output bits as the 4:4:4 aligned open does -- whichever chroma format, pitch, lane slot of the packed curve or alpha form --
     and at 12 bit the packed PQ of the YCbCr opens must give the bits of the scalar PQ behind the planar-RGB table wherever its
     argument is a code value i / 4095

against tests/read_truth64.py: |k - T32| <= eps |T32| + 1e-12 on every sample (the float32 step of the reference under the float64
curve), and on images of at most 2^21 pixels also the float64-chain bar; eps = truth64.KERNEL_EOTF_EPS, N_RB, N_G, OOTF_EPS and the
floor as they stand; the HLG low piece, which is two products, has a three-rounding bar of its own beside them (_hlg_low_piece).  Alpha is
bit-equal to its table value.  Every case asserts its kernel form from the launch label, 10-bit cases run
with contiguous planes (aligned, flat where the form has a flat launch) and with ODD_PAD samples behind each row (unaligned), and prints
worst error / bound for both bars and for the samples with 0 < V32 < 1 / max alone -- curve arguments below the first code value, which
only a YCbCr open produces and no table-built test ever saw.  With AVIFGPU_FLOAT_OPENS_RECORD=<directory> the lines are appended to
files there (profiles/float_opens/ was written so).

Inputs and cases: tests/float_open_cases.py; tests/test_whole_float_opens.py counts what they hold and keeps the oracle inside its own
bar on them.  The file is named to be collected after tests/test_zz_gpu_whole_float_domain.py: every earlier GPU test keeps its place.
"""
import os
import time

import numpy as np
import pytest

import exhaustive_inputs as xi
import float_open_cases as fc
import harness
import read_truth64 as rt
import truth64

pkg = harness.pkg
pytestmark = pytest.mark.gpu

RECORD = os.environ.get("AVIFGPU_FLOAT_OPENS_RECORD")
ODD_PAD = fc.ODD_PAD


def _record(name, line):
    print(line)
    if RECORD:
        os.makedirs(RECORD, exist_ok=True)
        with open(os.path.join(RECORD, name + ".txt"), "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The shared inputs and the value maps go when this file's tests are done."""
    yield
    fc.release_inputs()
    _VALUE_MAPS.clear()
    _SCALAR_CODES.clear()
    _SCALAR_TABLE.clear()


def _transfer(d):
    return rt._transfer(d.transfer_characteristics)


def _assert_form(gpu, d, pad):
    """read_px<cs=,depth=32,alpha=,xs=,ys=,transfer=,aligned=>, ' tables=none' exactly where read_arith_policy (csrc/read_kernels.hip)
    decodes a 32-bit host without tables -- full range, at most 12 bit, and 4:2:2 without alpha or gray -- and ' flat' where the launch
    is flat."""
    label = gpu.last_kernel()
    ycc, mono = d.colorspace == pkg.COLORSPACE_YCBCR, d.colorspace == pkg.COLORSPACE_MONOCHROME
    xs, ys = harness.chroma_shift(d.chroma) if ycc else (0, 0)
    alpha = int(d.alpha_state != pkg.ALPHA_NONE)
    transfer = pkg.TRANSFER_PQ if mono else _transfer(d)              # a gray open is PQ whatever the descriptor says
    assert label.startswith(f"read_px<cs={d.colorspace},depth=32,alpha={alpha},xs={xs},ys={ys},transfer={transfer},aligned={int(pad == 0)}>"), label
    arith = bool(d.full_range_flag) and d.bit_depth <= 12 and ((ycc and xs == 1 and ys == 0 and not alpha) or mono)
    assert (" tables=none" in label) == arith, label
    assert label.endswith(" flat") == (pad == 0 and ys == 0), label
    return label


def _fmt(v):
    return "-" if v is None else f"{v:.3f}"


def _open_and_judge(gpu, cid, d, planes, pads, section, after=None):
    """Truth once, then one open per pitch: label, both bars (the float64 chain up to CHAIN_BAR_PIXELS), alpha bits, the small window's
    own usage.  after(pad, out_bits, parts) runs the case's further assertions on the (H, W, ncol) uint32 colour bits."""
    t0 = time.perf_counter()
    eps = truth64.KERNEL_EOTF_EPS[_transfer(d)]
    chain_bar = d.width * d.height <= fc.CHAIN_BAR_PIXELS
    parts = rt.truth_parts(d, planes, eps, chain_bar)
    window = fc.small_window(parts.V32, d.bit_depth)
    nwin = int(window.sum())
    ncol = parts.V32.shape[-1]
    for pad in pads:
        got = harness.gpu_read(gpu, d, planes if pad == 0 else xi.with_stride_pad(planes, pad))
        label = _assert_form(gpu, d, pad)
        used = rt._check((cid, f"pad={pad}", label), d, got, eps, planes, parts=parts)
        col = rt._split(d, got)[0]
        win32 = float(np.max((np.abs(col - parts.T32) / parts.bound32)[window])) if nwin else None
        win64 = float(np.max((np.abs(col - parts.T) / parts.bound)[window])) if nwin and chain_bar else None
        extra = after(pad, got.reshape(d.height, d.width, -1)[..., :ncol].view(np.uint32), parts) if after else ""
        _record(section, f"{cid} pad={pad}: worst error / bound {_fmt(used[0])} (float64 chain) {_fmt(used[1])} (float32 step); on the {nwin} samples "
                         f"with 0 < V32 < 1/max {_fmt(win64)} / {_fmt(win32)}; {d.width} x {d.height}; {label}{extra}")
    _record(section, f"{cid}: {time.perf_counter() - t0:.2f} s")
    return parts


# ---- the HLG low piece: arithmetic only ---------------------------------------------------------------------------------------------------------
HLG_LOW_ROUNDINGS = 3


def _hlg_low_piece(what, obits, parts):
    """HLG without OOTF at or below the select (V32 <= 0.5) is v * v * RN(1/3): two float32 products, each rounded once, and no
    transcendental.  Against the float64 value of the same expression (truth64.hlg_to_linear64 keeps the reference's float32 constant)
    that is 2 x 2^-24 relative; a third rounding is allowed for a form that orders the products differently or divides by 3.  A bar of
    its own, 16 times tighter than KERNEL_EOTF_EPS (which has to cover the v_exp_f32 of the high piece), plus one denormal step."""
    lo = parts.V32 <= 0.5
    err = np.abs(obits.view(np.float32).astype(np.float64) - parts.T32)[lo]
    bound = HLG_LOW_ROUNDINGS * rt.U * parts.T32[lo] + 2.0 ** -149
    assert np.all(err <= bound), (what, "the HLG low piece is more than three roundings from v * v / 3", int(np.sum(err > bound)), float(np.max(err / bound)))
    return f"; low piece at most {float(np.max(err / bound)) * HLG_LOW_ROUNDINGS:.2f} x 2^-24 from v * v / 3 on {int(lo.sum())} samples"


# ---- D: one curve, one value ----------------------------------------------------------------------------------------------------------------
_VALUE_MAPS = {}                  # (curve, full range, matrix) -> (sorted distinct V32 bit patterns, the output bits of each)


def _bits32(V32):
    return np.ascontiguousarray(V32.astype(np.float32)).view(np.uint32).reshape(-1)


def _single_valued_map(vbits, obits, what):
    order = np.argsort(vbits, kind="stable")
    v, o = vbits[order], obits[order]
    same = v[1:] == v[:-1]
    clash = same & (o[1:] != o[:-1])
    assert not clash.any(), (what, "one argument, two results", int(clash.sum()),
                             [(hex(int(v[1:][i])), hex(int(o[:-1][i])), hex(int(o[1:][i]))) for i in np.flatnonzero(clash)[:4]])
    first = np.r_[True, ~same]
    return v[first], o[first]


def _value_map(gpu, curve, fr, matrix):
    """V32 bit pattern -> output bit pattern of the 4:4:4 aligned open without alpha of (curve, range, matrix) on the 10-bit square;
    asserted single-valued over its 3 x 2^20 samples (every channel, every lane slot of the packed PQ)."""
    key = (curve, fr, matrix)
    if key not in _VALUE_MAPS:
        planes = fc.ycc_planes(10, "444", fc.NONE)
        d = fc.ycc_desc(planes, 10, curve, "444", fr, fc.NONE, matrix)
        got = harness.gpu_read(gpu, d, planes)
        _assert_form(gpu, d, 0)
        _VALUE_MAPS[key] = _single_valued_map(_bits32(rt.ycc_v32(d, planes)), np.ascontiguousarray(got).view(np.uint32).reshape(-1), key)
    return _VALUE_MAPS[key]


def _agrees_with_value_map(gpu, key, vbits, obits, what):
    mv, mo = _value_map(gpu, *key)
    i = np.minimum(np.searchsorted(mv, vbits), mv.size - 1)
    hit = mv[i] == vbits
    bad = hit & (mo[i] != obits)
    assert not bad.any(), (what, "differs from the 4:4:4 aligned open on the same float32 argument", int(bad.sum()),
                           [(hex(int(vbits[j])), hex(int(obits[j])), hex(int(mo[i[j]]))) for j in np.flatnonzero(bad)[:4]])
    return int(hit.sum()), int(np.unique(vbits[hit]).size)


# ---- A: YCbCr on the 10-bit Latin square ---------------------------------------------------------------------------------------------------
CASES_A = fc.cases_a()


@pytest.mark.parametrize("curve,chroma,fr,alpha,matrix", CASES_A, ids=[fc.case_id(*c) for c in CASES_A])
def test_ycbcr_open_10bit_latin_square(gpu, curve, chroma, fr, alpha, matrix):
    cid = fc.case_id(curve, chroma, fr, alpha, matrix)
    planes = fc.ycc_planes(10, chroma, alpha)
    d = fc.ycc_desc(planes, 10, curve, chroma, fr, alpha, matrix)

    def after(pad, obits, parts):
        note = ""
        if curve in fc.ONE_VALUE_CURVES:                       # D: the same bits as the 4:4:4 aligned open on every argument they share
            shared, distinct = _agrees_with_value_map(gpu, (curve, fr, matrix), _bits32(parts.V32), obits.reshape(-1), (cid, f"pad={pad}"))
            note = f"; same bits as the 4:4:4 aligned open on {shared} samples, {distinct} distinct arguments"
        if curve == "hlg":
            note += _hlg_low_piece((cid, f"pad={pad}"), obits, parts)
        if curve == "hlg-ootf-g1":                             # powf(luma, 0) = 1: a black pixel is 0, not 0 * inf
            black = np.all(parts.V32 == 0, axis=-1)
            assert np.all(obits[black] == 0), (cid, "a black pixel is not +0")
            assert black.any() == (alpha == fc.PREMUL), cid
            note = f"; {int(black.sum())} black pixels, all +0"
        return note

    _open_and_judge(gpu, cid, d, planes, (0, ODD_PAD), "A_ycbcr_10bit", after)


@pytest.mark.parametrize("curve", ["hlg", "hlg-ootf"])
def test_ycbcr_open_around_the_hlg_select(gpu, curve):
    """Every (Y, alpha) pair, premultiplied, under the (Cb, Cr) of fc.HLG_SELECT: it holds pixels whose unpremultiplied G is one and two
    floats below 0.5, the low side of `value > 0.5f`; the premultiplied 4:4:4 square above holds the one sample just above it
    (tests/test_whole_float_opens.py counts both; no 10-bit input found gives 0.5 itself)."""
    planes = fc.select_planes()
    d = fc.ycc_desc(planes, 10, curve, "444", 1, fc.PREMUL)

    def after(pad, obits, parts):
        if curve != "hlg":
            return ""
        shared, distinct = _agrees_with_value_map(gpu, (curve, 1, "bt2020ncl"), _bits32(parts.V32), obits.reshape(-1), (curve, f"pad={pad}"))
        return f"; same bits as the 4:4:4 aligned open on {shared} samples, {distinct} distinct arguments" + _hlg_low_piece((curve, "select", f"pad={pad}"), obits, parts)

    _open_and_judge(gpu, f"{curve}-select-444-full-premul", d, planes, (0, ODD_PAD), "A_ycbcr_10bit", after)


# ---- B: YCbCr at 12 bit, in row bands ---------------------------------------------------------------------------------------------------------
CASES_B = fc.cases_b()
_SCALAR_TABLE = {}                # "bits": the opaque planar-RGB open of every 12-bit code: the scalar PQ through the table build
_SCALAR_CODES = {}                # first chroma row of a 4:4:4 band -> the codes i whose value i / 4095 the band's packed PQ was given


def _scalar_table(gpu):
    if "bits" not in _SCALAR_TABLE:
        n = 1 << fc.BITS_B
        codes = np.arange(n, dtype=np.uint16).reshape(n // 256, 256)
        planes = {0: codes, 1: codes.copy(), 2: codes.copy()}
        d = pkg.ReadDesc(width=256, height=n // 256, colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=fc.BITS_B, depth=32,
                         alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_RGB_GBR, color_primaries=pkg.PRIMARIES_BT2020, **fc.CURVES[fc.CURVE_B])
        got = harness.gpu_read(gpu, d, planes).view(np.uint32).reshape(n, 3)
        _assert_form(gpu, d, 0)
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 2])
        _SCALAR_TABLE["bits"] = got[:, 0].copy()
    return _SCALAR_TABLE["bits"]


def _packed_equals_scalar(gpu, r, vbits, obits):
    """Wherever an argument of the packed PQ is the code value i / 4095 (0 < i < 4095) exactly, its bits are those of code i's table entry."""
    n = 1 << fc.BITS_B
    cv = (np.arange(n, dtype=np.float32) / np.float32(n - 1)).view(np.uint32)          # ascending: non-negative floats order as their bits
    i = np.minimum(np.searchsorted(cv, vbits), n - 1)
    hit = (cv[i] == vbits) & (i > 0) & (i < n - 1)
    bad = hit & (_scalar_table(gpu)[i] != obits)
    assert not bad.any(), ("the packed PQ differs from the scalar one", r, int(bad.sum()), [(int(i[j]), hex(int(obits[j]))) for j in np.flatnonzero(bad)[:4]])
    _SCALAR_CODES[r] = np.unique(i[hit])
    return int(hit.sum()), int(_SCALAR_CODES[r].size)


def test_bands_cover_every_chroma_row_once():
    n = 1 << fc.BITS_B
    for family in fc.FAMILIES_B:
        seen = np.zeros(n, dtype=np.int64)
        for r, rows in fc.bands_b(family):
            seen[r:r + rows] += 1
            xs, ys = harness.chroma_shift(fc.CHROMA[fc.FAMILIES_B[family][0]])
            assert (rows << ys) * (n << xs) <= 1 << 22, (family, r)
        assert np.all(seen == 1), family


@pytest.mark.parametrize("family,r,rows", CASES_B, ids=[f"{f}-rows{r}" for f, r, _ in CASES_B])
def test_ycbcr_open_12bit_band(gpu, family, r, rows):
    chroma, fr, alpha, _ = fc.FAMILIES_B[family]
    planes = fc.ycc_planes(fc.BITS_B, chroma, alpha, band=(r, rows))
    d = fc.ycc_desc(planes, fc.BITS_B, fc.CURVE_B, chroma, fr, alpha)
    assert d.width * d.height <= 1 << 22

    def after(pad, obits, parts):
        if family != "444-full-opaque":
            return ""
        hits, codes = _packed_equals_scalar(gpu, r, _bits32(parts.V32), obits.reshape(-1))
        return f"; packed PQ = scalar PQ on {hits} samples whose argument is a code value, {codes} distinct codes"

    _open_and_judge(gpu, f"{fc.CURVE_B}-b12-{family}-rows{r}", d, planes, (0,), "B_ycbcr_12bit", after)


def test_packed_pq_equals_scalar_pq_on_at_least_1000_codes(gpu):
    """The distinct 12-bit codes on which the bands above compared the packed with the scalar PQ; a band that did not run (a selection
    of tests) is opened here, without its bars."""
    for r, rows in fc.bands_b("444-full-opaque"):
        if r not in _SCALAR_CODES:
            planes = fc.ycc_planes(fc.BITS_B, "444", fc.NONE, band=(r, rows))
            d = fc.ycc_desc(planes, fc.BITS_B, fc.CURVE_B, "444", 1, fc.NONE)
            got = harness.gpu_read(gpu, d, planes)
            _assert_form(gpu, d, 0)
            _packed_equals_scalar(gpu, r, _bits32(rt.ycc_v32(d, planes)), np.ascontiguousarray(got).view(np.uint32).reshape(-1))
    codes = np.unique(np.concatenate(list(_SCALAR_CODES.values())))
    _record("D_one_value", f"packed PQ (YCbCr 4:4:4 12 bit, every band) against scalar PQ (planar-RGB table): {codes.size} distinct codes compared, all bit-equal")
    assert codes.size >= 1000, codes.size


# ---- C: planar RGB and gray with alpha, every (code, alpha) pair ---------------------------------------------------------------------------------
def _same_bits_as_the_opaque_pixel(cid, d, planes, curve):
    """A table value is a function of the code alone: the colour of pixel (c, a) has the bits the same open gives code q(c, a) in an
    opaque pixel (q = the restated integer unpremultiply; alpha 0 -> 0, alpha max -> identity; straight alpha: q = c)."""
    n = 1 << d.bit_depth
    opaque = np.flatnonzero(planes[3][:, 0] == n - 1)
    assert opaque.size == 1 and np.all(planes[3][opaque[0]] == n - 1)

    def after(pad, obits, parts):
        if curve not in fc.ONE_VALUE_CURVES:
            return ""
        for ch, pl in enumerate((0,) if d.colorspace == pkg.COLORSPACE_MONOCHROME else (0, 1, 2)):
            by_code = np.zeros(n, dtype=np.uint32)
            by_code[planes[pl][opaque[0]]] = obits[opaque[0], :, ch]
            assert np.array_equal(np.sort(planes[pl][opaque[0]]), np.arange(n))
            want = by_code[parts.q[..., ch]]
            bad = want != obits[..., ch]
            assert not bad.any(), (cid, f"pad={pad}", f"channel {ch}", int(bad.sum()), "first (alpha row, col)", [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]])
        return "; every pixel has the bits of its code's opaque pixel" + (_hlg_low_piece((cid, f"pad={pad}"), obits, parts) if curve == "hlg" else "")
    return after


CASES_C10 = fc.cases_c10()


@pytest.mark.parametrize("cs,curve,alpha,fr", CASES_C10, ids=[f"{cs}-{curve}-{fc.ALPHA_NAME[a]}-{('limited', 'full')[fr]}" for cs, curve, a, fr in CASES_C10])
def test_planar_rgb_and_gray_open_10bit_every_code_alpha_pair(gpu, cs, curve, alpha, fr):
    cid = f"{cs}-{curve}-{fc.ALPHA_NAME[alpha]}-{('limited', 'full')[fr]}"
    planes = fc.pair_planes(10, cs)
    d = fc.pair_desc(planes, 10, cs, curve, alpha, fr)
    _open_and_judge(gpu, cid, d, planes, (0, ODD_PAD), "C_pairs", _same_bits_as_the_opaque_pixel(cid, d, planes, curve))


BANDS_C12 = [(r, fc.BAND_C12) for r in range(0, 4096, fc.BAND_C12)]


@pytest.mark.parametrize("r,rows", BANDS_C12, ids=[f"rows{r}" for r, _ in BANDS_C12])
def test_planar_rgb_open_12bit_premultiplied_band(gpu, r, rows):
    cid = f"rgb-pq80-b12-premul-rows{r}"
    planes = fc.pair_planes(12, "rgb", band=(r, rows))
    d = fc.pair_desc(planes, 12, "rgb", "pq80", fc.PREMUL)
    _open_and_judge(gpu, cid, d, planes, (0,), "C_pairs", _same_bits_as_the_opaque_pixel(cid, d, planes, "pq80"))


def test_one_argument_one_result_in_the_reference_opens(gpu):
    """D: the maps every case of A was compared with are single-valued (asserted where they are built); builds those a selection of
    tests left out, and records their sizes."""
    for curve in fc.ONE_VALUE_CURVES:
        for fr in (1, 0):
            mv, _ = _value_map(gpu, curve, fr, "bt2020ncl")
            _record("D_one_value", f"{curve} {('limited', 'full')[fr]} range: 4:4:4 aligned open, {3 << 20} samples, {mv.size} distinct float32 arguments, one result each")
