"""The GPU's stage program (write_px<..., icc = 8>, csrc/icc_pipeline32.h compiled for the device) held to its host form stage by stage.

The instrument: h = avifgpu_icc_pipeline32_eval of the source (the host floats of the program, tests/test_icc32_programs.py holds those
to a numpy restatement and to lcms2); one GPU save of the source WITH the program, one GPU save WITHOUT ICC of the rows h under the same
descriptor.  Both saves run the same transfer curve and stage B on the device, so a code differs only where the device's program
produced another float than the host's.

  tier A  pow-free programs (table curves, CLUTs with seeded 16-bit nodes -- the int32 sum wraps --, matrices, Lab -> XYZ, compositions,
          every save form): every sample equal, np.array_equal.  A 12-bit code shows 12 bits of a 16-bit output word; behind a window
          stage (gain 16, bias -j; icc32_programs.MAGNIFIER_BIASES) every word has codes of its own, so a rounding constant off by one
          shows.
  tier B  one stage with pow() (or the cube root) in front of the tail, Clip at 12 bit: every code in {code(h-), code(h), code(h+)} for
          the float32 neighbours of h, and at most 1 sample in 10^4 on a neighbour (the two pow()s agree to a few double ulps; float32
          rounding boundaries lie 2^29 doubles apart).
  tier C  pow() in front of a CLUT: equal on the determined pixels (the curve value and both its float neighbours give the same 16-bit
          word in all three channels: at least 95 % of the pixels, counted on the CPU too), |delta code| <= 1 on the rest.
  tier D  real lcms2 profiles (9- and 33-point grids, 1024-entry table curves, ramp and twisted nodes) through the check of
          tests/test_gpu_icc32_pipeline.py; the share equal to "host evaluation, then no-ICC save" is printed beside it, no bar on it.

Found by tier A and fixed: the device gave a NaN the word 0 where lcms2's _cmsQuickSaturateWord takes it from the NaN's low payload bits
(32767 for the default NaN), so a NaN in front of a table curve or a CLUT came out as another colour than on the host."""
import numpy as np
import pytest

import harness
import icc32_programs as ip
import test_gpu_icc32_pipeline as real
from test_gpu_icc32_pipeline import lcms  # noqa: F401  (the module's fixture: skips where lcms2 is absent)

pkg = harness.pkg
pytestmark = pytest.mark.gpu

W, H = 1024, 48
BT2020 = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
REF_CLIP12 = dict(planes=3, bit_depth=12, transfer=pkg.TRANSFER_CLIP, output=pkg.OUT_REFERENCE)
DEFAULT_TUNING = 1 | 2 | 4
TIER_A = ip.tier_a_programs()
TIER_B = ip.tier_b_programs()
REF_STREAM = "write_f32_ref_stream<"                        # the kernel form of a no-ICC 32-bit save to interleaved reference codes


def _desc(**kw):
    kw = dict(dict(width=W, height=H, depth=32, peak_nits=1000), **kw)
    return pkg.WriteDesc(**kw)


def _rows(d, x, seed=9):
    """The triples x as the R, G, B of a document of d's shape (alpha, where there is one, from the harness's generator)."""
    rows = harness.make_write_source(d, seed=seed, edge_values=False)
    rows.reshape(d.height * d.width, d.planes)[:, :3] = x[:d.height * d.width]
    return rows


def _host_rows(prog, d, rows):
    out = rows.copy()
    px = out.reshape(d.height * d.width, d.planes)
    px[:, :3] = ip.eval_host(prog, np.ascontiguousarray(px[:, :3]))
    return out


def _pair(gpu, prog, d, rows, lds, form=REF_STREAM, tuning=None, **kw):
    """(codes of the save with the program, codes of the no-ICC save of the host's floats), the kernels of both asserted."""
    try:
        if tuning is not None:
            gpu.lib.avifgpu_set_hot_variant(tuning)
        got = harness.gpu_write(gpu, d, rows, icc=prog, **kw)
        label = gpu.last_kernel()
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_TUNING)
    assert "icc=8" in label and (" lds" in label) == lds, label
    want = harness.gpu_write(gpu, d, _host_rows(prog, d, rows), **kw)
    label = gpu.last_kernel()
    assert form in label and "icc=" not in label, label
    return got, want


def _assert_equal(got, want, what):
    for pl in want:
        bad = got[pl] != want[pl]
        assert np.array_equal(got[pl], want[pl]), (what, pl, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[pl][bad][:5], want[pl][bad][:5])


# ---- tier A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIER_A))
def test_tier_a_pow_free_program_equals_its_host_form(gpu, name):
    spec, axes, lds, tuning = TIER_A[name]
    d = _desc(**REF_CLIP12)
    got, want = _pair(gpu, ip.stamp(ip.build(spec)), d, _rows(d, ip.make_inputs(axes, seed=3)), lds, tuning=tuning)
    _assert_equal(got, want, name)
    assert len(np.unique(want[0])) > (1000 if "nan" not in name and "matrix" not in name else 2), name    # the codes say something


@pytest.mark.parametrize("kind", ["tables", "clut"])
def test_tier_a_all_sixteen_bits_of_the_output_words(gpu, kind):
    """The table curves and the CLUT behind the window stage: one pair of saves per window."""
    name, axes = ip.MAGNIFIED[kind]
    d = _desc(**REF_CLIP12)
    rows = _rows(d, ip.make_inputs(axes, seed=3))
    for j in ip.MAGNIFIER_BIASES:
        prog = ip.stamp(ip.build(TIER_A[name][0][:-1] + [ip.magnifier(j), ip.TAIL]))
        got, want = _pair(gpu, prog, d, rows, True)
        _assert_equal(got, want, (kind, j))


FORMS = {
    "rgba straight, reference, PQ 12": dict(planes=4, alpha_state=pkg.ALPHA_STRAIGHT, bit_depth=12, transfer=pkg.TRANSFER_PQ, output=pkg.OUT_REFERENCE),
    "rgba premultiplied, reference, Clip 10": dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, bit_depth=10, transfer=pkg.TRANSFER_CLIP,
                                                   output=pkg.OUT_REFERENCE),
    "rgb 4:4:4 PQ 10": dict(planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020),
    "rgb 4:4:4 Clip 12": dict(planes=3, bit_depth=12, transfer=pkg.TRANSFER_CLIP, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020),
    "rgb 4:2:2 SMPTE 428 12": dict(planes=3, bit_depth=12, transfer=pkg.TRANSFER_SMPTE428, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, **BT2020),
    "rgb 4:2:2 PQ 10": dict(planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, **BT2020),
    "rgb 4:2:0 Clip 10": dict(planes=3, bit_depth=10, transfer=pkg.TRANSFER_CLIP, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT2020),
    "rgb 4:2:0 PQ 12": dict(planes=3, bit_depth=12, transfer=pkg.TRANSFER_PQ, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT2020),
    "rgba straight 4:4:4 SMPTE 428 10": dict(planes=4, alpha_state=pkg.ALPHA_STRAIGHT, bit_depth=10, transfer=pkg.TRANSFER_SMPTE428,
                                            output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020),
    "rgba premultiplied 4:2:0 PQ 12": dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, bit_depth=12, transfer=pkg.TRANSFER_PQ,
                                          output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT2020),
    "rgba premultiplied 4:2:2 Clip 12": dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, bit_depth=12, transfer=pkg.TRANSFER_CLIP,
                                            output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, **BT2020),
}


# the kernel form the no-ICC save of each form takes (every streaming float form is held to the generic kernel's bits by
# tests/test_gpu_kernel_equivalence.py and tests/test_zz_gpu_whole_float_domain.py)
FORM_KERNEL = {
    "rgba straight, reference, PQ 12": "write_f32_ref_stream<transfer=0,planes=4>",
    "rgba premultiplied, reference, Clip 10": "write_f32_ref_stream<transfer=3,planes=4>",
    "rgb 4:4:4 PQ 10": "write_rgb32_ycbcr444_hot<transfer=0,",
    "rgb 4:4:4 Clip 12": "write_rgb32_ycbcr444_hot<transfer=3,",
    "rgb 4:2:2 SMPTE 428 12": "write_rgb32_ycbcr_sub_hot<transfer=2,xs=1,ys=0>",
    "rgb 4:2:2 PQ 10": "write_rgb32_ycbcr_sub_hot<transfer=0,xs=1,ys=0>",
    "rgb 4:2:0 Clip 10": "write_rgb32_ycbcr_sub_hot<transfer=3,xs=1,ys=1>",
    "rgb 4:2:0 PQ 12": "write_rgb32_ycbcr_sub_hot<transfer=0,xs=1,ys=1>",
    "rgba straight 4:4:4 SMPTE 428 10": "write_rgba32_ycbcra444_hot<transfer=2>",
    "rgba premultiplied 4:2:0 PQ 12": "write_rgba32_ycbcra_sub_hot<transfer=0,xs=1,ys=1,",
    "rgba premultiplied 4:2:2 Clip 12": "write_rgba32_ycbcra_sub_hot<transfer=3,xs=1,ys=0,",
}


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("form", list(FORMS))
def test_tier_a_every_save_form_of_the_composition(gpu, form, mem):
    d = _desc(**FORMS[form])
    prog = ip.stamp(ip.build(ip.composition()))
    rows = _rows(d, ip.make_inputs((256, 1024, 33), seed=3))
    got, want = _pair(gpu, prog, d, rows, True, form=FORM_KERNEL[form], mem=mem)
    _assert_equal(got, want, (form, mem))
    if d.planes == 4:                                       # alpha is copied: the save without ICC of the SOURCE has the same alpha
        plain = harness.gpu_write(gpu, d, rows, mem=mem)
        a = (lambda p: p[0].reshape(H, W, 4)[..., 3]) if d.output == pkg.OUT_REFERENCE else (lambda p: p[3])
        assert np.array_equal(a(got), a(plain)), form


@pytest.mark.parametrize("form", ["rgb 4:2:0 PQ 12", "rgba premultiplied 4:2:2 Clip 12", "rgba straight, reference, PQ 12"])
def test_tier_a_row_window_and_padded_rows(gpu, form):
    """A call on rows [16, 40) of the image, padded destination rows, and (host pointers) padded source rows."""
    d = _desc(**FORMS[form])
    prog = ip.stamp(ip.build(ip.composition()))
    rows = _rows(d, ip.make_inputs((256, 1024, 33), seed=3))
    whole, _ = _pair(gpu, prog, d, rows, True, form=FORM_KERNEL[form])
    got, want = _pair(gpu, prog, d, rows, True, form=FORM_KERNEL[form], row0=16, nrows=24, stride_pad=8)
    _assert_equal(got, want, form)
    ys = 1 if d.output == pkg.OUT_YCBCR and d.chroma == pkg.CHROMA_420 else 0
    for pl in got:                                          # the window is the same rows of the whole save
        sh = ys if pl in (1, 2) else 0
        assert np.array_equal(got[pl], whole[pl][16 >> sh:40 >> sh]), (form, pl)
    padded = np.full((H, rows.shape[1] + 20), np.float32(np.nan))
    padded[:, :rows.shape[1]] = rows
    got, want = _pair(gpu, prog, d, padded[:, :rows.shape[1]], True, form=FORM_KERNEL[form], mem="host", stride_pad=24)
    _assert_equal(got, want, (form, "padded source"))
    _assert_equal(got, whole, (form, "padded source against the plain call"))


def test_tier_a_two_programs_in_the_same_struct_back_to_back(gpu):
    d = _desc(**REF_CLIP12)
    rows = _rows(d, ip.make_inputs((9, 9, 9), seed=3))
    prog = pkg.IccPipeline32()
    outs = []
    for spec in (TIER_A["clut 9x9x9"][0], ip.composition(), TIER_A["clut 21^3"][0], TIER_A["clut 9x9x9"][0]):
        ip.stamp(ip.fill_into(prog, spec))
        got, want = _pair(gpu, prog, d, rows, 0 < ip.build(spec).word_count * 2 <= 48 * 1024)
        _assert_equal(got, want, len(outs))
        outs.append(got[0])
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2]) and np.array_equal(outs[0], outs[3])


# ---- tier B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIER_B))
def test_tier_b_pow_stage_lands_on_the_host_float_or_a_neighbour(gpu, name):
    d = _desc(**REF_CLIP12)
    prog = ip.stamp(ip.build(TIER_B[name]))
    rows = _rows(d, ip.make_inputs(seed=4))
    got, want = _pair(gpu, prog, d, rows, False)
    h = _host_rows(prog, d, rows)
    lo, hi = ip.neighbours(h)
    c_lo, c_hi = harness.gpu_write(gpu, d, lo)[0], harness.gpu_write(gpu, d, hi)[0]
    g, c = got[0], want[0]
    off = g != c
    print("tier B %-28s: %d of %d samples on a neighbour's code" % (name, int(off.sum()), g.size))
    assert ((g == c) | (g == c_lo) | (g == c_hi)).all(), (name, int((off & (g != c_lo) & (g != c_hi)).sum()))
    assert off.sum() * 10_000 <= g.size, (name, int(off.sum()))


# ---- tier C ---------------------------------------------------------------------------------------------------------------------------
def test_tier_c_pow_in_front_of_a_clut(gpu):
    spec, curves = ip.tier_c_program()
    d = _desc(**REF_CLIP12)
    x = ip.make_inputs((9, 9, 9), seed=5)
    h1 = ip.eval_host(ip.build(curves), x)
    lo, hi = ip.neighbours(h1)
    det = ((ip.sat_word(lo) == ip.sat_word(h1)) & (ip.sat_word(hi) == ip.sat_word(h1))).all(axis=1)
    assert det.mean() >= 0.95
    got, want = _pair(gpu, ip.stamp(ip.build(spec)), d, _rows(d, x), True)
    g, c = got[0].reshape(-1, 3).astype(np.int64), want[0].reshape(-1, 3).astype(np.int64)
    off = (g != c).any(axis=1)
    print("tier C: determined %.4f of %d pixels; %d of the %d others differ" % (det.mean(), len(x), int(off[~det].sum()), int((~det).sum())))
    assert np.array_equal(g[det], c[det]), int(off[det].sum())
    assert np.abs(g - c).max() <= 1


# ---- tier D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [9, 33])
@pytest.mark.parametrize("twisted", [None, 21])
def test_tier_d_real_profiles_with_table_curves(gpu, lcms, grid, twisted):  # noqa: F811
    icc = ip.lut_profile(lcms, "A2B0", grid, table_curves=1024, twisted=twisted)
    rc, prog = pkg.icc_pipeline32_from_profile(icc, pkg.ICC_TARGET_REC2020_LINEAR, False)
    assert rc == 0, pkg.load().avifgpu_last_error()
    d = pkg.WriteDesc(width=517, height=22, depth=32, planes=3, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020)
    src = real._source(d, 31)
    got = real._gpu(gpu, d, src, prog, "device")
    label = gpu.last_kernel()
    assert "icc=8" in label and (" lds" in label) == (prog.word_count * 2 <= 48 * 1024), label
    real._check(harness.compare_write(d, real._reference(lcms, icc, d, src), got), "grid %d twisted %s" % (grid, twisted))
    st = harness.compare_write(d, harness.gpu_write(gpu, d, _host_rows(prog, d, src)), got)
    print("tier D grid %d twisted %s: %.5f equal to host evaluation + no-ICC save, max %d" % (grid, twisted, st["exact_frac"], st["max_abs"]))
