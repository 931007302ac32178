"""The host evaluation of avifgpu_icc_pipeline32 (avifgpu_icc_pipeline32_eval: csrc/icc_pipeline32.h compiled for the host) held to a
plain numpy restatement of every stage kind (tests/icc32_programs.py) on every program family the GPU file
(tests/test_zzzz_gpu_icc32_programs.py) runs, to lcms2 itself where it is present, and the COUNTS of what the shared inputs are claimed
to hold: word neighbourhoods, tied fractions, non-finite values, the share of determined pixels, the magnifier windows.

Bars: programs of integer and pow-free float stages bit-equal; programs with pow() or a cube root within one float32 step of the
restatement (numpy's pow is not the C library's); lcms2 bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import harness
import icc32_programs as ip

pkg = harness.pkg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICC_LIB = os.path.join(ROOT, "oracle", "liboracle_icc.so")

TIER_A = ip.tier_a_programs()
TIER_B = ip.tier_b_programs()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _steps(a, b):
    """Distance in float32 steps (monotone integer keys; +0 and -0 one step apart)."""
    def key(x):
        u = _bits(x).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7fffffff) - 1, u)
    return np.abs(key(a) - key(b))


# ---- the restatement against the library's host form --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIER_A))
def test_pow_free_programs_are_bit_equal_to_the_restatement(name):
    spec, axes, _, _ = TIER_A[name]
    x = ip.make_inputs(axes, seed=3)
    got, want = ip.eval_host(ip.build(spec), x), ip.eval_numpy(spec, x)
    same = (_bits(got) == _bits(want)).all(axis=1)
    assert same.all(), (name, int((~same).sum()), x[~same][:3], got[~same][:3], want[~same][:3])


@pytest.mark.parametrize("kind", ["tables", "clut"])
def test_magnified_programs_are_bit_equal_to_the_restatement(kind):
    name, axes = ip.MAGNIFIED[kind]
    x = ip.make_inputs(axes, seed=3)
    for j in (0, 7, 15):
        spec = TIER_A[name][0][:-1] + [ip.magnifier(j), ip.TAIL]
        assert np.array_equal(_bits(ip.eval_host(ip.build(spec), x)), _bits(ip.eval_numpy(spec, x))), (kind, j)


@pytest.mark.parametrize("name", list(TIER_B))
def test_programs_with_pow_are_within_one_float_step_of_the_restatement(name):
    spec = TIER_B[name]
    x = ip.make_inputs(seed=4)
    got, want = ip.eval_host(ip.build(spec), x), ip.eval_numpy(spec, x)
    far = _steps(got, want) > 1
    assert not far.any(), (name, int(far.sum()), x[far.any(axis=1)][:3], got[far.any(axis=1)][:3], want[far.any(axis=1)][:3])
    assert not np.isnan(got).any()                          # the tail's segment turns every NaN into -1e22


def test_tier_c_program_is_within_one_word_step_of_the_restatement_and_mostly_determined():
    """Parametric curves in front of a CLUT: a curve value one float step off may take the next word, so the whole program is held to
    the restatement on the DETERMINED pixels only -- and those are at least 95 % of what is drawn (the GPU file's condition)."""
    spec, curves = ip.tier_c_program()
    x = ip.make_inputs((9, 9, 9), seed=5)
    h1 = ip.eval_host(ip.build(curves), x)
    lo, hi = ip.neighbours(h1)
    det = ((ip.sat_word(lo) == ip.sat_word(h1)) & (ip.sat_word(hi) == ip.sat_word(h1))).all(axis=1)
    print("tier C: determined %.4f of %d pixels" % (det.mean(), len(x)))
    assert det.mean() >= 0.95
    got, want = ip.eval_host(ip.build(spec), x), ip.eval_numpy(spec, x)
    assert np.array_equal(_bits(got[det]), _bits(want[det]))


def test_every_program_is_stamped_by_the_library():
    for spec in [v[0] for v in TIER_A.values()] + list(TIER_B.values()) + [ip.tier_c_program()[0]]:
        prog = ip.stamp(ip.build(spec))
        assert prog.proof != 0
    bad = ip.build([("matrix", ip.M_PLAIN, None)])          # no destination curves: no stamp
    cb = pkg.TransformF32Fn(lambda user, pin, pout, n: None)
    assert pkg.load().avifgpu_icc_pipeline32_prove(ctypes.byref(bad), ctypes.cast(cb, ctypes.c_void_p), None) == pkg.formatCannotRead


def test_word_sizes_of_the_lds_boundary_programs():
    fit = ip.build(TIER_A["clut 20^3 + tables = 49152 bytes"][0])
    over = ip.build(TIER_A["clut 20^3 + tables = 49154 bytes"][0])
    assert fit.word_count * 2 == 48 * 1024 and over.word_count == fit.word_count + 1
    for name, (spec, _, lds, tuning) in TIER_A.items():
        fits = 0 < ip.build(spec).word_count * 2 <= 48 * 1024
        assert lds == (fits and tuning is None), name
        for st in spec:                                     # every CLUT sits at a non-zero offset[0], tables at odd and even ones
            if st[0] == "clut" and "20^3" not in name:
                assert st[2] > 0, name
    offs = [ip.build(TIER_A[n][0]).stages[0].offset[c] & 1 for n in TIER_A if n.startswith("tables") for c in range(3)]
    assert 0 in offs and 1 in offs


# ---- what the inputs are claimed to hold --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axes", [(17, 17, 17), (2, 33, 3), (33, 2, 17), (2, 3, 255), (256, 1024, 4096), (190, 190, 190), (33, 33, 33)])
def test_inputs_hold_what_they_claim(axes):
    x = ip.make_inputs(axes, seed=3)
    assert x.shape == (1024 * 48, 3)
    w = np.stack([ip.sat_word(x[:, c]) for c in range(3)], axis=1)
    on_word = _bits(x) == _bits(ip.word_to_float(w))
    for k, n in enumerate(axes):
        have = set(w[on_word[:, k], k].tolist())
        nodes = ip.node_words(n)
        if n <= 256:
            assert set(nodes.tolist()) <= have, (k, n)      # every node word and node +- 1, exactly on the word
        else:
            i = np.arange(n, dtype=np.int64)                # at least 400 nodes with all three words, the end nodes among them
            c = (i * 65535 + (n - 1) // 2) // (n - 1)
            full = np.array([{int(np.clip(c[q] + e, 0, 65535)) for e in (-1, 0, 1)} <= have for q in range(n)])
            assert full.sum() >= 400 and full[[0, 1, n - 2, n - 1]].all(), (k, n, int(full.sum()))
        # the floats on either side of a word
        for side in (-np.inf, np.inf):
            near = _bits(x[:, k]) == _bits(np.nextafter(ip.word_to_float(w[:, k]), np.float32(side)))
            assert near.sum() >= 1000, (k, side)
    for mask in range(1, 8):                                # 0xffff (the zeroed step) in every subset of the channels, and only there
        hit = np.ones(len(w), bool)
        for k in range(3):
            hit &= (w[:, k] == 0xffff) == bool(mask >> k & 1)
        assert (hit & on_word.all(axis=1)).sum() >= 48, mask
    fr = np.stack([ip.fraction(n, w[:, k]) for k, n in enumerate(axes)], axis=1)
    inside = on_word.all(axis=1) & (fr > 0).all(axis=1)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        k = 3 - i - j
        if max(axes) <= 33:                                 # grid axes (tables interpolate one channel each: no ties to break)
            assert (inside & (fr[:, i] == fr[:, j]) & (fr[:, k] != fr[:, i])).sum() >= 300, (i, j)     # pairwise-tied fractions
        assert (inside & (w[:, i] == w[:, j]) & (w[:, k] != w[:, i])).sum() >= 500, (i, j)          # pairwise-tied values
    if min(axes) > 3:
        assert (inside & (fr[:, 0] == fr[:, 1]) & (fr[:, 1] == fr[:, 2])).sum() >= 300              # all three tied
    assert (on_word.all(axis=1) & (w[:, 0] == w[:, 1]) & (w[:, 1] == w[:, 2])).sum() >= 2000        # neutrals
    wide = (x >= -0.25) & (x <= 4.0) & ~on_word
    assert wide.all(axis=1).sum() >= 8000 and (x[wide] > 1.0).sum() > 5000 and (x[wide] < 0.0).sum() > 300
    # every special value in every channel, beside every other one
    for k in range(3):
        col = set(_bits(x[:, k]).tolist())
        assert set(_bits(ip.SPECIALS).tolist()) <= col, k
    for pat in ip.NAN_PATTERNS:
        assert (_bits(x) == pat).any(axis=1).sum() >= 3 * len(ip.SPECIALS) - 2
    assert len({int(ip.sat_word(np.array([p], np.uint32).view(np.float32))[0]) for p in ip.NAN_PATTERNS}) >= 6   # NaN words differ


def test_lab_inputs_cross_the_limit_in_every_channel():
    x = ip.make_inputs(seed=3)
    x = x[np.isfinite(x).all(axis=1)].astype(np.float64)
    y = (x[:, 0] * 100.0 + 16.0) / 116.0
    for t in (y + 0.002 * (x[:, 1] * 255.0 - 128.0), y, y - 0.005 * (x[:, 2] * 255.0 - 128.0)):
        assert (t <= 24.0 / 116.0).sum() > 1000 and (t > 24.0 / 116.0).sum() > 1000
    lim = (24.0 / 116.0) ** 3                               # XYZ_TO_LAB's limit
    x4 = ip.make_inputs(seed=4)
    x4 = x4[np.isfinite(x4).all(axis=1)].astype(np.float64)
    for k in range(3):
        t = x4[:, k] * ip.MAX_XYZ / ip.D50[k]
        assert (t <= lim).sum() > 1000 and (t > lim).sum() > 1000


def test_parametric_inputs_reach_every_branch():
    """The tier B inputs on either side of every breakpoint the curves have: negative and positive R, e <= 0, R below the breakpoint."""
    x = ip.make_inputs(seed=4)
    for k in range(3):
        r = x[:, k][np.isfinite(x[:, k])].astype(np.float64)
        assert (r < 0).sum() > 300 and ((r > 0) & (r < 0.04045)).sum() > 100 and (r > 1).sum() > 3000
        for bp in (0.04045, 0.05, 0.2, 0.5 / 0.9, 0.6, 0.3 / 0.9):
            assert (r < bp).sum() > 300 and (r >= bp).sum() > 300, bp


def test_magnifier_windows_separate_all_words():
    """Gain 16, bias -j under Clip at 12 bit -- counted with the CPU oracle's own Clip.  The sixteen windows j = 0..15 show 4096 words
    each on 4095 code steps, so one adjacent pair per window shares all its codes, and so do words 0 and 1 (both code 0 in window 0):
    15 pairs.  With the seventeen half-shifted windows (icc32_programs.MAGNIFIER_BIASES) the codes of a word tell it from every other."""
    words = np.arange(65536)
    f = ip.word_to_float(words)
    d = pkg.WriteDesc(width=4096, height=16, depth=32, planes=3, bit_depth=12, transfer=pkg.TRANSFER_CLIP, output=pkg.OUT_REFERENCE)
    sig = []
    for j in ip.MAGNIFIER_BIASES:
        v = ip.eval_host(ip.build([ip.magnifier(j), ip.TAIL]), np.stack([f, f, f], axis=1))[:, 0]
        rows = np.zeros((16, 4096 * 3), np.float32)
        rows.reshape(-1, 3)[:, 0] = v
        sig.append(harness.oracle_write(d, rows)[0].reshape(-1, 3)[:, 0].astype(np.int64))
    sig = np.stack(sig, axis=1)
    assert ip.MAGNIFIER_BIASES[:16] == [float(j) for j in range(16)]
    shared = int((sig[1:, :16] == sig[:-1, :16]).all(axis=1).sum())
    print("magnifier: %d of 65535 adjacent word pairs share all of the first sixteen codes" % shared)
    assert shared == 15
    assert len(np.unique(sig, axis=0)) == 65536


# ---- lcms2 itself, where it is present ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lcms():
    if not os.path.exists(ICC_LIB) or pkg.lcms_bridge() is None:
        pytest.skip("oracle/liboracle_icc.so or libavifgpu_lcms_bridge.so not built (lcms2 absent)")
    L = ctypes.CDLL(ICC_LIB)
    fn = L.oracle_icc_convert_rows_to_rec2020
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    return L


LCMS_PROFILES = [(2, 2, None), (9, 256, 11), (17, 4096, 12), (33, 256, 13), (9, 4096, None), (33, 2, 14), (17, 0, 15), (2, 4096, 16)]


@pytest.mark.parametrize("grid,table,twisted", LCMS_PROFILES)
def test_host_form_is_bit_identical_to_lcms2(lcms, grid, table, twisted):
    """Grids 2, 9, 17, 33, ramp and twisted nodes, table curves of 2, 256 and 4096 entries: cmsDoTransform's floats, bit for bit --
    NaN-free inputs (a NaN pixel in lcms2 depends on its formatter; the stage arithmetic on NaN is held by the restatement above)."""
    icc = ip.lut_profile(lcms, "A2B0", grid, table_curves=table, twisted=twisted)
    rc, prog = pkg.icc_pipeline32_from_profile(icc, pkg.ICC_TARGET_REC2020_LINEAR, False)
    assert rc == 0, pkg.load().avifgpu_last_error()
    clut = [prog.stages[i] for i in range(prog.stage_count) if prog.stages[i].kind == pkg.ICC_STAGE_CLUT16][0]
    assert list(clut.entries) == [grid] * 3
    if table:
        assert list(prog.stages[0].curve_type) == [0, 0, 0] and list(prog.stages[0].entries) == [table] * 3
    x = ip.make_inputs((table or grid,) * 3, seed=6)
    x = x[~np.isnan(x).any(axis=1)]
    want = x.copy()
    assert lcms.oracle_icc_convert_rows_to_rec2020(icc, len(icc), 0, want.ctypes.data, len(x), 1, len(x) * 12) == 0
    got = ip.eval_host(prog, x)
    same = (_bits(got) == _bits(want)).all(axis=1)
    assert same.all(), (int((~same).sum()), x[~same][:3], got[~same][:3], want[~same][:3])
