"""32-bit documents behind a LUT-based (A2B) profile (include/avifgpu.h, avifgpu_icc_pipeline32): the adapter captures lcms2's float
stage program (integration/LcmsTableBridge.cpp), the library restates it and proves it against the caller's own transform.

Checker: the real Little CMS 2 driven like the reference (oracle/icc_oracle.c: ColorProfileConversion's float transforms to linear Rec.2020
and to sRGB).  Bar: bit-identical floats.  Tests that need lcms2 skip where the bridge or the ICC oracle is not built."""
import ctypes
import os

import numpy as np
import pytest

import harness

pkg = harness.pkg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICC_LIB = os.path.join(ROOT, "oracle", "liboracle_icc.so")
TARGETS = [pkg.ICC_TARGET_REC2020_LINEAR, pkg.ICC_TARGET_SRGB_FLOAT]


@pytest.fixture(scope="module")
def lcms():
    if not os.path.exists(ICC_LIB) or pkg.lcms_bridge() is None:
        pytest.skip("oracle/liboracle_icc.so or libavifgpu_lcms_bridge.so not built (lcms2 absent)")
    L = ctypes.CDLL(ICC_LIB)
    L.oracle_icc_make_a2b_profile.restype = ctypes.c_int32
    L.oracle_icc_make_a2b_profile.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]
    for name in ("oracle_icc_convert_rows_to_rec2020", "oracle_icc_convert_rows_to_srgb_float"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    return L


def _a2b(L, variant):
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.oracle_icc_make_a2b_profile(variant, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


def _lcms2_convert(L, icc, target, rgb):
    """lcms2's own float transform of interleaved RGB triples (the reference's ConvertRow on one row)."""
    out = np.ascontiguousarray(rgb, dtype=np.float32).copy()
    fn = L.oracle_icc_convert_rows_to_rec2020 if target == pkg.ICC_TARGET_REC2020_LINEAR else L.oracle_icc_convert_rows_to_srgb_float
    n = out.shape[0]
    assert fn(icc, len(icc), 0, out.ctypes.data, n, 1, n * 12) == 0
    return out


def _eval(prog, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.empty_like(rgb)
    assert pkg.load().avifgpu_icc_pipeline32_eval(ctypes.byref(prog), rgb.ctypes.data, out.ctypes.data, rgb.shape[0]) == 0
    return out


def _program(icc, target, alpha=False):
    rc, prog = pkg.icc_pipeline32_from_profile(icc, target, alpha)
    assert rc == 0, pkg.load().avifgpu_last_error()
    return prog


def _prove(L, icc, target, prog):
    """avifgpu_icc_pipeline32_prove with the lcms2 transform of `target` as the caller's float_fn."""
    def run(user, pin, pout, n):
        a = np.ctypeslib.as_array(pin, shape=(n, 3)).copy()
        np.ctypeslib.as_array(pout, shape=(n, 3))[:] = _lcms2_convert(L, icc, target, a)
    cb = pkg.TransformF32Fn(run)
    rc = pkg.load().avifgpu_icc_pipeline32_prove(ctypes.byref(prog), ctypes.cast(cb, ctypes.c_void_p), None)
    return rc, pkg.load().avifgpu_last_error().decode()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("alpha", [False, True])
def test_bridge_captures_and_proves_the_float_program(lcms, variant, target, alpha):
    prog = _program(_a2b(lcms, variant), target, alpha)
    assert prog.proof != 0 and prog.target == target
    kinds = [prog.stages[i].kind for i in range(prog.stage_count)]
    # A-curves, the profile's 17^3 CLUT, B-curves, Lab -> XYZ, the PCS / BPC matrix, the inverse destination matrix, destination curves
    assert kinds.count(pkg.ICC_STAGE_CLUT16) == 1 and pkg.ICC_STAGE_LAB_TO_XYZ in kinds and kinds[-1] == pkg.ICC_STAGE_CURVES
    clut = prog.stages[kinds.index(pkg.ICC_STAGE_CLUT16)]
    assert list(clut.entries) == [17, 17, 17]


def _probe_floats(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.25, 4.0, size=(n, 3)).astype(np.float32)
    a[: n // 4] = rng.uniform(0.0, 1.0, size=(n // 4, 3)).astype(np.float32)             # the SDR cube, densely
    w = rng.integers(0, 65536, size=(n // 8, 3))
    a[n // 4: n // 4 + n // 8] = (w / 65535.0).astype(np.float32)                           # on 16-bit words
    a[-4096:] = np.repeat(np.linspace(-0.5, 8.0, 4096, dtype=np.float32)[:, None], 3, axis=1)   # neutrals, below 0 and far above 1
    return a


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("target", TARGETS)
def test_restatement_is_bit_identical_to_lcms2(lcms, variant, target):
    """avifgpu_icc_pipeline32_eval against lcms2's own cmsDoTransform on ~10^6 floats, values above 1 and below 0 included."""
    icc = _a2b(lcms, variant)
    prog = _program(icc, target)
    rgb = _probe_floats(340_000, 100 + variant + target)
    want = _lcms2_convert(lcms, icc, target, rgb)
    got = _eval(prog, rgb)
    same = want.view(np.uint32) == got.view(np.uint32)
    assert same.all(), (int((~same).sum()), rgb[~same.all(axis=1)][:3], got[~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])


@pytest.mark.parametrize("target", TARGETS)
def test_proof_refuses_a_perturbed_program(lcms, target):
    icc = _a2b(lcms, 1)
    prog = _program(icc, target)
    rc, msg = _prove(lcms, icc, target, prog)
    assert rc == 0 and prog.proof != 0, msg                 # the callback form of the caller's transform proves the untouched program
    kinds = [prog.stages[i].kind for i in range(prog.stage_count)]

    bad = pkg.IccPipeline32.from_buffer_copy(prog)          # one matrix entry, perturbed by one part in 10^6
    m = kinds.index(pkg.ICC_STAGE_MATRIX)
    bad.stages[m].matrix[4] *= 1.000001
    rc, msg = _prove(lcms, icc, target, bad)
    assert rc == pkg.formatCannotRead and "differ" in msg and bad.proof == 0

    bad = pkg.IccPipeline32.from_buffer_copy(prog)          # one CLUT word, low bit flipped
    c = prog.stages[kinds.index(pkg.ICC_STAGE_CLUT16)]
    bad.words[c.offset[0] + 3 * (8 * 17 * 17 + 8 * 17 + 8) + 1] ^= 1
    rc, msg = _prove(lcms, icc, target, bad)
    assert rc == pkg.formatCannotRead and "differ" in msg

    bad = pkg.IccPipeline32.from_buffer_copy(prog)          # the other target's tag on this target's program
    bad.target = pkg.ICC_TARGET_SRGB_FLOAT if target == pkg.ICC_TARGET_REC2020_LINEAR else pkg.ICC_TARGET_REC2020_LINEAR
    rc, msg = _prove(lcms, icc, target, bad)
    assert rc == pkg.formatCannotRead and "target" in msg


def test_write_refuses_an_unstamped_or_altered_program(lcms):
    """avifgpu_write_rows_icc_pipeline32 checks the stamp before anything else (no device needed to see it)."""
    lib = pkg.load()
    prog = _program(_a2b(lcms, 0), pkg.ICC_TARGET_REC2020_LINEAR)
    d = pkg.WriteDesc(width=8, height=2, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      output=pkg.OUT_REFERENCE)
    src = np.zeros((2, 24), np.float32)
    dst = np.zeros((2, 48), np.uint8)
    planes = pkg.planes4([dst.ctypes.data])
    strides = pkg.strides4([48])
    for alter in ("unstamped", "word", "stage"):
        bad = pkg.IccPipeline32.from_buffer_copy(prog)
        if alter == "unstamped":
            bad.proof = 0
        elif alter == "word":
            bad.words[100] ^= 1
        else:
            bad.stages[0].params[0][0] = 1.01
        rc = lib.avifgpu_write_rows_icc_pipeline32(ctypes.byref(d), ctypes.byref(bad), 0, 2, src.ctypes.data, 96, ctypes.byref(planes),
                                                   ctypes.byref(strides), pkg.MEM_HOST, None)
        assert rc == pkg.formatBadParameters and b"not proven" in lib.avifgpu_last_error(), alter


def test_eval_rejects_a_malformed_program():
    lib = pkg.load()
    prog = pkg.IccPipeline32()
    x = np.zeros((1, 3), np.float32)
    assert lib.avifgpu_icc_pipeline32_eval(ctypes.byref(prog), x.ctypes.data, x.ctypes.data, 1) == pkg.formatBadParameters
    prog.stage_count, prog.stages[0].kind = 1, pkg.ICC_STAGE_CLUT16
    prog.stages[0].entries[:] = [34, 2, 2]                  # grids above 33 have no form
    prog.word_count = 3 * 34 * 4
    assert lib.avifgpu_icc_pipeline32_eval(ctypes.byref(prog), x.ctypes.data, x.ctypes.data, 1) == pkg.formatBadParameters
    assert b"33" in lib.avifgpu_last_error()


# ---- profiles built with lcms2 inside the test -------------------------------------------------------------------------------------
from icc32_programs import lut_profile as _lut_profile  # noqa: E402  (shared with the stage-program tests)


@pytest.mark.parametrize("target", TARGETS)
def test_table_curves_and_a_9_point_grid_are_taken_and_bit_identical(lcms, target):
    """16-bit TABLE curves in front of the CLUT (LinLerp1D on the word of the float) and another grid size."""
    icc = _lut_profile(lcms, "A2B0", 9, table_curves=1024)
    prog = _program(icc, target)
    first = prog.stages[0]
    assert first.kind == pkg.ICC_STAGE_CURVES and list(first.curve_type) == [0, 0, 0] and list(first.entries) == [1024] * 3
    rgb = _probe_floats(60_000, 7)
    want, got = _lcms2_convert(lcms, icc, target, rgb), _eval(prog, rgb)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("what", ["float CLUT (D2B0)", "16-bit CLUT with a 35-point grid"])
def test_refused_constructs_keep_lcms2(lcms, what):
    icc = _lut_profile(lcms, "D2B0", 5, float_clut=True) if what.startswith("float") else _lut_profile(lcms, "A2B0", 35)
    for target in TARGETS:
        rc, prog = pkg.icc_pipeline32_from_profile(icc, target, False)
        assert rc == pkg.formatCannotRead, (what, target, rc)
        assert prog.proof == 0
