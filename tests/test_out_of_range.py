"""Out-of-range samples, CPU half: the rules oracle/avif_oracle.c:31-38 sets where the reference has undefined behaviour, and the
data tests/test_gpu_out_of_range.py feeds the kernels.

 * a 16-bit document sample above 32768 counts as 32768 (every save);
 * a planar-RGB plane sample above 2^bits - 1 is MASKED by a 16-bit open and CLAMPED by a 32-bit one; YCbCr and gray opens clamp.

Shown here, before any kernel is judged: the oracle follows the rules on the sources of harness.make_*_source_over_range, every code
stays inside [0, max], and the sources discriminate -- a kernel that masked instead of clamping (or the other way round), or that
evaluated the rescale without its input clamp, would produce different output from the same bytes."""
import numpy as np
import pytest

import cases
import harness
import oracle_binding
import test_gpu_kernel_equivalence as equivalence
from test_icc16 import PROFILES, _a2b_profile, _profile, lcms          # noqa: F401  (lcms: the module-scoped fixture)

pkg = harness.pkg

WRITE16 = [(cid, kw) for cid, kw in cases.write_cases() if kw["depth"] == 16]
HOT16 = [(f"{k}-{i}", kw) for i, (k, kw) in enumerate(equivalence.CASES) if kw["depth"] == 16]
READ_10_12 = [(cid, kw) for cid, kw in cases.read_cases() if kw["bit_depth"] in (10, 12)]


def lut16(bits):
    """The reference's 16 -> bits table (WriteHeifImage.cpp:114-166) from the oracle, extended by the rule: index min(i, 32768)."""
    L = oracle_binding.load()
    if bits == 8:
        t = np.zeros(32769, dtype=np.uint8)
        L.oracle_build_lut_16_to_8(t.ctypes.data)
    else:
        t = np.zeros(32769, dtype=np.uint16)
        L.oracle_build_lut_16_to_n(bits, t.ctypes.data)
    return t.astype(np.uint16)[np.minimum(np.arange(65536), 32768)]


def unclamped_codes(i, bits):
    """What the kernels' rescale expressions give WITHOUT their input clamp: rescale16_to_8 stored as a byte, and
    exact_rescale16_pair's one multiply stored as a 16-bit word (device_math.h), IEEE single operations one at a time."""
    i = np.asarray(i)
    if bits == 8:
        return (((i.astype(np.int64) * 255 + 16384) >> 15) & 0xff).astype(np.uint16)
    maxv = (1 << bits) - 1
    scale = np.float32(maxv) * np.float32(1.0 / 32768.0)
    return ((i.astype(np.float32) * scale + np.float32(0.5)).astype(np.int64) & 0xffff).astype(np.uint16)


def differs(a, b):
    return any(not np.array_equal(a[pl], b[pl]) for pl in a)


@pytest.mark.parametrize("cid,kw", WRITE16 + HOT16, ids=[c for c, _ in WRITE16 + HOT16])
def test_write_rule_and_discriminating_source(cid, kw):
    d = pkg.WriteDesc(**kw)
    maxv = (1 << d.bit_depth) - 1
    src = harness.make_write_source_over_range(d, seed=41)                      # (the builder asserts what it planted)
    assert ((src > 32768).mean() > 0.15) or src.size < 200
    want = harness.oracle_write(d, src)
    clamped = harness.oracle_write(d, np.minimum(src, 32768))
    for pl in want:
        assert np.array_equal(want[pl], clamped[pl]), (cid, pl)                 # the rule
        assert int(want[pl].max()) <= maxv, (cid, pl)
    # a kernel that masked bit 15 away instead of clamping
    assert differs(want, harness.oracle_write(d, src & 0x7fff)), cid
    # a kernel that lost its input clamp: sample by sample its code differs from the table's in every channel ...
    px = src.reshape(-1, d.planes)
    wrong, right = unclamped_codes(px, d.bit_depth), lut16(d.bit_depth)[px]
    assert (wrong != right).any(axis=0).all(), cid
    if d.bit_depth == 8:
        # ... and so do the planes: an 8-bit document saved at 8 bit hands its bytes on as codes, so the oracle itself carries the
        # wrong codes through premultiplication, matrix and sub-sampling
        d8 = pkg.WriteDesc(**dict(kw, depth=8))
        assert differs(want, harness.oracle_write(d8, np.ascontiguousarray(wrong.astype(np.uint8).reshape(d.height, -1)))), cid
    else:
        assert int(wrong[wrong != right].min()) > maxv                          # ... every one of them a code above the maximum
        if d.output == pkg.OUT_REFERENCE and d.alpha_state != pkg.ALPHA_PREMULTIPLIED:
            codes = right.reshape(d.height, d.width, d.planes)                   # this hand-off IS the table, plane for plane
            if d.planes >= 3:
                assert np.array_equal(want[0], codes.reshape(d.height, -1)), cid
            else:
                assert np.array_equal(want[0], codes[..., 0]) and (d.planes == 1 or np.array_equal(want[3], codes[..., 1])), cid


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_rescale_of_all_65536_codes(bits):
    maxv = (1 << bits) - 1
    d = pkg.WriteDesc(width=65536, height=1, depth=16, planes=1, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    got = harness.oracle_write(d, np.arange(65536, dtype=np.uint16).reshape(1, -1))[0][0]
    assert np.array_equal(got, lut16(bits))
    assert np.all(got[32768:] == maxv) and got[0] == 0 and np.all(np.diff(got.astype(np.int64)) >= 0)
    i = np.arange(32769, dtype=np.float32)                                        # the table itself: the reference's float expression
    assert np.array_equal(got[:32769], (i / np.float32(32768.0) * np.float32(maxv) + np.float32(0.5)).astype(np.int64))
    # without the clamp: the byte wraps (254 for 0xFFFF), the word runs on to twice the maximum
    assert unclamped_codes(0xFFFF, bits) == (254 if bits == 8 else 2 * maxv)
    assert np.array_equal(unclamped_codes(np.arange(32769), bits), got[:32769])   # ... and inside the range the forms ARE the table


PREMUL_COLOURS = (0, 1, 16384, 32767, 32768, 32769, 65535)


def premultiply_grid():
    """(7, 65536 * 2): every alpha under each of the colours, gray + alpha layout."""
    a = np.arange(65536, dtype=np.uint16)
    return np.ascontiguousarray(np.stack([np.stack([np.full_like(a, c), a], axis=-1).reshape(-1) for c in PREMUL_COLOURS]))


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_premultiply_over_the_whole_alpha_domain(bits):
    maxv = (1 << bits) - 1
    d = pkg.WriteDesc(width=65536, height=len(PREMUL_COLOURS), depth=16, planes=2, bit_depth=bits, alpha_state=pkg.ALPHA_PREMULTIPLIED)
    src = premultiply_grid()
    want = harness.oracle_write(d, src)
    clamped = harness.oracle_write(d, np.minimum(src, 32768))
    assert np.array_equal(want[0], clamped[0]) and np.array_equal(want[3], clamped[3])
    assert int(want[0].max()) <= maxv and int(want[3].max()) <= maxv
    t = lut16(bits)
    assert np.array_equal(want[3], np.tile(t, (len(PREMUL_COLOURS), 1)))
    assert np.all(want[0][:, 32768:] == t[list(PREMUL_COLOURS)][:, None])          # alpha at or above white: the colour's own code
    assert np.all(want[0][:, 0] == 0) and np.all(want[0][0] == 0)
    assert np.all(want[0] <= t[list(PREMUL_COLOURS)][:, None]) and np.all(want[0] <= want[3])    # c * a / max exceeds neither factor
    assert np.all(want[0][4:] == want[0][4])                                   # 32768, 32769 and 65535 are one colour: white


@pytest.mark.parametrize("cid,kw", READ_10_12, ids=[c for c, _ in READ_10_12])
def test_read_rules_and_discriminating_planes(cid, kw):
    d = pkg.ReadDesc(**kw)
    maxc = (1 << d.bit_depth) - 1
    planes = harness.make_read_source_over_range(d, seed=43)
    for arr in planes.values():
        assert (arr > maxc).mean() > 0.05
    want = harness.oracle_read(d, planes)
    masked = harness.oracle_read(d, {pl: a & maxc for pl, a in planes.items()})
    clamped = harness.oracle_read(d, {pl: np.minimum(a, maxc) for pl, a in planes.items()})
    assert np.all(np.isfinite(want.astype(np.float64))), cid
    masks = d.colorspace == pkg.COLORSPACE_RGB and d.depth == 16
    assert np.array_equal(want.view(np.uint8), (masked if masks else clamped).view(np.uint8)), cid
    assert not np.array_equal(masked.view(np.uint8), clamped.view(np.uint8)), cid


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("profile", ["matrix-trc", "a2b"])
def test_icc16_flow_clamps_its_input(lcms, profile, planes):
    """The reference flow around lcms2 (range map, transform, range map back: oracle/icc_oracle.c) on an over-range frame equals the
    flow on the clamped frame -- host_to_lcms saturates at 65535, which 32768 maps to -- alpha included."""
    icc = _profile(lcms, *PROFILES[0][1:]) if profile == "matrix-trc" else _a2b_profile(lcms, 1)
    d = pkg.WriteDesc(width=128, height=10, depth=16, planes=planes, bit_depth=12,
                      alpha_state=pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    src = harness.make_write_source_over_range(d, seed=47)
    over, inside = src.copy(), np.minimum(src, 32768)
    for rows in (over, inside):
        assert lcms.oracle_icc_convert_rows_to_srgb16(icc, len(icc), int(planes == 4), 0, rows.ctypes.data, d.width, d.height, rows.strides[0]) == 0
    assert np.array_equal(over, inside)
    assert int(over.max()) <= 32768
    assert not np.array_equal(over, np.minimum(src, 32768))                       # the transform is not the identity
