"""The summary of a save's written planes, the host side (include/avifgpu.h "summary of a save"): avifgpu_summary_read against numpy
min / max / spread of random planes, every `neutral` rule at its boundary, the rejections, avifgpu_summary_merge against np.maximum,
arming and disarming without a device, and the rule for "neutral" held against the CPU oracle on a slice of the sweep it came from
(R = G = B input through oracle_write_rows).  CPU only: none of these calls touches a device.  counters_of is the reference the GPU
tests use too."""
import ctypes
import itertools

import numpy as np
import pytest

import harness
from test_thumbnail import channels, make_desc

pkg = harness.pkg

REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C444, C422, C420 = pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420
GBR = dict(matrix_coefficients=pkg.MATRIX_RGB_GBR)
N = pkg.SUMMARY_COUNTERS
HI, LO_INV, SPREAD = 0, 4, 8


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def spread_defined(d):
    return d.planes >= 3 and (d.output == REF or (d.matrix_coefficients == pkg.MATRIX_RGB_GBR and d.chroma == C444))


def counters_of(d, planes):
    """The counters a whole feed of trimmed write planes leaves: hi[c] = max, lo_inv[c] = 65535 - min, spread where it is defined."""
    c = np.zeros(N, dtype=np.uint32)
    ch = channels(d, planes)
    for k, (_, a) in enumerate(ch):
        c[HI + k] = int(a.max())
        c[LO_INV + k] = 65535 - int(a.min())
    if spread_defined(d):
        rgb = np.stack([a.astype(np.int64) for _, a in ch[:3]])
        c[SPREAD] = int((rgb.max(axis=0) - rgb.min(axis=0)).max())
    return c


def random_planes(d, rng, lo=0, hi=None):
    hi = (1 << d.bit_depth) - 1 if hi is None else hi
    dt = np.uint16 if d.bit_depth > 8 else np.uint8
    return {pl: rng.integers(lo, hi + 1, size=((d.height + ys) >> ys, w)).astype(dt) for pl, (w, xs, ys) in harness.write_planes(d).items()}


FORMS = [(1, REF, C444, {}), (2, REF, C444, {}), (3, REF, C444, {}), (4, REF, C444, {}), (3, YCC, C444, {}), (4, YCC, C422, {}),
         (3, YCC, C420, {}), (4, YCC, C420, dict(chroma_zero_point=pkg.CHROMA_ZERO_DECODER)), (3, YCC, C444, GBR), (4, YCC, C444, GBR)]


# ---- 1. avifgpu_summary_read --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes,output,chroma,kw", FORMS)
@pytest.mark.parametrize("bits", (8, 10, 12))
def test_read_is_numpy_min_max_spread(planes, output, chroma, kw, bits):
    rng = np.random.default_rng(planes * 100 + bits)
    d = make_desc(37, 11, planes, bits, output, chroma, **kw)
    for lo, hi in ((0, None), (3, 200), (17, 17)):
        p = random_planes(d, rng, lo, hi)
        c = counters_of(d, p)
        s = pkg.summary_read(d, c)
        ch = channels(d, p)
        assert s.channels == planes
        assert list(s.min_code)[:planes] == [int(a.min()) for _, a in ch] and list(s.max_code)[:planes] == [int(a.max()) for _, a in ch]
        assert list(s.min_code)[planes:] == [0] * (4 - planes) and list(s.max_code)[planes:] == [0] * (4 - planes)
        assert s.spread == (int(c[SPREAD]) if spread_defined(d) else -1)
        maxcode = (1 << bits) - 1
        if planes in (2, 4):
            alpha = ch[-1][1]
            assert s.alpha_opaque == int(alpha.min() == maxcode) and s.alpha_clear == int(alpha.max() == 0)
        else:
            assert s.alpha_opaque == -1 and s.alpha_clear == -1
        if planes <= 2:
            assert s.neutral == 1
        elif spread_defined(d):
            assert s.neutral == int(c[SPREAD] == 0)
        assert s.advice == (pkg.ADVICE_DROP_ALPHA if s.alpha_opaque == 1 else 0) | (pkg.ADVICE_MONOCHROME if planes >= 3 and s.neutral else 0)


def _fed(planes, values):
    """Counters of channels whose (min, max) are `values`."""
    c = np.zeros(N, dtype=np.uint32)
    for k, (lo, hi) in enumerate(values):
        c[HI + k], c[LO_INV + k] = hi, 65535 - lo
    return c


@pytest.mark.parametrize("bits", (8, 10, 12))
def test_neutral_rules_at_their_boundaries(bits):
    half, maxcode = 1 << (bits - 1), (1 << bits) - 1
    y = (0, maxcode)
    # LIBHEIF: exactly half on both chroma planes
    d = make_desc(8, 8, 3, bits, YCC, C420, chroma_zero_point=pkg.CHROMA_ZERO_LIBHEIF)
    for cb, cr, want in (((half, half), (half, half), 1), ((half - 1, half), (half, half), 0), ((half, half + 1), (half, half), 0),
                         ((half, half), (half - 1, half - 1), 0), ((half, half), (half, half + 1), 0)):
        s = pkg.summary_read(d, _fed(3, (y, cb, cr)))
        assert s.neutral == want and s.spread == -1 and s.advice == (pkg.ADVICE_MONOCHROME if want else 0), (cb, cr)
    # DECODER: within [half - 1, half] on both
    d = make_desc(8, 8, 4, bits, YCC, C444, chroma_zero_point=pkg.CHROMA_ZERO_DECODER)
    a = (maxcode, maxcode)
    for lo, hi, want in ((half - 1, half, 1), (half - 1, half - 1, 1), (half, half, 1), (half - 2, half, 0), (half - 2, half - 2, 0),
                         (half - 1, half + 1, 0), (half + 1, half + 1, 0)):
        for cb, cr in (((lo, hi), (half, half)), ((half - 1, half), (lo, hi))):
            s = pkg.summary_read(d, _fed(4, (y, cb, cr, a)))
            assert s.neutral == want and s.advice == pkg.ADVICE_DROP_ALPHA | (pkg.ADVICE_MONOCHROME if want else 0), (lo, hi)
    # REFERENCE colour and G,B,R planes: the spread, whatever the ranges
    for d in (make_desc(8, 8, 3, bits, REF), make_desc(8, 8, 3, bits, YCC, C444, **GBR)):
        c = _fed(3, ((0, maxcode),) * 3)
        assert pkg.summary_read(d, c).neutral == 1 and pkg.summary_read(d, c).advice == pkg.ADVICE_MONOCHROME
        c[SPREAD] = 1
        assert pkg.summary_read(d, c).neutral == 0 and pkg.summary_read(d, c).advice == 0
    # gray: always, and MONOCHROME is no advice for a save that is monochrome already
    s = pkg.summary_read(make_desc(8, 8, 2, bits, REF), _fed(2, ((3, 9), (0, 0))))
    assert s.neutral == 1 and s.advice == 0 and s.alpha_clear == 1 and s.alpha_opaque == 0
    # alpha: opaque means the MINIMUM is the maximum code
    d = make_desc(8, 8, 4, bits, REF)
    assert pkg.summary_read(d, _fed(4, (y, y, y, (maxcode - 1, maxcode)))).alpha_opaque == 0
    assert pkg.summary_read(d, _fed(4, (y, y, y, (maxcode, maxcode)))).alpha_opaque == 1


def test_read_rejections():
    d = make_desc(8, 8, 4, 10, YCC, C420)
    good = _fed(4, ((0, 1023), (500, 520), (512, 512), (1023, 1023)))
    assert pkg.summary_read(d, good).channels == 4
    for k in range(4):                                                   # a used channel was never fed
        c = good.copy()
        c[LO_INV + k] = 0
        with pytest.raises(pkg.AvifGpuError) as e:
            pkg.summary_read(d, c)
        assert e.value.code == pkg.formatBadParameters and "never fed" in e.value.message
    with pytest.raises(pkg.AvifGpuError):                                # the empty summary
        pkg.summary_read(d, np.zeros(N, dtype=np.uint32))
    for k in range(4):                                                   # a maximum above the range: not this descriptor's counters
        c = good.copy()
        c[HI + k] = 1024
        with pytest.raises(pkg.AvifGpuError) as e:
            pkg.summary_read(d, c)
        assert e.value.code == pkg.formatBadParameters and "not of this descriptor" in e.value.message
    c = good.copy()                                                      # channels the descriptor does not use are not looked at
    d3 = make_desc(8, 8, 3, 10, YCC, C420)
    c[HI + 3], c[LO_INV + 3] = 9999, 0
    assert pkg.summary_read(d3, c).channels == 3
    c = _fed(3, ((0, 255),) * 3)                                         # the spread too
    c[SPREAD] = 256
    with pytest.raises(pkg.AvifGpuError):
        pkg.summary_read(make_desc(8, 8, 3, 8, REF), c)
    lib = pkg.load()
    out = pkg.SaveSummary()
    assert lib.avifgpu_summary_read(None, good.ctypes.data, ctypes.byref(out)) == pkg.formatBadParameters
    assert lib.avifgpu_summary_read(ctypes.byref(d), None, ctypes.byref(out)) == pkg.formatBadParameters
    assert lib.avifgpu_summary_read(ctypes.byref(d), good.ctypes.data, None) == pkg.formatBadParameters
    bad = make_desc(8, 8, 4, 9, YCC, C420)
    assert lib.avifgpu_summary_read(ctypes.byref(bad), good.ctypes.data, ctypes.byref(out)) != 0


# ---- 2. merge, arming ---------------------------------------------------------------------------------------------------------------
def test_merge_is_np_maximum():
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
        want = np.maximum(a, b)
        keep = b.copy()
        assert pkg.summary_merge(a, b) is a
        assert np.array_equal(a, want) and np.array_equal(b, keep)
    z = np.zeros(N, dtype=np.uint32)                                    # the empty summary is the identity
    assert np.array_equal(pkg.summary_merge(z, want), want) and np.array_equal(pkg.summary_merge(want.copy(), np.zeros(N, np.uint32)), want)
    lib = pkg.load()
    assert lib.avifgpu_summary_merge(None, z.ctypes.data) == pkg.formatBadParameters
    assert lib.avifgpu_summary_merge(z.ctypes.data, None) == pkg.formatBadParameters
    # tiles of one image: the merge of the tiles' summaries is the summary of the image
    d = make_desc(37, 12, 3, 10, YCC, C420)
    p = random_planes(d, rng)
    top = {pl: a[:(6 >> harness.write_planes(d)[pl][2])] for pl, a in p.items()}
    bottom = {pl: a[(6 >> harness.write_planes(d)[pl][2]):] for pl, a in p.items()}
    assert np.array_equal(pkg.summary_merge(counters_of(d, top), counters_of(d, bottom)), counters_of(d, p))


def test_arming_needs_no_device():
    lib = pkg.load()
    c = np.zeros(N, dtype=np.uint32)
    for kind in (pkg.MEM_HOST, pkg.MEM_DEVICE):
        assert lib.avifgpu_summary_attach(c.ctypes.data, kind) == 0
        assert lib.avifgpu_summary_attach(None, kind) == 0
    assert lib.avifgpu_summary_attach(None, 77) == 0                     # disarming always succeeds
    for kind in (-1, 2, 77):
        assert lib.avifgpu_summary_attach(c.ctypes.data, kind) == pkg.formatBadParameters
        assert b"mem_kind" in lib.avifgpu_last_error()
    with pkg.plane_summary(c):
        pass
    with pytest.raises(pkg.AvifGpuError):
        with pkg.plane_summary(c, mem=5):
            pass
    with pytest.raises(ValueError):
        with pkg.plane_summary(np.zeros(N - 1, dtype=np.uint32)):
            pass
    with pytest.raises(ValueError):
        with pkg.plane_summary(np.zeros(N, dtype=np.uint64)):
            pass
    assert not c.any()


def test_symbols_and_abi():
    lib = pkg.load()
    assert lib.avifgpu_abi_version() == 5
    for name in ("avifgpu_summary_attach", "avifgpu_summary_read", "avifgpu_summary_merge", "avifgpu_probe_summary"):
        assert getattr(lib, name).argtypes is not None, name
        assert name in pkg.ABI4_NEW
    assert ctypes.sizeof(pkg.SaveSummary) == 14 * 4 and ctypes.sizeof(pkg.WriteDesc) == 16 * 4


# ---- 3. the rule for "neutral" and the oracle stay together ----------------------------------------------------------------------------
MATRICES = ((pkg.MATRIX_BT709, pkg.PRIMARIES_BT709), (pkg.MATRIX_FCC, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT470BG, pkg.PRIMARIES_BT709),
            (pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), (pkg.MATRIX_SMPTE240M, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020))


def _gray_source(depth, planes, w, h, rng):
    """R = G = B over the whole range of the depth, alpha (if any) opaque."""
    if depth == 8:
        v, opaque, dt = rng.integers(0, 256, size=(h, w)), 255, np.uint8
    elif depth == 16:
        v, opaque, dt = rng.integers(0, 32769, size=(h, w)), 32768, np.uint16
    else:
        v, opaque, dt = rng.random((h, w)) * np.where(rng.random((h, w)) < 0.1, 12.0, 1.0), 1.0, np.float32
    px = np.repeat(np.asarray(v)[..., None], planes, axis=2).astype(dt)
    if planes == 4:
        px[..., 3] = opaque
    return np.ascontiguousarray(px.reshape(h, w * planes))


def _sweep():
    out, k = [], 0
    for depth in (8, 16, 32):
        for bits in ((10, 12) if depth == 32 else (8, 10, 12)):
            for chroma in (C444, C422, C420):
                for zero in (pkg.CHROMA_ZERO_LIBHEIF, pkg.CHROMA_ZERO_DECODER):
                    # matrices, filters, alpha and transfers rotate through the cells: every value meets every depth
                    m = MATRICES[k % 6]
                    filt = (pkg.DOWNSAMPLE_AVERAGE, pkg.DOWNSAMPLE_NEAREST)[(k // 2) % 2]
                    planes = 3 + (k // 3) % 2
                    transfer = (pkg.TRANSFER_PQ, pkg.TRANSFER_CLIP, pkg.TRANSFER_SMPTE428)[k % 3] if depth == 32 else pkg.TRANSFER_CLIP
                    k += 1
                    out.append((depth, bits, chroma, zero, m, filt, planes, transfer))
    return out


def test_gray_input_is_neutral_by_the_rule_on_the_oracle():
    rng = np.random.default_rng(11)
    alternating = 0
    for depth, bits, chroma, zero, (matrix, prim), filt, planes, transfer in _sweep():
        d = pkg.WriteDesc(width=33, height=10, depth=depth, planes=planes, bit_depth=bits, transfer=transfer, peak_nits=1000,
                          alpha_state=pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE, output=YCC, chroma=chroma,
                          matrix_coefficients=matrix, color_primaries=prim, chroma_downsampling=filt, chroma_zero_point=zero)
        p = harness.oracle_write(d, _gray_source(depth, planes, d.width, d.height, rng))
        s = pkg.summary_read(d, counters_of(d, p))
        what = (depth, bits, chroma, zero, matrix, filt, planes, transfer)
        half = 1 << (bits - 1)
        assert s.neutral == 1 and s.advice & pkg.ADVICE_MONOCHROME, (what, list(s.min_code), list(s.max_code))
        if zero == pkg.CHROMA_ZERO_LIBHEIF:
            assert list(s.min_code)[1:3] == [half, half] and list(s.max_code)[1:3] == [half, half], what
        else:
            alternating += s.min_code[1] != s.max_code[1] or s.min_code[2] != s.max_code[2]
        if planes == 4:
            assert s.alpha_opaque == 1 and s.alpha_clear == 0 and s.advice & pkg.ADVICE_DROP_ALPHA, what
        else:
            assert s.alpha_opaque == -1
    assert alternating > 0                                              # the half-integer zero point does land on both neighbours


def test_coloured_input_is_not_neutral_on_the_oracle():
    for zero, chroma in itertools.product((pkg.CHROMA_ZERO_LIBHEIF, pkg.CHROMA_ZERO_DECODER), (C444, C420)):
        d = pkg.WriteDesc(width=33, height=10, depth=8, planes=4, bit_depth=8, alpha_state=pkg.ALPHA_STRAIGHT, output=YCC, chroma=chroma,
                          chroma_zero_point=zero)
        src = harness.make_write_source(d, seed=3)
        s = pkg.summary_read(d, counters_of(d, harness.oracle_write(d, src)))
        assert s.neutral == 0 and s.alpha_opaque == 0 and s.advice == 0
    d = pkg.WriteDesc(width=33, height=10, depth=8, planes=3, bit_depth=8, output=REF)
    src = _gray_source(8, 3, 33, 10, np.random.default_rng(1))
    assert pkg.summary_read(d, counters_of(d, harness.oracle_write(d, src))).neutral == 1
    src[4, 3 * 7 + 1] ^= 1                                               # one sample of one pixel, one code
    s = pkg.summary_read(d, counters_of(d, harness.oracle_write(d, src)))
    assert s.neutral == 0 and s.spread == 1
