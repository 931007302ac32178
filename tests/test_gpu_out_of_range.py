"""Out-of-range samples, GPU half: every kernel is held to the rules of oracle/avif_oracle.c:31-38 on samples the rules apply to.

 * saves of 16-bit documents whose samples (alpha included) run up to 65535: the planes equal the oracle's on the same bytes AND the
   GPU's own planes for min(source, 32768) -- the second check needs no oracle -- every code is <= the maximum, the padding of the
   plane rows keeps its fill; default dispatch, each named streaming kernel, the generic kernel, the host entry, odd plane strides;
 * the 16-bit ICC stage (its table position is only defined up to 32768), the thumbnail sums of such a save;
 * opens of 10- / 12-bit planes with samples up to 65535: masked by a 16-bit planar-RGB open, clamped by every other one;
 * NaN / +-Inf through every float kernel of the equivalence table: codes inside [0, max], finite neighbours unchanged.

tests/test_out_of_range.py shows on the CPU that the same sources follow the rules in the oracle and tell a wrong kernel apart."""
import numpy as np
import pytest

import cases
import harness
import test_gpu_kernel_equivalence as equivalence
from test_gpu_read import _check as check_read
from test_gpu_thumbnail import check as check_thumbnail, write_thumb
from test_icc16 import PROFILES, _a2b_profile, _clut_from_transform, _profile, lcms          # noqa: F401  (lcms: the module-scoped fixture)
from test_out_of_range import HOT16, PREMUL_COLOURS, READ_10_12, WRITE16, lut16, premultiply_grid

pkg = harness.pkg
pytestmark = pytest.mark.gpu

DEFAULT_VARIANT = 1 | 2 | 4
ODD_PAD = 3                                                   # samples: plane rows that are not even dword-aligned

_WANT = {}


def every(items, fn):
    """Run fn on every item -- the cases of one test are ONE test here, so that the suite grows by a handful of tests, not by hundreds --
    and report all the failing ones together (a case that fails does not hide the ones after it)."""
    failed = []
    for item in items:
        try:
            fn(*item)
        except AssertionError as e:
            failed.append(f"{next((x for x in item if isinstance(x, str)), item[0])}: {e}")
    assert not failed, f"{len(failed)} of {len(items)} cases:\n" + "\n".join(failed)


def over_range_case(kw, seed=41):
    """(descriptor, over-range source, the same source clamped, oracle planes with their row padding) -- computed once per case."""
    key = (tuple(sorted(kw.items())), seed)
    if key not in _WANT:
        d = pkg.WriteDesc(**kw)
        src = harness.make_write_source_over_range(d, seed=seed)
        _WANT[key] = (d, src, np.minimum(src, 32768), {})
    return _WANT[key]


def oracle_raw(case, stride_pad):
    d, src, _, cache = case
    if stride_pad not in cache:
        cache[stride_pad] = harness.oracle_write(d, src, stride_pad=stride_pad, return_raw=True)
    return cache[stride_pad]


def hold_to_the_rule(gpu, case, what, mem="device", stride_pad=0, kernel=None):
    d, src, inside, _ = case
    maxv = (1 << d.bit_depth) - 1
    want = oracle_raw(case, stride_pad)
    got = harness.gpu_write(gpu, d, src, mem=mem, stride_pad=stride_pad, return_raw=True)
    name = gpu.last_kernel()
    if kernel is not None:
        assert kernel in name, (what, name)
    own = harness.gpu_write(gpu, d, inside, mem=mem, stride_pad=stride_pad, return_raw=True)
    assert gpu.last_kernel() == name, (what, name, gpu.last_kernel())
    for pl, (w, xs, ys) in harness.write_planes(d).items():
        assert np.array_equal(got[pl], own[pl]), (what, name, pl, "differs from the GPU's own planes of the clamped source")
        assert np.array_equal(got[pl], want[pl]), (what, name, pl, "differs from the oracle (padding included)")
        assert int(got[pl][:, :w].max()) <= maxv, (what, name, pl)
        assert np.all(got[pl][:, w:] == (0xA5A5 if d.bit_depth > 8 else 0xA5)), (what, name, pl, "padding written")


def _default_dispatch(gpu, n, cid, kw):
    case = over_range_case(kw)
    hold_to_the_rule(gpu, case, cid)
    assert "write" in gpu.last_kernel()
    if n % 5 == 0:
        hold_to_the_rule(gpu, case, cid + " host", mem="host", stride_pad=24)
    if n % 5 == 1:
        hold_to_the_rule(gpu, case, cid + " odd stride", stride_pad=ODD_PAD)      # the unaligned instantiations


def test_saves_of_over_range_documents_default_dispatch(gpu):
    """Every depth-16 entry of cases.write_cases(); every fifth also through the host entry, every fifth also with odd plane strides."""
    every([(n, c, k) for n, (c, k) in enumerate(WRITE16)], lambda n, cid, kw: _default_dispatch(gpu, n, cid, kw))


def _each_kernel(gpu, n, cid, kw):
    case = over_range_case(kw)
    kernel = cid.rsplit("-", 1)[0]
    try:
        gpu.lib.avifgpu_set_hot_variant(1 | 2 | 4 | 8)
        hold_to_the_rule(gpu, case, cid, kernel=kernel)
        gpu.lib.avifgpu_set_hot_variant(0)
        hold_to_the_rule(gpu, case, cid + " generic", kernel="write_px")
        if n % 5 == 0:
            hold_to_the_rule(gpu, case, cid + " generic host", mem="host", stride_pad=24, kernel="write_px")
        if n % 5 == 1:
            hold_to_the_rule(gpu, case, cid + " generic odd stride", stride_pad=ODD_PAD, kernel="write_px")
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)


HOT16_KERNELS = sorted({cid.rsplit("-", 1)[0] for cid, _ in HOT16})


@pytest.mark.parametrize("kernel", HOT16_KERNELS)
def test_saves_of_over_range_documents_each_kernel(gpu, kernel):
    """Every depth-16 entry of the equivalence table that names this kernel: on the kernel itself (asserted) and on the generic one."""
    mine = [(n, c, k) for n, (c, k) in enumerate(HOT16) if c.rsplit("-", 1)[0] == kernel]
    assert mine
    every(mine, lambda n, cid, kw: _each_kernel(gpu, n, cid, kw))


def test_premultiply_over_the_whole_alpha_domain(gpu):
    """Colours at and beyond white under all 65536 alphas, gray + alpha: the streaming kernel (stage_a per pixel) and the generic one."""
    every([(bits,) for bits in (8, 10, 12)], lambda bits: _premultiply_domain(gpu, bits))


def _premultiply_domain(gpu, bits):
    maxv = (1 << bits) - 1
    d = pkg.WriteDesc(width=65536, height=len(PREMUL_COLOURS), depth=16, planes=2, bit_depth=bits, alpha_state=pkg.ALPHA_PREMULTIPLIED)
    src = premultiply_grid()
    want = harness.oracle_write(d, src)
    assert np.array_equal(want[3], np.tile(lut16(bits), (len(PREMUL_COLOURS), 1)))
    try:
        for variant, kernel in ((1 | 2 | 4 | 8, "write_ga_stream" if bits > 8 else "write"), (0, "write_px")):
            gpu.lib.avifgpu_set_hot_variant(variant)
            got = harness.gpu_write(gpu, d, src)
            assert kernel in gpu.last_kernel(), gpu.last_kernel()
            own = harness.gpu_write(gpu, d, np.minimum(src, 32768))
            for pl in (0, 3):
                assert np.array_equal(got[pl], want[pl]), (bits, variant, pl)
                assert np.array_equal(got[pl], own[pl]), (bits, variant, pl)
                assert int(got[pl].max()) <= maxv
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)


@pytest.mark.parametrize("profile", ["matrix-trc", "a2b"])
def test_icc16_stage_clamps_its_input(gpu, lcms, profile):
    """The table position of the 16-bit ICC stage (icc16_host_to_fixed) is defined up to 32768: full footprints take the packed clamp,
    ragged ones the scalar clamp (write_px).  Output = real lcms2 flow, then the oracle's pixel loop; = the GPU on the clamped source."""
    if profile == "matrix-trc":
        icc = _profile(lcms, *PROFILES[0][1:])
        clut = gpu.icc_prepare_clut16(icc)                      # avifgpu_icc_prepare_clut16
    else:
        icc = _a2b_profile(lcms, 1)
        rc, clut = _clut_from_transform(lcms, icc)
        assert rc == 0
    every([(f"{profile}-{planes}", planes) for planes in (3, 4)], lambda what, planes: _icc16_stage(gpu, lcms, profile, icc, clut, planes))


def _icc16_stage(gpu, lcms, profile, icc, clut, planes):
    alpha = pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE
    for width, height, pad in ((128, 10, 0), (67, 21, ODD_PAD)):
        for bits in (8, 12):
            for out in (dict(output=pkg.OUT_REFERENCE), dict(output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT601)):
                d = pkg.WriteDesc(width=width, height=height, depth=16, planes=planes, bit_depth=bits, alpha_state=alpha, **out)
                src = harness.make_write_source_over_range(d, seed=47)
                conv = src.copy()
                assert lcms.oracle_icc_convert_rows_to_srgb16(icc, len(icc), int(planes == 4), 0, conv.ctypes.data, d.width, d.height, conv.strides[0]) == 0
                want = harness.oracle_write(d, conv, stride_pad=pad, return_raw=True)
                got = harness.gpu_write(gpu, d, src, stride_pad=pad, return_raw=True, icc=clut)
                assert "icc=5" in gpu.last_kernel(), gpu.last_kernel()
                own = harness.gpu_write(gpu, d, np.minimum(src, 32768), stride_pad=pad, return_raw=True, icc=clut)
                for pl in want:
                    assert np.array_equal(got[pl], want[pl]), (profile, planes, width, bits, out, pl)
                    assert np.array_equal(got[pl], own[pl]), (profile, planes, width, bits, out, pl)


def test_thumbnail_of_an_over_range_save(gpu):
    """The sums are taken from the planes just written: they equal the box sums of the oracle's (clamped) planes."""
    d = pkg.WriteDesc(width=97, height=41, depth=16, planes=4, bit_depth=10, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_YCBCR,
                      chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709)
    src = harness.make_write_source_over_range(d, seed=53)
    want = harness.oracle_write(d, src)
    got, sums = write_thumb(gpu, d, src, 13, 7)
    for pl in want:
        assert np.array_equal(got[pl], want[pl]), pl
    check_thumbnail(d, got, sums, want, 13, 7, "over-range save")


# ---- opens ----------------------------------------------------------------------------------------------------------------------
def _ruled(d, planes):
    """The planes as the rule reads them: masked for a 16-bit planar-RGB open, clamped for every other one."""
    maxc = (1 << d.bit_depth) - 1
    if d.colorspace == pkg.COLORSPACE_RGB and d.depth == 16:
        return {pl: a & maxc for pl, a in planes.items()}
    return {pl: np.minimum(a, maxc) for pl, a in planes.items()}


def _hold_read(gpu, cid, kw, d, planes, mem="device"):
    want = harness.oracle_read(d, planes)
    got = harness.gpu_read(gpu, d, planes, mem=mem)
    name = gpu.last_kernel()
    check_read(cid, kw, got, want)                              # integer tiers: equal; float tier: the bar of tests/test_gpu_read.py
    own = harness.gpu_read(gpu, d, _ruled(d, planes), mem=mem)
    assert gpu.last_kernel() == name
    assert np.array_equal(got.view(np.uint8), own.view(np.uint8)), (cid, name, "differs from the GPU's own rows of the masked / clamped planes")
    return got


READ_FAMILIES = {"ycbcr": pkg.COLORSPACE_YCBCR, "planar-rgb": pkg.COLORSPACE_RGB, "gray": pkg.COLORSPACE_MONOCHROME}


@pytest.mark.parametrize("family", sorted(READ_FAMILIES))
def test_opens_of_over_range_planes(gpu, family):
    """Every 10- / 12-bit entry of cases.read_cases() of this colour space, every host depth; every sixth also through the host entry."""
    mine = [(n, c, k) for n, (c, k) in enumerate(READ_10_12) if k["colorspace"] == READ_FAMILIES[family]]
    assert mine
    every(mine, lambda n, cid, kw: _open_over_range(gpu, n, cid, kw))


def _open_over_range(gpu, n, cid, kw):
    d = pkg.ReadDesc(**kw)
    _hold_read(gpu, cid, kw, d, harness.make_read_source_over_range(d, seed=43))
    assert "read" in gpu.last_kernel()
    if n % 6 == 0:
        _hold_read(gpu, cid + " host", kw, d, harness.make_read_source_over_range(d, seed=99, stride_pad=40), mem="host")


READ_FLAT_10_12 = [(i, kw) for i, kw in enumerate(equivalence.READ_FLAT_CASES) if kw["bit_depth"] in (10, 12)]


def test_opens_of_over_range_planes_flat_and_by_rows(gpu):
    every([(f"read-flat-{i}", i, kw) for i, kw in READ_FLAT_10_12], lambda what, i, kw: _flat_and_by_rows(gpu, i, kw))


def _flat_and_by_rows(gpu, i, kw):
    d = pkg.ReadDesc(**kw)
    planes = harness.make_read_source_over_range(d, seed=23)
    try:
        flat = _hold_read(gpu, f"read-flat-{i}", kw, d, planes)
        assert gpu.last_kernel().endswith(" flat"), gpu.last_kernel()
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT | 16)
        rows = _hold_read(gpu, f"read-rows-{i}", kw, d, planes)
        assert "flat" not in gpu.last_kernel(), gpu.last_kernel()
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)
    assert np.array_equal(flat.view(np.uint8), rows.view(np.uint8))


# ---- non-finite floats ------------------------------------------------------------------------------------------------------------
HOT32 = [(f"{k}-{i}", kw) for i, (k, kw) in enumerate(equivalence.CASES) if kw["depth"] == 32]
SNAN = np.array([0x7fa00000], dtype=np.uint32).view(np.float32)[0]          # a signalling NaN bit pattern
POISON = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), SNAN)


def _poisoned_pixels(d):
    n = d.width * d.height
    return sorted({5 % n, (d.width + 6) % n, (2 * d.width + 7) % n, n - 1})          # a ragged last lane among them


def _untouched(d, pixels):
    """{plane: bool mask of the samples that share no pixel / chroma box with a poisoned pixel}."""
    out = {}
    for pl, (w, xs, ys) in harness.write_planes(d).items():
        h = (d.height + ys) >> ys
        m = np.ones((h, w), dtype=bool)
        for p in pixels:
            y, x = divmod(p, d.width)
            if d.output == pkg.OUT_REFERENCE and d.planes >= 3:
                m[y, x * d.planes:(x + 1) * d.planes] = False
            else:
                m[y >> ys, x >> xs] = False
        out[pl] = m
    return out


HOT32_KERNELS = sorted({cid.rsplit("-", 1)[0] for cid, _ in HOT32})


@pytest.mark.parametrize("kernel", HOT32_KERNELS)
def test_non_finite_samples_stay_in_range_in_every_float_kernel(gpu, kernel):
    """Every depth-32 entry of the equivalence table that names this kernel (see _non_finite)."""
    mine = [(c, k) for c, k in HOT32 if c.rsplit("-", 1)[0] == kernel]
    assert mine
    every(mine, lambda cid, kw: _non_finite(gpu, cid, kw))


def _non_finite(gpu, cid, kw):
    """The guarantees of test_gpu_extremes.py::test_non_finite_samples_stay_in_range, kernel by kernel: every code inside [0, max],
    samples that share no pixel and no chroma box with a poisoned pixel unchanged, alpha codes of pixels with finite alpha unchanged --
    with the colour channels poisoned and, separately, alpha."""
    d = pkg.WriteDesc(**kw)
    maxv = (1 << d.bit_depth) - 1
    has_alpha = d.planes in (2, 4)
    ncol = d.planes - 1 if has_alpha else d.planes
    src = harness.make_write_source(d, seed=31)
    pixels = _poisoned_pixels(d)
    keep = _untouched(d, pixels)
    sources = {}
    bad = src.copy().reshape(-1, d.planes)
    for j, p in enumerate(pixels):
        bad[p, :ncol] = POISON[j % 4]
    bad[pixels[-1], :ncol] = src.reshape(-1, d.planes)[pixels[-1], :ncol]
    bad[pixels[-1], ncol - 1] = SNAN                                                # one channel only, the others finite
    sources["colour"] = bad.reshape(src.shape)
    if has_alpha:
        bad = src.copy().reshape(-1, d.planes)
        for j, p in enumerate(pixels):
            bad[p, -1] = POISON[j % 4]
        sources["alpha"] = bad.reshape(src.shape)
    kernel = cid.rsplit("-", 1)[0]
    try:
        for variant, name in ((1 | 2 | 4 | 8, kernel), (0, "write_px")):
            gpu.lib.avifgpu_set_hot_variant(variant)
            clean = harness.gpu_write(gpu, d, src)
            assert name in gpu.last_kernel(), gpu.last_kernel()
            for which, poisoned in sources.items():
                got = harness.gpu_write(gpu, d, poisoned)
                assert name in gpu.last_kernel(), gpu.last_kernel()
                for pl in got:
                    assert int(got[pl].max()) <= maxv, (cid, name, which, pl)
                    assert np.array_equal(got[pl][keep[pl]], clean[pl][keep[pl]]), (cid, name, which, pl)
                if has_alpha and which == "colour":                              # alpha is finite everywhere: its codes do not move
                    if d.output == pkg.OUT_REFERENCE and d.planes == 4:
                        assert np.array_equal(got[0][:, 3::4], clean[0][:, 3::4]), (cid, name)
                    else:
                        assert np.array_equal(got[3], clean[3]), (cid, name)
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)
