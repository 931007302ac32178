"""Integer saves against the oracle on EVERY code combination their arithmetic can see, bit for bit (no tolerance anywhere).

The write kernels reach the oracle's bits by other routes than its plain expressions: the packed luma of the RGB hot kernels, luma
without its clip (luma_code_nc), clamp + floor + cast in one step, the integer premultiply (exact_premultiply_int,
exact_premultiply_fast_pair) in place of the float one, the 16 -> n bit rescale in arithmetic instead of a table.  Here:

  RGB8 -> Y, Cb, Cr     all 2^24 (R, G, B) triples, 4:4:4 at 8 / 10 / 12 bit under five matrices; the same document saved 4:2:2 and
                        4:2:0, box and nearest (luma stays exhaustive, chroma sees every average this document produces)
  16-bit documents      every 8-bit code triple, each channel at BOTH ends of the source interval that rescales to its code;
                        every sample value 0 .. 65535 in every channel position (GBR: the planes are the rescaled codes)
  integer premultiply   every (colour code, alpha code) pair at 8, 10 and 12 bit -- 256^2 + 1024^2 + 4096^2 pairs, the domain of
                        tools/divcheck_premul.hip -- through every kernel that premultiplies; straight alpha next to it

Each case runs the streaming kernel the dispatcher picks AND the generic write_px (tuning word 0) against ONE oracle run, and asserts
from the launch label which kernel ran.  10- / 12-bit code triples under a real matrix: tests/test_zzzzzzzzz_gpu_tie_triples.py holds, for
every (R, B) pair, the G that puts Y, Cb or Cr next to a rounding tie.  NOT exhaustive: ALL 10- / 12-bit code triples (2^30, 2^36),
16-bit SOURCE triples (2^45).
Inputs: tests/exhaustive_inputs.py (claims counted in tests/test_exhaustive_inputs.py, where the oracle's save is also held to a numpy
restatement on all triples).
The file is named to be collected after every earlier GPU test, so that those keep their places in the collection order.
"""
import functools

import numpy as np
import pytest

import exhaustive_inputs as xi
import harness

pkg = harness.pkg
pytestmark = pytest.mark.gpu

DEFAULT_VARIANT = 1 | 2 | 4
STREAMING = 1 | 2 | 4 | 8         # bit 3: streaming kernels at any size
GENERIC = 0

BT709 = dict(matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709)
GBR = dict(matrix_coefficients=pkg.MATRIX_RGB_GBR)
MATRICES = [("bt601", dict(matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709)), ("bt709", BT709),
            ("bt2020ncl", dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)),
            ("chromaderived432", dict(matrix_coefficients=pkg.MATRIX_CHROMA_DERIVED_NCL, color_primaries=pkg.PRIMARIES_SMPTE432)),
            ("gbr", GBR)]
CHROMA = {"444": pkg.CHROMA_444, "422": pkg.CHROMA_422, "420": pkg.CHROMA_420}
DOWN = {"box": pkg.DOWNSAMPLE_AVERAGE, "nearest": pkg.DOWNSAMPLE_NEAREST}


def _assert_kernel(label, d, variant, kernel):
    """The launch label names the kernel this run is about.  `kernel`: the label's beginning, or (beginning, a part it must contain)."""
    ys = harness.chroma_shift(d.chroma)[1] if d.output == pkg.OUT_YCBCR else 0
    if variant == STREAMING and kernel is not None:
        begin, part = kernel if isinstance(kernel, tuple) else (kernel, "")
        assert label.startswith(begin) and part in label, (label, kernel)
        # launch_write: contiguous 16- and 32-bit rows without vertical sub-sampling are one long row; so is a contiguous copy
        flat = (d.depth in (16, 32) and d.planes >= 3 and ys == 0) or begin.startswith("write_copy_rows_stream")
        assert label.endswith(" flat") == flat, label
    else:
        assert label.startswith(f"write_px<depth={d.depth},planes={d.planes},"), label
        assert f"dst16={int(d.bit_depth > 8)}," in label and "aligned=1" in label and "flat" not in label, label


def _save_both_ways(gpu, d, src, kernel, what=()):
    """One oracle run judges the streaming kernel `kernel` (None: the dispatcher has none for this descriptor) and the generic one.
    Returns the oracle's planes."""
    want = harness.oracle_write(d, src)
    try:
        for variant in (STREAMING, GENERIC):
            gpu.lib.avifgpu_set_hot_variant(variant)
            got = harness.gpu_write(gpu, d, src)
            label = gpu.last_kernel()
            _assert_kernel(label, d, variant, kernel)
            for pl in want:
                if not np.array_equal(got[pl], want[pl]):
                    bad = np.argwhere(got[pl] != want[pl])
                    raise AssertionError((what, label, f"plane {pl}: {len(bad)} samples differ", "first (row, col): got, oracle",
                                          [(tuple(int(v) for v in i), int(got[pl][tuple(i)]), int(want[pl][tuple(i)])) for i in bad[:8]]))
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)
    return want


@functools.lru_cache(maxsize=1)
def _rgb8_all_triples():
    return xi.interleaved(xi.all_triples_444())                      # R = k >> 16, G = k & 255, B = (k >> 8) & 255


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    """The shared document (48 MB) goes when this file's tests are done."""
    yield
    _rgb8_all_triples.cache_clear()


# ---- RGB8, all triples ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,matrix", MATRICES, ids=[n for n, _ in MATRICES])
@pytest.mark.parametrize("bits", [8, 10, 12])
def test_save_all_rgb8_triples_444(gpu, bits, name, matrix):
    src = _rgb8_all_triples()
    d = pkg.WriteDesc(width=4096, height=4096, depth=8, planes=3, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
                      chroma=pkg.CHROMA_444, **matrix)
    kernel = "write_rgb8_ycbcr_hot<xs=0,ys=0," if bits == 8 else "write_rgb8_ycbcr16_hot<xs=0,ys=0,"
    _save_both_ways(gpu, d, src, kernel, what=(bits, name))


@pytest.mark.parametrize("down", ["box", "nearest"])
@pytest.mark.parametrize("chroma", ["422", "420"])
@pytest.mark.parametrize("bits", [8, 12])
def test_save_all_rgb8_triples_subsampled(gpu, bits, chroma, down):
    src = _rgb8_all_triples()
    xs, ys = xi.sub_shifts(chroma)
    d = pkg.WriteDesc(width=4096, height=4096, depth=8, planes=3, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
                      chroma=CHROMA[chroma], chroma_downsampling=DOWN[down], **BT709)
    stem = "write_rgb8_ycbcr_hot" if bits == 8 else "write_rgb8_ycbcr16_hot"
    _save_both_ways(gpu, d, src, f"{stem}<xs={xs},ys={ys},nearest={int(down == 'nearest')}>", what=(bits, chroma, down))


# ---- 16-bit documents -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _preimages(bits):
    """(lo, hi): the two ends of the interval of Photoshop 16-bit values 0 .. 32768 that the ORACLE rescales to each `bits`-bit code."""
    d = pkg.WriteDesc(width=32769, height=1, depth=16, planes=1, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    codes = harness.oracle_write(d, np.arange(32769, dtype=np.uint16).reshape(1, -1))[0].reshape(-1)
    return xi.code_preimages(codes, bits)


def _source16(code, end, bits):
    lo, hi = _preimages(bits)
    return np.where(np.asarray(end).astype(bool), hi[code], lo[code])


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("chroma,down", [("444", "box"), ("420", "box"), ("422", "nearest")])
def test_save_16bit_document_at_8bit_every_code_triple(gpu, chroma, down, phase):
    """RGB16 -> u8 planes: every 8-bit code triple, each channel at the smallest or the largest source value of its code (the two
    phases are complementary), BT.709."""
    p = xi.all_triples_444()
    ends = xi.ends_for_triples(p[0], p[1], p[2], phase)
    src = xi.interleaved({k: _source16(p[k], ends[k], 8) for k in range(3)})
    assert src.dtype == np.uint16 and int(src.max()) == 32768
    d = pkg.WriteDesc(width=4096, height=4096, depth=16, planes=3, bit_depth=8, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
                      chroma=CHROMA[chroma], chroma_downsampling=DOWN[down], **BT709)
    kernel = ("write_rgb16_ycbcr444_hot<", ",to8>") if chroma == "444" else f"write_rgb16_ycbcr_sub_hot<ys={xi.sub_shifts(chroma)[1]},to8>"
    _save_both_ways(gpu, d, src, kernel, what=(chroma, down, phase))


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("bits", [8, 10, 12])
def test_save_16bit_document_every_sample_value_in_each_channel(gpu, bits, planes):
    """RGB16 / RGBA16 (straight alpha) under the GBR matrix: the planes ARE the rescaled codes, so every 16-bit sample value -- the
    over-range ones above 32768 included -- is seen in every channel position of the 4:4:4 streaming kernels and of write_px."""
    src = xi.every_u16_in_each_channel(planes)
    d = pkg.WriteDesc(width=256, height=256, depth=16, planes=planes, bit_depth=bits, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444,
                      alpha_state=pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE, **GBR)
    want = _save_both_ways(gpu, d, src, "write_rgb16_ycbcr444_hot<" if planes == 3 else "write_rgba16_ycbcra444_hot", what=(bits, planes))
    # ... and the oracle's planes are what this test says they are: plane <- rescale(min(sample, 32768)) of its channel
    d1 = pkg.WriteDesc(width=32769, height=1, depth=16, planes=1, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    codes = harness.oracle_write(d1, np.arange(32769, dtype=np.uint16).reshape(1, -1))[0].reshape(-1)
    px = np.minimum(src.reshape(256, 256, planes), 32768)
    for pl, ch in ((0, 1), (1, 2), (2, 0)) + (((3, 3),) if planes == 4 else ()):        # Y <- G, Cb <- B, Cr <- R, A <- A
        assert np.array_equal(want[pl], codes[px[..., ch]]), (pl, ch)


# ---- integer premultiply: every (colour code, alpha code) pair ------------------------------------------------------------------------
def _pair_document(bits, depth, channels):
    """An n x n document whose pixel (row, col) has alpha code `row` and colour codes derived from `col`: 'gray' (one channel),
    'rgb-spread' (R = col, G and B shifted by a third and two thirds of the range: every channel meets every pair) or 'rgb-equal'
    (R = G = B = col).  16-bit documents carry, for every code, the smallest or the largest source value that rescales to it --
    the colour's end chosen by the alpha code's parity and the other way round."""
    n = 1 << bits
    code, alpha = xi.pairs(bits)
    code, alpha = code.astype(np.int64), alpha.astype(np.int64)
    if channels == "gray":
        cols = [code]
    elif channels == "rgb-spread":
        cols = [code, (code + n // 3) % n, (code + 2 * (n // 3)) % n]
    else:
        cols = [code, code, code]
    if depth == 8:
        assert bits == 8
        chans = [c.astype(np.uint8) for c in cols] + [alpha.astype(np.uint8)]
    else:
        chans = [_source16(c, alpha & 1, bits) for c in cols] + [_source16(alpha, code & 1, bits)]
    return xi.interleaved(dict(enumerate(chans)), tuple(range(len(chans)))), cols, alpha


PREMUL_CASES = []
for _bits in (8, 10, 12):
    _to8 = _bits == 8
    # Gray16 + alpha -> Y and Alpha planes: write_ga_stream writes u16 planes; at 8 bit the generic kernel is the only one
    PREMUL_CASES.append((f"ga16-b{_bits}", _bits, 16, "gray", dict(planes=2), None if _to8 else "write_ga_stream<depth=16>"))
    PREMUL_CASES.append((f"rgba16-ref-b{_bits}", _bits, 16, "rgb-spread", dict(planes=4, output=pkg.OUT_REFERENCE),
                         "write_int_ref_stream<depth=16,planes=4,"))
    PREMUL_CASES.append((f"rgba16-444-gbr-b{_bits}", _bits, 16, "rgb-spread", dict(planes=4, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **GBR),
                         "write_rgba16_ycbcra444_hot"))
    # a GBR save is 4:4:4 by definition: the sub-sampled kernel gets gray pixels under BT.709, whose luma is the premultiplied code
    for _chroma, _ys in (("422", 0), ("420", 1)):
        PREMUL_CASES.append((f"rgba16-{_chroma}-b{_bits}", _bits, 16, "rgb-equal",
                             dict(planes=4, output=pkg.OUT_YCBCR, chroma=CHROMA[_chroma], **BT709), f"write_rgba16_ycbcra_sub_hot<ys={_ys},"))
PREMUL_CASES.append(("rgba8-ref-b8", 8, 8, "rgb-spread", dict(planes=4, output=pkg.OUT_REFERENCE), "write_int_ref_stream<depth=8,planes=4,"))
PREMUL_CASES.append(("rgba8-444-gbr-b8", 8, 8, "rgb-spread", dict(planes=4, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **GBR),
                     "write_rgba8_ycbcra_hot<xs=0,ys=0,"))
PREMUL_CASES.append(("rgba8-420-b8", 8, 8, "rgb-equal", dict(planes=4, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT709),
                     "write_rgba8_ycbcra_hot<xs=1,ys=1,"))


@pytest.mark.parametrize("alpha_state", [pkg.ALPHA_PREMULTIPLIED, pkg.ALPHA_STRAIGHT], ids=["premultiplied", "straight"])
@pytest.mark.parametrize("cid,bits,depth,channels,kw,kernel", PREMUL_CASES, ids=[c[0] for c in PREMUL_CASES])
def test_save_every_colour_alpha_pair(gpu, cid, bits, depth, channels, kw, kernel, alpha_state):
    src, cols, alpha = _pair_document(bits, depth, channels)
    n = 1 << bits
    d = pkg.WriteDesc(width=n, height=n, depth=depth, bit_depth=bits, alpha_state=alpha_state, **kw)
    if cid == "rgba8-ref-b8" and alpha_state == pkg.ALPHA_STRAIGHT:
        kernel = "write_copy_rows_stream<planes=4>"                      # nothing to premultiply, nothing to rescale: the hand-off is a copy
    if kernel and kernel.startswith("write_rgba8_ycbcra_hot"):
        kernel = (kernel, f"premultiply={int(alpha_state == pkg.ALPHA_PREMULTIPLIED)}>")
    want = _save_both_ways(gpu, d, src, kernel, what=(cid, alpha_state))
    # what the oracle's planes must show here, stated independently: the alpha plane is a copy of the alpha codes; with straight alpha
    # the colours are untouched; premultiplied colours are 0 under alpha 0 and the colour itself under opaque alpha
    if d.output == pkg.OUT_REFERENCE and d.planes == 4:
        px = want[0].reshape(n, n, 4).astype(np.int64)
        out_cols, out_alpha = [px[..., k] for k in range(3)], px[..., 3]
    elif d.planes == 2:
        out_cols, out_alpha = [want[0].astype(np.int64)], want[3].astype(np.int64)
    elif d.matrix_coefficients == pkg.MATRIX_RGB_GBR:
        out_cols, out_alpha = [want[2].astype(np.int64), want[0].astype(np.int64), want[1].astype(np.int64)], want[3].astype(np.int64)
    else:
        out_cols, out_alpha = [want[0].astype(np.int64)], want[3].astype(np.int64)          # gray pixels: luma of (c, c, c)
        cols = cols[:1]
    assert np.array_equal(out_alpha, alpha)
    for got_c, c in zip(out_cols, cols):
        if alpha_state == pkg.ALPHA_STRAIGHT:
            assert np.array_equal(got_c, c)
        else:
            assert not got_c[0].any() and np.array_equal(got_c[n - 1], c[n - 1])
            assert np.all(got_c <= c)
