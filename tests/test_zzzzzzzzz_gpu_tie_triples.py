"""10- / 12-bit opens and saves against the oracle on NEAR-TIE triples, bit for bit (no tolerance anywhere).

The whole-domain tests (tests/test_zz_gpu_whole_domain_read.py, tests/test_zz_gpu_whole_domain_write.py) enumerate all 2^24 8-bit
triples; at 10 and 12 bit they stop at code pairs, and G of an open as well as Y, Cb and Cr of a save depend on all three codes.  A
kernel whose route to the oracle's bits is one ulp off changes a code only where the exact value is about one float32 spacing from the
point at which the final truncation jumps.  tests/tie_inputs.py hunts that point: for EVERY (Cb, Cr) pair the Y -- and for every
(R, B) pair the G -- that puts the pixel next to a tie.  tests/test_zzzzzzzz_tie_inputs.py counts what the documents hold, how near the
ties they are and what two one-ulp mutants change on them (about 300 times what they change on the Latin square); the oracle is held
to a numpy restatement of the reference on every one of these documents there.

  opens to the 16-bit host   10 and 12 bit; 4:4:4, 4:2:2 (two near-ties per pair), 4:2:0 (four); four matrices, both ranges; without
                             alpha (4:4:4 full range is table-free) and with straight alpha (tabled); premultiplied alpha under BT.709 and
                             latin_alpha; contiguous planes, at 10 bit also odd pitches (the unaligned instantiation); IEEE division
                             (tuning bit 128) on the 12-bit 4:4:4 BT.709 document
  saves to 10 and 12 bit     four matrices; the hunts for Y, Cb and Cr side by side in one document, every pixel replicated over its
                             chroma footprint.  RGB16 4:4:4, 4:2:2 nearest, 4:2:0 box and RGBA16 (straight alpha) 4:4:4, 4:2:0, each
                             code at either end of its source interval (two phases); RGB f32 under PQ 4:4:4 (the headline kernel) and
                             4:2:2, RGBA f32 (straight alpha) 4:4:4 and 4:2:0, RGB f32 under Clip 4:4:4 -- their floats sit in the middle
                             of each code's interval, so stage A is exact (asserted on the oracle) and stage B is what is compared

Each save runs the streaming kernel the dispatcher picks AND the generic write_px against ONE oracle run; every case asserts the
kernel form from the launch label.  Sizes are the Latin square's.  The file is named to be collected after every earlier test.
"""
import numpy as np
import pytest

import exhaustive_inputs as xi
import harness
import tie_documents as td
from test_zz_gpu_whole_domain_read import DEFAULT_VARIANT, ODD_PAD, _open_and_compare, _ycc_desc
from test_zz_gpu_whole_domain_write import _save_both_ways

pkg = harness.pkg
pytestmark = pytest.mark.gpu

CHROMA = {"444": pkg.CHROMA_444, "422": pkg.CHROMA_422, "420": pkg.CHROMA_420}
DOWN = {"box": pkg.DOWNSAMPLE_AVERAGE, "nearest": pkg.DOWNSAMPLE_NEAREST}


# ---- opens ------------------------------------------------------------------------------------------------------------------------
# (the parameter named first varies fastest: the three chroma forms of one hunt follow each other and share it)
@pytest.mark.parametrize("chroma", ["444", "422", "420"])
@pytest.mark.parametrize("fr", [1, 0], ids=["full", "limited"])
@pytest.mark.parametrize("name,matrix,primaries", td.MATRICES, ids=td.MATRIX_IDS)
@pytest.mark.parametrize("bits", [10, 12])
def test_open_tie_triples_16bit_host(gpu, bits, name, matrix, primaries, fr, chroma):
    """Every (Cb, Cr) pair under the Y nearest a rounding tie of G (each footprint position under a near-tie of its own): without alpha
    and with straight alpha.  _open_and_compare asserts the kernel form (name, aligned=, tables=none, flat) of every launch."""
    planes = td.open_document(bits, matrix, primaries, fr, chroma)
    pads = (0, ODD_PAD) if bits == 10 else (0,)
    d = _ycc_desc(planes, chroma, bits, 16, matrix, fr, primaries=primaries)
    _open_and_compare(gpu, d, planes, harness.oracle_read(d, planes), pads=pads, what=(bits, chroma, name, fr, "opaque"))
    with_alpha = dict(planes)
    with_alpha[3] = xi.latin_alpha(bits, planes[0].shape)
    d = _ycc_desc(planes, chroma, bits, 16, matrix, fr, alpha=pkg.ALPHA_STRAIGHT, primaries=primaries)
    _open_and_compare(gpu, d, with_alpha, harness.oracle_read(d, with_alpha), pads=pads, what=(bits, chroma, name, fr, "straight alpha"))


@pytest.mark.parametrize("chroma", ["444", "422", "420"])
@pytest.mark.parametrize("fr", [1, 0], ids=["full", "limited"])
@pytest.mark.parametrize("bits", [10, 12])
def test_open_tie_triples_premultiplied_alpha(gpu, bits, fr, chroma):
    """BT.709 under latin_alpha (every alpha code, 0 and opaque among them, in every row and column): the near-tie G goes through the
    float unpremultiply."""
    planes = dict(td.open_document(bits, pkg.MATRIX_BT709, pkg.PRIMARIES_BT709, fr, chroma))
    planes[3] = xi.latin_alpha(bits, planes[0].shape)
    d = _ycc_desc(planes, chroma, bits, 16, pkg.MATRIX_BT709, fr, alpha=pkg.ALPHA_PREMULTIPLIED)
    _open_and_compare(gpu, d, planes, harness.oracle_read(d, planes), pads=(0, ODD_PAD) if bits == 10 else (0,), what=(bits, chroma, fr))


def test_open_tie_triples_with_ieee_division(gpu):
    """Tuning bit 128 (x / kg stays an IEEE division) on the 12-bit 4:4:4 BT.709 document, both ranges."""
    variant = DEFAULT_VARIANT | 128
    try:
        gpu.lib.avifgpu_set_hot_variant(variant)
        for fr in (1, 0):
            planes = td.open_document(12, pkg.MATRIX_BT709, pkg.PRIMARIES_BT709, fr, "444")
            d = _ycc_desc(planes, "444", 12, 16, pkg.MATRIX_BT709, fr)
            _open_and_compare(gpu, d, planes, harness.oracle_read(d, planes), pads=(0,), variant=variant, what=("ieee", fr))
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)


# ---- saves ------------------------------------------------------------------------------------------------------------------------
PQ, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_CLIP
# (id, document depth, planes, chroma, downsampling, transfer, the streaming kernel's label: its beginning or (beginning, a part))
SAVE_FORMS = [
    ("rgb16-444", 16, 3, "444", "box", CLIP, "write_rgb16_ycbcr444_hot<"),
    ("rgb16-422-nearest", 16, 3, "422", "nearest", CLIP, "write_rgb16_ycbcr_sub_hot<ys=0>"),
    ("rgb16-420-box", 16, 3, "420", "box", CLIP, "write_rgb16_ycbcr_sub_hot<ys=1>"),
    ("rgba16-444", 16, 4, "444", "box", CLIP, "write_rgba16_ycbcra444_hot"),
    ("rgba16-420-box", 16, 4, "420", "box", CLIP, "write_rgba16_ycbcra_sub_hot<ys=1,nearest=0>"),
    ("rgb32-pq-444", 32, 3, "444", "box", PQ, f"write_rgb32_ycbcr444_hot<transfer={PQ},"),
    ("rgb32-pq-422-box", 32, 3, "422", "box", PQ, f"write_rgb32_ycbcr_sub_hot<transfer={PQ},xs=1,ys=0>"),
    ("rgba32-pq-444", 32, 4, "444", "box", PQ, f"write_rgba32_ycbcra444_hot<transfer={PQ}>"),
    ("rgba32-pq-420-box", 32, 4, "420", "box", PQ, f"write_rgba32_ycbcra_sub_hot<transfer={PQ},xs=1,ys=1,nearest=0>"),
    ("rgb32-clip-444", 32, 3, "444", "box", CLIP, f"write_rgb32_ycbcr444_hot<transfer={CLIP},"),
]


# (the forms of one matrix follow each other: they share its hunts)
@pytest.mark.parametrize("form,depth,planes,chroma,down,transfer,kernel", SAVE_FORMS, ids=[f[0] for f in SAVE_FORMS])
@pytest.mark.parametrize("name,matrix,primaries", td.MATRICES, ids=td.MATRIX_IDS)
@pytest.mark.parametrize("bits", [10, 12])
def test_save_tie_triples(gpu, bits, name, matrix, primaries, form, depth, planes, chroma, down, transfer, kernel):
    """For every (R, B) pair the G nearest a rounding tie of Y, of Cb and of Cr, as the codes stage B is given."""
    codes = td.save_codes(bits, matrix, primaries, chroma)
    h, w = codes[0].shape
    alpha = xi.latin_alpha(bits, (h, w)) if planes == 4 else None
    d = pkg.WriteDesc(width=w, height=h, depth=depth, planes=planes, bit_depth=bits, output=pkg.OUT_YCBCR, chroma=CHROMA[chroma],
                      chroma_downsampling=DOWN[down], alpha_state=pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE,
                      matrix_coefficients=matrix, color_primaries=primaries, transfer=transfer, peak_nits=td.PQ_PEAK)
    # stage A gives the intended codes: the whole document at 10 bit; at 12 bit every 16th row (rows are independent, and
    # tests/test_zzzzzzzz_tie_inputs.py shows every code of every channel to the oracle)
    rows = slice(None) if bits == 10 else slice(None, None, 16)
    part = tuple(np.ascontiguousarray(c[rows]) for c in codes)
    part_alpha = None if alpha is None else np.ascontiguousarray(alpha[rows])
    dpart = pkg.WriteDesc(width=w, height=part[0].shape[0], depth=depth, planes=planes, bit_depth=bits, alpha_state=d.alpha_state,
                          transfer=transfer, peak_nits=td.PQ_PEAK)
    for phase in ((0, 1) if depth == 16 else (0,)):
        build = (lambda c, a: td.rgb16_document(c, bits, phase, a)) if depth == 16 else (lambda c, a: td.f32_document(c, bits, transfer, a))
        td.stage_a_codes(dpart, build(part, part_alpha), part, part_alpha)
        want = _save_both_ways(gpu, d, build(codes, alpha), kernel, what=(bits, name, form, phase))
        if alpha is not None:
            assert np.array_equal(want[3], alpha)                        # straight alpha: the plane is the alpha codes, colours untouched
