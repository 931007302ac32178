"""Every grid-stride loop walked several times on tiles of a few thousand pixels.

A wave of a conversion kernel takes span s, then s + gridDim.x * waves per workgroup, and so on to the end of the tile; the grids are
capped by compile-time constants that only frames of hundreds of megapixels reach, so without help the second trip of most loops
never runs in a test.  Bits 8.. of the tuning word (avifgpu_set_hot_variant; csrc/kernel_params.h) lower the grid of every capped
launch, and the launch label then carries " cap=N/M": N workgroups launched where one trip per wave takes M.

Caps.  1: ONE workgroup walks the whole tile: its stride (2, 4 or 8 spans) is no multiple of the three spans of a row, so a wave meets
whole and ragged spans (global-load and buffer-resource paths) in turn, and its waves leave the loop after different trip counts.
3: several workgroups, whose stride IS a multiple of a row's spans: a wave stays in one column of spans, the ragged one included, and
walks down the rows (a FLAT launch has no rows: there the spans just follow each other).  Every capped launch is asserted from its
label to have N == cap and M >= 3 N: every wave of the grid makes at least three trips.

Geometry.  Widths: two whole spans of the kernel under test plus a ragged tail it still accepts (1064 = 2 x 512 + 40 where whole
8-pixel groups are wanted, 2088 for the 1024-pixel spans of the RGB8 kernels, 1061 / 549 where any width is taken; 1072 where a
4:2:2 tile is to be contiguous, i.e. FLAT, in the test's 16-byte aligned buffers); three per-wave chunks plus a tail for the
elementwise kernels.  Heights are odd, so that the replicated last chroma row of 4:2:0 falls on a late trip, and each case runs as the
whole frame and as an inner row tile from row 2 with rows_to_end != nrows (an even number of rows for 4:2:0, which the C-ABI asks of
every tile that does not end the image).  M >= 3 N decides the heights: workgroups are 2 to 8 waves, so a frame of 9 rows holds
fewer than 9 workgroups' worth of spans (and its 5-row tile fewer than 3 for the 4-wave f32 kernels); 15 rows (tile: 11 / 10) serve
cap 1, 39 rows (35 / 34) cap 3, and the generic kernels, whose workgroups of 256 or 512 lanes take up to 16 pixels a lane, 45 and 133.
Each case runs with contiguous rows (the FLAT launch where one exists: asserted) and with padded rows (launched row by row).

Judgement -- no new numbers.  The raw output of the capped launch, padding included, equals that of the same call with bits 8.. zero
byte for byte (include/avifgpu.h promises it for every value of the word) and the padding keeps its fill; and against the CPU oracle:
integer documents and integer opens equal, 32-bit saves |delta code| <= 1 and harness.T2_MIN_EXACT (behind a profile: the real lcms2
and harness.T2_MIN_EXACT_ICC), 32-bit opens rtol 1e-4 / atol 1e-9 (the bar of tests/test_gpu_read.py).

The byte movers (orient_rows, orient_transpose, crop_rows) wrap grid.y at 65 535 rows / tiles inside the kernel: the last three tests
feed them more than that through their probes, against numpy's own move of the bytes.

(The file's name makes it the last one collected: the tests of the suite keep their places in the collection order.)"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import harness
import icc_profiles as ip
from orientation_truth import orient
from test_gpu_kernel_equivalence import BT2020
from test_gpu_light_level import write_hist

pkg = harness.pkg
pytestmark = pytest.mark.gpu

DEFAULT_WORD = 1 | 2 | 4
STREAM_WORD = 1 | 2 | 4 | 8              # bit 3: the streaming kernels that the default takes for large frames only
CAPS = (1, 3)
# family -> cap -> (height, (row0, nrows) of the inner tile, the same for 4:2:0): see "Geometry" above
GEOMETRY = {"stream": {1: (15, (2, 11), (2, 10)), 3: (39, (2, 35), (2, 34))},
            "px": {1: (45, (2, 41), (2, 40)), 3: (133, (2, 129), (2, 128))}}
BT709 = dict(matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709)
BT601 = dict(matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709)
PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP
REF, YCC = pkg.OUT_REFERENCE, pkg.OUT_YCBCR
C444, C422, C420 = pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420
NEAREST = dict(chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
STRAIGHT, PREMUL = dict(alpha_state=pkg.ALPHA_STRAIGHT), dict(alpha_state=pkg.ALPHA_PREMULTIPLIED)
ICC_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "liboracle_icc.so")
SENTINEL = 0xA5


def cap_of(label):
    """(N, M) of a label's " cap=N/M", or None."""
    m = re.search(r" cap=(\d+)/(\d+)", label)
    return (int(m.group(1)), int(m.group(2))) if m else None


def check_capped_label(label, base_label, kernel, cap):
    """The capped launch is the uncapped one (same kernel, same FLAT decision) with " cap=N/M" in front of " flat": N == cap, M >= 3 N."""
    assert kernel in label, (kernel, label)
    assert cap_of(base_label) is None, base_label
    got = cap_of(label)
    assert got is not None, (label, "the word did not lower this grid")
    assert got[0] == cap and got[1] >= 3 * cap, (label, "every wave must make at least three trips")
    assert re.sub(r" cap=\d+/\d+", "", label) == base_label, (label, base_label)
    if " flat" in label:
        assert label.endswith(" flat"), label


def expect_flat(d, kernel, word, nrows, stride_pad):
    """launch_write's FLAT rule (and the copy kernel's own), restated: rows that do not depend on where a row ends, contiguous on both
    sides.  harness allocates plane rows of a multiple of 16 bytes, so a plane is contiguous where its row is one."""
    if stride_pad or not (word & 1) or (word & 16) or nrows <= 1:
        return False
    ssz = 2 if d.bit_depth > 8 else 1
    contiguous = all((w * ssz) % 16 == 0 for w, _, _ in harness.write_planes(d).values())
    if kernel == "write_copy_rows_stream":
        return contiguous
    xs, ys = harness.chroma_shift(d.chroma) if d.output == YCC else (0, 0)
    return contiguous and d.planes >= 3 and d.depth in (16, 32) and ys == 0 and (xs == 0 or d.width % 2 == 0)


def walk_write(gpu, kernel, kw, cap, word, family, pad, icc=None, oracle_rows=None, min_exact=None, make_source=None, label_has=()):
    """One descriptor under one cap: whole frame and inner tile, contiguous and padded rows; see the module's docstring."""
    height, tile, tile420 = GEOMETRY[family][cap]
    d = pkg.WriteDesc(**dict(kw, height=height))
    ys = harness.chroma_shift(d.chroma)[1] if (d.output == YCC and d.planes >= 3) else 0
    src = make_source(d) if make_source else harness.make_write_source(d, seed=31)
    rows = oracle_rows(d, src) if oracle_rows else src
    fill = 0xA5A5 if d.bit_depth > 8 else 0xA5
    for row0, nrows in ((0, height), tile420 if ys else tile):
        for stride_pad in (0, pad):
            try:
                gpu.lib.avifgpu_set_hot_variant(word)
                base = harness.gpu_write(gpu, d, src, row0=row0, nrows=nrows, stride_pad=stride_pad, return_raw=True, icc=icc)
                base_label = gpu.last_kernel()
                gpu.lib.avifgpu_set_hot_variant(word | (cap << 8))
                got = harness.gpu_write(gpu, d, src, row0=row0, nrows=nrows, stride_pad=stride_pad, return_raw=True, icc=icc)
                label = gpu.last_kernel()
            finally:
                gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
            what = (label, row0, nrows, stride_pad)
            check_capped_label(label, base_label, kernel, cap)
            for s in label_has:
                assert s in label, (s, label)
            if family == "px":
                assert ("aligned=1" in label) == (stride_pad == 0), what       # an odd pad: the unaligned instantiation
            assert (" flat" in label) == expect_flat(d, kernel, word, nrows, stride_pad), what
            # the capped launch writes the bytes of the uncapped one, and nothing else
            for pl, (w, _, _) in harness.write_planes(d).items():
                assert np.array_equal(got[pl], base[pl]), (what, pl, np.argwhere(got[pl] != base[pl])[:4].tolist())
                assert (got[pl][:, w:] == fill).all(), (what, pl, "padding")
            # ... and they are the oracle's
            want = harness.oracle_write(d, rows, row0=row0, nrows=nrows)
            trimmed = harness._trim(d, got, nrows, harness.write_planes)
            if d.depth != 32:
                for pl in want:
                    assert np.array_equal(trimmed[pl], want[pl]), (what, pl, np.argwhere(trimmed[pl] != want[pl])[:4].tolist())
                print(f"{label} rows {row0}+{nrows} pad {stride_pad}: equal")
            else:
                st = harness.compare_write(d, want, trimmed)
                print(f"{label} rows {row0}+{nrows} pad {stride_pad}: exact {st['exact_frac']:.5f} max {st['max_abs']}")
                assert st["max_abs"] <= 1, (what, st)
                assert harness.t2_exact_ok(st, min_exact or harness.T2_MIN_EXACT[d.bit_depth]), (what, st)


# ---- the streaming write kernels ------------------------------------------------------------------------------------------------
def f32(width, planes, bits, transfer, output, chroma=C444, peak=1000, **kw):
    return dict(width=width, depth=32, planes=planes, bit_depth=bits, transfer=transfer, peak_nits=peak, output=output, chroma=chroma, **BT2020, **kw)


def i16(width, planes, bits, output, chroma=C444, **kw):
    return dict(width=width, depth=16, planes=planes, bit_depth=bits, output=output, chroma=chroma, **kw)


def i8(width, planes, bits, output, chroma=C444, **kw):
    return dict(width=width, depth=8, planes=planes, bit_depth=bits, output=output, chroma=chroma, **kw)


COMPACT, CLOSE = dict(pq_evaluation=pkg.PQ_COMPACT), dict(pq_evaluation=pkg.PQ_CLOSE)
PXL4_WORD = 1 | 4 | 8                    # the headline kernel with 4 pixels a lane: spans of 256 pixels
# (kernel, word, descriptor without its height)
STREAM_CASES = [
    # the headline kernel: both lane widths; 1061 -- whole spans on the global-load path and a ragged one through the buffer resource in
    # turn within one wave -- and 1064, whose contiguous tile is FLAT; every curve, PQ in both forms
    ("write_rgb32_ycbcr444_hot", STREAM_WORD, f32(1061, 3, 10, PQ, YCC, **COMPACT)),
    ("write_rgb32_ycbcr444_hot", STREAM_WORD, f32(1064, 3, 12, PQ, YCC, peak=80, **CLOSE)),
    ("write_rgb32_ycbcr444_hot", STREAM_WORD, f32(1061, 3, 10, HLG, YCC)),
    ("write_rgb32_ycbcr444_hot", STREAM_WORD, f32(1064, 3, 12, S428, YCC)),
    ("write_rgb32_ycbcr444_hot", STREAM_WORD, f32(1061, 3, 12, CLIP, YCC)),
    ("write_rgb32_ycbcr444_hot", PXL4_WORD, f32(549, 3, 10, PQ, YCC, **CLOSE)),
    ("write_rgb32_ycbcr444_hot", PXL4_WORD, f32(552, 3, 12, CLIP, YCC)),
    # RGB f32, sub-sampled chroma: the rotated loop (the next span's loads behind this span's stores); ys = 1 replicates the last image row
    ("write_rgb32_ycbcr_sub_hot", STREAM_WORD, f32(1061, 3, 12, PQ, YCC, C420, **COMPACT)),
    ("write_rgb32_ycbcr_sub_hot", STREAM_WORD, f32(1064, 3, 10, PQ, YCC, C420, **CLOSE, **NEAREST)),
    ("write_rgb32_ycbcr_sub_hot", STREAM_WORD, f32(1072, 3, 10, HLG, YCC, C422)),
    ("write_rgb32_ycbcr_sub_hot", STREAM_WORD, f32(1072, 3, 12, S428, YCC, C422, **NEAREST)),
    ("write_rgb32_ycbcr_sub_hot", STREAM_WORD, f32(1061, 3, 12, CLIP, YCC, C420)),
    # RGBA f32: spans of 256 pixels
    ("write_rgba32_ycbcra_sub_hot", STREAM_WORD, f32(549, 4, 12, PQ, YCC, C420, **CLOSE, **PREMUL)),
    ("write_rgba32_ycbcra_sub_hot", STREAM_WORD, f32(560, 4, 10, HLG, YCC, C422, **STRAIGHT, **NEAREST)),
    ("write_rgba32_ycbcra_sub_hot", STREAM_WORD, f32(549, 4, 10, PQ, YCC, C420, **COMPACT, **STRAIGHT, **NEAREST)),
    ("write_rgba32_ycbcra_sub_hot", STREAM_WORD, f32(552, 4, 12, CLIP, YCC, C422, **PREMUL)),
    ("write_rgba32_ycbcra444_hot", STREAM_WORD, f32(549, 4, 12, PQ, YCC, **CLOSE, **PREMUL)),
    ("write_rgba32_ycbcra444_hot", STREAM_WORD, f32(552, 4, 10, S428, YCC, **STRAIGHT)),
    # RGB16 / RGBA16: u16 planes and the `to8` forms
    ("write_rgb16_ycbcr444_hot", STREAM_WORD, i16(1064, 3, 12, YCC, **BT2020)),
    ("write_rgb16_ycbcr444_hot", STREAM_WORD, i16(1072, 3, 8, YCC, **BT601)),
    ("write_rgb16_ycbcr_sub_hot", STREAM_WORD, i16(1064, 3, 12, YCC, C420, **BT2020)),
    ("write_rgb16_ycbcr_sub_hot", STREAM_WORD, i16(1064, 3, 10, YCC, C420, **BT601, **NEAREST)),
    ("write_rgb16_ycbcr_sub_hot", STREAM_WORD, i16(1072, 3, 10, YCC, C422, **BT709)),
    ("write_rgb16_ycbcr_sub_hot", STREAM_WORD, i16(1064, 3, 8, YCC, C420, **BT709)),
    ("write_rgba16_ycbcra444_hot", STREAM_WORD, i16(1064, 4, 12, YCC, **BT2020, **PREMUL)),
    ("write_rgba16_ycbcra444_hot", STREAM_WORD, i16(1072, 4, 8, YCC, **BT601, **STRAIGHT)),
    ("write_rgba16_ycbcra_sub_hot", STREAM_WORD, i16(1064, 4, 10, YCC, C420, **BT709, **STRAIGHT)),
    ("write_rgba16_ycbcra_sub_hot", STREAM_WORD, i16(1072, 4, 12, YCC, C422, **BT2020, **PREMUL, **NEAREST)),
    ("write_rgba16_ycbcra_sub_hot", STREAM_WORD, i16(1064, 4, 8, YCC, C420, **BT601, **PREMUL, **NEAREST)),
    # RGB8 -> u8 / u16 planes: spans of 1024 pixels
    ("write_rgb8_ycbcr_hot", STREAM_WORD, i8(2088, 3, 8, YCC, C420, **BT709)),
    ("write_rgb8_ycbcr_hot", STREAM_WORD, i8(2088, 3, 8, YCC, C420, **BT601, **NEAREST)),
    ("write_rgb8_ycbcr_hot", STREAM_WORD, i8(2088, 3, 8, YCC, C422, **BT601, **NEAREST)),
    ("write_rgb8_ycbcr_hot", STREAM_WORD, i8(2088, 3, 8, YCC, C444, **BT2020)),
    ("write_rgb8_ycbcr16_hot", STREAM_WORD, i8(2088, 3, 10, YCC, C420, **BT709)),
    ("write_rgb8_ycbcr16_hot", STREAM_WORD, i8(2088, 3, 12, YCC, C420, **BT601, **NEAREST)),
    ("write_rgb8_ycbcr16_hot", STREAM_WORD, i8(2088, 3, 12, YCC, C422, **BT709)),
    ("write_rgb8_ycbcr16_hot", STREAM_WORD, i8(2088, 3, 10, YCC, C444, **BT2020)),
    ("write_rgba8_ycbcra_hot", STREAM_WORD, i8(1064, 4, 8, YCC, C420, **BT601, **PREMUL)),
    ("write_rgba8_ycbcra_hot", STREAM_WORD, i8(1064, 4, 8, YCC, C422, **BT709, **STRAIGHT, **NEAREST)),
    ("write_rgba8_ycbcra_hot", STREAM_WORD, i8(1064, 4, 8, YCC, C444, **BT2020, **PREMUL)),
    # the elementwise kernels: three of a wave's chunks and a ragged tail a row (1024 samples, 4 KiB, 256 gray + alpha pairs, 2 KiB)
    ("write_f32_ref_stream", STREAM_WORD, f32(1040, 3, 10, PQ, REF, peak=80, **CLOSE)),
    ("write_f32_ref_stream", STREAM_WORD, f32(780, 4, 12, CLIP, REF, **PREMUL)),
    ("write_f32_ref_stream", STREAM_WORD, dict(width=3108, depth=32, planes=1, bit_depth=12, transfer=PQ, peak_nits=1000, **COMPACT)),
    ("write_ga_stream", STREAM_WORD, dict(width=3108, depth=16, planes=2, bit_depth=12, **PREMUL)),
    ("write_ga_stream", STREAM_WORD, dict(width=3108, depth=16, planes=2, bit_depth=10, **STRAIGHT)),
    ("write_ga_stream", STREAM_WORD, dict(width=1554, depth=32, planes=2, bit_depth=10, transfer=PQ, peak_nits=80, **CLOSE, **PREMUL)),
    ("write_ga_stream", STREAM_WORD, dict(width=1554, depth=32, planes=2, bit_depth=12, transfer=CLIP, **STRAIGHT)),
    ("write_int_ref_stream", STREAM_WORD, i16(2056, 3, 12, REF)),
    ("write_int_ref_stream", STREAM_WORD, i16(1544, 4, 8, REF, **PREMUL)),
    ("write_int_ref_stream", STREAM_WORD, i8(3084, 4, 8, REF, **PREMUL)),
    ("write_int_ref_stream", STREAM_WORD, dict(width=6168, depth=16, planes=1, bit_depth=10)),
    ("write_copy_rows_stream", STREAM_WORD, i8(2064, 3, 8, REF)),
    ("write_copy_rows_stream", STREAM_WORD, i8(1545, 4, 8, REF, **STRAIGHT)),
    ("write_copy_rows_stream", STREAM_WORD, dict(width=6192, depth=8, planes=1, bit_depth=8)),
]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kernel,word,kw", STREAM_CASES, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(STREAM_CASES)])
def test_streaming_kernel_walks_its_loop(gpu, kernel, word, kw, cap):
    has = (f"pxl={8 if word & 2 else 4},",) if kernel == "write_rgb32_ycbcr444_hot" else ()        # both lane widths of the headline kernel
    walk_write(gpu, kernel, kw, cap, word, "stream", pad=16, label_has=has)


# ---- the streaming kernels behind a document profile: icc = 1, 2, 4 against the real lcms2 ---------------------------------------------
def _icc_cases():
    out = []
    for icc, name, target, transfer in ((1, ip.LINEAR[1], ip.REC2020, PQ), (2, ip.CURVED[0], ip.REC2020, PQ), (4, ip.LINEAR[2], ip.SRGB, CLIP)):
        col = BT601 if target == ip.SRGB else BT2020
        base = dict(depth=32, bit_depth=12, transfer=transfer, peak_nits=1000, **col)
        out += [(icc, name, target, "write_rgb32_icc1_ycbcr444_hot", dict(base, width=1064, planes=3, output=YCC, chroma=C444)),
                (icc, name, target, "write_rgb32_icc1_ycbcr444_hot", dict(base, width=1064, planes=3, output=REF, bit_depth=10)),
                (icc, name, target, "write_rgb32_ycbcr_sub_hot", dict(base, width=1061, planes=3, output=YCC, chroma=C420)),
                (icc, name, target, "write_rgba32_ycbcra444_hot", dict(base, width=549, planes=4, output=YCC, chroma=C444, **STRAIGHT))]
    return out


ICC_CASES = _icc_cases()


def _lcms_rows(name, target):
    def rows(d, src):
        return ip.lcms_rows(name, target, src, d.width, d.planes)
    return rows


def _icc_source(name):
    def make(d):
        src = harness.make_write_source(d, seed=31)
        return np.abs(src) if name in ip.CURVED else src          # non-linear curves: where every lcms2 build agrees (tests/test_gpu_icc.py)
    return make


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("icc,name,target,kernel,kw", ICC_CASES, ids=[f"icc{c[0]}-{c[3]}-{i}" for i, c in enumerate(ICC_CASES)])
def test_streaming_icc_kernel_walks_its_loop(gpu, icc, name, target, kernel, kw, cap):
    if ip.lcms() is None:
        pytest.skip(ip.NO_LCMS)
    has = (f"icc={icc}",) + (("out=ref",) if kw["output"] == REF else ())
    walk_write(gpu, kernel, kw, cap, STREAM_WORD, "stream", pad=16, icc=ip.prepared(name, target), oracle_rows=_lcms_rows(name, target),
               min_exact=harness.T2_MIN_EXACT_ICC, make_source=_icc_source(name), label_has=has)


# ---- the generic kernel: word = cap << 8, low byte 0 ------------------------------------------------------------------------------------
def _px_cases():
    out = []
    for depth, bits in ((8, 8), (8, 10), (16, 12), (16, 8), (32, 10), (32, 12)):
        t = dict(transfer=PQ, peak_nits=1000, **COMPACT) if depth == 32 else {}
        base = dict(width=1072, depth=depth, bit_depth=bits, **t)
        if (depth, bits) in ((8, 8), (16, 12), (32, 10)):
            out += [dict(base, planes=1), dict(base, planes=2, **PREMUL), dict(base, planes=3, output=REF), dict(base, planes=4, output=REF, **PREMUL),
                    dict(base, planes=3, output=YCC, chroma=C444, **BT2020), dict(base, planes=3, output=YCC, chroma=C422, **BT709),
                    dict(base, planes=4, output=YCC, chroma=C420, **BT601, **STRAIGHT)]
        else:
            out += [dict(base, planes=2, **STRAIGHT), dict(base, planes=4, output=YCC, chroma=C444, **BT709, **PREMUL),
                    dict(base, planes=4, output=YCC, chroma=C422, **BT601, **STRAIGHT, **NEAREST),
                    dict(base, planes=3, output=YCC, chroma=C420, **BT2020, **NEAREST)]
    # PQ in its close form (kTransferPqHi: the exponent table copied to LDS per workgroup, AG_PQ_TABLE_BLOCK_CAP); HLG, SMPTE 428, Clip
    out += [dict(width=1072, depth=32, bit_depth=12, transfer=PQ, peak_nits=80, planes=1, **CLOSE),
            dict(width=1072, depth=32, bit_depth=10, transfer=PQ, peak_nits=1000, planes=3, output=YCC, chroma=C420, **BT2020, **CLOSE),
            dict(width=1072, depth=32, bit_depth=12, transfer=PQ, peak_nits=1000, planes=4, output=YCC, chroma=C444, **BT2020, **CLOSE, **PREMUL),
            dict(width=1072, depth=32, bit_depth=10, transfer=HLG, planes=3, output=YCC, chroma=C422, **BT2020),
            dict(width=1072, depth=32, bit_depth=12, transfer=S428, planes=3, output=REF),
            dict(width=1072, depth=32, bit_depth=10, transfer=CLIP, planes=4, output=YCC, chroma=C420, **BT2020, **STRAIGHT)]
    return out


PX_CASES = _px_cases()


def _px_id(kw):
    return f"d{kw['depth']}-b{kw['bit_depth']}-p{kw['planes']}-o{kw.get('output', 0)}-c{kw.get('chroma', 3)}-t{kw.get('transfer', CLIP)}-q{kw.get('pq_evaluation', 0)}"


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kw", PX_CASES, ids=[f"{_px_id(kw)}-{i}" for i, kw in enumerate(PX_CASES)])
def test_generic_write_kernel_walks_its_loop(gpu, kw, cap):
    has = ("transfer=4",) if kw.get("pq_evaluation") == pkg.PQ_CLOSE else ()
    walk_write(gpu, "write_px<", kw, cap, 0, "px", pad=3, label_has=has)


@functools.lru_cache(maxsize=None)
def _lcms_int():
    """The live lcms2 oracle's 8- and 16-bit row conversions and its A2B profiles (the fixtures of tests/test_icc8.py / test_icc16.py)."""
    if not os.path.exists(ICC_LIB):
        return None
    L = ctypes.CDLL(ICC_LIB)
    L.oracle_icc_make_profile.restype = ctypes.c_int32
    L.oracle_icc_make_profile.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32]
    L.oracle_icc_convert_rows_to_srgb8.restype = ctypes.c_int32
    L.oracle_icc_convert_rows_to_srgb8.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.oracle_icc_convert_rows_to_srgb16.restype = ctypes.c_int32
    L.oracle_icc_convert_rows_to_srgb16.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32,
                                                     ctypes.c_uint32, ctypes.c_uint32]
    for name in ("oracle_icc_convert_rows_to_rec2020", "oracle_icc_convert_rows_to_srgb_float"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.oracle_icc_make_a2b_profile.restype = ctypes.c_int32
    L.oracle_icc_make_a2b_profile.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]
    L.oracle_icc_transform8_open.restype = ctypes.c_void_p
    L.oracle_icc_transform8_open.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    L.oracle_icc_transform16_close.argtypes = [ctypes.c_void_p]
    return L


def _matrix_profile(L, kind, trc, g):
    buf = ctypes.create_string_buffer(1 << 18)
    n = L.oracle_icc_make_profile(kind, trc, g, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


def _px_icc_setup(gpu, n):
    """(descriptor, ICC argument of the write call, rows the oracle's pixel loop gets, source maker, exact-match bar) of the write_px<..., icc = n> case."""
    L = _lcms_int()
    hdr = dict(width=1072, depth=32, bit_depth=12, transfer=PQ, peak_nits=1000, **BT2020, **COMPACT)
    if n in (1, 2, 4, 6):
        name, target = {1: (ip.LINEAR[0], ip.REC2020), 2: (ip.CURVED[1], ip.REC2020), 4: (ip.CURVED[0], ip.SRGB), 6: (ip.TABLES[0], ip.REC2020)}[n]
        kw = {1: dict(hdr, planes=3, output=YCC, chroma=C444), 2: dict(hdr, planes=3, output=YCC, chroma=C420),
              4: dict(width=1072, depth=32, bit_depth=10, transfer=CLIP, planes=4, output=YCC, chroma=C422, **BT601, **STRAIGHT),
              6: dict(hdr, planes=4, output=YCC, chroma=C444, **PREMUL)}[n]
        make = (lambda d: np.abs(harness.make_write_source(d, seed=31))) if n != 1 else None
        return kw, ip.prepared(name, target), _lcms_rows(name, target), make, harness.T2_MIN_EXACT_ICC
    if n == 3:                                                      # an 8-bit document behind a matrix / TRC profile: lcms2's 8-bit matrix-shaper
        icc = _matrix_profile(L, 3, 0, 2.19921875)
        kw = dict(width=1072, depth=8, planes=3, bit_depth=8, output=YCC, chroma=C420, **BT601)
        xf, conv = gpu.icc_prepare_shaper8(icc), (lambda c, d: L.oracle_icc_convert_rows_to_srgb8(icc, len(icc), int(d.planes == 4), c.ctypes.data, d.width, d.height, c.strides[0]))
        make = None
    elif n == 5:                                                    # a 16-bit document: the 33^3 table
        icc = _matrix_profile(L, 2, 0, 1.8)
        kw = dict(width=1072, depth=16, planes=3, bit_depth=12, output=YCC, chroma=C444, **BT601)
        xf, conv = gpu.icc_prepare_clut16(icc), (lambda c, d: L.oracle_icc_convert_rows_to_srgb16(icc, len(icc), int(d.planes == 4), 0, c.ctypes.data, d.width, d.height, c.strides[0]))
        make = lambda d: np.minimum(harness.make_write_source(d, seed=31), 32768)       # noqa: E731  (Photoshop's range: the reference indexes its table with the sample)
    elif n == 7:                                                    # an 8-bit document behind a LUT-based profile: the caller's table
        import test_icc8
        icc = test_icc8._a2b_profile(L, 1)
        rc, xf = test_icc8._clut8_from_transform(L, icc)
        assert rc == 0, pkg.load().avifgpu_last_error()
        kw = dict(width=1072, depth=8, planes=4, bit_depth=8, output=YCC, chroma=C422, **BT601, **STRAIGHT)
        conv = lambda c, d: L.oracle_icc_convert_rows_to_srgb8(icc, len(icc), int(d.planes == 4), c.ctypes.data, d.width, d.height, c.strides[0])   # noqa: E731
        make = None
    else:                                                           # 8: a 32-bit document behind a LUT-based profile: lcms2's stage program
        import test_gpu_icc32_pipeline as t8
        icc = t8._a2b(L, 1)
        rc, xf = pkg.icc_pipeline32_from_profile(icc, pkg.ICC_TARGET_REC2020_LINEAR, False)
        assert rc == 0, pkg.load().avifgpu_last_error()
        kw = dict(hdr, planes=3, output=YCC, chroma=C420)
        conv = lambda c, d: L.oracle_icc_convert_rows_to_rec2020(icc, len(icc), 0, c.ctypes.data, d.width, d.height, c.strides[0])                 # noqa: E731
        make = lambda d: t8._source(d, 31)                                                                                                       # noqa: E731

    def rows(d, src):
        c = src.copy()
        assert conv(c, d) == 0
        return c
    return kw, xf, rows, make, harness.T2_MIN_EXACT_ICC


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_generic_write_kernel_behind_a_profile_walks_its_loop(gpu, n, cap):
    """One case for each icc= instantiation launch_one can label."""
    if ip.lcms() is None or _lcms_int() is None or (n == 8 and pkg.lcms_bridge() is None):
        pytest.skip(ip.NO_LCMS)
    kw, xf, rows, make, bar = _px_icc_setup(gpu, n)
    walk_write(gpu, "write_px<", kw, cap, 0, "px", pad=3, icc=xf, oracle_rows=rows, min_exact=bar, make_source=make, label_has=(f"icc={n}",))


# ---- read_px ----------------------------------------------------------------------------------------------------------------------------
def rd(cs, chroma, bits, depth, alpha=pkg.ALPHA_NONE, **kw):
    return dict(width=1100, colorspace=cs, chroma=chroma, bit_depth=bits, depth=depth, alpha_state=alpha, **kw)


YCBCR, RGB, MONO = pkg.COLORSPACE_YCBCR, pkg.COLORSPACE_RGB, pkg.COLORSPACE_MONOCHROME
A_STRAIGHT, A_PREMUL = pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED
HDR_READ = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
GBR = dict(matrix_coefficients=pkg.MATRIX_RGB_GBR)
READ_CASES = [
    rd(YCBCR, C444, 8, 8, matrix_coefficients=pkg.MATRIX_BT601),
    rd(YCBCR, C420, 8, 8, matrix_coefficients=pkg.MATRIX_BT709, full_range_flag=0),
    rd(YCBCR, C422, 8, 8, A_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT601),
    rd(YCBCR, C420, 8, 8, A_PREMUL, matrix_coefficients=pkg.MATRIX_BT709, full_range_flag=0),
    rd(YCBCR, C444, 10, 16, A_PREMUL, matrix_coefficients=pkg.MATRIX_BT709),
    rd(YCBCR, C420, 12, 16, matrix_coefficients=pkg.MATRIX_BT709, full_range_flag=0),
    rd(YCBCR, C422, 10, 16, A_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT709, full_range_flag=0),
    rd(YCBCR, C444, 10, 32, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=80, **HDR_READ),
    rd(YCBCR, C420, 12, 32, A_PREMUL, transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=1, hlg_display_gamma=1.2, hlg_peak_nits=1000, **HDR_READ),
    rd(YCBCR, C422, 12, 32, A_STRAIGHT, transfer_characteristics=pkg.TC_SMPTE428, **HDR_READ),
    rd(YCBCR, C420, 10, 32, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000, full_range_flag=0, **HDR_READ),
    rd(RGB, C444, 8, 8, **GBR),
    rd(RGB, C444, 12, 16, A_STRAIGHT, **GBR),
    rd(RGB, C444, 10, 32, A_PREMUL, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=80, color_primaries=pkg.PRIMARIES_BT2020, **GBR),
    rd(RGB, C444, 12, 32, transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=1, hlg_display_gamma=1.5, hlg_peak_nits=400, color_primaries=pkg.PRIMARIES_BT709, **GBR),
    rd(MONO, pkg.CHROMA_MONOCHROME, 8, 8),
    rd(MONO, pkg.CHROMA_MONOCHROME, 8, 8, A_STRAIGHT, full_range_flag=0),
    rd(MONO, pkg.CHROMA_MONOCHROME, 12, 16, A_PREMUL),
    rd(MONO, pkg.CHROMA_MONOCHROME, 10, 16, full_range_flag=0),
    rd(MONO, pkg.CHROMA_MONOCHROME, 12, 32, A_STRAIGHT, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000),
]


def _strided(d, planes, mode):
    """The planes of harness.make_read_source with rows that are tight (contiguous: FLAT where nothing depends on a row's end), of a multiple
    of 16 bytes (the aligned paths: the 8-bit buffer loads), or off the 16-byte grid (an unaligned pitch)."""
    out = {}
    for pl, (w, _, _) in harness.read_planes(d).items():
        a = planes[pl][:, :w]
        per16 = 16 // a.itemsize
        stride = {"tight": w, "aligned": harness.align(w, per16), "odd": harness.align(w, per16) + 3}[mode]
        b = np.zeros((a.shape[0], stride), a.dtype)
        b[:, :w] = a
        out[pl] = b
    return out


def _gpu_read_raw(gpu, d, planes, row0, nrows, dst_stride):
    import torch
    dev = f"cuda:{gpu.device}"
    buf = np.full((nrows, dst_stride), SENTINEL, dtype=np.uint8)
    d_pl = {pl: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for pl, a in planes.items()}
    d_out = torch.from_numpy(buf.reshape(-1).copy()).to(dev)
    ptrs, strides = harness._tile_read_ptrs(d, planes, row0, lambda pl: d_pl[pl].data_ptr())
    gpu.read_rows(d, row0, nrows, ptrs, strides, d_out.data_ptr(), dst_stride, mem=pkg.MEM_DEVICE, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return d_out.cpu().numpy().reshape(buf.shape)


def _read_id(kw):
    return (f"cs{kw['colorspace']}-c{kw['chroma']}-b{kw['bit_depth']}-d{kw['depth']}-a{kw['alpha_state']}-fr{kw.get('full_range_flag', 1)}"
            f"-tc{kw.get('transfer_characteristics', 0)}")


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kw", READ_CASES, ids=[f"{_read_id(kw)}-{i}" for i, kw in enumerate(READ_CASES)])
def test_read_kernel_walks_its_loop(gpu, kw, cap):
    height, tile, tile420 = GEOMETRY["stream"][cap]
    d = pkg.ReadDesc(**dict(kw, height=height))
    xs, ys = harness.chroma_shift(d.chroma) if d.colorspace == YCBCR else (0, 0)
    source = harness.make_read_source(d, seed=23)
    row_bytes = d.width * harness.read_channels(d) * (d.depth // 8)
    for mode in ("tight", "aligned", "odd"):
        planes = _strided(d, source, mode)
        dst_stride = {"tight": row_bytes, "aligned": harness.align(row_bytes, 16), "odd": harness.align(row_bytes, 16) + 12}[mode]
        for row0, nrows in ((0, height), tile420 if ys else tile):
            try:
                gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
                base = _gpu_read_raw(gpu, d, planes, row0, nrows, dst_stride)
                base_label = gpu.last_kernel()
                gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD | (cap << 8))
                got = _gpu_read_raw(gpu, d, planes, row0, nrows, dst_stride)
                label = gpu.last_kernel()
            finally:
                gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
            what = (label, mode, row0, nrows)
            check_capped_label(label, base_label, "read_px<", cap)
            assert (" flat" in label) == (mode == "tight" and ys == 0 and (xs == 0 or d.width % 2 == 0)), what
            if mode == "aligned":
                assert "aligned=1" in label, what
            if mode == "odd":
                assert "aligned=0" in label, what
            assert np.array_equal(got, base), (what, np.argwhere(got != base)[:4].tolist())
            assert (got[:, row_bytes:] == SENTINEL).all(), (what, "padding")
            want = harness.oracle_read(d, planes, row0=row0, nrows=nrows)
            out = got[:, :row_bytes].copy().view(harness.src_dtype(d.depth)).reshape(nrows, -1)
            if d.depth == 32:
                np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-9, err_msg=str(what))
            else:
                assert np.array_equal(out, want), (what, np.argwhere(out != want)[:4].tolist())
            print(f"{label} rows {row0}+{nrows} {mode}: {'within the bar' if d.depth == 32 else 'equal'}")


def test_a_cap_in_bits_8_does_not_switch_flat_reads_on(gpu):
    """launch_read reads the word as a switch (0 = no FLAT launches): it must look at the low byte only."""
    d = pkg.ReadDesc(**dict(rd(YCBCR, C444, 10, 16, matrix_coefficients=pkg.MATRIX_BT709), width=1104, height=15))
    planes = harness.make_read_source(d, seed=23)
    try:
        gpu.lib.avifgpu_set_hot_variant(0)
        base = harness.gpu_read(gpu, d, planes)
        assert " flat" not in gpu.last_kernel(), gpu.last_kernel()
        gpu.lib.avifgpu_set_hot_variant(1 << 8)
        got = harness.gpu_read(gpu, d, planes)
        label = gpu.last_kernel()
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
    assert " flat" not in label and cap_of(label) is not None and cap_of(label)[0] == 1, label
    assert np.array_equal(got, base) and np.array_equal(got, harness.oracle_read(d, planes))


# ---- write_hist_px ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("bits,planes,chroma", [(10, 3, C444), (12, 4, C420)])
def test_code_histogram_walks_its_loop(gpu, bits, planes, chroma, cap):
    """A PQ save with a histogram armed, device and host counters: the capped grid (at most `cap` workgroups of write_hist_px; 1061 x 39
    pixels are 11 workgroups of one-trip waves) counts what the uncapped one counts, every pixel once, and writes the same planes."""
    alpha = PREMUL if planes == 4 else {}
    d = pkg.WriteDesc(**dict(f32(1061, planes, bits, PQ, YCC, chroma, **alpha), height=39))
    src = harness.make_write_source(d, seed=31)
    for mem in ("device", "host"):
        try:
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
            base_planes, base_bins = write_hist(gpu, d, src, mem=mem, return_raw=True)
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD | (cap << 8))
            planes_out, bins = write_hist(gpu, d, src, mem=mem, return_raw=True)
        finally:
            gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
        assert int(bins.sum()) == d.width * d.height, (mem, int(bins.sum()))
        assert np.array_equal(bins, base_bins), (mem, int(np.abs(bins - base_bins).sum()))
        for pl in base_planes:
            assert np.array_equal(planes_out[pl], base_planes[pl]), (mem, pl)


# ---- the byte movers: more than 65 535 rows / tiles, where grid.y stops covering them and the kernels wrap -------------------------------
def _probe_orient(gpu, code, src, aligned):
    """src (h, w, bpp) through avifgpu_probe_orient; aligned: 16-byte pitches on both sides, else a source pitch off the grid by one byte
    and a destination pitch by three.  Returns the oriented pixels after checking the bytes beyond each row."""
    import torch
    dev = f"cuda:{gpu.device}"
    h, w, bpp = src.shape
    want_shape = orient(code, src).shape
    oh, ow = want_shape[:2]
    sp = harness.align(w * bpp, 16) if aligned else w * bpp + 1
    dp = harness.align(ow * bpp, 16) if aligned else ow * bpp + 3
    wide = np.zeros((h, sp), np.uint8)
    wide[:, :w * bpp] = src.reshape(h, -1)
    d_src = torch.from_numpy(wide.reshape(-1)).to(dev)
    d_dst = torch.full((oh * dp,), SENTINEL, dtype=torch.uint8, device=dev)
    gpu.probe_orient(code, bpp, w, h, d_src.data_ptr(), sp, d_dst.data_ptr(), dp, None)
    torch.cuda.synchronize(dev)
    got = d_dst.cpu().numpy().reshape(oh, dp)
    assert (got[:, ow * bpp:] == SENTINEL).all(), (code, bpp, aligned, "bytes beyond the row")
    return got[:, :ow * bpp].reshape(want_shape)


@pytest.mark.parametrize("bpp", [1, 6, 16])
def test_orient_rows_wraps_its_row_grid(gpu, bpp):
    """orient_rows launches min(rows, 65 535) in grid.y: 8 pixels x 65 600 rows, the forms with flips."""
    src = np.random.default_rng(bpp).integers(0, 256, size=(65600, 8, bpp), dtype=np.uint8)
    for code in (2, 3, 4):
        want = np.ascontiguousarray(orient(code, src))
        for aligned in (True, False):
            assert np.array_equal(_probe_orient(gpu, code, src, aligned), want), (bpp, code, aligned)


@pytest.mark.parametrize("code", [5, 6, 7, 8])
@pytest.mark.parametrize("bpp,width", [(1, 64 * 65535 + 70), (8, 32 * 65535 + 40)])
def test_orient_transpose_wraps_its_tile_grid(gpu, bpp, width, code):
    """orient_transpose launches min(ceil(width / T), 65 535) tiles in grid.y (T = 64 pixels up to 4 bytes a pixel, 32 above): three rows
    of the first width at which the tiles outnumber the grid, plus a ragged tile."""
    src = np.random.default_rng(bpp + code).integers(0, 256, size=(3, width, bpp), dtype=np.uint8)
    want = np.ascontiguousarray(orient(code, src))
    for aligned in (True, False):
        assert np.array_equal(_probe_orient(gpu, code, src, aligned), want), (bpp, code, aligned)


@pytest.mark.parametrize("soff,doff,dstride", [(0, 0, 48), (1, 5, 51)])
def test_crop_rows_wraps_its_row_grid(gpu, soff, doff, dstride):
    """crop_rows launches min(rows, 65 535) in grid.y: 65 600 rows of 40 payload bytes, aligned and from an odd base."""
    import torch
    dev = f"cuda:{gpu.device}"
    rows, rb, pitch = 65600, 40, 64
    src = np.random.default_rng(5).integers(0, 256, size=(rows * pitch + 16,), dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    total = doff + (rows + 2) * dstride
    d_dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    assert soff + (rows - 1) * pitch + rb <= src.size and doff + dstride + (rows - 1) * dstride + rb <= total
    gpu.probe_crop(d_src.data_ptr() + soff, pitch, d_dst.data_ptr() + doff + dstride, dstride, rb, rows, None)
    torch.cuda.synchronize(dev)
    got = d_dst.cpu().numpy()
    assert (got[:doff + dstride] == SENTINEL).all() and (got[doff + (rows + 1) * dstride:] == SENTINEL).all(), "guard rows"
    body = got[doff + dstride:doff + (rows + 1) * dstride].reshape(rows, dstride)
    want = src[soff:soff + rows * pitch].reshape(rows, pitch)[:, :rb]
    assert np.array_equal(body[:, :rb], want)
    assert (body[:, rb:] == SENTINEL).all(), "bytes beyond the payload"
