"""The write launcher against the record of its choices (tests/golden/write_dispatch_labels.json.gz, recorded before the choice moved to
csrc/write_dispatch.h; tests/golden/make_write_dispatch_labels.py): every recorded case is saved again through avifgpu_write_rows on
device pointers and must carry the recorded label, under its tuning word and under that word with a block cap of 1 -- the kernel, its
template values, FLAT, and (" cap=1/M") the grid.  tools/write_dispatch_check.cpp holds the decision alone to the same record on the
CPU (tests/test_write_dispatch.py); this is the library, launches included.

One case per streaming candidate also has its planes compared, padding included, with the same save under tuning word 0 (the generic
kernel): byte for byte, which is what tests/test_gpu_kernel_equivalence.py demands of every such pair, 32-bit documents included.  The
two candidates that exist only behind an ICC stage (write_rgb32_icc1_ycbcr444_hot, planes and hand-off) have no such pair there -- the
streaming ICC stage is single precision, the generic one is not; tests/test_gpu_icc.py holds both to lcms2 -- and are not compared here."""
import numpy as np
import pytest

import harness
import write_dispatch_cases as wc

pkg = harness.pkg
pytestmark = pytest.mark.gpu

CASES, BIG = wc.load_fixture()


def _replay(gpu, arena, cases):
    wrong = []
    for i, c in enumerate(cases):
        for key, word in (("label", c["word"]), ("label_cap", c["word"] | wc.CAP1)):
            got = wc.run_case(gpu, arena, c, word)
            if got != c[key]:
                wrong.append((i, key, c[key], got))
    arena.sync()
    return wrong


@pytest.mark.parametrize("depth", [8, 16, 32])
def test_every_recorded_case_takes_its_recorded_kernel(gpu, depth):
    cases = [c for c in CASES if c["depth"] == depth]
    assert len(cases) > 1000
    wrong = _replay(gpu, wc.Arena(gpu), cases)
    assert not wrong, (len(wrong), wrong[:5])


def test_two_spans_per_wave_from_32768_whole_spans(gpu):
    """512 x 32767 and 512 x 32768 pixels, 4:2:2: the second tile's waves take two spans each (half the workgroups of a one-trip grid)."""
    assert [c["rows"] for c in BIG] == [32767, 32768]
    assert BIG[0]["label_cap"].endswith(" cap=1/8192 flat") and BIG[1]["label_cap"].endswith(" cap=1/4096 flat")
    wrong = _replay(gpu, wc.big_arena(gpu), BIG)
    assert not wrong, wrong


# (kernel, descriptor): one per streaming candidate that has a generic twin
F32 = dict(depth=32, transfer=pkg.TRANSFER_PQ, peak_nits=1000)
YCC = dict(output=pkg.OUT_YCBCR)
SAME_BYTES = [
    ("write_copy_rows_stream", dict(width=1032, depth=8, planes=3, bit_depth=8)),
    ("write_int_ref_stream", dict(width=1032, depth=16, planes=3, bit_depth=12)),
    ("write_ga_stream<depth=16>", dict(width=1032, depth=16, planes=2, bit_depth=12, alpha_state=pkg.ALPHA_PREMULTIPLIED)),
    ("write_rgb8_ycbcr_hot", dict(width=1032, depth=8, planes=3, bit_depth=8, chroma=pkg.CHROMA_420, **YCC)),
    ("write_rgb8_ycbcr16_hot", dict(width=1032, depth=8, planes=3, bit_depth=10, chroma=pkg.CHROMA_422, **YCC)),
    ("write_rgba8_ycbcra_hot", dict(width=1032, depth=8, planes=4, bit_depth=8, chroma=pkg.CHROMA_420, alpha_state=pkg.ALPHA_PREMULTIPLIED, **YCC)),
    ("write_rgb16_ycbcr444_hot", dict(width=1032, depth=16, planes=3, bit_depth=12, **YCC)),
    ("write_rgba16_ycbcra444_hot", dict(width=1032, depth=16, planes=4, bit_depth=8, alpha_state=pkg.ALPHA_STRAIGHT, **YCC)),
    ("write_rgba16_ycbcra_sub_hot", dict(width=1032, depth=16, planes=4, bit_depth=10, chroma=pkg.CHROMA_420, alpha_state=pkg.ALPHA_PREMULTIPLIED, **YCC)),
    ("write_rgb16_ycbcr_sub_hot", dict(width=1032, depth=16, planes=3, bit_depth=8, chroma=pkg.CHROMA_422, **YCC)),
    ("write_ga_stream<depth=32", dict(width=1032, planes=2, bit_depth=10, alpha_state=pkg.ALPHA_STRAIGHT, **F32)),
    ("write_rgba32_ycbcra_sub_hot", dict(width=1032, planes=4, bit_depth=10, chroma=pkg.CHROMA_420, alpha_state=pkg.ALPHA_PREMULTIPLIED, **F32, **YCC)),
    ("write_rgba32_ycbcra444_hot", dict(width=1032, planes=4, bit_depth=12, alpha_state=pkg.ALPHA_STRAIGHT, **F32, **YCC)),
    ("write_rgb32_ycbcr_sub_hot", dict(width=1032, planes=3, bit_depth=10, chroma=pkg.CHROMA_422, **F32, **YCC)),
    ("write_f32_ref_stream", dict(width=1032, planes=3, bit_depth=12, **F32)),
    ("write_rgb32_ycbcr444_hot", dict(width=1032, planes=3, bit_depth=10, **F32, **YCC)),
]


@pytest.mark.parametrize("kernel,kw", SAME_BYTES, ids=[k for k, _ in SAME_BYTES])
def test_candidate_writes_the_generic_kernels_bytes(gpu, kernel, kw):
    d = pkg.WriteDesc(**dict(kw, height=3))
    src = harness.make_write_source(d, seed=31)
    fill = 0xA5A5 if d.bit_depth > 8 else 0xA5
    for stride_pad in (0, 16):                                  # contiguous planes (FLAT where the rule allows it) and padded ones
        try:
            gpu.lib.avifgpu_set_hot_variant(wc.DEFAULT_WORD)
            fast = harness.gpu_write(gpu, d, src, stride_pad=stride_pad, return_raw=True)
            assert gpu.last_kernel().startswith(kernel), gpu.last_kernel()
            gpu.lib.avifgpu_set_hot_variant(0)
            slow = harness.gpu_write(gpu, d, src, stride_pad=stride_pad, return_raw=True)
            assert gpu.last_kernel().startswith("write_px<"), gpu.last_kernel()
        finally:
            gpu.lib.avifgpu_set_hot_variant(wc.DEFAULT_WORD)
        for pl, (w, _, _) in harness.write_planes(d).items():
            assert np.array_equal(fast[pl], slow[pl]), (kernel, stride_pad, pl)
            assert (fast[pl][:, w:] == fill).all(), (kernel, stride_pad, pl, "padding")
