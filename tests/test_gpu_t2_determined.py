"""Float-tier saves held EXACTLY on determined sources (tests/truth64.py).

The rate bars of tests/test_gpu_write.py pool every plane: a kernel that gets a whole replicated chroma column or a few codes of
stage B wrong passes them.  Here the source is drawn (harness.make_write_source's distribution) so that every colour sample's
code is determined -- its float64 value, widened by the curve's evaluation band, does not straddle a code boundary -- and then
every output sample, padding included, must equal the oracle's bit for bit: PQ (peaks 80 / 1000 / 10000, every pq_evaluation),
HLG and SMPTE 428; OUT_REFERENCE with 1-4 planes and OUT_YCBCR 4:4:4 / 4:2:2 / 4:2:0, box and nearest, BT.601 / 709 / 2020 / GBR;
straight and premultiplied alpha; shapes that reach the generic kernel and every streaming kernel
(tests/test_gpu_kernel_equivalence.py), under the default tuning word, with the streaming kernels forced on, and with all of them
off; device memory and host memory with padded strides; a row tile that starts after row 0 and ends before the image does."""
import numpy as np
import pytest

import harness
import truth64

pkg = harness.pkg
pytestmark = pytest.mark.gpu

DEFAULT_WORD = 1 | 2 | 4                 # the library's default tuning word
WORDS = {"default": DEFAULT_WORD, "stream": 1 | 2 | 4 | 8, "generic": 0}
BT2020 = dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
MATS = {"601": dict(matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709),
        "709": dict(matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709),
        "2020": BT2020,
        "gbr": dict(matrix_coefficients=pkg.MATRIX_RGB_GBR, color_primaries=pkg.PRIMARIES_BT709)}
CURVES = [("pq80", dict(transfer=pkg.TRANSFER_PQ, peak_nits=80)), ("pq1000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=1000)),
          ("hlg", dict(transfer=pkg.TRANSFER_HLG)), ("pq10000", dict(transfer=pkg.TRANSFER_PQ, peak_nits=10000)),
          ("smpte428", dict(transfer=pkg.TRANSFER_SMPTE428))]
PLANE_ALPHAS = [(1, pkg.ALPHA_NONE), (2, pkg.ALPHA_STRAIGHT), (2, pkg.ALPHA_PREMULTIPLIED), (3, pkg.ALPHA_NONE),
                (4, pkg.ALPHA_STRAIGHT), (4, pkg.ALPHA_PREMULTIPLIED)]


def _run(gpu, kw, word=DEFAULT_WORD, mem="device", row0=0, nrows=None, seed=harness.SEED):
    d = pkg.WriteDesc(**kw)
    src, replaced = truth64.make_determined_source(d, seed=seed)
    pad = 24 if mem == "host" else 0
    want = harness.oracle_write(d, src, row0=row0, nrows=nrows, stride_pad=pad, return_raw=True)
    try:
        gpu.lib.avifgpu_set_hot_variant(word)
        got = harness.gpu_write(gpu, d, src, row0=row0, nrows=nrows, mem=mem, stride_pad=pad, return_raw=True)
        kernel = gpu.last_kernel()
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
    assert sorted(got) == sorted(want)
    for pl in want:
        bad = np.argwhere(got[pl] != want[pl])
        assert bad.shape[0] == 0, (kernel, pl, bad.shape[0], bad[:8].tolist(), got[pl][tuple(bad[0])], want[pl][tuple(bad[0])])
    return kernel, replaced


def _ref_cases():
    out = []
    for bits in (10, 12):
        for peak in (80, 1000, 10000):
            for ev in (0, 1, 2):
                for planes, a in PLANE_ALPHAS:
                    out.append((f"ref-pq{peak}-e{ev}-b{bits}-p{planes}-a{a}",
                                dict(width=67, height=21, depth=32, planes=planes, bit_depth=bits, transfer=pkg.TRANSFER_PQ, peak_nits=peak,
                                     pq_evaluation=ev, alpha_state=a, output=pkg.OUT_REFERENCE)))
        for name, tr in (("hlg", pkg.TRANSFER_HLG), ("smpte428", pkg.TRANSFER_SMPTE428)):
            for planes, a in PLANE_ALPHAS[3:]:                     # gray saves take PQ or Clip only (WriteHeifImage.cpp:581)
                out.append((f"ref-{name}-b{bits}-p{planes}-a{a}",
                            dict(width=67, height=21, depth=32, planes=planes, bit_depth=bits, transfer=tr, alpha_state=a,
                                 output=pkg.OUT_REFERENCE)))
    return out


def _ycc_cases():
    out = []
    combos = [(pkg.CHROMA_444, pkg.DOWNSAMPLE_AVERAGE, m) for m in MATS]
    combos += [(c, ds, m) for c in (pkg.CHROMA_422, pkg.CHROMA_420) for ds in (pkg.DOWNSAMPLE_AVERAGE, pkg.DOWNSAMPLE_NEAREST)
               for m in ("601", "709", "2020")]
    i = 0
    for chroma, ds, m in combos:
        for planes, a in ((3, pkg.ALPHA_NONE), (4, pkg.ALPHA_STRAIGHT), (4, pkg.ALPHA_PREMULTIPLIED)):
            cname, ckw = CURVES[i % len(CURVES)]
            bits = (10, 12)[(i // len(CURVES)) % 2]
            i += 1
            out.append((f"ycc-c{chroma}-ds{ds}-{m}-p{planes}-a{a}-{cname}-b{bits}",
                        dict(width=67, height=21, depth=32, planes=planes, bit_depth=bits, alpha_state=a, output=pkg.OUT_YCBCR,
                             chroma=chroma, chroma_downsampling=ds, **ckw, **MATS[m])))
    return out


# what each streaming kernel takes (tests/test_gpu_kernel_equivalence.py), at the shapes where its edge paths run
KERNEL_CONFIGS = [
    ("rgb32_444", dict(planes=3, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020)),
    ("rgb32_420_box", dict(planes=3, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **BT2020)),
    ("rgb32_422_box", dict(planes=3, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, **MATS["709"])),
    ("rgb32_422_nearest", dict(planes=3, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST, **BT2020)),
    ("rgba32_444_premul", dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, **BT2020)),
    ("rgba32_420_straight", dict(planes=4, alpha_state=pkg.ALPHA_STRAIGHT, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, **MATS["601"])),
    ("rgba32_422_premul_nearest", dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422,
                                       chroma_downsampling=pkg.DOWNSAMPLE_NEAREST, **BT2020)),
    ("f32_ref_rgb", dict(planes=3, output=pkg.OUT_REFERENCE)),
    ("f32_ref_rgba_premul", dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_REFERENCE)),
    ("gray", dict(planes=1, output=pkg.OUT_REFERENCE)),
    ("gray_alpha_premul", dict(planes=2, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_REFERENCE)),
]
SHAPES = [(67, 21), (1003, 7), (1004, 7), (515, 5), (259, 5), (513, 3), (1, 3), (6, 2), (1024, 6)]


def _kernel_cases():
    out = []
    i = 0
    for w, h in SHAPES:
        for kname, kkw in KERNEL_CONFIGS:
            gray = kkw["planes"] < 3
            cname, ckw = (CURVES[0] if gray else CURVES[i % len(CURVES)]) if i % 3 else ("pq80", CURVES[0][1])
            if gray and i % 2:
                cname, ckw = CURVES[1]
            bits = (12, 10)[i % 2]
            i += 1
            out.append((f"{kname}-{w}x{h}-{cname}-b{bits}", dict(width=w, height=h, depth=32, bit_depth=bits, **ckw, **kkw)))
    return out


@pytest.mark.parametrize("cid,kw", _ref_cases() + _ycc_cases())
def test_determined_write_is_exact(gpu, cid, kw):
    kernel, replaced = _run(gpu, kw)
    assert "write" in kernel, kernel


@pytest.mark.parametrize("word", list(WORDS))
@pytest.mark.parametrize("cid,kw", _kernel_cases())
def test_determined_write_is_exact_on_every_kernel(gpu, cid, kw, word):
    kernel, _ = _run(gpu, kw, word=WORDS[word], seed=harness.SEED + len(cid))
    if word == "generic":
        assert "write_px" in kernel, kernel


@pytest.mark.parametrize("cid,kw", (_ref_cases() + _ycc_cases())[::4] + _kernel_cases()[::5])
def test_determined_write_is_exact_host_padded(gpu, cid, kw):
    _run(gpu, kw, mem="host", seed=77)


@pytest.mark.parametrize("word", list(WORDS))
@pytest.mark.parametrize("chroma,ds", [(pkg.CHROMA_420, pkg.DOWNSAMPLE_AVERAGE), (pkg.CHROMA_420, pkg.DOWNSAMPLE_NEAREST),
                                       (pkg.CHROMA_422, pkg.DOWNSAMPLE_AVERAGE), (pkg.CHROMA_444, pkg.DOWNSAMPLE_AVERAGE)])
@pytest.mark.parametrize("planes,a", [(3, pkg.ALPHA_NONE), (4, pkg.ALPHA_PREMULTIPLIED)])
def test_determined_write_is_exact_on_an_inner_tile(gpu, word, chroma, ds, planes, a):
    """An even-row tile with row0 > 0 that ends before the image does (what the multi-GPU sharding hands each device)."""
    kw = dict(width=1003, height=11, depth=32, planes=planes, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=1000, alpha_state=a,
              output=pkg.OUT_YCBCR, chroma=chroma, chroma_downsampling=ds, **BT2020)
    _run(gpu, kw, word=WORDS[word], row0=4, nrows=4)
