"""CPU pins of tests/truth64.py (no GPU): the float64 truth that tests/test_gpu_t2_determined.py, tests/test_gpu_fullsize.py and
tests/test_gpu_read_truth.py judge the kernels by is first held against the oracle itself.

 * On sources where every colour sample is determined, the oracle's stage-A codes (OUT_REFERENCE) equal truth64.determined_codes
   sample for sample -- every curve, peak 1 / 80 / 1000 / 10000, 10 and 12 bit, straight and premultiplied alpha, gray PQ.
 * The HLG and SMPTE 428 write bands are measured: the oracle's deviation from float64 is a small fraction of the band.
 * The footprint masks of stage B agree with a per-sample restatement of the oracle's loops."""
import ctypes

import numpy as np
import pytest

import harness
import truth64

pkg = harness.pkg

W, H = 67, 21


def _write_descs():
    out = []
    curves = [(pkg.TRANSFER_PQ, p) for p in (1, 80, 1000, 10000)] + [(pkg.TRANSFER_HLG, 80), (pkg.TRANSFER_SMPTE428, 80)]
    for tr, peak in curves:
        for bits in (10, 12):
            for planes, alphas in ((3, (pkg.ALPHA_NONE,)), (4, (pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED))):
                for a in alphas:
                    out.append((f"t{tr}-pq{peak}-b{bits}-p{planes}-a{a}", dict(width=W, height=H, depth=32, planes=planes, bit_depth=bits,
                                                                          transfer=tr, peak_nits=peak, alpha_state=a,
                                                                          output=pkg.OUT_REFERENCE)))
    for peak in (80, 10000):                       # gray documents take PQ only (WriteHeifImage.cpp:581)
        for bits in (10, 12):
            for planes, alphas in ((1, (pkg.ALPHA_NONE,)), (2, (pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED))):
                for a in alphas:
                    out.append((f"gray-pq{peak}-b{bits}-p{planes}-a{a}", dict(width=W, height=H, depth=32, planes=planes, bit_depth=bits,
                                                                             transfer=pkg.TRANSFER_PQ, peak_nits=peak, alpha_state=a,
                                                                             output=pkg.OUT_REFERENCE)))
    return out


@pytest.mark.parametrize("cid,kw", _write_descs())
def test_oracle_stage_a_equals_determined_codes(cid, kw):
    d = pkg.WriteDesc(**kw)
    src, replaced = truth64.make_determined_source(d)
    ncol = 3 if d.planes >= 3 else 1
    print(f"{cid}: {replaced} of {H * W * ncol} colour samples drawn again")
    assert replaced <= 0.3 * H * W * ncol, replaced           # redraws counted with repeats: the 2e-5 PQ band is wide at 12 bit
    codes, mask = truth64.determined_codes(d, src)
    assert mask.all()
    want = harness.oracle_write(d, src)
    if d.planes >= 3:
        got = want[0].reshape(H, W, d.planes).astype(np.int64)
        col, alpha = got[..., :3], (got[..., 3] if d.planes == 4 else None)
    else:
        col, alpha = want[0].reshape(H, W, 1).astype(np.int64), (want[3].astype(np.int64) if d.planes == 2 else None)
    assert np.array_equal(col, codes), (cid, int(np.sum(col != codes)))
    if alpha is not None:
        assert np.array_equal(alpha, truth64.alpha_codes(d, src))


def test_determined_source_keeps_the_distribution():
    d = pkg.WriteDesc(width=W, height=H, depth=32, planes=4, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=80,
                      alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_REFERENCE)
    src, _ = truth64.make_determined_source(d)
    px = src.reshape(H, W, 4)
    col, a = px[..., :3], px[..., 3]
    assert 0.05 < np.mean(col > 1.0) < 0.15                        # highlights up to 12.5
    assert np.any(col < 0) and col.max() <= 125.0
    assert np.any(a == 0) and np.any(a == 1) and np.any(a > 1) and np.any(a < 0)
    specials = np.array([0.0, 1.0, 0.5, 125.0, 1e-9, 1e-4, 12.5, 0.0125], np.float32)
    assert np.sum(px.reshape(-1, 4)[:8, 0] == specials) >= 6        # the special values stay unless they sit in a band


@pytest.mark.parametrize("curve", ["hlg", "smpte428"])
def test_hlg_428_write_bands_are_measured(oracle, curve):
    """The oracle's float32 OETF against float64 on a dense sweep: measured 1.2e-7 (HLG) and 1.0e-7 (SMPTE 428) relative, at most
    5e-4 codes at 12 bit.  The band (2e-6 * t + 1e-3 codes) must hold at least ten times that."""
    x = np.concatenate([np.linspace(0, 1, 20001, dtype=np.float32), np.geomspace(1e-9, 12.5, 20001).astype(np.float32),
                        np.linspace(1, 130, 2001, dtype=np.float32)])
    fn, truth = {"hlg": (oracle.oracle_linear_to_hlg, truth64.linear_to_hlg64),
                 "smpte428": (oracle.oracle_linear_to_smpte428, truth64.linear_to_smpte428_64)}[curve]
    o = np.array([fn(float(v)) for v in x], dtype=np.float64)
    t = truth(x)
    for bits in (10, 12):
        maxv = (1 << bits) - 1
        dev = np.abs(o - t) * maxv
        band = truth64.HLG_BAND_REL * t * maxv + truth64.BAND_ABS
        print(f"{curve} {bits}-bit: oracle max deviation {dev.max():.2e} codes, {np.max(np.abs(o - t)[t > 0] / t[t > 0]):.2e} relative")
        assert np.all(dev <= 0.1 * band)


def _box_mask_slow(d, pix):
    """The oracle's stage-B loop (avif_oracle.c:530-566), one output sample at a time."""
    xs, ys = harness.chroma_shift(d.chroma)
    Hh, Ww = pix.shape
    out = np.zeros(((Hh + ys) >> ys, (Ww + xs) >> xs), bool)
    for r in range(0, Hh, 1 << ys):
        for x in range(0, Ww, 1 << xs):
            if d.chroma_downsampling == pkg.DOWNSAMPLE_AVERAGE and (xs or ys):
                x2 = x + 1 if xs and x + 1 < Ww else x
                r2 = r + 1 if ys and r + 1 < Hh else r
                out[r >> ys, x >> xs] = pix[r, x] and pix[r, x2] and pix[r2, x] and pix[r2, x2]
            else:
                out[r >> ys, x >> xs] = pix[r, x]
    return out


@pytest.mark.parametrize("shape", [(21, 67), (20, 66), (1, 1), (3, 6), (2, 3)])
@pytest.mark.parametrize("chroma", [pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420])
@pytest.mark.parametrize("ds", [pkg.DOWNSAMPLE_AVERAGE, pkg.DOWNSAMPLE_NEAREST])
def test_output_masks_match_the_oracle_footprints(shape, chroma, ds):
    Hh, Ww = shape
    d = pkg.WriteDesc(width=Ww, height=Hh, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, output=pkg.OUT_YCBCR,
                      chroma=chroma, chroma_downsampling=ds, matrix_coefficients=pkg.MATRIX_BT709)
    pix = np.random.default_rng(Hh * 100 + Ww).random((Hh, Ww)) > 0.2
    m = truth64.output_masks(d, pix)
    want = _box_mask_slow(d, pix)
    assert np.array_equal(m[0], pix) and np.array_equal(m[1], want) and np.array_equal(m[2], want)


@pytest.mark.parametrize("kw", [dict(planes=3, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420, transfer=pkg.TRANSFER_PQ, peak_nits=80),
                                dict(planes=4, alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422,
                                     transfer=pkg.TRANSFER_HLG),
                                dict(planes=4, alpha_state=pkg.ALPHA_STRAIGHT, output=pkg.OUT_REFERENCE, transfer=pkg.TRANSFER_SMPTE428),
                                dict(planes=1, output=pkg.OUT_REFERENCE, transfer=pkg.TRANSFER_PQ, peak_nits=10000)])
def test_torch_masks_equal_numpy_masks(kw):
    """tests/test_gpu_fullsize.py evaluates the determined mask with torch on the device: the same functions on torch tensors
    (here on the CPU) give the same codes and masks as on numpy arrays."""
    import torch
    d = pkg.WriteDesc(width=W, height=H, depth=32, bit_depth=12, matrix_coefficients=pkg.MATRIX_BT709, **kw)
    src = harness.make_write_source(d, seed=5)
    codes, mask = truth64.determined_codes(d, src)
    tc, tm = truth64.codes_from_values(d, truth64.stage_a_values(d, torch.from_numpy(src)))
    assert np.array_equal(tc.numpy().astype(np.int64), codes) and np.array_equal(tm.numpy(), mask)
    pix = mask.all(-1)
    mn, mt = truth64.output_masks(d, pix), truth64.output_masks(d, torch.from_numpy(pix), xp=torch)
    assert sorted(mn) == sorted(mt)
    for pl in mn:
        assert np.array_equal(mn[pl], mt[pl].numpy()), pl
