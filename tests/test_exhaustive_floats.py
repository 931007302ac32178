"""The claims of tests/exhaustive_floats.py, counted, and the ORACLE held to float64 truth on whole binades (CPU only).

The GPU tests (tests/test_zz_gpu_whole_float_domain.py) take the oracle as the judge of every float of a curve's window and
tests/truth64.py as the judge of every float there is; here the two judges are held to each other on every float of three binades per
curve -- the first binade with a non-zero code, the last one below saturation, and the binade where the oracle's float32 evaluation was
measured to need the most of the band (PQ 80 nits at 12 bit: 1.40e-5 at 37.6874; PQ 10 000 nits at 10 bit: 1.28e-5 at 0.29592; HLG
and SMPTE 428: nothing beyond BAND_ABS anywhere, the binade below 1.0 stands in).  The bands are tests/truth64.py's, unchanged.
"""
import numpy as np
import pytest

import exhaustive_floats as xf
import truth64

pkg = xf.pkg
PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP


# ---- generator claims ---------------------------------------------------------------------------------------------------------------
def test_chunks_tile_the_patterns_once():
    ch = xf.chunks()
    assert len(ch) == 64 and ch[0][0] == 0 and all(n == xf.CHUNK for _, n in ch)
    assert all(a + n == b for (a, n), (b, _) in zip(ch, ch[1:])) and ch[-1][0] + ch[-1][1] == 1 << 32


@pytest.mark.parametrize("first,count", [(0, 4099), (xf.INF_BITS - 7, 40), (xf.NEG_ZERO_BITS - 5, 11), ((1 << 32) - 4100, 4100),
                                         (xf.binade_first(5), 1 << 16)])
def test_numpy_and_torch_generators_give_the_same_bits(first, count):
    import torch
    a = xf.patterns(first, count)
    b = xf.patterns(first, count, device="cpu")
    assert a.dtype == np.float32 and b.dtype == torch.float32
    want = np.arange(first, first + count, dtype=np.int64)
    assert np.array_equal(xf.bits_of(a), want) and np.array_equal(xf.bits_of(b).numpy(), want)
    assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32))
    for shift in (0, 1):
        da, db = xf.document(first, count, shift), xf.document(first, count, shift, device="cpu")
        assert da.shape == db.shape and da.shape[1] == xf.ROW and da.shape[0] * xf.ROW >= count + shift
        assert np.array_equal(da.view(np.uint32), db.numpy().view(np.uint32))
        flat = da.reshape(-1).view(np.uint32)
        assert np.array_equal(flat[shift:shift + count], want.astype(np.uint32))
        assert not flat[:shift].any() and not flat[shift + count:].any()
    for planes in (2, 4):
        pa, pb = xf.pair_document(first, count, planes), xf.pair_document(first, count, planes, device="cpu")
        assert np.array_equal(pa.view(np.uint32), pb.numpy().view(np.uint32))
        px = pa.reshape(-1, planes)
        assert np.array_equal(px[:count, -1].view(np.uint32), want.astype(np.uint32)) and np.all(px[:count, :-1] == np.float32(0.5))
    ga = xf.gray_document(first, count)
    assert np.array_equal(ga.view(np.uint32), xf.gray_document(first, count, device="cpu").numpy().view(np.uint32))
    assert np.array_equal(ga.reshape(-1)[:count].view(np.uint32), want.astype(np.uint32))


def test_a_shift_of_one_puts_every_float_in_another_slot():
    n = 3 * 1000
    a, b = xf.document(12345, n, 0).reshape(-1), xf.document(12345, n, 1).reshape(-1)
    slot_a = {int(v): i % 3 for i, v in enumerate(a[:n].view(np.uint32))}
    slot_b = {int(v): (i + 1) % 3 for i, v in enumerate(b[1:n + 1].view(np.uint32))}
    assert all(slot_a[v] != slot_b[v] for v in slot_a)
    assert [sum(1 for s in slot_a.values() if s == k) for k in range(3)] == [n // 3] * 3


def test_binades_are_runs_of_patterns_in_float_order():
    for e in (-126, -27, 0, 7, 127):
        x = xf.patterns(xf.binade_first(e), xf.BINADE)
        assert x[0] == np.float32(2.0 ** e) and np.all(np.diff(x.astype(np.float64)) > 0)
        assert float(x[-1]) < 2.0 ** (e + 1)
        if e < 127:
            assert float(np.nextafter(x[-1], np.float32(np.inf))) == 2.0 ** (e + 1)
    assert np.isinf(xf.patterns(xf.INF_BITS, 1)[0]) and np.all(np.isnan(xf.patterns(xf.INF_BITS + 1, 5)))
    z = xf.patterns(xf.NEG_ZERO_BITS, 1)
    assert z[0] == 0 and np.signbit(z[0]) and xf.patterns(xf.NEG_INF_BITS, 1)[0] == -np.inf


CURVES = [("pq80-12", PQ, 80, 12), ("pq80-10", PQ, 80, 10), ("pq1000-10", PQ, 1000, 10), ("pq1000-12", PQ, 1000, 12),
          ("pq10000-10", PQ, 10000, 10), ("pq10000-12", PQ, 10000, 12), ("hlg-10", HLG, 80, 10), ("hlg-12", HLG, 80, 12),
          ("smpte428-10", S428, 80, 10), ("smpte428-12", S428, 80, 12), ("clip-10", CLIP, 80, 10), ("clip-12", CLIP, 80, 12)]


@pytest.mark.parametrize("name,tr,peak,bits", CURVES, ids=[c[0] for c in CURVES])
def test_window_edges_meet_their_conditions(name, tr, peak, bits):
    d = xf.document_desc(1, bits, tr, peak)
    maxv = float((1 << bits) - 1)
    e0, e1 = xf.window(d)
    assert -126 < e0 < e1 <= 8
    assert xf.curve64_scalar(d, 2.0 ** e0) * maxv < 0.5 <= xf.curve64_scalar(d, 2.0 ** (e0 + 1)) * maxv
    if tr == CLIP:
        assert 2.0 ** e1 >= 2.0 > 2.0 ** (e1 - 1)
    else:
        assert xf.curve64_scalar(d, 2.0 ** e1) >= 1.0 + xf.band(d) > xf.curve64_scalar(d, 2.0 ** (e1 - 1))
        # what the edges are for: below the window the whole truth interval is code 0; above it the curve is past max by more than
        # its band (truth_interval clips T first, so its lower end there is max - 1)
        lo, hi = xf.truth_interval(d, np.array([2.0 ** e0, 2.0 ** e1], dtype=np.float32))
        assert (lo[0], hi[0], hi[1]) == (0.0, 0.0, maxv) and lo[1] >= maxv - 1
        assert xf.curve64_scalar(d, 2.0 ** e1) * maxv * (1.0 - truth64.band_rel(d)) - truth64.BAND_ABS >= maxv
    groups = xf.window_groups(e0, e1)
    assert groups[0][0] == xf.binade_first(e0) and sum(n for _, n, _ in groups) == (e1 - e0) * xf.BINADE
    assert all(a + n == b for (a, n, _), (b, _, _) in zip(groups, groups[1:])) and all(n <= xf.CHUNK for _, n, _ in groups)


# ---- the oracle against float64 truth, every float of a binade ------------------------------------------------------------------------
ORACLE_BINADES = []
for _name, _tr, _peak, _bits, _worst in (("pq80-12", PQ, 80, 12, 5), ("pq10000-10", PQ, 10000, 10, -2), ("hlg-12", HLG, 80, 12, -1),
                                          ("smpte428-12", S428, 80, 12, -1)):
    _e0, _e1 = xf.window(xf.document_desc(1, _bits, _tr, _peak))
    ORACLE_BINADES += [(_name, _tr, _peak, _bits, e) for e in (_e0 + 1, _worst, _e1 - 1)]


@pytest.mark.parametrize("name,tr,peak,bits,e", ORACLE_BINADES, ids=[f"{c[0]}-2^{c[4]}" for c in ORACLE_BINADES])
def test_oracle_codes_lie_in_the_truth_interval_on_a_whole_binade(name, tr, peak, bits, e):
    first = xf.binade_first(e)
    src = xf.document(first, xf.BINADE)
    d = xf.document_desc(src.shape[0], bits, tr, peak)
    codes = xf.oracle_planes(d, src)[0].reshape(-1)[:xf.BINADE].astype(np.float64)
    x = src.reshape(-1)[:xf.BINADE]
    lo, hi = xf.truth_interval(d, x)
    need = xf.band_needed(d, x, codes)
    i = int(np.argmax(need))
    t = np.clip(truth64.oetf64(d, x) * ((1 << bits) - 1), 0, (1 << bits) - 1)
    print(f"oracle {name} binade 2^{e}: relative band needed {need[i]:.3e} at {float(x[i])!r}; |code - floor(truth)| <= "
          f"{int(np.max(np.abs(codes - np.floor(t))))}; descents {int(np.sum(np.diff(codes) < 0))}")
    bad = np.nonzero((codes < lo) | (codes > hi))[0]
    assert bad.size == 0, [(float(x[k]), int(codes[k]), int(lo[k]), int(hi[k])) for k in bad[:8]]
    assert np.max(np.abs(codes - np.floor(t))) <= 1
    assert need[i] <= truth64.band_rel(d)
