"""The per-context device accumulators behind the three statistics of a host-pointer save (csrc/pipeline.hip DeviceAccum, csrc/save_stats.cpp):
the code histogram, the thumbnail sums and the summary counters, all three armed on host memory in every step.

The features' own test files pin each statistic alone, the three together, several contexts and cuts, mismatches.  The sequence below makes
one binding's accumulators CHANGE SIZE AND CHANGE HANDS: a small thumbnail, a larger one (the buffer grows), the small one again (below the
capacity: the sums' row stride is not what the buffer last held), a call that fails in its argument checks, the larger one again, then a
12-bit save with 4096 bins and the 10-bit one after it.  After every successful step the host bins, sums, counters and planes must be EQUAL
to those of the same save through the device-pointer path armed on device memory, which uses no accumulator at all.  Exact integers: no
tolerances.

97 x 41, 4:2:0, a 32-bit PQ document: all three statistics apply, chroma is odd; rows cut so that both contexts get tiles.

The file sorts behind the features' own test files, as the suite's other late additions do: in a run of the whole suite the accumulators
it meets have been used by every one of them."""
import os

import numpy as np
import pytest

import harness
from test_summary import N
from test_written_planes_gpu import C420, YCC, desc_for, source, write_summary

pkg = harness.pkg
pytestmark = pytest.mark.gpu

W, H = 97, 41
CUTS = [(0, 2), (2, 20), (22, 19)]


def _save(g, d, src, tw, th, mem):
    """One armed save; returns (planes, bins, sums, counters) as numpy."""
    import torch
    n_bins, n_sums = 1 << d.bit_depth, tw * th * d.planes
    if mem == "host":
        bins, sums = np.zeros(n_bins, dtype=np.uint64), np.zeros(n_sums, dtype=np.uint64)
        planes, c = write_summary(g, d, src, mem="host", cuts=CUTS, hist=bins, thumb=(sums, tw, th))
        return planes, bins, sums, c
    dev = f"cuda:{g.device}"
    bins, sums = torch.zeros(n_bins, dtype=torch.int64, device=dev), torch.zeros(n_sums, dtype=torch.int64, device=dev)
    planes, c = write_summary(g, d, src, mem="device", hist=bins, thumb=(sums, tw, th))
    return planes, bins.cpu().numpy().view(np.uint64), sums.cpu().numpy().view(np.uint64), c


def test_accumulators_change_size_and_change_hands(gpu):
    d10 = desc_for(16, 3, YCC, C420, width=W, height=H, depth=32)
    d12 = desc_for(16, 3, YCC, C420, width=W, height=H, depth=32, bits=12)
    assert (d10.bit_depth, d12.bit_depth) == (10, 12)
    src = source(d10, seed=23)
    try:
        g = pkg.AvifGpu(devices=[gpu.device, gpu.device])

        def step(what, d, tw, th):
            want = _save(g, d, src, tw, th, "device")
            got = _save(g, d, src, tw, th, "host")
            assert int(want[1].sum()) == W * H and want[2].any() and want[3].any(), what      # the device path did count
            for name, a, b in zip(("bins", "sums", "counters"), got[1:], want[1:]):
                assert np.array_equal(a, b), (what, name, a.tolist(), b.tolist())
            assert got[0].keys() == want[0].keys()
            for pl in want[0]:
                assert np.array_equal(got[0][pl], want[0][pl]), (what, "plane", pl)
            return got

        step("1: thumbnail 3x2", d10, 3, 2)
        step("2: thumbnail 13x7, the first growth", d10, 13, 7)
        planes, bins, sums, counters = step("3: thumbnail 3x2 below the capacity", d10, 3, 2)

        # 4: rows outside the image, an ordinary error return; the targets keep what step 3 left in them
        kept = bins.copy(), sums.copy(), counters.copy()
        bufs = harness._alloc_write_out(d10, H)
        ptrs = [bufs[i].ctypes.data if i in bufs else None for i in range(4)]
        strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
        with pkg.code_histogram(bins, 10, pkg.MEM_HOST), pkg.thumbnail_sums(sums, 3, 2, pkg.MEM_HOST), pkg.plane_summary(counters, pkg.MEM_HOST):
            with pytest.raises(pkg.AvifGpuError) as e:
                g.write_rows(d10, 0, H + 2, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST)
        assert e.value.code == pkg.formatBadParameters
        for name, a, b in zip(("bins", "sums", "counters"), (bins, sums, counters), kept):
            assert np.array_equal(a, b), ("4: the failing call", name)

        step("5: thumbnail 13x7 again", d10, 13, 7)
        step("6a: 12 bit, 4096 bins", d12, 13, 7)
        step("6b: 10 bit again", d10, 13, 7)

        plain, none = write_summary(g, d10, src, mem="host", cuts=CUTS, arm=False)
        assert not none.any()
        for pl in planes:
            assert np.array_equal(plain[pl], planes[pl]), ("disarmed", pl)
    finally:
        pkg.AvifGpu(int(os.environ.get("LOCAL_RANK", "0")))                        # the rest of the suite runs on one binding
