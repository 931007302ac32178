"""The code histogram at FULL size on one MI355X: the headline frame (8192^2 RGB f32 -> 10-bit PQ) and the plug-in's default HDR save
(12-bit 4:2:2).  The persistent grid, the flat walk of 67 M pixels as one row and counters beyond 2^16 per workgroup exist only here.
 * the bins equal torch.bincount of the max code of what the same call wrote in OUT_REFERENCE form, and the fused-output call of the
   same frame counts the same bins (stage A is shared);
 * against the all-cores oracle: sum |count_gpu - count_oracle| <= 2 u, u = pixels with an undetermined colour sample (the mask
   computed on the device in float64, as tests/test_gpu_fullsize.py does);
 * a flat frame and a two-valued checker frame: exact."""
import numpy as np
import pytest

import harness
import test_gpu_fullsize as fs
import truth64

pkg = harness.pkg
pytestmark = pytest.mark.gpu

CONFIGS = {
    "C4-8192-f32-pq-10bit-444": fs.CONFIGS["C4-8192-f32-pq-10bit-444"],
    "D12-8192-f32-pq-12bit-422-nearest": fs.CONFIGS["D12-8192-f32-pq-12bit-422-nearest (the plug-in's default HDR save)"],
}


def _armed_run(gpu, torch, dev, d, frame):
    bins = torch.zeros(1 << d.bit_depth, dtype=torch.int64, device=dev)
    with pkg.code_histogram(bins, d.bit_depth, pkg.MEM_DEVICE):
        out = fs._run(gpu, torch, dev, d, frame, [(0, d.height)])
    return out, bins


def _max_codes(torch, d, plane0):
    return plane0.view(torch.int16).view(d.height, d.width, 3).to(torch.int64).amax(dim=2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fullsize_bins(gpu, name):
    import torch
    dev = f"cuda:{gpu.device}"
    d = pkg.WriteDesc(**CONFIGS[name])
    dref = pkg.WriteDesc(**dict(CONFIGS[name], output=pkg.OUT_REFERENCE))
    nb = 1 << d.bit_depth
    frame = fs._device_frame(torch, dev, d)
    _, bins = _armed_run(gpu, torch, dev, d, frame)
    kernel = gpu.last_kernel()
    written, bins_ref = _armed_run(gpu, torch, dev, dref, frame)
    assert int(bins.sum()) == d.width * d.height
    assert torch.equal(bins, bins_ref), name                                        # both outputs share stage A
    want = torch.bincount(_max_codes(torch, d, written[0]).view(-1), minlength=nb)
    assert torch.equal(bins_ref, want), (name, int((bins_ref - want).abs().sum()))
    del written
    # the oracle on every host core, and the pixels that may differ from it
    host = frame.cpu().numpy()
    oracle = fs._oracle_frame(dref, host)
    om = np.ascontiguousarray(oracle[0][:, :d.width * 3]).astype(np.int64).reshape(d.height, d.width, 3).max(axis=2)
    want_o = torch.from_numpy(np.bincount(om.reshape(-1), minlength=nb)).to(dev)
    u = int((~fs._determined_pixels(torch, d, frame)).sum())
    dist = int((bins - want_o).abs().sum())
    print(f"{name}: kernel {kernel}; {d.width * d.height} pixels, {u} undetermined, sum |dcount| against the oracle = {dist}")
    assert dist <= 2 * u, (name, dist, u)
    # 8 even row tiles (the 8-GPU sharding) count the same bins
    tiled = torch.zeros(nb, dtype=torch.int64, device=dev)
    with pkg.code_histogram(tiled, d.bit_depth, pkg.MEM_DEVICE):
        fs._run(gpu, torch, dev, d, frame, pkg.sharding.all_tiles(d.height, 8))
    assert torch.equal(tiled, bins), name


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fullsize_flat_and_checker_frames_are_exact(gpu, name):
    import torch
    dev = f"cuda:{gpu.device}"
    d = pkg.WriteDesc(**CONFIGS[name])
    nb = 1 << d.bit_depth
    # the codes of the two pixel values, from the oracle on a 2 x 2 tile
    tiny = pkg.WriteDesc(**dict(CONFIGS[name], width=2, height=2, output=pkg.OUT_REFERENCE))
    a, b = (0.18, 0.21, 0.05), (0.9, 3.5, 0.02)
    src = np.array([[*a, *b], [*b, *a]], dtype=np.float32)
    codes = harness.oracle_write(tiny, src)[0].astype(np.int64).reshape(2, 2, 3).max(axis=2)
    assert truth64.determined_codes(tiny, src)[1].all()                             # away from code boundaries: oracle and kernel must agree
    ca, cb = int(codes[0, 0]), int(codes[0, 1])
    assert ca != cb and codes[1, 0] == cb and codes[1, 1] == ca
    n = d.width * d.height
    flat = torch.tensor(a, dtype=torch.float32, device=dev).repeat(n).view(d.height, d.width * 3)
    _, bins = _armed_run(gpu, torch, dev, d, flat)
    want = torch.zeros(nb, dtype=torch.int64, device=dev)
    want[ca] = n
    assert torch.equal(bins, want), (name, "flat", bins.nonzero().view(-1).tolist()[:8])
    del flat
    x = torch.arange(d.width, device=dev).view(1, d.width, 1)
    y = torch.arange(d.height, device=dev).view(d.height, 1, 1)
    odd = ((x + y) & 1).bool()
    checker = torch.where(odd, torch.tensor(b, dtype=torch.float32, device=dev).view(1, 1, 3),
                          torch.tensor(a, dtype=torch.float32, device=dev).view(1, 1, 3)).contiguous().view(d.height, d.width * 3)
    _, bins = _armed_run(gpu, torch, dev, d, checker)
    want.zero_()
    want[ca] = n // 2
    want[cb] = n // 2
    assert torch.equal(bins, want), (name, "checker", bins.nonzero().view(-1).tolist()[:8])
