#!/usr/bin/env python3
"""What the grid open (avifgpu_read_rows_grid) costs, 8192^2 8-bit 4:2:0 in 512^2 tiles by default.  A measuring aid, no gate.  One JSON
line per measurement; every comparison times both sides in ONE process, alternating, over FRESH data (calls rotate over >= 4 disjoint
buffer sets, so nothing is served from a cache the previous call filled).

  --gather   grid_gather ALONE (avifgpu_probe_grid_gather) on the Y plane -- tiles of their own allocations, 256-byte pitches -- beside
             crop_rows (avifgpu_probe_crop) on the same byte count; HIP events around back-to-back launches.  The expectation of the grid
             open's design is a ratio crop_rows_ms / grid_gather_ms of at least 0.8.
  --open     device pointers: the grid open (gather + cropped open on the gathered planes) beside avifgpu_read_rows_cropped on
             pre-assembled planes, whole canvas, nearest code 1 / nearest code 6 / bilinear code 1: what the extra pass costs.
  --host     host pointers, page-locked: the grid open (one strided copy per tile piece, assembled by the copy engine) beside numpy
             assembly of the canvas on the CPU followed by the cropped open of it; wall clock, best and median of N."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BYTES_S = 8.0e12


def pitch(nbytes):
    return (nbytes + 255) // 256 * 256


def timed(torch, dev, args, fn):
    for k in range(args.warmup):
        fn(k)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(args.steps):
        fn(k)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / args.steps


def desc_of(pkg, W, H):
    return pkg.ReadDesc(width=W, height=H, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE,
                        matrix_coefficients=pkg.MATRIX_BT601)


def plane_dims(W, H, T):
    """{plane: (canvas columns, canvas rows, tile columns, tile rows)} of an 8-bit 4:2:0 image"""
    return {0: (W, H, T, T), 1: ((W + 1) // 2, (H + 1) // 2, T // 2, T // 2), 2: ((W + 1) // 2, (H + 1) // 2, T // 2, T // 2)}


def device_tiles(torch, pkg, dev, W, H, T, seed):
    """(one tensor per tile and plane, the device table, the assembled planes as tensors): random tiles, rows of 256-byte pitch"""
    import numpy as np
    cols, rows = (W + T - 1) // T, (H + T - 1) // T
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    table = (pkg.GridTile * (cols * rows))()
    keep, whole = [], {}
    for pl, (cw, ch, tw, th) in plane_dims(W, H, T).items():
        canvas = torch.empty((rows * th, pitch(cols * tw)), dtype=torch.uint8, device=dev)
        for k in range(cols * rows):
            t = torch.randint(0, 256, (th, pitch(tw)), generator=g, device=dev, dtype=torch.uint8)
            keep.append(t)
            table[k].plane[pl] = t.data_ptr()
            table[k].stride[pl] = t.stride(0)
            c, r = k % cols, k // cols
            canvas[r * th:(r + 1) * th, c * tw:(c + 1) * tw] = t[:, :tw]
        whole[pl] = canvas
    dtable = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
    return keep, dtable, whole, (cols, rows, T, T)


def gather(args):
    import numpy as np
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H, T = args.width, args.height, args.tile
    stream = torch.cuda.current_stream(dev).cuda_stream
    sets = [device_tiles(torch, pkg, dev, W, H, T, 11 + k) for k in range(args.sets)]
    grid = sets[0][3]
    dp = pitch(W)
    dst = [torch.empty(H * dp, dtype=torch.uint8, device=dev) for _ in range(args.sets)]
    src = [torch.randint(0, 256, (H * dp,), device=dev, dtype=torch.uint8) for _ in range(args.sets)]
    cdst = [torch.empty(H * dp, dtype=torch.uint8, device=dev) for _ in range(args.sets)]

    def run_gather(k):
        gpu.probe_grid_gather(sets[k % args.sets][1].data_ptr(), grid[0], 0, T, T, 1, 0, 0, W, H, dst[k % args.sets].data_ptr(), dp, stream)

    def run_crop(k):
        gpu.probe_crop(src[k % args.sets].data_ptr(), dp, cdst[k % args.sets].data_ptr(), dp, W, H, stream)

    res = {"measurement": "grid_gather alone beside crop_rows on the same bytes, device pointers, HIP events around back-to-back launches", "plane": "Y",
           "image": f"{W}x{H}", "tile": T, "tiles": grid[0] * grid[1], "buffer_sets": args.sets, "launches": args.steps, "bytes_moved": 2 * W * H}
    g0 = timed(torch, dev, args, run_gather)
    c0 = timed(torch, dev, args, run_crop)
    g1 = timed(torch, dev, args, run_gather)
    c1 = timed(torch, dev, args, run_crop)
    gm, cm = min(g0, g1), min(c0, c1)
    res.update(grid_gather_ms=[round(g0, 5), round(g1, 5)], crop_rows_ms=[round(c0, 5), round(c1, 5)],
               grid_gather_fraction_of_8TBs=round(2 * W * H / (gm * 1e-3) / PEAK_BYTES_S, 4), crop_rows_fraction_of_8TBs=round(2 * W * H / (cm * 1e-3) / PEAK_BYTES_S, 4),
               crop_rows_ms_over_grid_gather_ms=round(cm / gm, 4))
    run_gather(0)
    torch.cuda.synchronize(dev)
    res["rows_correct"] = bool(torch.equal(dst[0].view(H, dp)[:, :W], sets[0][2][0][:H, :W]))
    print(json.dumps(res), flush=True)


def open_device(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H, T = args.width, args.height, args.tile
    d = desc_of(pkg, W, H)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sets = [device_tiles(torch, pkg, dev, W, H, T, 31 + k) for k in range(args.sets)]
    grid = sets[0][3]
    rect = (0, 0, W, H)
    side = max(W, H)
    outs = [torch.empty(side * pitch(side * 3), dtype=torch.uint8, device=dev) for _ in range(args.sets)]
    for mode, code, label in ((0, 1, "nearest code 1"), (0, 6, "nearest code 6"), (1, 1, "bilinear code 1")):
        out_w, out_h = pkg.read_cropped_geometry(d, rect, code)
        need_g = pkg.read_grid_scratch_bytes(d, grid, None, mode, code, out_h)
        need_c = max(pkg.read_cropped_scratch_bytes(d, rect, mode, code, out_h), 16)
        scratch = [torch.empty(max(need_g, need_c), dtype=torch.uint8, device=dev) for _ in range(args.sets)]

        def run_grid(k):
            gpu.read_rows_grid(d, grid, sets[k % args.sets][1].data_ptr(), None, mode, code, 0, out_h, outs[k % args.sets].data_ptr(), pitch(out_w * 3),
                               scratch[k % args.sets].data_ptr(), need_g, mem=pkg.MEM_DEVICE, stream=stream)

        def run_cropped(k):
            whole = sets[k % args.sets][2]
            gpu.read_rows_cropped(d, rect, mode, code, 0, out_h, [whole[0].data_ptr(), whole[1].data_ptr(), whole[2].data_ptr(), None],
                                  [whole[0].stride(0), whole[1].stride(0), whole[2].stride(0), 0], outs[k % args.sets].data_ptr(), pitch(out_w * 3),
                                  scratch[k % args.sets].data_ptr(), need_c, mem=pkg.MEM_DEVICE, stream=stream)
        c0 = timed(torch, dev, args, run_cropped)
        g0 = timed(torch, dev, args, run_grid)
        c1 = timed(torch, dev, args, run_cropped)
        g1 = timed(torch, dev, args, run_grid)
        run_grid(0)
        torch.cuda.synchronize(dev)
        got = outs[0][:out_h * pitch(out_w * 3)].clone()
        run_cropped(0)
        torch.cuda.synchronize(dev)
        same = bool(torch.equal(got.view(out_h, -1)[:, :out_w * 3], outs[0][:out_h * pitch(out_w * 3)].view(out_h, -1)[:, :out_w * 3]))
        print(json.dumps({"measurement": "open on device pointers, HIP events around back-to-back calls", "case": label, "image": f"{W}x{H}", "tile": T,
                          "buffer_sets": args.sets, "launches": args.steps, "cropped_on_assembled_planes_ms": [round(c0, 5), round(c1, 5)],
                          "grid_open_ms": [round(g0, 5), round(g1, 5)], "grid_over_cropped": round(min(g0, g1) / min(c0, c1), 4), "scratch_bytes": need_g,
                          "same_bytes": same}), flush=True)
        del scratch
        torch.cuda.empty_cache()


def host(args):
    import numpy as np
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H, T = args.width, args.height, args.tile
    d = desc_of(pkg, W, H)
    cols, rows = (W + T - 1) // T, (H + T - 1) // T
    grid = (cols, rows, T, T)
    dims = plane_dims(W, H, T)
    table = (pkg.GridTile * (cols * rows))()
    tiles = []
    for k in range(cols * rows):
        t = {}
        for pl, (cw, ch, tw, th) in dims.items():
            a = torch.randint(0, 256, (th, pitch(tw)), dtype=torch.uint8).pin_memory()
            t[pl] = a
            table[k].plane[pl] = a.data_ptr()
            table[k].stride[pl] = a.stride(0)
        tiles.append(t)
    canvas = {pl: torch.empty((rows * th, pitch(cols * tw)), dtype=torch.uint8).pin_memory() for pl, (cw, ch, tw, th) in dims.items()}
    out = torch.empty((H, W * 3), dtype=torch.uint8).pin_memory()
    out2 = torch.empty((H, W * 3), dtype=torch.uint8).pin_memory()

    def run_grid():
        t0 = time.perf_counter()
        gpu.read_rows_grid(d, grid, table, None, 0, 1, 0, H, out.data_ptr(), out.stride(0), mem=pkg.MEM_HOST)
        return time.perf_counter() - t0

    def run_cpu():
        t0 = time.perf_counter()
        for pl, (cw, ch, tw, th) in dims.items():
            c = canvas[pl].numpy()
            for k in range(cols * rows):
                c[(k // cols) * th:(k // cols + 1) * th, (k % cols) * tw:(k % cols + 1) * tw] = tiles[k][pl].numpy()[:, :tw]
        t1 = time.perf_counter()
        gpu.read_rows_cropped(d, (0, 0, W, H), 0, 1, 0, H, [canvas[0].data_ptr(), canvas[1].data_ptr(), canvas[2].data_ptr(), None],
                              [canvas[0].stride(0), canvas[1].stride(0), canvas[2].stride(0), 0], out2.data_ptr(), out2.stride(0), mem=pkg.MEM_HOST)
        return time.perf_counter() - t0, t1 - t0

    run_grid(); run_cpu()
    tg, tc, ta = [], [], []
    for _ in range(args.host_passes):
        tg.append(run_grid())
        c, a = run_cpu()
        tc.append(c); ta.append(a)
    print(json.dumps({"measurement": "host pointers (page-locked), wall clock, alternating in one process", "case": "nearest code 1, whole canvas", "image": f"{W}x{H}",
                      "tile": T, "passes": args.host_passes, "grid_open_ms": {"best": round(min(tg) * 1e3, 3), "median": round(statistics.median(tg) * 1e3, 3)},
                      "numpy_assembly_plus_cropped_open_ms": {"best": round(min(tc) * 1e3, 3), "median": round(statistics.median(tc) * 1e3, 3)},
                      "numpy_assembly_alone_ms": {"best": round(min(ta) * 1e3, 3), "median": round(statistics.median(ta) * 1e3, 3)},
                      "grid_over_cpu_assembly_path": round(min(tg) / min(tc), 4), "same_bytes": bool(np.array_equal(out.numpy(), out2.numpy()))}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--open", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--host-passes", type=int, default=7)
    args = ap.parse_args()
    if args.tile % 2:
        ap.error("--tile must be even (4:2:0)")
    if not (args.gather or args.open or args.host):
        args.gather = args.open = args.host = True
    if args.gather:
        gather(args)
    if args.open:
        open_device(args)
    if args.host:
        host(args)


if __name__ == "__main__":
    main()
