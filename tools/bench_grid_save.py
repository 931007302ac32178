#!/usr/bin/env python3
"""What the grid save (avifgpu_write_rows_grid) costs on device pointers.  A measuring aid, no gate.  One JSON line per shape; every
comparison times its sides in ONE process, alternating, over FRESH data (calls rotate over >= 4 disjoint buffer sets, so nothing is served
from a cache the previous call filled); HIP events around back-to-back calls.

Shapes: the headline save (8192^2 RGB f32 -> 10-bit PQ 4:4:4, 2 x 2 tiles of 4096^2) and the default 12-bit 4:2:2 save of a 16-bit
document (same canvas and tiles).  Per shape:

  plain_save_ms        avifgpu_write_rows into planes whose base and pitch are multiples of 256
  grid_save_ms         avifgpu_write_rows_grid: the same save into scratch, then grid_scatter into the tiles
  grid_scatter_ms      grid_scatter ALONE (avifgpu_probe_grid_scatter) on the Y plane
  grid_scatter_all_planes_ms   grid_scatter alone on every plane, one launch per plane, back to back: the mover's share of a grid save
  grid_gather_ms       grid_gather ALONE (avifgpu_probe_grid_gather) at the mirrored shape: the same tiles back into a plane
  copy_ms              a device-to-device copy of the Y plane: the copy ceiling of this session

The yardsticks: grid_scatter against grid_gather at the same bytes; the grid save against the plain save plus one more read and one more
write of all output planes at the copy ceiling (extra_pass_at_copy_ceiling_ms)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def shapes(pkg, W, H):
    return [("headline rgb f32 -> 10-bit pq 4:4:4",
             pkg.WriteDesc(width=W, height=H, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=80, alpha_state=pkg.ALPHA_NONE,
                           output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)),
            ("default rgb16 -> 12-bit 4:2:2",
             pkg.WriteDesc(width=W, height=H, depth=16, planes=3, bit_depth=12, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422,
                           matrix_coefficients=pkg.MATRIX_BT601))]


def run(args):
    import numpy as np
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H, T = args.width, args.height, args.tile
    stream = torch.cuda.current_stream(dev).cuda_stream
    for label, d in shapes(pkg, W, H):
        grid = pkg.grid_fit(d, T, T, 2)
        cols, rows, tw, th = grid
        xs, ys = harness.chroma_shift(d.chroma)
        planes = {0: (W, H, tw, th), 1: ((W + xs) >> xs, (H + ys) >> ys, (tw + xs) >> xs, (th + ys) >> ys)}
        planes[2] = planes[1]
        src_row = W * 3 * (d.depth // 8)
        out_bytes = sum(pw * 2 * ph for pw, ph, _, _ in planes.values())
        sets = []
        for k in range(args.sets):
            if d.depth == 32:
                src = torch.rand((H, W * 3), device=dev, dtype=torch.float32)
            else:
                src = torch.randint(0, 32769, (H, W * 3), device=dev, dtype=torch.int32).to(torch.int16)
            plain = {pl: torch.empty((ph, pitch(pw * 2)), dtype=torch.uint8, device=dev) for pl, (pw, ph, _, _) in planes.items()}
            table = (pkg.GridTile * (cols * rows))()
            keep = []
            for t in range(cols * rows):
                for pl, (_, _, twp, thp) in planes.items():
                    a = torch.empty((thp, pitch(twp * 2)), dtype=torch.uint8, device=dev)
                    keep.append(a)
                    table[t].plane[pl] = a.data_ptr()
                    table[t].stride[pl] = a.stride(0)
            dtable = torch.from_numpy(np.frombuffer(bytes(table), dtype=np.uint8).copy()).to(dev)
            need = pkg.write_grid_scratch_bytes(d, H)
            scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
            back = torch.empty((H, pitch(W * 2)), dtype=torch.uint8, device=dev)
            sets.append(dict(src=src, plain=plain, keep=keep, dtable=dtable, scratch=scratch, need=need, back=back))

        def run_plain(k):
            s = sets[k % args.sets]
            gpu.write_rows(d, 0, H, s["src"].data_ptr(), src_row, [s["plain"][pl].data_ptr() for pl in range(3)] + [None],
                           [s["plain"][pl].stride(0) for pl in range(3)] + [0], mem=pkg.MEM_DEVICE, stream=stream)

        def run_grid(k):
            s = sets[k % args.sets]
            gpu.write_rows_grid(d, grid, s["dtable"].data_ptr(), 0, H, s["src"].data_ptr(), src_row, s["scratch"].data_ptr(), s["need"], mem=pkg.MEM_DEVICE, stream=stream)

        def run_scatter(k):
            s = sets[k % args.sets]
            gpu.probe_grid_scatter(s["dtable"].data_ptr(), cols, 0, tw, th, 2, W, H, 0, rows * th, s["plain"][0].data_ptr(), s["plain"][0].stride(0), stream)

        def run_scatter_all(k):
            s = sets[k % args.sets]
            for pl, (pw, ph, twp, thp) in planes.items():
                gpu.probe_grid_scatter(s["dtable"].data_ptr(), cols, pl, twp, thp, 2, pw, ph, 0, rows * thp, s["plain"][pl].data_ptr(), s["plain"][pl].stride(0), stream)

        def run_gather(k):
            s = sets[k % args.sets]
            gpu.probe_grid_gather(s["dtable"].data_ptr(), cols, 0, tw, th, 2, 0, 0, W, H, s["back"].data_ptr(), s["back"].stride(0), stream)

        def run_copy(k):
            s = sets[k % args.sets]
            s["back"].copy_(s["plain"][0], non_blocking=True)

        t = {}
        for name, fn in (("plain_save_ms", run_plain), ("grid_save_ms", run_grid), ("grid_scatter_ms", run_scatter), ("grid_gather_ms", run_gather), ("copy_ms", run_copy),
                         ("grid_scatter_all_planes_ms", run_scatter_all)) * 2:
            if args.only and name != args.only:                      # a kernel trace of one side alone (rocprofv3 --kernel-trace --stats)
                continue
            t.setdefault(name, []).append(round(timed(torch, dev, args, fn), 5))
        if args.only:
            print(json.dumps({"case": label, "only": args.only, **t}), flush=True)
            del sets
            torch.cuda.empty_cache()
            continue
        # the bytes: the tiles of a grid save are the padded split of the plain save's planes, and the gather of them is the plane again
        run_plain(0); run_grid(0); run_gather(0)
        torch.cuda.synchronize(dev)
        s = sets[0]
        same = bool(torch.equal(s["back"][:, :W * 2], s["plain"][0][:, :W * 2]))
        y_bytes = W * 2 * H
        copy_rate = 2 * y_bytes / (min(t["copy_ms"]) * 1e-3)
        extra = 2 * out_bytes / copy_rate * 1e3
        print(json.dumps({"measurement": "grid save on device pointers, HIP events around back-to-back calls", "case": label, "image": f"{W}x{H}", "grid": list(grid),
                          "buffer_sets": args.sets, "launches": args.steps, **t, "y_plane_bytes": y_bytes, "output_bytes": out_bytes,
                          "copy_ceiling_TBs": round(copy_rate / 1e12, 3),
                          "scatter_over_gather": round(min(t["grid_scatter_ms"]) / min(t["grid_gather_ms"]), 4),
                          "extra_pass_at_copy_ceiling_ms": round(extra, 5),
                          "grid_save_minus_plain_ms": round(min(t["grid_save_ms"]) - min(t["plain_save_ms"]), 5),
                          "gather_of_the_saved_tiles_is_the_plain_y_plane": same}), flush=True)
        del sets
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--tile", type=int, default=4096, help="cap on a tile's side (avifgpu_grid_fit picks the grid)")
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="time this one measurement alone, e.g. grid_save_ms, for a kernel trace")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
