#!/usr/bin/env python3
"""What the code histogram of a 32-bit save (avifgpu_histogram_attach) costs, on the headline frame (8192^2 RGB f32 -> 10-bit PQ
YCbCr 4:4:4).  One JSON line per measurement.

  --host-gate          the frame through avifgpu_write_rows(AVIFGPU_MEM_HOST) from page-locked memory, armed and not armed, alternating
                       in one process: best of N and median of each, and their ratio (the gate: armed <= 1.05 x unarmed).
  --device FRAME...    device pointers, FRESH data (launches rotate over >= 4 disjoint buffer sets, 3.2 GB of sources between two visits
                       of an address), HIP events around K back-to-back launches: the conversion kernel, the histogram kernel alone
                       (avifgpu_probe_histogram), its atomics-free and math-free twins, and the armed call (conversion + histogram).
                       FRAME: noise (harness.make_write_source's distribution), flat, checker (two values), ramp (horizontal).
                       Run it under `rocprofv3 --kernel-trace --stats -d DIR/FRAME -- python tools/bench_light_level.py --device FRAME`
                       for the kernel times themselves, then
  --summarize DIR      per FRAME directory: every kernel's launches from the trace (the first --warmup of each name dropped), mean /
                       median / min, the histogram kernel's ratio to the conversion kernel and its fraction of 8 TB/s over 12 B/px."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BYTES_S = 8.0e12


def headline(pkg, W, H):
    return pkg.WriteDesc(width=W, height=H, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=80,
                         alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444,
                         matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)


def make_frame(torch, kind, W, H, dev, seed):
    if kind == "noise":
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        n = H * W * 3
        t = torch.rand(n, generator=g, device=dev, dtype=torch.float32)
        m = torch.rand(n, generator=g, device=dev, dtype=torch.float32)
        t = torch.where(m < 0.10, 1.0 + 11.5 * t, t)
        t = torch.where(m > 0.999, -0.01 * t, t)
        return t.view(H, W * 3)
    if kind == "flat":
        return torch.full((H, W * 3), 0.18, device=dev, dtype=torch.float32)
    if kind == "checker":
        x = torch.arange(W, device=dev).view(1, W, 1)
        y = torch.arange(H, device=dev).view(H, 1, 1)
        return torch.where(((x + y) & 1).bool(), 0.9, 0.05).to(torch.float32).expand(H, W, 3).contiguous().view(H, W * 3)
    if kind == "ramp":
        x = torch.linspace(0.0, 4.0, W, device=dev, dtype=torch.float32).view(1, W, 1)
        return x.expand(H, W, 3).contiguous().view(H, W * 3)
    raise SystemExit(f"unknown frame {kind}")


def host_gate(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H = args.width, args.height
    d = headline(pkg, W, H)
    src = torch.rand((H, W * 3), dtype=torch.float32).pin_memory()
    outs = [torch.empty((H, W * 2), dtype=torch.uint8).pin_memory() for _ in range(3)]
    ptrs = [o.data_ptr() for o in outs] + [None]
    strides = [o.stride(0) for o in outs] + [0]
    bins = torch.zeros(1024, dtype=torch.int64).numpy().view("uint64")

    def once(armed):
        t0 = time.perf_counter()
        if armed:
            with pkg.code_histogram(bins, 10, pkg.MEM_HOST):
                gpu.write_rows(d, 0, H, src.data_ptr(), src.stride(0) * 4, ptrs, strides, mem=pkg.MEM_HOST)
        else:
            gpu.write_rows(d, 0, H, src.data_ptr(), src.stride(0) * 4, ptrs, strides, mem=pkg.MEM_HOST)
        return time.perf_counter() - t0
    for _ in range(2):
        once(False)
        once(True)
    ref = [o.clone() for o in outs]
    t = {False: [], True: []}
    for _ in range(args.reps):                                     # alternating: both see the same box
        for armed in (False, True):
            t[armed].append(once(armed))
    same = all(bool((a == b).all()) for a, b in zip(ref, outs))
    counted = int(bins.sum())
    res = {"measurement": "host gate", "config": f"{W}x{H} RGB f32 -> 10-bit PQ YCbCr 4:4:4, host pointers, page-locked", "reps": args.reps,
           "unarmed_best_ms": round(min(t[False]) * 1e3, 3), "unarmed_median_ms": round(statistics.median(t[False]) * 1e3, 3),
           "armed_best_ms": round(min(t[True]) * 1e3, 3), "armed_median_ms": round(statistics.median(t[True]) * 1e3, 3),
           "planes_identical": same, "pixels_counted_per_armed_call": counted // (args.reps + 2), "kernel": gpu.last_kernel()}
    res["ratio_best"] = round(res["armed_best_ms"] / res["unarmed_best_ms"], 4)
    res["ratio_median"] = round(res["armed_median_ms"] / res["unarmed_median_ms"], 4)
    res["gate_armed_within_5_percent"] = bool(res["ratio_best"] <= 1.05)
    print(json.dumps(res), flush=True)


def device(args):
    import ctypes
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    lib = gpu.lib
    dev = f"cuda:{gpu.device}"
    W, H = args.width, args.height
    d = headline(pkg, W, H)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for kind in args.device:
        sets = []
        for k in range(args.sets):                                  # disjoint buffers: a launch never finds its lines in the caches
            sets.append((make_frame(torch, kind, W, H, dev, 1234 + k), [torch.empty((H, W * 2), dtype=torch.uint8, device=dev) for _ in range(3)]))
        bins = torch.zeros(1024, dtype=torch.int64, device=dev)

        def conv(k):
            f, o = sets[k % args.sets]
            gpu.write_rows(d, 0, H, f.data_ptr(), f.stride(0) * 4, [x.data_ptr() for x in o] + [None], [x.stride(0) for x in o] + [0],
                           mem=pkg.MEM_DEVICE, stream=stream)

        def hist(twin):
            def go(k):
                f, _ = sets[k % args.sets]
                rc = lib.avifgpu_probe_histogram(ctypes.byref(d), twin, f.data_ptr(), f.stride(0) * 4, bins.data_ptr(), stream)
                if rc:
                    raise SystemExit(lib.avifgpu_last_error().decode())
            return go

        def timed(fn):
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
        res = {"measurement": "device path, HIP events around back-to-back launches", "frame": kind, "config": f"{W}x{H} RGB f32, 10-bit PQ",
               "buffer_sets": args.sets, "launches": args.steps}
        res["conversion_ms"] = round(timed(conv), 5)
        res["conversion_kernel"] = gpu.last_kernel()
        bins.zero_()
        res["histogram_ms"] = round(timed(hist(0)), 5)
        counted = int(bins.sum().item())
        res["histogram_counts_ok"] = counted == (args.steps + args.warmup) * W * H
        res["atomics_free_twin_ms"] = round(timed(hist(1)), 5)
        res["math_free_twin_ms"] = round(timed(hist(2)), 5)
        with pkg.code_histogram(bins, 10, pkg.MEM_DEVICE):
            res["armed_call_ms"] = round(timed(conv), 5)
        res["ratio_histogram_to_conversion"] = round(res["histogram_ms"] / res["conversion_ms"], 4)
        res["histogram_fraction_of_8TBs_at_12Bpx"] = round(W * H * 12 / (res["histogram_ms"] * 1e-3) / PEAK_BYTES_S, 4)
        print(json.dumps(res), flush=True)
        del sets


def summarize(args):
    for frame_dir in sorted(glob.glob(os.path.join(args.summarize, "*"))):
        if not os.path.isdir(frame_dir):
            continue
        rows = {}
        for f in glob.glob(frame_dir + "/**/*kernel_trace.csv", recursive=True):
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        out = {"measurement": "kernel trace (rocprofv3 --kernel-trace)", "frame": os.path.basename(frame_dir), "kernels": {}}
        for name, v in rows.items():
            if "write_hist_px" not in name and "write_rgb32_ycbcr444_hot" not in name:
                continue
            v.sort()
            dur = [x[1] for x in v][args.warmup:] or [x[1] for x in v]
            out["kernels"][name.replace("avifgpu::", "").replace("(avifgpu::WriteParams, avifgpu::HistParams)", "").replace("(avifgpu::WriteParams)", "")] = {
                "launches": len(dur), "mean_us": round(statistics.mean(dur) / 1e3, 2), "median_us": round(statistics.median(dur) / 1e3, 2),
                "min_us": round(min(dur) / 1e3, 2)}
        conv = [k for k in out["kernels"] if "ycbcr444_hot" in k]
        for k, s in out["kernels"].items():
            if "write_hist_px" in k:
                s["fraction_of_8TBs_at_12Bpx"] = round(args.width * args.height * 12 / (s["median_us"] * 1e-6) / PEAK_BYTES_S, 4)
                if conv:
                    s["ratio_to_conversion_median"] = round(s["median_us"] / out["kernels"][conv[0]]["median_us"], 4)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host-gate", action="store_true")
    ap.add_argument("--device", nargs="+", metavar="FRAME")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_light_level.py measures on the GPU: no device, no number")
    if args.host_gate:
        host_gate(args)
    if args.device:
        device(args)


if __name__ == "__main__":
    main()
