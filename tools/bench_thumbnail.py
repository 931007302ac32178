#!/usr/bin/env python3
"""What the box-average thumbnail of a save (avifgpu_thumbnail_attach) costs, 8192^2 frames, 256 x 256 thumbnail.  One JSON line per
measurement.

  --host-gate          the headline frame (C4: RGB f32 -> 10-bit PQ YCbCr 4:4:4) through avifgpu_write_rows(AVIFGPU_MEM_HOST) from
                       page-locked memory, armed and not armed, alternating in one process: best of N and median of each, and their
                       ratio (the gate: armed <= 1.05 x unarmed).
  --device CONFIG...   device pointers, FRESH data (launches rotate over >= 4 disjoint buffer sets), HIP events around K back-to-back
                       launches: the conversion kernel, the thumbnail kernel alone on the planes it wrote (avifgpu_probe_thumbnail), its
                       atomics-free twin, and the armed call (conversion + thumbnail).  CONFIG: c4 (10-bit 4:4:4 planes, 6 B/px read), d12 (12-bit 4:2:2
                       nearest, 4 B/px), sdr8 (RGB8 -> 8-bit 4:2:2 nearest, 2 B/px), ref8 (RGB8 -> interleaved RGB, 3 B/px).
                       Run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR/CONFIG -- python tools/bench_thumbnail.py --device CONFIG`
                       for the kernel times themselves, then
  --summarize DIR      per CONFIG directory: every kernel's launches from the trace (the first --warmup of each name dropped), mean /
                       median / min, the thumbnail kernel's ratio to the conversion kernel and its fraction of 8 TB/s over the bytes
                       it reads."""
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
TW = TH = 256


def config(pkg, name, W, H):
    """(descriptor, source dtype name, bytes per pixel the thumbnail kernel reads)"""
    hdr = dict(width=W, height=H, depth=32, planes=3, transfer=pkg.TRANSFER_PQ, peak_nits=80, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
               matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
    sdr = dict(width=W, height=H, depth=8, planes=3, bit_depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT601,
               color_primaries=pkg.PRIMARIES_BT709)
    if name == "c4":
        return pkg.WriteDesc(bit_depth=10, chroma=pkg.CHROMA_444, **hdr), "float32", 6.0
    if name == "d12":
        return pkg.WriteDesc(bit_depth=12, chroma=pkg.CHROMA_422, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST, **hdr), "float32", 4.0
    if name == "sdr8":
        return pkg.WriteDesc(output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST, **sdr), "uint8", 2.0
    if name == "ref8":
        return pkg.WriteDesc(output=pkg.OUT_REFERENCE, **sdr), "uint8", 3.0
    raise SystemExit(f"unknown config {name}")


def host_gate(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H = args.width, args.height
    d, _, _ = config(pkg, "c4", W, H)
    src = torch.rand((H, W * 3), dtype=torch.float32).pin_memory()
    outs = [torch.empty((H, W * 2), dtype=torch.uint8).pin_memory() for _ in range(3)]
    ptrs = [o.data_ptr() for o in outs] + [None]
    strides = [o.stride(0) for o in outs] + [0]
    sums = torch.zeros(TW * TH * 3, dtype=torch.int64).numpy().view("uint64")

    def once(armed):
        t0 = time.perf_counter()
        if armed:
            with pkg.thumbnail_sums(sums, TW, TH, pkg.MEM_HOST):
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
    total = sum(int(o.view(torch.int16).to(torch.int64).sum()) for o in outs)         # the codes of the planes, summed on the host
    res = {"measurement": "host gate", "config": f"{W}x{H} RGB f32 -> 10-bit PQ YCbCr 4:4:4, host pointers, page-locked, thumbnail {TW}x{TH}",
           "reps": args.reps,
           "unarmed_best_ms": round(min(t[False]) * 1e3, 3), "unarmed_median_ms": round(statistics.median(t[False]) * 1e3, 3),
           "armed_best_ms": round(min(t[True]) * 1e3, 3), "armed_median_ms": round(statistics.median(t[True]) * 1e3, 3),
           "planes_identical": same, "sums_equal_the_planes_total": int(sums.sum()) == total * (args.reps + 2), "kernel": gpu.last_kernel()}
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
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name in args.device:
        d, dt, bpp = config(pkg, name, W, H)
        geom = harness.write_planes(d)
        ssz = 2 if d.bit_depth > 8 else 1
        sets = []
        for k in range(args.sets):                                  # disjoint buffers: a launch never finds its lines in the caches
            g = torch.Generator(device=dev)
            g.manual_seed(1234 + k)
            if dt == "float32":
                f = torch.rand((H, W * 3), generator=g, device=dev, dtype=torch.float32)
            else:
                f = torch.randint(0, 256, (H, W * 3), generator=g, device=dev, dtype=torch.uint8)
            o = {pl: torch.empty(((H + ys) >> ys, w * ssz), dtype=torch.uint8, device=dev) for pl, (w, xs, ys) in geom.items()}
            sets.append((f, o))
        sums = torch.zeros(TW * TH * 3, dtype=torch.int64, device=dev)

        def planes_of(o):
            return [o[i].data_ptr() if i in o else None for i in range(4)], [o[i].stride(0) if i in o else 0 for i in range(4)]

        def conv(k):
            f, o = sets[k % args.sets]
            ptrs, strides = planes_of(o)
            gpu.write_rows(d, 0, H, f.data_ptr(), f.stride(0) * f.element_size(), ptrs, strides, mem=pkg.MEM_DEVICE, stream=stream)

        def thumb(k, twin=0):
            _, o = sets[k % args.sets]
            ptrs, strides = planes_of(o)
            rc = lib.avifgpu_probe_thumbnail(ctypes.byref(d), twin, TW, TH, ctypes.byref((ctypes.c_void_p * 4)(*ptrs)),
                                             ctypes.byref((ctypes.c_int64 * 4)(*strides)), sums.data_ptr(), stream)
            if rc:
                raise SystemExit(lib.avifgpu_last_error().decode())

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
        res = {"measurement": "device path, HIP events around back-to-back launches", "config": name, "frame": f"{W}x{H}", "thumbnail": f"{TW}x{TH}",
               "thumbnail_reads_bytes_per_px": bpp, "buffer_sets": args.sets, "launches": args.steps}
        res["conversion_ms"] = round(timed(conv), 5)
        res["conversion_kernel"] = gpu.last_kernel()
        sums.zero_()
        res["thumbnail_ms"] = round(timed(thumb), 5)
        total = sum(int(p.view(torch.int16 if ssz == 2 else torch.uint8).to(torch.int64).sum()) for _, o in sets for p in o.values())
        launches = args.steps + args.warmup
        res["sums_equal_the_planes_total"] = launches % args.sets == 0 and int(sums.sum()) == total * (launches // args.sets)
        res["atomics_free_twin_ms"] = round(timed(lambda k: thumb(k, 1)), 5)
        with pkg.thumbnail_sums(sums, TW, TH, pkg.MEM_DEVICE):
            res["armed_call_ms"] = round(timed(conv), 5)
        res["ratio_thumbnail_to_conversion"] = round(res["thumbnail_ms"] / res["conversion_ms"], 4)
        res["thumbnail_fraction_of_8TBs"] = round(W * H * bpp / (res["thumbnail_ms"] * 1e-3) / PEAK_BYTES_S, 4)
        print(json.dumps(res), flush=True)
        del sets


def summarize(args):
    import harness
    pkg = harness.pkg
    for cfg_dir in sorted(glob.glob(os.path.join(args.summarize, "*"))):
        if not os.path.isdir(cfg_dir):
            continue
        name = os.path.basename(cfg_dir)
        try:
            _, _, bpp = config(pkg, name, args.width, args.height)
        except SystemExit:
            continue
        rows = {}
        for f in glob.glob(cfg_dir + "/**/*kernel_trace.csv", recursive=True):
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        out = {"measurement": "kernel trace (rocprofv3 --kernel-trace)", "config": name, "kernels": {}}
        for kname, v in rows.items():
            if "avifgpu::" not in kname:
                continue
            v.sort()
            short = kname.replace("avifgpu::", "").replace("(anonymous namespace)::", "").replace("(ThumbParams)", "").replace("(WriteParams)", "")
            # --device launches the thumbnail kernel in three series of warmup + steps: alone, its atomics-free twin, behind the conversion
            n = args.warmup + args.steps
            series = [(short, v)]
            if "thumb_box_sums" in kname and len(v) == 3 * n:
                series = [(short, v[:n]), (short + " atomics-free twin", v[n:2 * n]), (short + " in the armed call", v[2 * n:])]
            for label, part in series:
                dur = [x[1] for x in part][args.warmup:] or [x[1] for x in part]
                out["kernels"][label] = {"launches": len(dur), "mean_us": round(statistics.mean(dur) / 1e3, 2),
                                         "median_us": round(statistics.median(dur) / 1e3, 2), "min_us": round(min(dur) / 1e3, 2)}
        conv = [k for k in out["kernels"] if "thumb_box_sums" not in k]
        for k, s in out["kernels"].items():
            if "thumb_box_sums" in k and "armed" not in k:
                s["fraction_of_8TBs"] = round(args.width * args.height * bpp / (s["median_us"] * 1e-6) / PEAK_BYTES_S, 4)
                if len(conv) == 1:
                    s["ratio_to_conversion_median"] = round(s["median_us"] / out["kernels"][conv[0]]["median_us"], 4)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host-gate", action="store_true")
    ap.add_argument("--device", nargs="+", metavar="CONFIG")
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
        raise SystemExit("bench_thumbnail.py measures on the GPU: no device, no number")
    if args.host_gate:
        host_gate(args)
    if args.device:
        device(args)


if __name__ == "__main__":
    main()
