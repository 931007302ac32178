#!/usr/bin/env python3
"""What bilinear chroma upsampling of an open (avifgpu_read_rows_upsampled) costs, 8192^2 images.  One JSON line per measurement.

  --device        chroma_upsample ALONE on device pointers (avifgpu_probe_upsample), FRESH data (launches rotate over >= 4 disjoint buffer
                  sets, rows padded to 256 bytes): u8 / u16 x 4:2:0 / 4:2:2 x CENTER / LEFT, its store-only and math-free twins, then the runtime's device-to-device
                  copy of the same byte count (read + written bytes of the kernel = 2 x the copied bytes); HIP events around the timed
                  launches.
  --open          device pointers: the interpolating open (pre-pass + the 4:4:4 decode) against the nearest open of the same planes, the
                  open_d8 and open_d12 shapes of bench.py; HIP events around back-to-back calls.
                  Run both under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_upsample.py --device --open`
                  for the kernel times themselves, then
  --summarize DIR per series of that run (the plan is written to DIR/plan.json by the traced run: pass --plan DIR/plan.json to it): the
                  trace's median / min of every kernel of the series, the first --warmup launches dropped.
  --host          end to end: the two default opens through avifgpu_read_rows_upsampled(AVIFGPU_MEM_HOST) from page-locked memory against
                  avifgpu_read_rows(AVIFGPU_MEM_HOST) (codes 1-4) and against the oriented nearest open (code 6), alternating in one
                  process: best of N and median of each, and their ratios."""
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
PLAN = []


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


def device(args):
    import torch
    import harness
    from upsample_truth import upsample_plane
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H = args.width, args.height
    stream = torch.cuda.current_stream(dev).cuda_stream
    for ssz, chroma, ys in ((1, pkg.CHROMA_420, 1), (2, pkg.CHROMA_422, 0), (2, pkg.CHROMA_420, 1), (1, pkg.CHROMA_422, 0)):
        cw, ch = (W + 1) >> 1, (H + ys) >> ys
        sp, dp = pitch(cw * ssz), pitch(W * ssz)
        read_bytes, written = 2 * cw * ssz * ch, 2 * W * ssz * H
        sets = []
        for k in range(args.sets):                                  # disjoint buffers: a launch never finds its lines in the caches
            g = torch.Generator(device=dev)
            g.manual_seed(1234 + k)
            sets.append(([torch.randint(0, 256, (ch, sp), generator=g, device=dev, dtype=torch.uint8) for _ in range(2)],
                         [torch.empty(H * dp, dtype=torch.uint8, device=dev) for _ in range(2)]))
        half = (read_bytes + written) // 2                          # a copy of `half` bytes reads and writes what the kernel reads and writes
        csrc = [torch.randint(0, 256, (half,), device=dev, dtype=torch.uint8) for _ in range(args.sets)]
        cdst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(args.sets)]

        def up(mode, twin=0):
            def fn(k):
                s, d = sets[k % args.sets]
                gpu.probe_upsample(ssz, chroma, mode, W, H, 0, 0, W, H, [t.data_ptr() for t in s], [sp, sp], [t.data_ptr() for t in d], dp, stream, twin)
            return fn

        def copy(k):
            cdst[k % args.sets].copy_(csrc[k % args.sets])
        res = {"measurement": "chroma_upsample alone, device pointers, HIP events around back-to-back launches", "bytes_per_sample": ssz,
               "chroma": {pkg.CHROMA_420: "4:2:0", pkg.CHROMA_422: "4:2:2"}[chroma], "image": f"{W}x{H}", "buffer_sets": args.sets,
               "launches": args.steps, "bytes_read": read_bytes, "bytes_written": written}
        for mode, label in ((1, "center"), (2, "left")):
            ms = timed(torch, dev, args, up(mode))
            PLAN.append({"series": f"upsample u{8 * ssz} {res['chroma']} {label}", "kernels": ["upsample"], "bytes": read_bytes + written})
            res[f"{label}_ms"] = round(ms, 5)
            res[f"{label}_fraction_of_8TBs"] = round((read_bytes + written) / (ms * 1e-3) / PEAK_BYTES_S, 4)
        # the twins, for attribution: store-only (writes only), math-free (the same loads and stores, no neighbour samples, no sums)
        for twin, label, nbytes in ((1, "store_only_twin", written), (2, "math_free_twin", read_bytes + written)):
            ms = timed(torch, dev, args, up(1, twin))
            PLAN.append({"series": f"upsample u{8 * ssz} {res['chroma']} {label}", "kernels": ["upsample"], "bytes": nbytes})
            res[f"{label}_ms"] = round(ms, 5)
            res[f"{label}_fraction_of_8TBs"] = round(nbytes / (ms * 1e-3) / PEAK_BYTES_S, 4)
        ms = timed(torch, dev, args, copy)
        PLAN.append({"series": f"copy of {half} bytes", "kernels": ["copy"], "bytes": read_bytes + written})
        res["copy_ms"] = round(ms, 5)
        res["copy_fraction_of_8TBs"] = round((read_bytes + written) / (ms * 1e-3) / PEAK_BYTES_S, 4)
        for label in ("center", "left"):
            res[f"{label}_speed_relative_to_copy"] = round(res["copy_ms"] / res[f"{label}_ms"], 4)
        # the last launch against the definition, on a corner: the kernel that was timed is the kernel that is right
        s, d = sets[0]
        up(1)(0)
        PLAN.append({"series": "corner check", "kernels": ["upsample"], "count": 1})
        torch.cuda.synchronize(dev)
        import numpy as np
        dt = np.uint8 if ssz == 1 else np.uint16
        c = s[0][:64, :40 * ssz].cpu().numpy().copy().view(dt)
        got = d[0].view(H, dp)[:32, :32 * ssz].cpu().numpy().copy().view(dt)
        want = upsample_plane(np.ascontiguousarray(c[:(64 + ys) >> ys, :32]), 64, 64, ys, 1)[:32, :32]
        res["corner_correct"] = bool((got == want).all())
        print(json.dumps(res), flush=True)
        del sets, csrc, cdst
        torch.cuda.empty_cache()


def shapes(pkg, W, H, chroma):
    return {
        "open_d12": dict(width=W, height=H, colorspace=0, chroma=chroma, bit_depth=12, depth=32, alpha_state=0, matrix_coefficients=9,
                         color_primaries=9, transfer_characteristics=16, pq_peak_nits=80),
        "open_d8": dict(width=W, height=H, colorspace=0, chroma=chroma, bit_depth=8, depth=8, alpha_state=0, matrix_coefficients=6),
    }


def open_device(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H = args.width, args.height
    stream = torch.cuda.current_stream(dev).cuda_stream
    for chroma, cname in ((pkg.CHROMA_422, "4:2:2"), (pkg.CHROMA_420, "4:2:0")):
        for name, kw in shapes(pkg, W, H, chroma).items():
            d = pkg.ReadDesc(**kw)
            ssz = 2 if d.bit_depth > 8 else 1
            maxc = (1 << d.bit_depth) - 1
            bpp = 3 * (d.depth // 8)
            sets = []
            for k in range(args.sets):
                g = torch.Generator(device=dev)
                g.manual_seed(99 + k)
                planes = {}
                for pl, (w, xs, ys) in harness.read_planes(d).items():
                    planes[pl] = torch.randint(0, maxc + 1, ((H + ys) >> ys, pitch(w * ssz) // ssz), generator=g, device=dev,
                                               dtype=torch.int16 if ssz == 2 else torch.uint8)
                sets.append((planes, torch.empty(H * pitch(W * bpp), dtype=torch.uint8, device=dev)))
            need = pkg.read_upsampled_scratch_bytes(d, 1, 1, H)
            scratch = [torch.empty(need, dtype=torch.uint8, device=dev) for _ in range(args.sets)]

            def call(mode):
                def fn(k):
                    planes, out = sets[k % args.sets]
                    ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
                    strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
                    if mode == 0:
                        gpu.read_rows(d, 0, H, ptrs, strides, out.data_ptr(), pitch(W * bpp), mem=pkg.MEM_DEVICE, stream=stream)
                    else:
                        gpu.read_rows_upsampled(d, mode, 1, 0, H, ptrs, strides, out.data_ptr(), pitch(W * bpp), scratch[k % args.sets].data_ptr(), need,
                                                mem=pkg.MEM_DEVICE, stream=stream)
                return fn
            res = {"measurement": "open on device pointers, HIP events around back-to-back calls", "config": name, "chroma": cname, "image": f"{W}x{H}",
                   "buffer_sets": args.sets, "launches": args.steps}
            ms0 = timed(torch, dev, args, call(0))
            PLAN.append({"series": f"{name} {cname} nearest", "kernels": ["read"]})
            ms1 = timed(torch, dev, args, call(1))
            PLAN.append({"series": f"{name} {cname} bilinear", "kernels": ["upsample", "read"]})
            res.update(nearest_ms=round(ms0, 5), bilinear_ms=round(ms1, 5), bilinear_over_nearest=round(ms1 / ms0, 4))
            print(json.dumps(res), flush=True)
            del sets, scratch
            torch.cuda.empty_cache()


def summarize(args):
    rows = []
    for f in glob.glob(args.summarize + "/**/*kernel_trace.csv", recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    plan = json.load(open(args.plan or os.path.join(args.summarize, "plan.json")))
    n = args.warmup + args.steps

    def kind(name):
        if "chroma_upsample" in name:
            return "upsample"
        if "build_read_tables" in name:
            return "tables"                                         # once per descriptor change, in front of a decode: not part of a series
        if "avifgpu" in name:
            return "read"
        return "copy"
    i = 0
    for s in plan:
        want = s["kernels"]
        need = s.get("count", n) * len(want)
        block = []
        while i < len(rows) and len(block) < need:
            kd = kind(rows[i][2])
            if kd in want and rows[i][1] > 0:
                block.append(rows[i])
            elif want == ["copy"] and kd in ("upsample", "read"):
                break                                               # the runtime copied without a kernel: nothing of this series is in the trace
            i += 1
        if "count" in s:
            continue
        out = {"measurement": "kernel trace (rocprofv3 --kernel-trace)", "series": s["series"]}
        total = 0.0
        for kd in want:
            dur = [r[1] for r in block if kind(r[2]) == kd][args.warmup:]
            if not dur:
                continue
            names = sorted({r[2] for r in block if kind(r[2]) == kd})
            med = statistics.median(dur) / 1e3
            total += med
            out[kd] = {"launches": len(dur), "median_us": round(med, 2), "min_us": round(min(dur) / 1e3, 2), "kernel": names[0][:120], "distinct_kernels": len(names)}
            if "bytes" in s:
                out[kd]["fraction_of_8TBs"] = round(s["bytes"] / (med * 1e-6) / PEAK_BYTES_S, 4)
        out["sum_of_medians_us"] = round(total, 2)
        print(json.dumps(out), flush=True)


def host(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H = args.width, args.height
    for name, kw in shapes(pkg, W, H, pkg.CHROMA_422).items():
        d = pkg.ReadDesc(**kw)
        ssz = 2 if d.bit_depth > 8 else 1
        maxc = (1 << d.bit_depth) - 1
        planes = {}
        for pl, (w, xs, ys) in harness.read_planes(d).items():
            planes[pl] = torch.randint(0, maxc + 1, ((H + ys) >> ys, w), dtype=torch.int16 if ssz == 2 else torch.uint8).pin_memory()
        ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
        strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
        bpp = 3 * (d.depth // 8)
        out = torch.empty((max(W, H), max(W, H) * bpp), dtype=torch.uint8).pin_memory()
        out2 = torch.empty((max(W, H), max(W, H) * bpp), dtype=torch.uint8).pin_memory()

        def run(label):
            t0 = time.perf_counter()
            if label == "read_rows":
                gpu.read_rows(d, 0, H, ptrs, strides, out.data_ptr(), out.stride(0), mem=pkg.MEM_HOST)
            elif label == "oriented6_nearest":
                gpu.read_rows_oriented(d, 6, 0, W, ptrs, strides, out.data_ptr(), out.stride(0), mem=pkg.MEM_HOST)
            else:
                code = int(label.split("code")[1])
                gpu.read_rows_upsampled(d, 1, code, 0, W if code >= 5 else H, ptrs, strides, out2.data_ptr(), out2.stride(0), mem=pkg.MEM_HOST)
            return time.perf_counter() - t0
        labels = ("read_rows", "bilinear_code1", "bilinear_code2", "bilinear_code3", "bilinear_code4", "oriented6_nearest", "bilinear_code6")
        for _ in range(2):
            for l in labels:
                run(l)
        t = {l: [] for l in labels}
        for _ in range(args.reps):                                  # alternating: all see the same box
            for l in labels:
                t[l].append(run(l))
        res = {"measurement": "end to end, host pointers, page-locked", "config": name, "chroma": "4:2:2", "image": f"{W}x{H}", "reps": args.reps}
        for l in labels:
            res[f"{l}_best_ms"] = round(min(t[l]) * 1e3, 3)
            res[f"{l}_median_ms"] = round(statistics.median(t[l]) * 1e3, 3)
        for l in labels[1:5]:
            res[f"{l}_over_read_rows_best"] = round(res[f"{l}_best_ms"] / res["read_rows_best_ms"], 4)
            res[f"{l}_over_read_rows_median"] = round(res[f"{l}_median_ms"] / res["read_rows_median_ms"], 4)
        res["bilinear_code6_over_oriented6_nearest_best"] = round(res["bilinear_code6_best_ms"] / res["oriented6_nearest_best_ms"], 4)
        res["bilinear_code6_over_oriented6_nearest_median"] = round(res["bilinear_code6_median_ms"] / res["oriented6_nearest_median_ms"], 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--open", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--plan", metavar="FILE")
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample.py measures on the GPU: no device, no number")
    if args.device:
        device(args)
    if args.open:
        open_device(args)
    if args.plan:
        with open(args.plan, "w") as f:
            json.dump(PLAN, f)
    if args.host:
        host(args)


if __name__ == "__main__":
    main()
