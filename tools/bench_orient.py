#!/usr/bin/env python3
"""What the orientation of an open (avifgpu_read_rows_oriented) costs, 8192^2 images.  One JSON line per measurement.

  --device [BPP ...]   the orient kernel ALONE on device pointers (avifgpu_probe_orient), FRESH data (launches rotate over >= 4 disjoint
                       buffer sets, rows padded to 256 bytes; --width 8189 makes every row length but the 16-byte pixel's no multiple of 16 bytes),
                       for each pixel size (default: all eight) codes 2, 6 and 8 and a plain device-to-device copy of the
                       same bytes, each as one series of warmup + steps launches in that order; HIP events around the timed launches.
                       Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_orient.py --device`
                       for the kernel times themselves, then
  --summarize DIR      per pixel size: the trace's median / min of every series (the first --warmup launches of each dropped), each as a
                       fraction of 8 TB/s over 2 * bpp * pixels, and the ratio to the copy of the same run.
  --pmc [BPP ...]      one launch series per pixel size and code, no copy: run it under `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT
                       SQ_LDS_IDX_ACTIVE --output-format csv -d DIR -- ...` (counters in a run of their own), then
  --summarize-pmc DIR  per kernel: bank-conflict cycles as a share of all LDS-array cycles.
  --host               end to end: the 8192^2 default opens (bench.py's open_d12 and open_d8 shapes) through
                       avifgpu_read_rows_oriented(AVIFGPU_MEM_HOST) from page-locked memory, codes 6, 8 and 2 against code 1, alternating in
                       one process: best of N and median of each, and their ratios.  (The staged column bands of codes 6 and 8 are as wide
                       as 32 MiB of output allows: their row length is no multiple of 16 bytes.)"""
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
SIZES = (1, 2, 3, 4, 6, 8, 12, 16)
CODES = (2, 6, 8)


def device(args, with_copy=True):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H = args.width, args.height
    stream = torch.cuda.current_stream(dev).cuda_stream
    for bpp in args.sizes or SIZES:
        def pitch(px, bpp=bpp):
            return (px * bpp + 255) // 256 * 256
        sets = []
        for k in range(args.sets):                                  # disjoint buffers: a launch never finds its lines in the caches
            g = torch.Generator(device=dev)
            g.manual_seed(1234 + k)
            # rows padded to 256 bytes, as the library's own scratch and staging rows are: bases and strides stay on the 16-byte grid at
            # every width, only the row's LENGTH is off it when --width says so
            sets.append((torch.randint(0, 256, (H, pitch(W)), generator=g, device=dev, dtype=torch.uint8),
                         torch.empty(max(H * pitch(W), W * pitch(H)), dtype=torch.uint8, device=dev)))

        def orient(code):
            def fn(k):
                s, d = sets[k % args.sets]
                gpu.probe_orient(code, bpp, W, H, s.data_ptr(), pitch(W), d.data_ptr(), pitch(H if code >= 5 else W), stream)
            return fn

        def copy(k):
            s, d = sets[k % args.sets]
            d[:s.numel()].copy_(s.view(-1))

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
        res = {"measurement": "orient kernel alone, device pointers, HIP events around back-to-back launches", "bytes_per_pixel": bpp,
               "image": f"{W}x{H}", "row_bytes_mod_16": (W * bpp) % 16, "buffer_sets": args.sets, "launches": args.steps, "bytes_moved": 2 * bpp * W * H}
        for code in CODES:
            ms = timed(orient(code))
            res[f"code{code}_ms"] = round(ms, 5)
            res[f"code{code}_fraction_of_8TBs"] = round(2 * bpp * W * H / (ms * 1e-3) / PEAK_BYTES_S, 4)
        if with_copy:
            ms = timed(copy)
            res["copy_ms"] = round(ms, 5)
            res["copy_fraction_of_8TBs"] = round(2 * bpp * W * H / (ms * 1e-3) / PEAK_BYTES_S, 4)
            for code in CODES:
                res[f"code{code}_speed_relative_to_copy"] = round(res["copy_ms"] / res[f"code{code}_ms"], 4)
        # the last launch of code 8 against numpy, on a corner: the kernel that was timed is the kernel that is right
        s, d = sets[(args.warmup + args.steps - 1) % args.sets]
        orient(8)(args.warmup + args.steps - 1)
        torch.cuda.synchronize(dev)
        got = d[:W * pitch(H)].view(W, pitch(H))[:64, :64 * bpp].reshape(64, 64, bpp).cpu()
        want = s[:64, (W - 64) * bpp:W * bpp].reshape(64, 64, bpp).flip(1).transpose(0, 1).cpu()
        res["code8_corner_correct"] = bool((got == want).all())
        print(json.dumps(res), flush=True)
        del sets
        torch.cuda.empty_cache()


def trace_rows(d):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def summarize(args):
    rows = trace_rows(args.summarize)
    n = args.warmup + args.steps
    pixels = args.width * args.height
    # the launches of interest in time order: orient kernels, and the copies (whatever kernel the runtime uses for them) that follow the
    # three orient series of a pixel size
    i = 0
    while i < len(rows):
        if "orient_rows<" not in rows[i][2]:
            i += 1
            continue
        bpp = int(rows[i][2].split("orient_rows<")[1].split(">")[0])
        series = {}
        block = rows[i:i + 3 * n + 1]                                # + the correctness launch of code 8
        if len(block) < 3 * n or any("orient_" not in r[2] for r in block[:3 * n]):
            break
        for j, code in enumerate(CODES):
            series[f"code {code}"] = [r[1] for r in block[j * n:(j + 1) * n]][args.warmup:]
        i += 3 * n
        copies = []
        while i < len(rows) and "orient_rows<" not in rows[i][2]:
            if "orient_" not in rows[i][2] and rows[i][1] > 0:
                copies.append(rows[i])
            i += 1
        # the copies of this pixel size: the n launches of the most frequent non-orient kernel
        names = {}
        for r in copies:
            names.setdefault(r[2], []).append(r[1])
        if names:
            cname = max(names, key=lambda k: len(names[k]))
            if len(names[cname]) >= n:
                series["copy"] = names[cname][:n][args.warmup:]
                series_copy_kernel = cname[:80]
        out = {"measurement": "kernel trace (rocprofv3 --kernel-trace)", "bytes_per_pixel": bpp, "image": f"{args.width}x{args.height}",
               "bytes_moved": 2 * bpp * pixels}
        for label, dur in series.items():
            med = statistics.median(dur) / 1e3
            out[label] = {"launches": len(dur), "median_us": round(med, 2), "min_us": round(min(dur) / 1e3, 2),
                          "fraction_of_8TBs": round(2 * bpp * pixels / (med * 1e-6) / PEAK_BYTES_S, 4)}
        if "copy" in series:
            out["copy"]["kernel"] = series_copy_kernel
            for code in CODES:
                out[f"code {code}"]["speed_relative_to_copy"] = round(out["copy"]["median_us"] / out[f"code {code}"]["median_us"], 4)
        print(json.dumps(out), flush=True)


def summarize_pmc(args):
    acc = {}
    for f in glob.glob(args.summarize_pmc + "/**/*counter_collection.csv", recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "orient_" not in r["Kernel_Name"]:
                    continue
                key = (r["Kernel_Name"].replace("avifgpu::(anonymous namespace)::", "").replace("(OrientParams)", "").replace("void ", ""), r["Counter_Name"])
                acc.setdefault(key, []).append(float(r["Counter_Value"]))
    kernels = sorted({k for k, _ in acc})
    for k in kernels:
        conflict = sum(acc.get((k, "SQ_LDS_BANK_CONFLICT"), [0.0]))
        active = sum(acc.get((k, "SQ_LDS_IDX_ACTIVE"), [0.0]))
        print(json.dumps({"measurement": "LDS bank conflicts (rocprofv3 --pmc, a run of its own)", "kernel": k, "launches": len(acc.get((k, "SQ_LDS_IDX_ACTIVE"), [])),
                          "SQ_LDS_BANK_CONFLICT": conflict, "SQ_LDS_IDX_ACTIVE": active,
                          "bank_conflict_share_of_lds_cycles": round(conflict / active, 4) if active else None}), flush=True)


def host(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H = args.width, args.height
    shapes = {
        "open_d12": dict(width=W, height=H, colorspace=0, chroma=pkg.CHROMA_422, bit_depth=12, depth=32, alpha_state=0, matrix_coefficients=9,
                         color_primaries=9, transfer_characteristics=16, pq_peak_nits=80),
        "open_d8": dict(width=W, height=H, colorspace=0, chroma=pkg.CHROMA_422, bit_depth=8, depth=8, alpha_state=0, matrix_coefficients=6),
    }
    for name, kw in shapes.items():
        d = pkg.ReadDesc(**kw)
        ssz = 2 if d.bit_depth > 8 else 1
        maxc = (1 << d.bit_depth) - 1
        planes = {}
        for pl, (w, xs, ys) in harness.read_planes(d).items():
            t = torch.randint(0, maxc + 1, ((H + ys) >> ys, w), dtype=torch.int16 if ssz == 2 else torch.uint8).pin_memory()
            planes[pl] = t
        ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
        strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
        row_bytes = W * 3 * (d.depth // 8)                          # W == H here; kept general below
        bpp = 3 * (d.depth // 8)
        codes = (1, 6, 8, 2)
        outs = {c: (torch.empty((W, H * bpp), dtype=torch.uint8) if c >= 5 else torch.empty((H, W * bpp), dtype=torch.uint8)).pin_memory() for c in codes}

        def once(code):
            o = outs[code]
            t0 = time.perf_counter()
            gpu.read_rows_oriented(d, code, 0, W if code >= 5 else H, ptrs, strides, o.data_ptr(), o.stride(0), mem=pkg.MEM_HOST)
            return time.perf_counter() - t0
        for _ in range(2):
            for code in codes:
                once(code)
        t = {c: [] for c in codes}
        for _ in range(args.reps):                                  # alternating: all see the same box
            for code in codes:
                t[code].append(once(code))
        I = outs[1].view(H, W, bpp)
        a = I[:48, :48]
        res = {"measurement": "end to end, host pointers, page-locked", "config": name, "image": f"{W}x{H}", "reps": args.reps, "row_bytes": row_bytes,
               # rot90 clockwise: out[x][H - 1 - y] = I[y][x]; anticlockwise: out[W - 1 - x][y] = I[y][x]; mirrored: out[y][W - 1 - x] = I[y][x]
               "corners_correct": bool((outs[6].view(W, H, bpp)[:48, H - 48:].flip(1).transpose(0, 1) == a).all()
                                       and (outs[8].view(W, H, bpp)[W - 48:, :48].flip(0).transpose(0, 1) == a).all()
                                       and (outs[2].view(H, W, bpp)[:48, W - 48:].flip(1) == a).all())}
        for c in codes:
            res[f"code{c}_best_ms"] = round(min(t[c]) * 1e3, 3)
            res[f"code{c}_median_ms"] = round(statistics.median(t[c]) * 1e3, 3)
        for c in codes[1:]:
            res[f"code{c}_ratio_best"] = round(res[f"code{c}_best_ms"] / res["code1_best_ms"], 4)
            res[f"code{c}_ratio_median"] = round(res[f"code{c}_median_ms"] / res["code1_median_ms"], 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", nargs="*", type=int, metavar="BPP", dest="device")
    ap.add_argument("--pmc", nargs="*", type=int, metavar="BPP")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--summarize-pmc", metavar="DIR")
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    if args.summarize_pmc:
        return summarize_pmc(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_orient.py measures on the GPU: no device, no number")
    if args.device is not None:
        args.sizes = args.device
        device(args)
    if args.pmc is not None:
        args.sizes = args.pmc
        device(args, with_copy=False)
    if args.host:
        host(args)


if __name__ == "__main__":
    main()
