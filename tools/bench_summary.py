#!/usr/bin/env python3
"""What the summary of a save's written planes (avifgpu_summary_attach) costs, 8192^2 frames.  One JSON line per CONFIG.

  --device CONFIG...   device pointers, FRESH data (launches rotate over >= 4 disjoint buffer sets), HIP events around K back-to-back
                       launches: the conversion kernel (the unarmed call), the summary kernel alone on the planes it wrote
                       (avifgpu_probe_summary), its atomics-free twin, the thumbnail kernel alone on the same planes
                       (avifgpu_probe_thumbnail twin 0, 256 x 256: the same bytes read, more arithmetic -- the comparison), and the
                       armed call (conversion + summary).  CONFIG as in tools/bench_thumbnail.py: c4 (10-bit 4:4:4 planes, 6 B/px read),
                       d12 (12-bit 4:2:2 nearest, 4 B/px), sdr8 (RGB8 -> 8-bit 4:2:2 nearest, the default SDR save, 2 B/px), ref8
                       (RGB8 -> interleaved RGB, 3 B/px).
  --unarmed-only       the conversion alone: for a library that has no summary (AVIFGPU_LIB=<the parent's build> AVIFGPU_AB_OLD_LIB=1),
                       to set this library's unarmed and armed calls against the parent's on the same box."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_thumbnail import PEAK_BYTES_S, TH, TW, config  # noqa: E402


def device(args):
    import numpy as np
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

        def planes_of(o):
            return [o[i].data_ptr() if i in o else None for i in range(4)], [o[i].stride(0) if i in o else 0 for i in range(4)]

        def conv(k):
            f, o = sets[k % args.sets]
            ptrs, strides = planes_of(o)
            gpu.write_rows(d, 0, H, f.data_ptr(), f.stride(0) * f.element_size(), ptrs, strides, mem=pkg.MEM_DEVICE, stream=stream)

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
        res = {"measurement": "device path, HIP events around back-to-back launches", "library": os.path.basename(os.path.dirname(pkg.LIB_PATH)) + "/" + os.path.basename(pkg.LIB_PATH),
               "config": name, "frame": f"{W}x{H}", "planes_bytes_per_px": bpp, "buffer_sets": args.sets, "launches": args.steps}
        res["unarmed_call_ms"] = round(timed(conv), 5)
        res["conversion_kernel"] = gpu.last_kernel()
        if args.unarmed_only:
            res["unarmed_call_second_pass_ms"] = round(timed(conv), 5)
            print(json.dumps(res), flush=True)
            del sets
            continue
        counters = torch.zeros(pkg.SUMMARY_COUNTERS, dtype=torch.int32, device=dev)
        sums = torch.zeros(TW * TH * 3, dtype=torch.int64, device=dev)

        def summary(k, twin=0):
            _, o = sets[k % args.sets]
            ptrs, strides = planes_of(o)
            rc = lib.avifgpu_probe_summary(ctypes.byref(d), twin, ctypes.byref((ctypes.c_void_p * 4)(*ptrs)),
                                           ctypes.byref((ctypes.c_int64 * 4)(*strides)), counters.data_ptr(), stream)
            if rc:
                raise SystemExit(lib.avifgpu_last_error().decode())

        def thumb(k):
            _, o = sets[k % args.sets]
            ptrs, strides = planes_of(o)
            rc = lib.avifgpu_probe_thumbnail(ctypes.byref(d), 0, TW, TH, ctypes.byref((ctypes.c_void_p * 4)(*ptrs)),
                                             ctypes.byref((ctypes.c_int64 * 4)(*strides)), sums.data_ptr(), stream)
            if rc:
                raise SystemExit(lib.avifgpu_last_error().decode())
        res["summary_ms"] = round(timed(summary), 5)
        # the counters against the planes, on the device: torch's own min / max per channel
        got = counters.cpu().numpy().view(np.uint32)
        want = np.zeros_like(got)
        for c, pl in enumerate(sorted(geom) if d.output == pkg.OUT_YCBCR else [0, 0, 0]):
            views = [o[pl].view(torch.int16 if ssz == 2 else torch.uint8) for _, o in sets]
            if d.output != pkg.OUT_YCBCR:
                views = [v.reshape(H, W, 3)[..., c] for v in views]
            want[c] = max(int(v.max()) for v in views)
            want[4 + c] = 65535 - min(int(v.min()) for v in views)
        if d.output != pkg.OUT_YCBCR:
            want[8] = max(int((v.reshape(H, W, 3).amax(dim=2).to(torch.int32) - v.reshape(H, W, 3).amin(dim=2).to(torch.int32)).max())
                          for v in (o[0].view(torch.uint8) for _, o in sets))
        res["counters_equal_the_planes_extremes"] = bool((got == want).all())
        res["atomics_free_twin_ms"] = round(timed(lambda k: summary(k, 1)), 5)
        res["thumbnail_kernel_alone_ms"] = round(timed(thumb), 5)
        with pkg.plane_summary(counters, pkg.MEM_DEVICE):
            res["armed_call_ms"] = round(timed(conv), 5)
        res["unarmed_call_second_pass_ms"] = round(timed(conv), 5)
        res["ratio_summary_to_thumbnail_kernel"] = round(res["summary_ms"] / res["thumbnail_kernel_alone_ms"], 4)
        res["ratio_armed_to_unarmed_call"] = round(res["armed_call_ms"] / min(res["unarmed_call_ms"], res["unarmed_call_second_pass_ms"]), 4)
        res["summary_fraction_of_8TBs"] = round(W * H * bpp / (res["summary_ms"] * 1e-3) / PEAK_BYTES_S, 4)
        print(json.dumps(res), flush=True)
        del sets


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", nargs="+", metavar="CONFIG", required=True)
    ap.add_argument("--unarmed-only", action="store_true")
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_summary.py measures on the GPU: no device, no number")
    device(args)


if __name__ == "__main__":
    main()
