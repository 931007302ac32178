#!/usr/bin/env python3
"""What the cropped open (avifgpu_read_rows_cropped) costs, 8192^2 images.  One JSON line per measurement.

  --device        crop_rows ALONE on device pointers (avifgpu_probe_crop), FRESH data (launches rotate over >= 4 disjoint buffer sets, source
                  rows of 256-byte pitch read from one pixel in): the bytes of the open_d8 and open_d12 outputs, beside the runtime's
                  device-to-device copy of the same bytes; HIP events around the timed launches.
  --open          device pointers, the open_d12 and open_d8 shapes of bench.py (4:2:0): rect (2, 2, W - 4, H - 4) -- the zero-copy case --
                  and rect (1, 1, W - 2, H - 2) -- covering + mover -- with code 1, code 6 and the bilinear mode, each beside the EXISTING
                  entry (avifgpu_read_rows / _oriented / _upsampled) on an image of the rectangle's size; HIP events around back-to-back
                  calls, fresh buffer sets.
  --host          end to end from page-locked memory: the cropped open (AVIFGPU_MEM_HOST) against avifgpu_read_rows(AVIFGPU_MEM_HOST) on an
                  image of the rectangle's size, alternating in one process: best of N and median of each, and their ratios.
  --base-only     with --open / --host: the existing entries only (what a library without the cropped open can run).
  --parent-lib SO [--passes N]   the driver: runs `--open --host --base-only` with AVIFGPU_LIB=SO and `--open --host` with the tree's
                  library, alternating, N passes each, one child process per run; prints the children's lines with a "library" field.
Run `--device --open` under `rocprofv3 --kernel-trace --stats` for the kernel times themselves."""
import argparse
import json
import os
import statistics
import subprocess
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


def shapes(W, H):
    return {
        "open_d12": dict(width=W, height=H, colorspace=0, chroma=1, bit_depth=12, depth=32, alpha_state=0, matrix_coefficients=9,
                         color_primaries=9, transfer_characteristics=16, pq_peak_nits=80),
        "open_d8": dict(width=W, height=H, colorspace=0, chroma=1, bit_depth=8, depth=8, alpha_state=0, matrix_coefficients=6),
    }


def device(args):
    import numpy as np
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H = args.width - 2, args.height - 2
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, bpp in (("open_d8", 3), ("open_d12", 12)):
        rb, sp, dp = W * bpp, pitch((W + 1) * bpp), pitch(W * bpp)
        src = [torch.randint(0, 256, ((H + 1) * sp,), device=dev, dtype=torch.uint8) for _ in range(args.sets)]
        dst = [torch.empty(H * dp, dtype=torch.uint8, device=dev) for _ in range(args.sets)]
        csrc = [torch.randint(0, 256, (rb * H,), device=dev, dtype=torch.uint8) for _ in range(args.sets)]
        cdst = [torch.empty(rb * H, dtype=torch.uint8, device=dev) for _ in range(args.sets)]

        def mover(k):
            gpu.probe_crop(src[k % args.sets].data_ptr() + sp + bpp, sp, dst[k % args.sets].data_ptr(), dp, rb, H, stream)

        def copy(k):
            cdst[k % args.sets].copy_(csrc[k % args.sets])
        res = {"measurement": "crop_rows alone, device pointers, HIP events around back-to-back launches", "bytes_of": name, "rows": H, "row_bytes": rb,
               "buffer_sets": args.sets, "launches": args.steps, "bytes_moved": 2 * rb * H}
        ms = timed(torch, dev, args, mover)
        res["crop_rows_ms"] = round(ms, 5)
        res["crop_rows_fraction_of_8TBs"] = round(2 * rb * H / (ms * 1e-3) / PEAK_BYTES_S, 4)
        ms = timed(torch, dev, args, copy)
        res["copy_ms"] = round(ms, 5)
        res["copy_fraction_of_8TBs"] = round(2 * rb * H / (ms * 1e-3) / PEAK_BYTES_S, 4)
        res["crop_rows_speed_relative_to_copy"] = round(res["copy_ms"] / res["crop_rows_ms"], 4)
        mover(0)
        torch.cuda.synchronize(dev)
        got = dst[0].view(H, dp)[:3, :rb].cpu().numpy()
        want = src[0].view(H + 1, sp)[1:4].cpu().numpy().reshape(-1)
        res["rows_correct"] = bool(all(np.array_equal(got[r], want[r * sp + bpp:r * sp + bpp + rb]) for r in range(3)))
        print(json.dumps(res), flush=True)
        del src, dst, csrc, cdst
        torch.cuda.empty_cache()


def make_sets(torch, harness, pkg, d, dev, nsets, seed, pinned=False):
    ssz = 2 if d.bit_depth > 8 else 1
    maxc = (1 << d.bit_depth) - 1
    sets = []
    for k in range(nsets):
        planes = {}
        if pinned:
            for pl, (w, xs, ys) in harness.read_planes(d).items():
                planes[pl] = torch.randint(0, maxc + 1, ((d.height + ys) >> ys, pitch(w * ssz) // ssz), dtype=torch.int16 if ssz == 2 else torch.uint8).pin_memory()
        else:
            g = torch.Generator(device=dev)
            g.manual_seed(seed + k)
            for pl, (w, xs, ys) in harness.read_planes(d).items():
                planes[pl] = torch.randint(0, maxc + 1, ((d.height + ys) >> ys, pitch(w * ssz) // ssz), generator=g, device=dev,
                                           dtype=torch.int16 if ssz == 2 else torch.uint8)
        sets.append(planes)
    return sets, ssz


def open_device(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    dev = f"cuda:{gpu.device}"
    W, H = args.width, args.height
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, kw in shapes(W, H).items():
        d = pkg.ReadDesc(**kw)
        bpp = 3 * (d.depth // 8)
        whole, ssz = make_sets(torch, harness, pkg, d, dev, args.sets, 99)
        for rect, rname in (((2, 2, W - 4, H - 4), "zero-copy (2, 2)"), ((1, 1, W - 2, H - 2), "covering + mover (1, 1)")):
            sub = pkg.ReadDesc.from_buffer_copy(d)
            sub.width, sub.height = rect[2], rect[3]
            small, _ = make_sets(torch, harness, pkg, sub, dev, args.sets, 7)
            side = max(rect[2], rect[3])
            outs = [torch.empty(side * pitch(side * bpp), dtype=torch.uint8, device=dev) for _ in range(args.sets)]
            for mode, code, label in ((0, 1, "nearest code 1"), (0, 6, "nearest code 6"), (1, 1, "bilinear code 1")):
                out_w, out_h = (rect[2], rect[3]) if code == 1 else (rect[3], rect[2])
                need_b = max(pkg.read_upsampled_scratch_bytes(sub, mode, code, out_h), pkg.read_oriented_scratch_bytes(sub, code, out_h), 16)
                need_c = 16 if args.base_only else max(pkg.read_cropped_scratch_bytes(d, rect, mode, code, out_h), 16)
                scratch = [torch.empty(max(need_b, need_c), dtype=torch.uint8, device=dev) for _ in range(args.sets)]

                def base(k):
                    planes, out = small[k % args.sets], outs[k % args.sets]
                    ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
                    strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
                    if mode == 0 and code == 1:
                        gpu.read_rows(sub, 0, out_h, ptrs, strides, out.data_ptr(), pitch(out_w * bpp), mem=pkg.MEM_DEVICE, stream=stream)
                    elif mode == 0:
                        gpu.read_rows_oriented(sub, code, 0, out_h, ptrs, strides, out.data_ptr(), pitch(out_w * bpp), scratch[k % args.sets].data_ptr(), need_b,
                                               mem=pkg.MEM_DEVICE, stream=stream)
                    else:
                        gpu.read_rows_upsampled(sub, mode, code, 0, out_h, ptrs, strides, out.data_ptr(), pitch(out_w * bpp), scratch[k % args.sets].data_ptr(), need_b,
                                                mem=pkg.MEM_DEVICE, stream=stream)

                def crop(k):
                    planes, out = whole[k % args.sets], outs[k % args.sets]
                    ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
                    strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
                    gpu.read_rows_cropped(d, rect, mode, code, 0, out_h, ptrs, strides, out.data_ptr(), pitch(out_w * bpp), scratch[k % args.sets].data_ptr(), need_c,
                                          mem=pkg.MEM_DEVICE, stream=stream)
                res = {"measurement": "open on device pointers, HIP events around back-to-back calls", "config": name, "rect": rname, "case": label,
                       "image": f"{W}x{H}", "buffer_sets": args.sets, "launches": args.steps}
                b0 = timed(torch, dev, args, base)
                res["existing_entry_rect_sized_ms"] = round(b0, 5)
                if not args.base_only:
                    c = timed(torch, dev, args, crop)
                    b1 = timed(torch, dev, args, base)
                    res.update(cropped_ms=round(c, 5), existing_entry_rect_sized_again_ms=round(b1, 5), cropped_over_existing=round(c / min(b0, b1), 4),
                               last_kernel=gpu.last_kernel()[:80])
                print(json.dumps(res), flush=True)
                del scratch
            del small, outs
            torch.cuda.empty_cache()
        del whole
        torch.cuda.empty_cache()


def host(args):
    import torch
    import harness
    pkg = harness.pkg
    gpu = pkg.AvifGpu(0)
    W, H = args.width, args.height
    for name, kw in shapes(W, H).items():
        d = pkg.ReadDesc(**kw)
        bpp = 3 * (d.depth // 8)
        (planes,), ssz = make_sets(torch, harness, pkg, d, "cpu", 1, 0, pinned=True)
        ptrs = [planes[i].data_ptr() if i in planes else None for i in range(4)]
        strides = [planes[i].stride(0) * ssz if i in planes else 0 for i in range(4)]
        out = torch.empty((H, W * bpp), dtype=torch.uint8).pin_memory()
        out2 = torch.empty((H, W * bpp), dtype=torch.uint8).pin_memory()
        rects = {"even": (2, 2, W - 4, H - 4), "odd": (1, 1, W - 2, H - 2)}
        subs = {}
        for rn, r in rects.items():
            sub = pkg.ReadDesc.from_buffer_copy(d)
            sub.width, sub.height = r[2], r[3]
            subs[rn] = sub

        def run(label):
            kind, rn = label.split(":")
            r, sub = rects[rn], subs[rn]
            t0 = time.perf_counter()
            if kind == "read_rows":
                gpu.read_rows(sub, 0, r[3], ptrs, strides, out.data_ptr(), out.stride(0), mem=pkg.MEM_HOST)
            else:
                gpu.read_rows_cropped(d, r, 0, 1, 0, r[3], ptrs, strides, out2.data_ptr(), out2.stride(0), mem=pkg.MEM_HOST)
            return time.perf_counter() - t0
        labels = ["read_rows:even", "read_rows:odd"] + ([] if args.base_only else ["cropped:even", "cropped:odd"])
        for _ in range(2):
            for l in labels:
                run(l)
        t = {l: [] for l in labels}
        for _ in range(args.reps):                                  # alternating: all see the same box
            for l in labels:
                t[l].append(run(l))
        res = {"measurement": "end to end, host pointers, page-locked, code 1, nearest", "config": name, "image": f"{W}x{H}", "reps": args.reps}
        for l in labels:
            res[f"{l}_best_ms"] = round(min(t[l]) * 1e3, 3)
            res[f"{l}_median_ms"] = round(statistics.median(t[l]) * 1e3, 3)
        if not args.base_only:
            for rn in rects:
                res[f"cropped_over_read_rows:{rn}_best"] = round(res[f"cropped:{rn}_best_ms"] / res[f"read_rows:{rn}_best_ms"], 4)
                res[f"cropped_over_read_rows:{rn}_median"] = round(res[f"cropped:{rn}_median_ms"] / res[f"read_rows:{rn}_median_ms"], 4)
        print(json.dumps(res), flush=True)


def driver(args):
    base = [sys.executable, os.path.abspath(__file__), "--open", "--host", "--width", str(args.width), "--height", str(args.height), "--steps", str(args.steps),
            "--warmup", str(args.warmup), "--sets", str(args.sets), "--reps", str(args.reps)]
    for p in range(args.passes):
        for lib in ("parent", "this"):
            env = dict(os.environ)
            cmd = list(base)
            if lib == "parent":
                env.update(AVIFGPU_LIB=os.path.abspath(args.parent_lib), AVIFGPU_AB_OLD_LIB="1")
                cmd.append("--base-only")
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"bench_crop.py: the {lib} run failed with status {r.returncode}")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    rec.update(library=lib, run=p)
                    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--open", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--parent-lib", metavar="SO")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--width", type=int, default=8192)
    ap.add_argument("--height", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    if args.parent_lib:
        return driver(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop.py measures on the GPU: no device, no number")
    if args.device:
        device(args)
    if args.open:
        open_device(args)
    if args.host:
        host(args)


if __name__ == "__main__":
    main()
