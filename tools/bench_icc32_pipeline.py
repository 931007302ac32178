#!/usr/bin/env python3
"""32-bit documents behind a LUT-based (A2B) profile: the GPU stage-program kernel (write_px<..., icc = 8>) against the save path it
replaces (lcms2's ConvertRow on the CPU, then the plain GPU kernel), for an 8192^2 RGB f32 document saved as 12-bit PQ 4:2:2.

GPU rows: HIP-event kernel time over rotating (source, destination) buffer sets (>= 3 sets, > 3.5 GB, as tools/bench_configs.py does:
no launch finds its bytes in the Infinity Cache).  Fallback row: single-thread cmsDoTransform on a band of rows of the same frame
(ConvertRow, ColorProfileConversion.cpp:159-187, through the ICC oracle), scaled to the frame, plus the plain kernel's time.
Prints one JSON line per row.  Needs the ICC oracle and the lcms2 bridge (built where lcms2.h exists)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
import harness  # noqa: E402

W = H = int(os.environ.get("BENCH_SIZE", "8192"))
ITERS = int(os.environ.get("BENCH_ITERS", "12"))
BAND = int(os.environ.get("BENCH_LCMS_ROWS", "64"))
dev = torch.device("cuda", 0)
gpu = pkg.AvifGpu(0)
L = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle_icc.so"))
L.oracle_icc_make_a2b_profile.restype = ctypes.c_int32
L.oracle_icc_make_a2b_profile.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]
L.oracle_icc_convert_rows_to_rec2020.restype = ctypes.c_int32
L.oracle_icc_convert_rows_to_rec2020.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_uint32]

d = pkg.WriteDesc(width=W, height=H, depth=32, planes=3, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                  output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                  color_primaries=pkg.PRIMARIES_BT2020)
planes = harness.write_planes(d)
src_bytes = W * H * 12
out_bytes = sum(w * 2 * ((H + ys) >> ys) for w, xs, ys in planes.values())
nsets = max(3, int(np.ceil(3.5e9 / (src_bytes + out_bytes))))
rng = torch.Generator(device=dev).manual_seed(7)
sets = []
for _ in range(nsets):
    s = torch.rand(H, W * 3, device=dev, generator=rng) * 1.5
    outs = {pl: torch.empty(((H + ys) >> ys, w), dtype=torch.uint16, device=dev) for pl, (w, xs, ys) in planes.items()}
    sets.append((s, outs))
stream = torch.cuda.current_stream(dev).cuda_stream


def launch(k, icc):
    s, outs = sets[k % nsets]
    ptrs = [outs[i].data_ptr() if i in outs else None for i in range(4)]
    strides = [outs[i].stride(0) * 2 if i in outs else 0 for i in range(4)]
    gpu.write_rows(d, 0, H, s.data_ptr(), W * 12, ptrs, strides, mem=pkg.MEM_DEVICE, stream=stream, icc=icc)


def time_kernel(icc):
    for k in range(2 * nsets):
        launch(k, icc)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(k, icc)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.mean(ms)), gpu.last_kernel()


plain_ms, plain_mean, plain_kernel = time_kernel(None)
band = sets[0][0][:BAND].cpu().numpy().copy()
for variant in (0, 1):
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.oracle_icc_make_a2b_profile(variant, buf, len(buf))
    icc = buf.raw[:n]
    t0 = time.perf_counter()
    rc, prog = pkg.icc_pipeline32_from_profile(icc, pkg.ICC_TARGET_REC2020_LINEAR, False)
    prepare_ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, gpu.lib.avifgpu_last_error()
    ms, mean, kernel = time_kernel(prog)
    print(json.dumps({"row": "icc8_gpu", "profile": f"a2b variant {variant}", "size": W, "save": "RGB f32 -> 12-bit PQ 4:2:2",
                      "kernel_ms_p50": round(ms, 4), "kernel_ms_mean": round(mean, 4), "gpx_s": round(W * H / ms / 1e6, 3),
                      "program_prepare_ms": round(prepare_ms, 1), "buffer_sets": nsets, "kernel": kernel}), flush=True)
    x = band.copy()
    t0 = time.perf_counter()
    assert L.oracle_icc_convert_rows_to_rec2020(icc, len(icc), 0, x.ctypes.data, W, BAND, W * 12) == 0
    lcms_s = (time.perf_counter() - t0) * H / BAND
    print(json.dumps({"row": "fallback_lcms2_cpu_plus_gpu", "profile": f"a2b variant {variant}", "size": W,
                      "lcms2_convert_row_s_frame": round(lcms_s, 3), "lcms2_rows_timed": BAND, "plain_kernel_ms_p50": round(plain_ms, 4),
                      "total_ms": round(lcms_s * 1e3 + plain_ms, 1), "speedup_icc8": round((lcms_s * 1e3 + plain_ms) / ms, 1),
                      "plain_kernel": plain_kernel}), flush=True)
