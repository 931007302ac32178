"""The upsampled open on the GPU (include/avifgpu.h "upsampled open", csrc/upsample_kernels.hip).

The expected image is always the definition in numpy (tests/upsample_truth.py) on the raw container values, followed by the existing
oracle on the 4:4:4 descriptor (harness.oracle_read).  8- and 16-bit hosts: array_equal.  32-bit hosts: array_equal, floats compared as
bits, against the GPU's own avifgpu_read_rows on the truth's 4:4:4 planes, and the T2 read bar of tests/test_gpu_read.py
(|gpu - oracle| <= 1e-4 |oracle| + 1e-9) against the oracle.

Shapes are the smallest at which the kernel as built can go wrong: a lane owns 16 output bytes (16 u8 / 8 u16 samples), a wave 1024,
a workgroup 4096 (four neighbouring spans), and a wave walks down a band of 32 output rows.

The cases are grouped under four test ids (the last section of this file); every group of an id runs even when an earlier one failed,
and the failure message names each failing group and case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harness
from fake_host import FakeHost
from orientation_truth import orient
from upsample_truth import CENTER, LEFT, NEAREST, upsample_plane, upsample_planes

pkg = harness.pkg
H = pkg.host
pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
T2_RTOL, T2_ATOL = 1e-4, 1e-9                                  # tests/test_gpu_read.py


def same(a, b):
    """array_equal on the bytes: bit for bit, so that a float NaN or a -0.0 cannot hide a difference."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def desc444(desc):
    d = pkg.ReadDesc.from_buffer_copy(desc)
    d.chroma = pkg.CHROMA_444
    return d


_refs = {}


def refs(gpu, desc, planes, mode, key):
    """(oracle image, the GPU's own 4:4:4 open of the truth planes -- depth 32 only) as (H, W, C), computed once per key."""
    key = (key, mode)
    if key not in _refs:
        xs, ys = harness.chroma_shift(desc.chroma)
        p444 = upsample_planes(planes, desc.width, desc.height, xs, ys, mode)
        d4 = desc444(desc)
        shape = (desc.height, desc.width, harness.read_channels(desc))
        want = harness.oracle_read(d4, p444).reshape(shape)
        own = harness.gpu_read(gpu, d4, p444).reshape(shape) if desc.depth == 32 else None
        want.setflags(write=False)
        _refs[key] = (want, own)
    return _refs[key]


def check(got, desc, ref, code, what):
    want, own = ref
    if desc.depth != 32:
        assert same(got, orient(code, want)), what
        return
    assert same(got, orient(code, own)), (what, "against the GPU's own 4:4:4 open")
    w64, g64 = np.ascontiguousarray(orient(code, want)).astype(np.float64), got.astype(np.float64)
    assert np.all(np.isfinite(g64)), what
    assert np.all(np.abs(g64 - w64) <= T2_RTOL * np.abs(w64) + T2_ATOL), (what, "T2 read bar against the oracle")


def tiles(desc, code, max_rows):
    out_h = pkg.read_oriented_geometry(desc, code)[1]
    o = 0
    while o < out_h:
        n = pkg.read_oriented_next_tile(desc, code, o, max_rows)
        assert n > 0
        yield o, n
        o += n


def open_upsampled(gpu, desc, planes, mode, code=1, mem="device", max_rows=None, pad=0, guard_rows=0, pinned=False, base_off=0):
    """The (oriented) upsampled image as (out_h, out_w, C), opened tile by tile (max_rows=None: one call).  `pad` extra bytes per
    destination row and `guard_rows` rows above and below are pre-filled with a sentinel and must come back untouched; `base_off` bytes
    in front of every source plane put its base off the 16-byte grid."""
    import torch
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16) + pad
    buf = np.full((out_h + 2 * guard_rows, stride), SENTINEL, dtype=np.uint8)
    cuts = list(tiles(desc, code, max_rows)) if max_rows else [(0, out_h)]
    used = harness.read_planes(desc)
    strides = [planes[pl].strides[0] if pl in used else 0 for pl in range(4)]
    if mem == "device":
        dev = f"cuda:{gpu.device}"
        d_pl = {}
        for pl in used:
            flat = np.concatenate([np.zeros(base_off, np.uint8), planes[pl].view(np.uint8).reshape(-1)])
            d_pl[pl] = torch.from_numpy(flat).to(dev)
        d_out = torch.from_numpy(buf.reshape(-1).copy()).to(dev)
        ptrs = [d_pl[pl].data_ptr() + base_off if pl in used else None for pl in range(4)]
        stream = torch.cuda.current_stream(dev).cuda_stream
        need = max([max(pkg.read_upsampled_scratch_bytes(desc, mode, code, n), pkg.read_oriented_scratch_bytes(desc, code, n)) for _, n in cuts] + [16])
        scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
        for o, n in cuts:
            gpu.read_rows_upsampled(desc, mode, code, o, n, ptrs, strides, d_out.data_ptr() + (guard_rows + o) * stride, stride,
                                    scratch.data_ptr(), need, mem=pkg.MEM_DEVICE, stream=stream)
        torch.cuda.synchronize(dev)
        buf = d_out.cpu().numpy().reshape(buf.shape)
    else:
        keep = []
        if pinned:
            host_planes = {}
            for pl in used:
                t = torch.from_numpy(planes[pl].copy()).pin_memory()
                keep.append(t)
                host_planes[pl] = t.numpy()
            t = torch.from_numpy(buf).pin_memory()
            keep.append(t)
            buf = t.numpy()
        else:
            host_planes = planes
        ptrs = [host_planes[pl].ctypes.data if pl in used else None for pl in range(4)]
        for o, n in cuts:
            gpu.read_rows_upsampled(desc, mode, code, o, n, ptrs, strides, buf.ctypes.data + (guard_rows + o) * stride, stride, mem=pkg.MEM_HOST)
        buf = buf.copy()
    body = buf[guard_rows:guard_rows + out_h]
    assert (body[:, row_bytes:] == SENTINEL).all(), "bytes beyond out_w * bytes per pixel were touched"
    if guard_rows:
        assert (buf[:guard_rows] == SENTINEL).all() and (buf[guard_rows + out_h:] == SENTINEL).all(), "rows outside the call were touched"
    return np.ascontiguousarray(body[:, :row_bytes]).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


# ---- formats: chroma x siting x bit depth x host depth, with the other descriptor fields varied over them ----------------------------
def _format_cases():
    mats = [(pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT709, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020),
            (pkg.MATRIX_RGB_GBR, pkg.PRIMARIES_BT709)]
    alphas = (pkg.ALPHA_NONE, pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED)
    out, n = [], 0
    for chroma in (pkg.CHROMA_420, pkg.CHROMA_422):
        for mode in (CENTER, LEFT):
            for bits, depth in ((8, 8), (10, 16), (12, 16), (10, 32), (12, 32)):
                # four descriptors per combination, from independent indices: both ranges x both transfer curves (depth 32), every alpha
                # state and every matrix rotating over them (the identity matrix: integer hosts only)
                for j in range(4):
                    fr, t = j & 1, j >> 1
                    m, pr = mats[(n + j) % (3 if depth == 32 else 4)]
                    kw = dict(width=37, height=21, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=bits, depth=depth,
                              alpha_state=alphas[(n + j) % 3], matrix_coefficients=m, color_primaries=pr, full_range_flag=fr)
                    if depth == 32:
                        kw.update(transfer_characteristics=(pkg.TC_PQ, pkg.TC_HLG)[t], color_primaries=pkg.PRIMARIES_BT2020, pq_peak_nits=(80, 1000)[fr],
                                  hlg_apply_ootf=(n + fr) % 2, hlg_display_gamma=1.2, hlg_peak_nits=1000)
                    out.append((f"c{chroma}-s{mode}-b{bits}-d{depth}-m{m}-a{kw['alpha_state']}-fr{fr}-tc{kw.get('transfer_characteristics', 0)}", mode, kw))
                n += 1
    # the coverage the issue names, asserted so that it cannot collapse: per host depth both ranges and all three alpha states; per
    # chroma x siting x bit depth x host depth both ranges; depth 32: PQ and HLG, HLG with and without the OOTF; every matrix
    for depth in (8, 16, 32):
        sel = [kw for _, _, kw in out if kw["depth"] == depth]
        assert {kw["full_range_flag"] for kw in sel} == {0, 1} and {kw["alpha_state"] for kw in sel} == set(alphas), depth
    for chroma in (pkg.CHROMA_420, pkg.CHROMA_422):
        for mode in (CENTER, LEFT):
            for bits, depth in ((8, 8), (10, 16), (12, 16), (10, 32), (12, 32)):
                sel = [kw for _, md, kw in out if md == mode and (kw["chroma"], kw["bit_depth"], kw["depth"]) == (chroma, bits, depth)]
                assert {kw["full_range_flag"] for kw in sel} == {0, 1}, (chroma, mode, bits, depth)
                if depth == 32:
                    assert {kw["transfer_characteristics"] for kw in sel} == {pkg.TC_PQ, pkg.TC_HLG}, (chroma, mode, bits)
    hlg = [kw for _, _, kw in out if kw["depth"] == 32 and kw["transfer_characteristics"] == pkg.TC_HLG]
    assert {kw["hlg_apply_ootf"] for kw in hlg} == {0, 1} and {kw["full_range_flag"] for kw in hlg} == {0, 1}
    assert {kw["matrix_coefficients"] for _, _, kw in out} == {m for m, _ in mats}
    assert len({cid for cid, _, _ in out}) == len(out)
    return out


def _formats(gpu):
    for cid, mode, kw in _format_cases():
        desc = pkg.ReadDesc(**kw)
        planes = harness.make_read_source(desc, seed=len(cid) * 7 + mode)
        got = open_upsampled(gpu, desc, planes, mode)
        check(got, desc, refs(gpu, desc, planes, mode, ("fmt", cid)), 1, cid)
        # not the nearest image: the interpolation happened
        assert not same(got, harness.gpu_read(gpu, desc, planes).reshape(got.shape)), cid


# ---- sizes around every unit of the kernel ------------------------------------------------------------------------------------------
def _sizes(ssz):
    lane, wave, wg = 16 // ssz, 1024 // ssz, 4096 // ssz
    widths = sorted({1, 2, 3, 5, lane - 1, lane, lane + 1, 2 * lane - 1, 2 * lane + 1, wave - 1, wave, wave + 1, wg - 1, wg, wg + 1})
    heights = (1, 2, 3, 5, 31, 32, 33, 65)
    sizes = [(w, h) for w in widths for h in (3, 33)] + [(w, h) for w in (lane + 1, wave + 1) for h in heights]
    return sorted(set(sizes + [(1, 1), (1, 70), (70, 1)]))


def _sizes_around_lane_wave_workgroup_and_band(gpu):
    for chroma, bits, depth in ((c, b, d) for b, d in ((8, 8), (12, 16)) for c in (pkg.CHROMA_420, pkg.CHROMA_422)):
        for W, Hh in _sizes(1 if bits == 8 else 2):
            desc = pkg.ReadDesc(width=W, height=Hh, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=bits, depth=depth,
                                alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT709)
            planes = harness.make_read_source(desc, seed=W * 131 + Hh)
            for mode in (CENTER, LEFT):
                got = open_upsampled(gpu, desc, planes, mode)
                check(got, desc, refs(gpu, desc, planes, mode, ("size", chroma, bits, W, Hh)), 1, (chroma, bits, W, Hh, mode))


# ---- tile invariance: a clamp against the tile instead of the plane shows here -------------------------------------------------------
SUBSAMPLED = [
    dict(chroma=pkg.CHROMA_420, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT601),
    dict(chroma=pkg.CHROMA_422, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT709),
    dict(chroma=pkg.CHROMA_420, bit_depth=12, depth=16, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=pkg.MATRIX_BT2020_NCL, full_range_flag=0),
    dict(chroma=pkg.CHROMA_422, bit_depth=10, depth=32, alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
         color_primaries=pkg.PRIMARIES_BT2020, transfer_characteristics=pkg.TC_PQ, pq_peak_nits=203),
]


def _tile_invariance(gpu):
    """33 x 31 and 34 x 32 in tiles of 1, 2 and 7 rows cut with avifgpu_read_oriented_next_tile: the single call, byte for byte."""
    for size in ((33, 31), (34, 32)):
        for i, kw in enumerate(SUBSAMPLED):
            desc = pkg.ReadDesc(width=size[0], height=size[1], colorspace=pkg.COLORSPACE_YCBCR, **kw)
            planes = harness.make_read_source(desc, seed=size[0] + i)
            mode = (CENTER, LEFT)[i % 2]
            ref = refs(gpu, desc, planes, mode, ("tile", i, size))
            for code in range(1, 9):
                whole = open_upsampled(gpu, desc, planes, mode, code)
                check(whole, desc, ref, code, (size, i, code, "whole"))
                for max_rows in (1, 2, 7):
                    assert same(open_upsampled(gpu, desc, planes, mode, code, max_rows=max_rows), whole), (size, i, code, max_rows)
                assert same(open_upsampled(gpu, desc, planes, mode, code, mem="host", max_rows=7), whole), (size, i, code, "host tiles")


# ---- nearest and the degenerate modes are today's entry points, byte for byte ---------------------------------------------------------
def _open_oriented_today(gpu, desc, planes, code):
    import torch
    dev = f"cuda:{gpu.device}"
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    row_bytes = out_w * nch * (desc.depth // 8)
    stride = harness.align(row_bytes, 16)
    used = harness.read_planes(desc)
    d_pl = {pl: torch.from_numpy(planes[pl].view(np.uint8).reshape(-1).copy()).to(dev) for pl in used}
    d_out = torch.full((out_h * stride,), SENTINEL, dtype=torch.uint8, device=dev)
    ptrs = [d_pl[pl].data_ptr() if pl in used else None for pl in range(4)]
    strides = [planes[pl].strides[0] if pl in used else 0 for pl in range(4)]
    need = max(pkg.read_oriented_scratch_bytes(desc, code, out_h), 16)
    scratch = torch.zeros((need,), dtype=torch.uint8, device=dev)
    gpu.read_rows_oriented(desc, code, 0, out_h, ptrs, strides, d_out.data_ptr(), stride, scratch.data_ptr(), need, mem=pkg.MEM_DEVICE,
                           stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = d_out.cpu().numpy().reshape(out_h, stride)[:, :row_bytes]
    return np.ascontiguousarray(got).view(harness.src_dtype(desc.depth)).reshape(out_h, out_w, nch)


def _nearest_and_degenerate_modes_are_the_existing_entry_points(gpu):
    sub = pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[0])
    others = [pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_444, bit_depth=8, depth=8,
                           alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_BT709),
              pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=12, depth=16,
                           alpha_state=pkg.ALPHA_STRAIGHT),
              pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=10, depth=16,
                           alpha_state=pkg.ALPHA_NONE, matrix_coefficients=pkg.MATRIX_RGB_GBR)]
    for desc, modes in [(sub, (NEAREST,))] + [(d, (NEAREST, CENTER, LEFT)) for d in others]:
        planes = harness.make_read_source(desc, seed=31)
        plain = harness.gpu_read(gpu, desc, planes).reshape(desc.height, desc.width, -1)
        for code in (1, 3, 6):
            today = _open_oriented_today(gpu, desc, planes, code)
            if code == 1:
                assert same(today, plain)
            for mode in modes:
                for mem in ("device", "host"):
                    got = open_upsampled(gpu, desc, planes, mode, code, mem=mem, max_rows=None if mem == "device" else 8)
                    assert same(got, today), (desc.colorspace, desc.chroma, mode, code, mem)


# ---- orientation: a missing horizontal halo shows in the column bands of codes 5-8 --------------------------------------------------
def _every_orientation_whole_and_in_bands(gpu):
    for size in ((67, 35), (130, 66)):
        for i, kw in enumerate(SUBSAMPLED):
            desc = pkg.ReadDesc(width=size[0], height=size[1], colorspace=pkg.COLORSPACE_YCBCR, **kw)
            planes = harness.make_read_source(desc, seed=size[1] + i)
            for mode in (CENTER, LEFT):
                ref = refs(gpu, desc, planes, mode, ("orient", i, size))
                for code in range(1, 9):
                    check(open_upsampled(gpu, desc, planes, mode, code), desc, ref, code, (size, i, mode, code, "whole"))
                    check(open_upsampled(gpu, desc, planes, mode, code, max_rows=16), desc, ref, code, (size, i, mode, code, "bands of 16"))


# ---- out-of-range container values: filtered as they are, then the decode's own rule ------------------------------------------------
def _out_of_range_container_values(gpu):
    for i, (chroma, bits, depth) in enumerate(((pkg.CHROMA_420, 10, 16), (pkg.CHROMA_422, 12, 16), (pkg.CHROMA_420, 12, 32), (pkg.CHROMA_422, 10, 32))):
        kw = dict(width=70, height=37, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=bits, depth=depth,
                  alpha_state=(pkg.ALPHA_STRAIGHT, pkg.ALPHA_NONE, pkg.ALPHA_PREMULTIPLIED, pkg.ALPHA_NONE)[i], matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                  color_primaries=pkg.PRIMARIES_BT2020)
        if depth == 32:
            kw.update(transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000)
        desc = pkg.ReadDesc(**kw)
        planes = harness.make_read_source_over_range(desc, seed=40 + i)
        assert max(int(planes[1].max()), int(planes[2].max())) == 0xFFFF           # 16 * 65535 in the joint sum
        for mode in (CENTER, LEFT):
            ref = refs(gpu, desc, planes, mode, ("over", i))
            for code in (1, 6):
                check(open_upsampled(gpu, desc, planes, mode, code), desc, ref, code, (i, mode, code))


# ---- buffers: plane bases and strides off the 16-byte grid, padded destination rows, guard rows -----------------------------------
def _unaligned_bases_strides_padding_and_guard_rows(gpu):
    for i, kw in enumerate(SUBSAMPLED):
        desc = pkg.ReadDesc(width=130, height=66, colorspace=pkg.COLORSPACE_YCBCR, **kw)
        planes = harness.make_read_source(desc, seed=5 + i, stride_pad=3)             # strides that are no multiple of 16 (nor of 8) bytes
        assert all(a.strides[0] % 8 for a in planes.values())
        off = 6 if desc.bit_depth > 8 else 3
        mode = (LEFT, CENTER)[i % 2]
        ref = refs(gpu, desc, planes, mode, ("pad", i))
        for code in (1, 2, 6, 7):
            check(open_upsampled(gpu, desc, planes, mode, code, pad=48, guard_rows=2, base_off=off), desc, ref, code, (i, code, "base and stride"))
            check(open_upsampled(gpu, desc, planes, mode, code, pad=48, guard_rows=2, max_rows=7, base_off=off), desc, ref, code, (i, code, "tiles"))
            check(open_upsampled(gpu, desc, planes, mode, code, mem="host", pad=48, guard_rows=2), desc, ref, code, (i, code, "host"))
            check(open_upsampled(gpu, desc, planes, mode, code, pad=4, guard_rows=1, base_off=16), desc, ref, code, (i, code, "destination stride no multiple of 16"))


# ---- HOST path: equals DEVICE for every number of bound contexts, pinned and pageable -------------------------------------------
def _host_equals_device_for_every_context_count(gpu):
    cases = [pkg.ReadDesc(width=130, height=66, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[0]),
             pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[1]),
             pkg.ReadDesc(width=33, height=31, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[2]),
             pkg.ReadDesc(width=67, height=35, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[3])]
    sources = [harness.make_read_source(d, seed=21 + i) for i, d in enumerate(cases)]
    modes = [CENTER, LEFT, CENTER, LEFT]
    codes = (1, 3, 6)
    device = [{code: open_upsampled(gpu, d, p, m, code) for code in codes} for d, p, m in zip(cases, sources, modes)]
    for i, (d, p, m) in enumerate(zip(cases, sources, modes)):
        for code in codes:
            check(device[i][code], d, refs(gpu, d, p, m, ("ctx", i)), code, (i, code, "device"))
    try:
        for n in (1, 2, 3):
            g = pkg.AvifGpu(devices=[gpu.device] * n)
            for i, (d, p, m) in enumerate(zip(cases, sources, modes)):
                for code in codes:
                    for pinned in (False, True):
                        assert same(open_upsampled(g, d, p, m, code, mem="host", pinned=pinned), device[i][code]), (n, i, code, pinned)
    finally:
        pkg.AvifGpu(gpu.device)                                            # the session's binding


def _host_stages_more_than_one_tile(gpu):
    """A whole-image HOST call larger than one staged tile (32 MiB of output): both slots, row tiles and several column bands, each with
    its own chroma window and halo."""
    desc = pkg.ReadDesc(width=2048, height=1100, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12, depth=32,
                        alpha_state=pkg.ALPHA_STRAIGHT, matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020,
                        transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000)                # 36 MB of output
    planes = harness.make_read_source(desc, seed=3)
    ref = refs(gpu, desc, planes, CENTER, ("hosttiles",))
    for code in (1, 6):
        dev = open_upsampled(gpu, desc, planes, CENTER, code)
        check(dev, desc, ref, code, ("device", code))
        assert same(open_upsampled(gpu, desc, planes, CENTER, code, mem="host", pinned=(code == 6)), dev), code


# ---- the FormatRecord shim ---------------------------------------------------------------------------------------------------
def _shim_open(gpu, desc, planes, mode, code, max_data, abort_after=None):
    out_w, out_h = pkg.read_oriented_geometry(desc, code)
    nch = harness.read_channels(desc)
    host = FakeHost(out_w, out_h, desc.depth, nch, max_data=max_data, abort_after=abort_after)
    img = H.Image(width=desc.width, height=desc.height, colorspace=desc.colorspace, chroma=desc.chroma, bit_depth=desc.bit_depth)
    for pl, a in planes.items():
        img.plane[pl] = a.ctypes.data
        img.stride[pl] = a.strides[0]
    nclx = H.Nclx(desc.color_primaries, desc.transfer_characteristics, desc.matrix_coefficients, desc.full_range_flag)
    rc = gpu.lib.avifgpu_host_read_heif_image_upsampled(ctypes.byref(img), code, mode, desc.alpha_state, ctypes.byref(nclx), None, ctypes.byref(host.fr))
    return host, rc


def _shim_delivers_upsampled_tiles_and_survives_a_cancel(gpu):
    desc = pkg.ReadDesc(width=34, height=31, colorspace=pkg.COLORSPACE_YCBCR, **SUBSAMPLED[0])
    planes = harness.make_read_source(desc, seed=17)
    nch = harness.read_channels(desc)
    for mode in (CENTER, LEFT):
        ref = refs(gpu, desc, planes, mode, ("shim",))
        for code in (1, 3, 6):
            out_w, out_h = pkg.read_oriented_geometry(desc, code)
            row_bytes = out_w * nch
            max_data = row_bytes * (out_h // 6)                            # tiles of a few rows, at least 6 of them
            host, rc = _shim_open(gpu, desc, planes, mode, code, max_data)
            assert rc == 0, gpu.lib.avifgpu_last_error()
            got = host.image.reshape(out_h, out_w, nch)
            check(got, desc, ref, code, (mode, code))
            assert same(got, open_upsampled(gpu, desc, planes, mode, code)), (mode, code, "equals the device result")
            assert len(host.rects) >= 5 and host.rects[0][0] == 0 and host.rects[-1][2] == out_h
            assert all(a[2] == b[0] for a, b in zip(host.rects[:-1], host.rects[1:]))
            assert all(r[1] == 0 and r[3] == out_w and (r[2] - r[0]) * row_bytes <= max_data for r in host.rects)
            assert host.polls == len(host.rects)
            assert [(r[0], r[2] - r[0]) for r in host.rects] == list(tiles(desc, code, out_h // 6))
    # a cancel at tile 2 leaves the next open intact
    host, rc = _shim_open(gpu, desc, planes, CENTER, 6, 31 * 3 * 5, abort_after=2)
    assert rc == pkg.userCanceledErr and len(host.rects) == 2
    host, rc = _shim_open(gpu, desc, planes, CENTER, 6, 31 * 3 * 5)
    assert rc == 0
    check(host.image.reshape(34, 31, 3), desc, refs(gpu, desc, planes, CENTER, ("shim",)), 6, "after the cancel")
    # an unknown mode delivers nothing; nearest is the oriented entry
    host, rc = _shim_open(gpu, desc, planes, 3, 6, 31 * 3 * 5)
    assert rc == pkg.formatBadParameters and not host.rects
    host, rc = _shim_open(gpu, desc, planes, NEAREST, 6, 31 * 3 * 5)
    assert rc == 0 and same(host.image.reshape(34, 31, 3), _open_oriented_today(gpu, desc, planes, 6))


def _cli_read_bilinear_orientation_6(gpu, tmp_path):
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avif-format_amd", "avifgpu_cli")
    desc = pkg.ReadDesc(width=203, height=37, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=8, depth=8,
                        alpha_state=pkg.ALPHA_NONE, has_nclx=0, color_primaries=0, transfer_characteristics=0, matrix_coefficients=0)
    planes = harness.make_read_source(desc, seed=8)
    want = open_upsampled(gpu, desc, planes, CENTER, 6)                    # the API
    with open(tmp_path / "in.planes", "wb") as f:
        for pl, (w, xs, ys) in harness.read_planes(desc).items():
            f.write(np.ascontiguousarray(planes[pl][:, :w]).tobytes())
    r = subprocess.run([cli, "read", "--width", "203", "--height", "37", "--depth", "8", "--bits", "8", "--colorspace", "ycbcr", "--chroma", "420",
                        "--chroma-upsampling", "bilinear", "--orientation", "6", "--maxdata", str(37 * 3 * 40), str(tmp_path / "in.planes"),
                        str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), dtype=np.uint8).reshape(203, 37, 3)
    assert same(got, want)
    check(got, desc, refs(gpu, desc, planes, CENTER, ("cli",)), 6, "cli")


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------
def _probe_upsample_alone(gpu):
    """2101 x 5: whole waves and a ragged lane; 128 x 96: whole lanes only, three bands.  Rows padded to 256 bytes (the aligned paths, as
    the library's own scratch), then tight (sample by sample); then an inner rectangle with an odd origin."""
    import torch
    dev = f"cuda:{gpu.device}"
    rng = np.random.default_rng(9)
    for W, Hh in ((2101, 5), (128, 96)):
        for dtype, top in ((np.uint8, 255), (np.uint16, 65535)):
            ssz = np.dtype(dtype).itemsize
            for chroma, ys in ((pkg.CHROMA_420, 1), (pkg.CHROMA_422, 0)):
                cw, ch = (W + 1) >> 1, (Hh + ys) >> ys
                C = [rng.integers(0, top + 1, size=(ch, cw)).astype(dtype) for _ in range(2)]
                for padded in (True, False):
                    sp = harness.align(cw * ssz, 256) if padded else cw * ssz
                    d_src = []
                    for c in C:
                        wide = np.zeros((ch, sp), np.uint8)
                        wide[:, :cw * ssz] = c.view(np.uint8).reshape(ch, -1)
                        d_src.append(torch.from_numpy(wide.reshape(-1)).to(dev))
                    for mode in (CENTER, LEFT):
                        want = [upsample_plane(c, W, Hh, ys, mode) for c in C]
                        for x0, y0, w, h in ((0, 0, W, Hh), (3, 1, W - 8, Hh - 2)):
                            dp = harness.align(w * ssz, 256) if padded else w * ssz
                            d_dst = [torch.full((h * dp,), SENTINEL, dtype=torch.uint8, device=dev) for _ in range(2)]
                            gpu.probe_upsample(ssz, chroma, mode, W, Hh, x0, y0, w, h, [t.data_ptr() for t in d_src], [sp, sp],
                                               [t.data_ptr() for t in d_dst], dp, None)
                            torch.cuda.synchronize(dev)
                            for k in range(2):
                                got = d_dst[k].cpu().numpy().reshape(h, dp)
                                what = (W, Hh, dtype.__name__, chroma, padded, mode, (x0, y0, w, h), k)
                                assert np.array_equal(got[:, :w * ssz].copy().view(dtype), want[k][y0:y0 + h, x0:x0 + w]), what
                                assert (got[:, w * ssz:] == SENTINEL).all(), what


# ---- the tests: few ids, many cases ------------------------------------------------------------------------------------------------------
def _run_groups(gpu, *groups):
    """Every group runs whatever the earlier ones did: a failure in one does not hide the others, and each message names its group
    and, through the group's own assertion message, its case."""
    failures = []
    for group in groups:
        try:
            group(gpu)
        except AssertionError as e:
            failures.append(f"{group.__name__.lstrip('_')}: {e!r}"[:2000])
    assert not failures, "\n".join(failures)


def test_kernel_alone_formats_sizes_and_out_of_range_values(gpu):
    _run_groups(gpu, _probe_upsample_alone, _formats, _sizes_around_lane_wave_workgroup_and_band, _out_of_range_container_values)


def test_tiles_orientations_buffers_and_degenerate_modes(gpu):
    _run_groups(gpu, _tile_invariance, _every_orientation_whole_and_in_bands, _unaligned_bases_strides_padding_and_guard_rows,
                _nearest_and_degenerate_modes_are_the_existing_entry_points)


def test_host_path_equals_device(gpu):
    _run_groups(gpu, _host_equals_device_for_every_context_count, _host_stages_more_than_one_tile)


def test_shim_and_cli(gpu, tmp_path):
    _run_groups(gpu, _shim_delivers_upsampled_tiles_and_survives_a_cancel, lambda g: _cli_read_bilinear_orientation_6(g, tmp_path))
