"""32-bit documents behind a LUT-based (A2B) profile on the GPU: write_px<..., icc = 8> runs lcms2's float stage program
(avifgpu_icc_pipeline32, captured by integration/LcmsTableBridge.cpp) in front of the transfer curve.

Checker: the real Little CMS 2 converting every row in place as ColorProfileConversion::ConvertRow does, then the oracle's pixel loop
(oracle/icc_oracle.c + harness.oracle_write).  Bar: tier 2 as for icc = 1 / 2 / 4 / 6, |delta code| <= 1 and >= 99.5 % exact."""
import ctypes
import os

import numpy as np
import pytest

import harness

pkg = harness.pkg
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICC_LIB = os.path.join(ROOT, "oracle", "liboracle_icc.so")


@pytest.fixture(scope="module")
def lcms():
    if not os.path.exists(ICC_LIB) or pkg.lcms_bridge() is None:
        pytest.skip("oracle/liboracle_icc.so or libavifgpu_lcms_bridge.so not built (lcms2 absent)")
    L = ctypes.CDLL(ICC_LIB)
    L.oracle_icc_make_a2b_profile.restype = ctypes.c_int32
    L.oracle_icc_make_a2b_profile.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]
    for name in ("oracle_icc_convert_rows_to_rec2020", "oracle_icc_convert_rows_to_srgb_float"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int32
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    return L


def _a2b(L, variant):
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.oracle_icc_make_a2b_profile(variant, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


def _program(icc, target, alpha):
    rc, prog = pkg.icc_pipeline32_from_profile(icc, target, alpha)
    assert rc == 0, pkg.load().avifgpu_last_error()
    return prog


def _reference(L, icc, d, src):
    """ConvertRow on every row (lcms2, in place), then the plug-in's pixel loop (the oracle)."""
    conv = src.copy()
    fn = L.oracle_icc_convert_rows_to_srgb_float if d.transfer == pkg.TRANSFER_CLIP else L.oracle_icc_convert_rows_to_rec2020
    assert fn(icc, len(icc), int(d.planes == 4), conv.ctypes.data, d.width, d.height, conv.strides[0]) == 0
    return harness.oracle_write(d, conv)


def _source(d, seed):
    """Random rows with HDR values (up to ~8x diffuse white) and a few negatives -- what a 32-bit document holds."""
    src = harness.make_write_source(d, seed=seed)
    rng = np.random.default_rng(seed)
    px = src.reshape(d.height, d.width, d.planes)
    px[..., :3] = rng.uniform(-0.05, 1.0, size=px[..., :3].shape).astype(np.float32)
    hdr = rng.random(size=(d.height, d.width)) < 0.2
    px[hdr, :3] *= rng.uniform(1.0, 8.0, size=(int(hdr.sum()), 1)).astype(np.float32)
    return src


def _gpu(gpu, d, src, prog, mem):
    if mem == "host":
        return _host_write(gpu, d, src, prog)
    import torch
    dev = f"cuda:{gpu.device}"
    bufs = harness._alloc_write_out(d, d.height)
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1)).to(dev)
    d_out = {pl: torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).to(dev) for pl, b in bufs.items()}
    ptrs = [d_out[i].data_ptr() if i in d_out else None for i in range(4)]
    strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
    gpu.write_rows(d, 0, d.height, d_src.data_ptr(), src.strides[0], ptrs, strides, mem=pkg.MEM_DEVICE,
                   stream=torch.cuda.current_stream(dev).cuda_stream, icc=prog)
    torch.cuda.synchronize(dev)
    for pl in bufs:
        bufs[pl] = d_out[pl].cpu().numpy().view(bufs[pl].dtype).reshape(bufs[pl].shape)
    return harness._trim(d, bufs, d.height, harness.write_planes)


def _host_write(gpu, d, src, prog):
    bufs = harness._alloc_write_out(d, d.height)
    ptrs = [bufs[i].ctypes.data if i in bufs else None for i in range(4)]
    strides = [bufs[i].strides[0] if i in bufs else 0 for i in range(4)]
    gpu.write_rows(d, 0, d.height, src.ctypes.data, src.strides[0], ptrs, strides, mem=pkg.MEM_HOST, icc=prog)
    return harness._trim(d, bufs, d.height, harness.write_planes)


def _check(st, what):
    print(f"icc=8 {what}: exact {st['exact_frac']:.5f} max {st['max_abs']}")
    assert st["max_abs"] <= 1, (what, st)
    assert harness.t2_exact_ok(st, harness.T2_MIN_EXACT_ICC), (what, st)


SAVES = [(pkg.TRANSFER_PQ, pkg.OUT_YCBCR, pkg.CHROMA_444, 10), (pkg.TRANSFER_PQ, pkg.OUT_YCBCR, pkg.CHROMA_422, 12),
         (pkg.TRANSFER_SMPTE428, pkg.OUT_YCBCR, pkg.CHROMA_420, 12), (pkg.TRANSFER_CLIP, pkg.OUT_YCBCR, pkg.CHROMA_420, 10),
         (pkg.TRANSFER_CLIP, pkg.OUT_YCBCR, pkg.CHROMA_422, 12), (pkg.TRANSFER_PQ, pkg.OUT_REFERENCE, pkg.CHROMA_444, 12),
         (pkg.TRANSFER_CLIP, pkg.OUT_REFERENCE, pkg.CHROMA_444, 10), (pkg.TRANSFER_SMPTE428, pkg.OUT_REFERENCE, pkg.CHROMA_444, 10)]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("transfer,output,chroma,bits", SAVES)
def test_icc8_matches_lcms2_then_the_pixel_loop(gpu, lcms, variant, planes, transfer, output, chroma, bits):
    icc = _a2b(lcms, variant)
    target = pkg.ICC_TARGET_SRGB_FLOAT if transfer == pkg.TRANSFER_CLIP else pkg.ICC_TARGET_REC2020_LINEAR
    prog = _program(icc, target, planes == 4)
    alpha = pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE
    d = pkg.WriteDesc(width=517, height=22, depth=32, planes=planes, bit_depth=bits, transfer=transfer, peak_nits=1000,
                      alpha_state=alpha, output=output, chroma=chroma, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                      color_primaries=pkg.PRIMARIES_BT2020)
    src = _source(d, 31 + variant)
    want = _reference(lcms, icc, d, src)
    got = _gpu(gpu, d, src, prog, "device")
    _check(harness.compare_write(d, want, got), f"v{variant} planes {planes} transfer {transfer} out {output} chroma {chroma} {bits}-bit")
    assert "icc=8" in gpu.last_kernel()


@pytest.mark.parametrize("mem", ["device", "host"])
def test_icc8_memory_kinds_and_the_device_memory_table_path(gpu, lcms, mem):
    """Host and device pointers; and the words read from device memory instead of LDS (tuning word bit 6), same codes."""
    icc = _a2b(lcms, 1)
    prog = _program(icc, pkg.ICC_TARGET_REC2020_LINEAR, True)
    d = pkg.WriteDesc(width=1030, height=40, depth=32, planes=4, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      alpha_state=pkg.ALPHA_PREMULTIPLIED, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_420,
                      matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
    src = _source(d, 77)
    want = _reference(lcms, icc, d, src)
    got = _gpu(gpu, d, src, prog, mem)
    _check(harness.compare_write(d, want, got), f"mem {mem}")
    lib = pkg.load()
    lib.avifgpu_set_hot_variant(1 | 2 | 4 | 64)
    try:
        got2 = _gpu(gpu, d, src, prog, mem)
        assert "icc=8" in gpu.last_kernel() and " lds" not in gpu.last_kernel()
    finally:
        lib.avifgpu_set_hot_variant(1 | 2 | 4)            # the library's default tuning word
    for pl in got:
        assert np.array_equal(got[pl], got2[pl]), pl


def test_icc8_second_save_with_another_program_at_the_same_address(gpu, lcms):
    """Two consecutive saves, the second with a different program written into the SAME struct: it must take the new program."""
    prog = pkg.IccPipeline32()
    d = pkg.WriteDesc(width=300, height=16, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444, matrix_coefficients=pkg.MATRIX_BT2020_NCL,
                      color_primaries=pkg.PRIMARIES_BT2020)
    src = _source(d, 5)
    outs = []
    for variant in (0, 1):
        icc = _a2b(lcms, variant)
        rc = pkg.lcms_bridge().avifgpu_lcms_document_to_pipeline32(icc, len(icc), pkg.ICC_TARGET_REC2020_LINEAR, 0, ctypes.byref(prog))
        assert rc == 0
        for mem in ("device", "host"):
            got = _gpu(gpu, d, src, prog, mem)
            _check(harness.compare_write(d, _reference(lcms, icc, d, src), got), f"save {variant} mem {mem}")
        outs.append(got)
    assert any(not np.array_equal(outs[0][pl], outs[1][pl]) for pl in outs[0])


def test_icc8_refuses_what_the_reference_never_does(gpu, lcms):
    icc = _a2b(lcms, 0)
    prog = _program(icc, pkg.ICC_TARGET_SRGB_FLOAT, False)
    d = pkg.WriteDesc(width=16, height=2, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      output=pkg.OUT_REFERENCE)
    with pytest.raises(pkg.AvifGpuError) as e:                # the sRGB target belongs to the Clip save
        _gpu(gpu, d, harness.make_write_source(d), prog, "device")
    assert e.value.code == pkg.formatBadParameters
    d16 = pkg.WriteDesc(width=16, height=2, depth=16, planes=3, bit_depth=10, output=pkg.OUT_REFERENCE)
    with pytest.raises(pkg.AvifGpuError) as e:                # 32-bit documents only
        _gpu(gpu, d16, harness.make_write_source(d16), prog, "device")
    assert e.value.code == pkg.formatBadParameters


def test_icc8_whole_document_through_the_host_shim(gpu, lcms):
    """One whole 8192^2 32-bit document behind an A2B profile through avifgpu_host_create_heif_image_with_pipeline in advanceState tiles,
    against lcms2's ConvertRow row by row (row bands on at most 16 threads: every oracle call opens its own lcms2 context) and the
    oracle's pixel loop."""
    import concurrent.futures
    from fake_host import FakeHost
    from test_gpu_fullsize import _oracle_frame
    H_ = pkg.host
    W = 8192
    icc = _a2b(lcms, 1)
    d = pkg.WriteDesc(width=W, height=W, depth=32, planes=3, bit_depth=12, transfer=pkg.TRANSFER_PQ, peak_nits=1000,
                      output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_422, chroma_downsampling=pkg.DOWNSAMPLE_NEAREST,
                      matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
    rng = np.random.default_rng(2024)
    src = rng.random((W, W * 3), dtype=np.float32)
    hdr = rng.random((W, W * 3), dtype=np.float32) < 0.1
    src[hdr] *= 6.0
    prog = _program(icc, pkg.ICC_TARGET_REC2020_LINEAR, False)

    host = FakeHost(W, W, 32, 3, max_data=64 << 20, image=src)
    keep = ctypes.create_string_buffer(icc, len(icc))
    host.fr.iCCprofileData = ctypes.cast(keep, ctypes.c_void_p)
    host.fr.iCCprofileSize = len(icc)
    opts = H_.SaveUIOptions(imageBitDepth=12, hdrTransferFunction=pkg.TRANSFER_PQ, pq=H_.PQOptions(1000),
                            chromaSubsampling=pkg.CHROMA_422, lossless=0, convertToRec2020=1)
    # the plain entry cannot take the profile: that is where the plug-in used to fall back to lcms2
    img0 = H_.Image()
    assert gpu.lib.avifgpu_host_create_heif_image(ctypes.byref(host.fr), pkg.ALPHA_NONE, ctypes.byref(opts), pkg.OUT_YCBCR,
                                                  pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020, ctypes.byref(img0)) == pkg.formatCannotRead
    gpu.lib.avifgpu_image_free(ctypes.byref(img0))
    host = FakeHost(W, W, 32, 3, max_data=64 << 20, image=src)
    host.fr.iCCprofileData = ctypes.cast(keep, ctypes.c_void_p)
    host.fr.iCCprofileSize = len(icc)
    img = H_.Image()
    code = gpu.lib.avifgpu_host_create_heif_image_with_pipeline(ctypes.byref(host.fr), pkg.ALPHA_NONE, ctypes.byref(opts), pkg.OUT_YCBCR,
                                                                pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020, ctypes.byref(prog), ctypes.byref(img))
    assert code == 0, gpu.lib.avifgpu_last_error()
    got = {}
    for pl, (w, xs, ys) in harness.write_planes(d).items():
        h = (d.height + ys) >> ys
        raw = (ctypes.c_uint8 * (img.stride[pl] * h)).from_address(img.plane[pl])
        got[pl] = np.frombuffer(raw, dtype=np.uint8).reshape(h, img.stride[pl])[:, :w * 2].view(np.uint16).copy()
    gpu.lib.avifgpu_image_free(ctypes.byref(img))

    conv = src.copy()
    step = W // 32
    def one(r0):
        part = conv[r0:r0 + step]
        return lcms.oracle_icc_convert_rows_to_rec2020(icc, len(icc), 0, part.ctypes.data, W, part.shape[0], conv.strides[0])
    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        assert all(rc == 0 for rc in ex.map(one, range(0, W, step)))
    want = _oracle_frame(d, conv)
    want = {pl: want[pl][:(d.height + ys) >> ys, :w] for pl, (w, xs, ys) in harness.write_planes(d).items()}
    _check(harness.compare_write(d, want, got), "whole 8192^2 document through the shim")
    # a program for the other target is refused (its proof ran against another transform)
    other = _program(icc, pkg.ICC_TARGET_SRGB_FLOAT, False)
    host = FakeHost(64, 8, 32, 3, image=src[:8, :64 * 3].copy())
    host.fr.iCCprofileData = ctypes.cast(keep, ctypes.c_void_p)
    host.fr.iCCprofileSize = len(icc)
    img2 = H_.Image()
    assert gpu.lib.avifgpu_host_create_heif_image_with_pipeline(ctypes.byref(host.fr), pkg.ALPHA_NONE, ctypes.byref(opts), pkg.OUT_YCBCR,
                                                                pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020, ctypes.byref(other),
                                                                ctypes.byref(img2)) == pkg.formatBadParameters
    gpu.lib.avifgpu_image_free(ctypes.byref(img2))
