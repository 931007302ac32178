"""The exponent-field sweep of the close PQ form: its inputs, and the launches whose planes show the stage-A codes.

Shared by tests/test_zzzzzz_gpu_pq_half_table.py and tests/golden/make_pq_exponent_fields_codes.py, so that the fixture and the test
cannot drift apart.

  floats()     all 512 sign + exponent fields x mantissas {0, 1, 0x2AAAAA, 0x400000, 0x7FFFFF}: 2 560 float32, +-0, denormals,
               +-Inf, both NaN signs and negative normals down to -3.4e38 among them
  rgb()        a 512 x 15 RGB document of 7 680 pixels: pixel 3 i + c holds float i in channel slot c and OTHER (a plain
               positive sample) in the two other slots -- every float meets every slot, 15 whole 512-pixel spans
  gray()       the same floats as a 512 x 15 gray document: pixel 3 i + c holds float i
  FORMS        (name, planes, descriptor extras, tuning word, (kernel, label part))
  run(...)     one form at one depth -> (7 680, 3) int32 stage-A codes [pixel, channel] (gray: (7 680, 1)), launch label asserted
"""
import numpy as np

import harness

pkg = harness.pkg

WIDTH, HEIGHT = 512, 15
MANTISSAS = (0, 1, 0x2AAAAA, 0x400000, 0x7FFFFF)
OTHER = np.float32(0.18)
DEPTHS = (10, 12)
PEAK = 80
FILL = 0x5A5A                            # above every code: a sample nothing wrote
STREAMING, STREAMING_PXL4, GENERIC, DEFAULT_WORD = 1 | 2 | 4 | 8, 1 | 4 | 8, 0, 1 | 2 | 4
GBR = dict(matrix_coefficients=pkg.MATRIX_RGB_GBR, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444)
REF = dict(output=pkg.OUT_REFERENCE)
# under the GBR matrix the planes are the stage-A codes: Y <- G, Cb <- B, Cr <- R
GBR_PLANE_OF_CHANNEL = (2, 0, 1)

FORMS = (
    ("hot_pxl8", 3, GBR, STREAMING, ("write_rgb32_ycbcr444_hot", "pxl=8")),
    ("hot_pxl4", 3, GBR, STREAMING_PXL4, ("write_rgb32_ycbcr444_hot", "pxl=4")),
    ("rgba_hot", 4, GBR, STREAMING, ("write_rgba32_ycbcra444_hot", "transfer=")),
    ("write_px", 3, GBR, GENERIC, ("write_px", "transfer=4,")),          # 4: the close evaluation's template argument
    ("ref_stream", 3, REF, STREAMING, ("write_f32_ref_stream", "planes=3")),
    ("gray", 1, REF, STREAMING, ("write_f32_ref_stream", "planes=1")),
)


def floats():
    fields = np.arange(512, dtype=np.uint32)[:, None] << 23
    return (fields | np.asarray(MANTISSAS, dtype=np.uint32)[None, :]).reshape(-1).view(np.float32)


def rgb():
    v = floats()
    px = np.full((3 * v.shape[0], 3), OTHER, dtype=np.float32)
    for c in range(3):
        px[c::3, c] = v
    assert px.shape[0] == WIDTH * HEIGHT
    return px


def gray():
    return np.repeat(floats(), 3).reshape(WIDTH * HEIGHT, 1)


def source(planes):
    """(HEIGHT, WIDTH * planes) float32 of a form's document; alpha, where there is one, is 1."""
    px = gray() if planes == 1 else rgb()
    if planes == 4:
        px = np.concatenate([px, np.ones((px.shape[0], 1), dtype=np.float32)], 1)
    return np.ascontiguousarray(px.reshape(HEIGHT, WIDTH * planes))


def desc(planes, bits, extras):
    return pkg.WriteDesc(width=WIDTH, height=HEIGHT, depth=32, planes=planes, bit_depth=bits, transfer=pkg.TRANSFER_PQ, peak_nits=PEAK,
                         alpha_state=pkg.ALPHA_STRAIGHT if planes == 4 else pkg.ALPHA_NONE, **extras)


def save(gpu, d, src_np, word, kernel):
    """`src_np` through avifgpu_write_rows under the tuning word `word`; the launch label must begin with kernel[0] and hold kernel[1].
    Returns {plane: (rows, samples) int32 numpy array}."""
    import torch
    dev = f"cuda:{gpu.device}"
    src = torch.from_numpy(src_np).to(dev)
    out = {pl: torch.full((d.height, w), FILL, dtype=torch.int16, device=dev) for pl, (w, _, _) in harness.write_planes(d).items()}
    ptrs = [out[i].data_ptr() if i in out else None for i in range(4)]
    strides = [out[i].stride(0) * 2 if i in out else 0 for i in range(4)]
    gpu.lib.avifgpu_set_hot_variant(word)
    try:
        gpu.write_rows(d, 0, d.height, src.data_ptr(), src.stride(0) * 4, ptrs, strides, mem=pkg.MEM_DEVICE,
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_WORD)
    label = gpu.last_kernel()
    assert label.startswith(kernel[0] + "<") and kernel[1] in label, (label, kernel)
    torch.cuda.synchronize(dev)
    return {pl: t.cpu().numpy().astype(np.int32) for pl, t in out.items()}


def run(gpu, form, bits):
    name, planes, extras, word, kernel = form
    d = desc(planes, bits, extras)
    out = save(gpu, d, source(planes), word, kernel)
    if planes == 4:
        assert (out[3] == (1 << bits) - 1).all(), (name, bits, "alpha 1")
    if extras is GBR:
        return np.stack([out[GBR_PLANE_OF_CHANNEL[c]].reshape(-1) for c in range(3)], 1)
    return out[0].reshape(WIDTH * HEIGHT, planes)
