"""The definition of the upsampled open (include/avifgpu.h "upsampled open"), as integer numpy: shared by the CPU and the GPU tests.

U[y, x] = (sum_a sum_b wy_a wx_b C[jy_a, ix_b] + 8) >> 4, taps as (index, weight in quarters), indices clamped to the plane."""
import numpy as np

NEAREST, CENTER, LEFT = 0, 1, 2


def taps(n, size, rule):
    """(idx0, w0, idx1, w1) for output positions 0..n-1 over `size` source samples; rule: "center", "left" or "copy" (not subsampled)."""
    p = np.arange(n)
    if rule == "copy":
        return p, np.full(n, 4, np.uint32), p, np.zeros(n, np.uint32)
    i, odd = p >> 1, (p & 1).astype(bool)
    if rule == "center":
        idx0, w0 = np.where(odd, i, i - 1), np.where(odd, 3, 1)
        idx1, w1 = np.where(odd, i + 1, i), np.where(odd, 1, 3)
    else:
        idx0, w0 = i, np.where(odd, 2, 4)
        idx1, w1 = np.where(odd, i + 1, i), np.where(odd, 2, 0)
    return np.clip(idx0, 0, size - 1), w0.astype(np.uint32), np.clip(idx1, 0, size - 1), w1.astype(np.uint32)


def upsample_plane(C, W, H, ys, siting, separable=False):
    """U (H, W) of chroma plane C ((H + ys) >> ys, (W + 1) >> 1), same dtype.  separable=True rounds once per direction instead of once:
    NOT the definition -- there so that a test can show the two differ."""
    assert siting in (CENTER, LEFT)
    cw, ch = (W + 1) >> 1, (H + ys) >> ys
    assert C.shape == (ch, cw), (C.shape, ch, cw)
    c = C.astype(np.uint32)
    ix0, wx0, ix1, wx1 = taps(W, cw, "center" if siting == CENTER else "left")
    jy0, wy0, jy1, wy1 = taps(H, ch, "center" if ys else "copy")
    h = wx0[None, :] * c[:, ix0] + wx1[None, :] * c[:, ix1]                      # (ch, W): unrounded horizontal sums
    if separable:
        h = (h + 2) >> 2
        return ((wy0[:, None] * h[jy0] + wy1[:, None] * h[jy1] + 2) >> 2).astype(C.dtype)
    return ((wy0[:, None] * h[jy0] + wy1[:, None] * h[jy1] + 8) >> 4).astype(C.dtype)


def upsample_planes(planes, W, H, xs, ys, siting):
    """The 4:4:4 planes (Y, U(Cb), U(Cr), A) of a 4:2:x source {plane: (rows, stride) array}: chroma rows padded to 8 samples like
    harness.make_read_source's, Y and A passed through."""
    assert xs == 1
    out = {}
    for pl, a in planes.items():
        if pl in (1, 2):
            u = upsample_plane(np.ascontiguousarray(a[:(H + ys) >> ys, :(W + 1) >> 1]), W, H, ys, siting)
            wide = np.zeros((H, (W + 7) // 8 * 8), dtype=a.dtype)
            wide[:, :W] = u
            out[pl] = wide
        else:
            out[pl] = a
    return out
