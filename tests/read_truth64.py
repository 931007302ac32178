"""Float64 truth of a 32-bit (float-host) open, sample by sample, and the two bars that hold an open to it.  Shared by
tests/test_gpu_read_truth.py (random frames), tests/test_whole_float_opens.py and tests/test_zz_gpu_whole_float_opens.py (whole code
domains); the derivation of the bars is in the docstring of tests/test_gpu_read_truth.py.

    R = Y + 2(1 - kr) Cr,  B = Y + 2(1 - kb) Cb,  G = Y - 2(kr(1 - kr) Cr + kb(1 - kb) Cb) / kg   (kg = 1 - kr - kb), clamped;
    unpremultiply min(c / A, 1); EOTF; HLG OOTF

 * the float64-chain bar   |k - T|   <= eps |T| + dT(dV) + 1e-12: everything in float64 from the float32 tables and kr, kb; dV is the
                           rounding budget of the float32 YCbCr -> RGB step (N_RB, N_G roundings) and dT(dV) the chain's excursion
                           under it.  Seven evaluations of the curve per sample: chain_bar=False leaves it out.
 * the float32-step bar    |k - T32| <= eps |T32| + 1e-12: the YCbCr -> RGB step, clamp and unpremultiply in float32 exactly as the
                           reference orders them (_ycc_float32), only the curve in float64.  Always computed; the tighter of the two.

Numpy and the CPU oracle only; nothing here touches a GPU."""
import ctypes
import types

import numpy as np

import harness
import oracle_binding
import truth64

pkg = harness.pkg
U = truth64.U32
N_RB, N_G = 3, 9
OOTF_EPS = 1e-6                  # float32 luma sum, powf and product of the OOTF (about 6 roundings of 6e-8, with margin)


def _transfer(tc):
    return {pkg.TC_PQ: pkg.TRANSFER_PQ, pkg.TC_HLG: pkg.TRANSFER_HLG, pkg.TC_SMPTE428: pkg.TRANSFER_SMPTE428}[tc]


def unpremultiply_codes(color, alpha, maxc):
    """UnpremultiplyColor on codes as oracle/avif_oracle.c has it (oracle_unpremultiply_u16), vectorised: in float32
    v = min(color * max / alpha, max), then min(roundf(v), max).  color * max is below 2^24 for max <= 4095, so the product is exact
    and the quotient is the one float32 rounding; roundf (halves away from zero) of a non-negative float is floor(v + 0.5) taken where
    the sum is exact, in float64.  alpha must be >= 1 (callers select alpha == 0 away, as the reference does before it divides).
    tests/test_whole_float_opens.py holds this equal to the oracle on every (code, alpha) pair at 10 bit and on every 16th alpha row
    at 12 bit."""
    f = np.float32
    c, a = np.asarray(color).astype(f), np.asarray(alpha).astype(f)
    v = np.minimum((c * f(maxc)) / a, f(maxc))
    assert v.dtype == np.float32
    return np.minimum(np.floor(v.astype(np.float64) + 0.5), float(maxc)).astype(np.int64)


def _full(d, planes, pl):
    """Plane pl sampled at every pixel (chroma index x >> xs, row >> ys), clamped to maxc as the reference does."""
    w, xs, ys = harness.read_planes(d)[pl]
    arr = planes[pl].astype(np.int64)
    r = np.arange(d.height) >> ys
    x = np.arange(d.width) >> xs
    return np.minimum(arr[r][:, x], (1 << d.bit_depth) - 1)


def _chain(d, V):
    """EOTF (+ HLG OOTF) of (..., 3) or (..., 1) float64 values in float64."""
    tr = _transfer(d.transfer_characteristics)
    if tr == pkg.TRANSFER_PQ:
        return truth64.pq_to_linear64(V, d.pq_peak_nits)
    if tr == pkg.TRANSFER_SMPTE428:
        return truth64.smpte428_to_linear64(V)
    e = truth64.hlg_to_linear64(V)
    if d.hlg_apply_ootf and V.shape[-1] == 3:
        L = oracle_binding.load()
        luma = (ctypes.c_float * 3)()
        assert L.oracle_hlg_luma_coefficients(d.color_primaries, ctypes.byref(luma)) == 0
        e = truth64.hlg_ootf64(e, list(luma), d.hlg_display_gamma, float(np.float32(d.hlg_peak_nits)))
    return e


def _ycc_tables(d):
    """(T_Y, T_UV, T_A, (kr, kg, kb)) as the reference builds them, float32."""
    L = oracle_binding.load()
    count = 1 << d.bit_depth
    ty, tuv, ta = (np.zeros(count, np.float32) for _ in range(3))
    L.oracle_build_yuv_tables(1, d.matrix_coefficients, d.full_range_flag, d.bit_depth, 0, ty.ctypes.data, tuv.ctypes.data, ta.ctypes.data)
    k = (ctypes.c_float * 3)()
    L.oracle_get_yuv_coefficients(1, d.matrix_coefficients, d.color_primaries, ctypes.byref(k))
    return ty, tuv, ta, k


def ycc_v32(d, planes):
    """What a YCbCr open hands its curve: _ycc_float32 alone, no curve evaluated."""
    maxc = (1 << d.bit_depth) - 1
    ua = _full(d, planes, 3) if d.alpha_state != pkg.ALPHA_NONE else np.full((d.height, d.width), maxc)
    ty, tuv, ta, k = _ycc_tables(d)
    return _ycc_float32(d, ty, tuv, ta, k, planes, ua)


def truth_parts(d, planes, eps, chain_bar=True):
    """Everything a comparison may want, as a namespace:
      T, bound      (H, W, ncol) float64: the float64 chain and its bar -- None with chain_bar=False
      T32, bound32  the float32 step under the float64 curve, and its bar
      V32           what the curve is given by the float32 step (float64 holding float32 values; table values for planar RGB and gray)
      q             planar RGB / gray: the code whose table value V32 is (after the integer unpremultiply); None for YCbCr
      alpha         (H, W) float32 table values, or None"""
    L = oracle_binding.load()
    maxc = (1 << d.bit_depth) - 1
    count = 1 << d.bit_depth
    mono = d.colorspace == pkg.COLORSPACE_MONOCHROME
    rgb = d.colorspace == pkg.COLORSPACE_RGB
    has_alpha = d.alpha_state != pkg.ALPHA_NONE
    premul = d.alpha_state == pkg.ALPHA_PREMULTIPLIED
    ua = _full(d, planes, 3) if has_alpha else np.full((d.height, d.width), maxc)
    q = None

    if rgb or mono:                          # integer-domain unpremultiply (exact), then a table value: dV = 0
        q = np.stack([_full(d, planes, k) for k in ((0,) if mono else (0, 1, 2))], -1)
        if premul:
            sel = ua < maxc
            uq = np.where(ua[..., None] == 0, 0, unpremultiply_codes(q, np.maximum(ua, 1)[..., None], maxc))   # (a == 0 is selected away)
            q = np.where(sel[..., None], uq, q)
        if rgb:
            tab = np.arange(count, dtype=np.float32) / np.float32(count - 1)      # ReadHeifImage.cpp:402-415
            alpha = tab[ua] if has_alpha else None
        else:
            ty, ta = (np.zeros(count, np.float32) for _ in range(2))
            L.oracle_build_yuv_tables(1, d.matrix_coefficients, d.full_range_flag, d.bit_depth, 1, ty.ctypes.data, None, ta.ctypes.data)
            tab = ty
            alpha = ta[ua] if has_alpha else None
        V = tab[q].astype(np.float64)
        dV = np.zeros_like(V)
        V32 = V
    else:
        ty, tuv, ta, k = _ycc_tables(d)
        alpha = ta[ua] if has_alpha else None
        V32 = _ycc_float32(d, ty, tuv, ta, k, planes, ua)
        if chain_bar:
            kr, kb = float(k[0]), float(k[2])
            kg = 1.0 - kr - kb
            Y = ty[_full(d, planes, 0)].astype(np.float64)
            Cb = tuv[_full(d, planes, 1)].astype(np.float64)
            Cr = tuv[_full(d, planes, 2)].astype(np.float64)
            r_t, b_t = 2 * (1 - kr) * Cr, 2 * (1 - kb) * Cb
            g_t = 2 * (kr * (1 - kr) * Cr + kb * (1 - kb) * Cb) / kg
            V = np.clip(np.stack([Y + r_t, Y - g_t, Y + b_t], -1), 0.0, 1.0)
            g_mag = 2 * (np.abs(kr * (1 - kr) * Cr) + np.abs(kb * (1 - kb) * Cb)) / kg
            dV = np.stack([N_RB * U * (np.abs(Y) + np.abs(r_t)), N_G * U * (np.abs(Y) + g_mag), N_RB * U * (np.abs(Y) + np.abs(b_t))], -1)
            if premul:
                A = ta[ua].astype(np.float64)[..., None]
                sel = (ua < maxc)[..., None]
                with np.errstate(divide="ignore", invalid="ignore"):
                    Vu = np.minimum(V / A, 1.0)
                    dVu = dV / A + U * Vu
                V = np.where(sel, np.where(A == 0, 0.0, Vu), V)
                dV = np.where(sel, np.where(A == 0, 0.0, dVu), dV)

    eps_t = eps
    if _transfer(d.transfer_characteristics) == pkg.TRANSFER_HLG and d.hlg_apply_ootf and not mono:
        eps_t = eps * (1 + abs(float(np.float32(d.hlg_display_gamma)) - 1)) + OOTF_EPS
    T = bound = None
    if chain_bar:
        T = _chain(d, V)
        exc = np.zeros_like(T)
        for ch in range(V.shape[-1]):
            if not np.any(dV[..., ch]):
                continue
            worst = np.zeros_like(T)
            for s in (-1.0, 1.0):
                Vs = V.copy()
                Vs[..., ch] = np.clip(V[..., ch] + s * dV[..., ch], 0.0, 1.0)
                worst = np.maximum(worst, np.abs(_chain(d, Vs) - T))
            exc += worst
        bound = eps_t * np.abs(T) + exc + 1e-12
    T32 = _chain(d, V32)
    return types.SimpleNamespace(T=T, bound=bound, alpha=alpha, T32=T32, bound32=eps_t * np.abs(T32) + 1e-12, V32=V32, q=q)


def truth_and_bound(d, planes, eps, chain_bar=True):
    """(T, bound, alpha, T32, bound32) -- T, T32 and the bounds (H, W, ncol) float64; alpha (H, W) float32 or None.  With
    chain_bar=False T and bound are None (the float64-chain bar is skipped), the float32-step bar is computed all the same."""
    p = truth_parts(d, planes, eps, chain_bar)
    return p.T, p.bound, p.alpha, p.T32, p.bound32


def _ycc_float32(d, ty, tuv, ta, k, planes, ua):
    """The YCbCr -> RGB step, clamp and unpremultiply restated in float32 operation by operation as the reference performs them
    (YuvDecode.cpp:312-314, :369-388) -- the kernels claim these very bits (the integer tiers hold them bit-exact)."""
    f = np.float32
    one, two = f(1.0), f(2.0)
    kr, kg, kb = f(k[0]), f(k[1]), f(k[2])
    Y, Cb, Cr = ty[_full(d, planes, 0)], tuv[_full(d, planes, 1)], tuv[_full(d, planes, 2)]
    R = Y + (two * (one - kr)) * Cr
    B = Y + (two * (one - kb)) * Cb
    G = Y - ((two * ((kr * (one - kr) * Cr) + (kb * (one - kb) * Cb))) / kg)
    V = np.clip(np.stack([R, G, B], -1), f(0.0), f(1.0))
    assert V.dtype == np.float32
    if d.alpha_state == pkg.ALPHA_PREMULTIPLIED:
        maxc = (1 << d.bit_depth) - 1
        A = ta[ua][..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            Vu = np.minimum((V * one) / A, one)
        V = np.where((ua < maxc)[..., None], np.where(A == 0, f(0.0), Vu), V)
    return V.astype(np.float64)


def _split(d, out):
    nch = harness.read_channels(d)
    ncol = 1 if d.colorspace == pkg.COLORSPACE_MONOCHROME else 3
    px = out.reshape(d.height, d.width, nch)
    return px[..., :ncol].astype(np.float64), (px[..., ncol] if nch > ncol else None)


def _check(cid, d, got, eps, planes, chain_bar=True, parts=None):
    """Every colour sample under both bars (the float32-step bar alone with chain_bar=False), alpha bit-equal.  Returns the worst
    error / bound of the float64 chain (None where skipped) and of the float32 step.  `parts` takes a truth_parts() already computed."""
    p = parts if parts is not None else truth_parts(d, planes, eps, chain_bar)
    col, a = _split(d, got)
    assert np.all(np.isfinite(col)), cid
    used = []
    for t, b in ((p.T, p.bound), (p.T32, p.bound32)):
        if t is None:
            used.append(None)
            continue
        err = np.abs(col - t)
        ratio = err / b
        worst = np.unravel_index(np.argmax(ratio), err.shape)
        assert np.all(err <= b), (cid, int(np.sum(err > b)), worst, float(col[worst]), float(t[worst]), float(b[worst]))
        used.append(float(ratio[worst]))
    if p.alpha is not None:
        assert np.array_equal(a.view(np.uint32), p.alpha.view(np.uint32)), cid
    return tuple(used)
