"""Float-tier opens (32-bit documents) against float64 truth of the WHOLE chain, sample by sample (avif_oracle.c:750-790,
YuvDecode.cpp:281-696, ReadHeifImage.cpp:1027-1176).

tests/test_gpu_read.py holds every 32-bit open to 1e-4 relative of the oracle, and tests/test_gpu_t2_truth.py holds the EOTF alone
to 1e-5 (PQ) / 2e-6 (HLG, SMPTE 428) on planar RGB.  A kernel whose YCbCr -> RGB step, chroma index, limited-range table, float
unpremultiply or HLG OOTF is a few ulps off fits under 1e-4.  Here the truth is computed in float64 from the float32 tables as the
reference builds them and the float32 kr, kb:

    R = Y + 2(1 - kr) Cr,  B = Y + 2(1 - kb) Cb,  G = Y - 2(kr(1 - kr) Cr + kb(1 - kb) Cb) / kg   (kg = 1 - kr - kb), clamped;
    unpremultiply min(c / A, 1); EOTF; HLG OOTF

and every colour sample must satisfy |k - T| <= eps |T| + dT(dV) + 1e-12, where
 * eps is the EOTF bar (KERNEL_EOTF_EPS for the kernels; ORACLE_EOTF_EPS for the oracle, whose float32 PQ formula cancels),
   widened by the OOTF's own float32 evaluation where one is applied;
 * dV bounds the float32 roundings of the YCbCr -> RGB step: N * 2^-24 * (|Y| + |coef * C|) with N = 3 for R and B (1 - kr, the
   product, the sum) and N = 9 for G (1 - kr, kr(1 - kr), the product, twice; the sum; kg = 1 - kr - kb rounded twice in float32;
   the quotient; the difference), then / A plus one rounding of the quotient where the colour is unpremultiplied;
 * dT(dV) is the largest excursion of the float64 chain (curve and OOTF) when each channel's V moves by its dV, summed over the
   channels (for each channel the chain is monotone in V, so this is |dT/dV| * dV taken at its worst point).
Alpha is table lookup only and must be bit-exact.  Mono and planar RGB carry no float32 step in front of the curve (dV = 0).

A second, tighter bar takes the YCbCr -> RGB step, clamp and unpremultiply in float32 exactly as the reference orders them (the
kernels claim those bits: the integer tiers hold them bit-exact) and only the curve in float64: |k - T32| <= eps |T32| + 1e-12.
That is the bar a kr / kg / kb a few ulps off, or a reordered sum, fails where the float64 bound's rounding budget would hide it.

The CPU half checks both bounds against the oracle, so they are shown sound before they judge a kernel."""
import ctypes

import numpy as np
import pytest

import cases
import harness
import oracle_binding
import truth64

pkg = harness.pkg
U = truth64.U32
N_RB, N_G = 3, 9
OOTF_EPS = 1e-6                  # float32 luma sum, powf and product of the OOTF (about 6 roundings of 6e-8, with margin)


def _transfer(tc):
    return {pkg.TC_PQ: pkg.TRANSFER_PQ, pkg.TC_HLG: pkg.TRANSFER_HLG, pkg.TC_SMPTE428: pkg.TRANSFER_SMPTE428}[tc]


def _read_truth_cases():
    out = [(cid, kw) for cid, kw in cases.read_cases() if cases.is_float_tier_read(kw)]
    for tc in (pkg.TC_PQ, pkg.TC_HLG, pkg.TC_SMPTE428):              # limited range, every chroma format
        for chroma, a in ((pkg.CHROMA_420, pkg.ALPHA_PREMULTIPLIED), (pkg.CHROMA_422, pkg.ALPHA_STRAIGHT), (pkg.CHROMA_444, pkg.ALPHA_NONE)):
            for bits in (10, 12):
                out.append((f"f32-limited-tc{tc}-c{chroma}-a{a}-b{bits}",
                            dict(width=67, height=21, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=bits, depth=32, alpha_state=a,
                                 matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709, full_range_flag=0,
                                 transfer_characteristics=tc, pq_peak_nits=1000)))
    for m, pr in ((pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), (pkg.MATRIX_BT709, pkg.PRIMARIES_BT709)):   # the other kg
        out.append((f"f32-m{m}-420-premul", dict(width=67, height=21, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, bit_depth=12,
                                                 depth=32, alpha_state=pkg.ALPHA_PREMULTIPLIED, matrix_coefficients=m, color_primaries=pr,
                                                 transfer_characteristics=pkg.TC_PQ, pq_peak_nits=80)))
    return out


OVER_RANGE = [cid for cid, kw in _read_truth_cases() if kw["colorspace"] != pkg.COLORSPACE_RGB][::3]


def make_source(d, cid, seed=harness.SEED):
    """harness.make_read_source, plus (for a third of the YCbCr / mono cases) 3 % of every plane at maxc + 1 ... maxc + 7."""
    planes = harness.make_read_source(d, seed=seed)
    if cid in OVER_RANGE:
        rng = np.random.default_rng(seed + 7)
        maxc = (1 << d.bit_depth) - 1
        for pl, arr in planes.items():
            w = harness.read_planes(d)[pl][0]
            m = rng.random(arr[:, :w].shape) < 0.03
            arr[:, :w][m] = maxc + rng.integers(1, 8, size=int(m.sum()))
    return planes


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


def truth_and_bound(d, planes, eps):
    """(T, bound, alpha) -- T and bound (H, W, ncol) float64; alpha (H, W) float32 or None."""
    L = oracle_binding.load()
    maxc = (1 << d.bit_depth) - 1
    count = 1 << d.bit_depth
    mono = d.colorspace == pkg.COLORSPACE_MONOCHROME
    rgb = d.colorspace == pkg.COLORSPACE_RGB
    has_alpha = d.alpha_state != pkg.ALPHA_NONE
    premul = d.alpha_state == pkg.ALPHA_PREMULTIPLIED
    ua = _full(d, planes, 3) if has_alpha else np.full((d.height, d.width), maxc)
    unprem_u16 = np.vectorize(lambda c, a: L.oracle_unpremultiply_u16(int(c), max(int(a), 1), maxc))   # (a == 0 is selected away)

    if rgb or mono:                          # integer-domain unpremultiply (exact), then a table value: dV = 0
        q = np.stack([_full(d, planes, k) for k in ((0,) if mono else (0, 1, 2))], -1)
        if premul:
            sel = ua < maxc
            uq = np.where(ua[..., None] == 0, 0, unprem_u16(q, ua[..., None]))
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
        ty, tuv, ta = (np.zeros(count, np.float32) for _ in range(3))
        L.oracle_build_yuv_tables(1, d.matrix_coefficients, d.full_range_flag, d.bit_depth, 0, ty.ctypes.data, tuv.ctypes.data, ta.ctypes.data)
        k = (ctypes.c_float * 3)()
        L.oracle_get_yuv_coefficients(1, d.matrix_coefficients, d.color_primaries, ctypes.byref(k))
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
        alpha = ta[ua] if has_alpha else None
        V32 = _ycc_float32(d, ty, tuv, ta, k, planes, ua)
        if premul:
            A = ta[ua].astype(np.float64)[..., None]
            sel = (ua < maxc)[..., None]
            with np.errstate(divide="ignore", invalid="ignore"):
                Vu = np.minimum(V / A, 1.0)
                dVu = dV / A + U * Vu
            V = np.where(sel, np.where(A == 0, 0.0, Vu), V)
            dV = np.where(sel, np.where(A == 0, 0.0, dVu), dV)

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
    eps_t = eps
    if _transfer(d.transfer_characteristics) == pkg.TRANSFER_HLG and d.hlg_apply_ootf and not mono:
        eps_t = eps * (1 + abs(float(np.float32(d.hlg_display_gamma)) - 1)) + OOTF_EPS
    bound = eps_t * np.abs(T) + exc + 1e-12
    T32 = _chain(d, V32)
    return T, bound, alpha, T32, eps_t * np.abs(T32) + 1e-12


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


def _check(cid, d, got, eps, planes):
    T, bound, alpha, T32, bound32 = truth_and_bound(d, planes, eps)
    col, a = _split(d, got)
    assert np.all(np.isfinite(col)), cid
    for t, b in ((T, bound), (T32, bound32)):
        err = np.abs(col - t)
        worst = np.unravel_index(np.argmax(err / b), err.shape)
        assert np.all(err <= b), (cid, int(np.sum(err > b)), worst, float(col[worst]), float(t[worst]), float(b[worst]))
    if alpha is not None:
        assert np.array_equal(a.view(np.uint32), alpha.view(np.uint32)), cid
    return float(np.max(np.abs(col - T) / bound)), float(np.max(np.abs(col - T32) / bound32))


@pytest.mark.parametrize("cid,kw", _read_truth_cases())
def test_oracle_open_within_float64_bound(cid, kw):
    """CPU: the oracle itself meets the bound with its own EOTF error (PQ: 5.9e-5 measured, bar 7e-5)."""
    d = pkg.ReadDesc(**kw)
    planes = make_source(d, cid)
    eps = truth64.ORACLE_EOTF_EPS[_transfer(d.transfer_characteristics)]
    _check(cid, d, harness.oracle_read(d, planes), eps, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,kw", _read_truth_cases())
def test_kernel_open_within_float64_bound(gpu, cid, kw):
    d = pkg.ReadDesc(**kw)
    planes = make_source(d, cid)
    eps = truth64.KERNEL_EOTF_EPS[_transfer(d.transfer_characteristics)]
    got = harness.gpu_read(gpu, d, planes, mem="device")
    assert "read" in gpu.last_kernel()
    r = _check(cid, d, got, eps, planes)
    print(f"{cid}: worst error / bound {r[0]:.3f} (float64 chain), {r[1]:.3f} (float32 step, float64 curve)")
