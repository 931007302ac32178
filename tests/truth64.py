"""Float64 truth for the float-tier (T2) saves and opens: the reference's formulas (ColorTransfer.cpp:69-220, the reference's
float32 constants kept as they are) evaluated in float64, and what follows from them.

Writes.  Away from code boundaries a float save is exact.  A colour sample's code is DETERMINED when its float64 value t (in
codes), widened by the documented evaluation noise of the curve (the band below), does not straddle an integer: both the oracle's
float32 evaluation and the kernel's land inside the band, so both truncate to the same code.  Stage B (matrix, chroma box or
nearest pick, clip_round) takes integer codes in and is float32 arithmetic the integer tiers already hold bit-exact, so every
output sample whose whole footprint is determined must equal the oracle bit for bit.

Bands (codes):
 * PQ: 2e-5 * t + 1e-3 -- the band tests/test_gpu_t2_truth.py proves for every pq_evaluation (the reference formula's own
   float32 noise: q^78.84 multiplies 2-3 roundings of 6e-8 by 78.84, measured up to 1.3e-5 relative).
 * HLG and SMPTE 428: 2e-6 * t + 1e-3.  Measured on the CPU (dense sweep of 420 k floats in [0, 130]): the oracle's deviation
   from float64 is at most 1.2e-7 relative (HLG) and 1.0e-7 (428), i.e. at most 5e-4 codes at 12 bit.  The band is the
   kernels' stated EOTF bar for the same curves (tests/test_gpu_t2_truth.py: 2e-6 relative), 17x the oracle's own deviation,
   so a v_log/v_exp evaluation of a few ulps fits and a wrong constant does not.

Behind a document profile.  A 32-bit save behind an ICC stage (avifgpu_icc_transform, avifgpu_icc_sampled32) runs the curve on
the stage's float32 output, which two evaluations produce: lcms2's float pipeline (the reference converts the row in place, then
runs the pixel loop) and the kernels'.  The truth of the stage is computable from the prepared struct alone: t_j = curve_j(x_j) in
float64 (a parametric channel as DefaultEvalParametricFn has it; a sampled channel as curve[j][word], word the exact integer
_cmsQuickSaturateWord(x * 65535.0), magic-number floor included), v_i = sum_j m_ij t_j, and w_i = inverse type-4 curve(v_i) for the
sRGB target.  A sample is determined when every float32 within +-dv of that value gives one code: the ends go through the
premultiply (clamp and a float32 product: monotone) and the curve, each end is widened by the curve's band above (Clip has no
curve: the absolute part alone), and both must truncate to the same code or sit beyond the same clamped end.  dv is the larger of
two half-widths, in units of u = 2^-24 (S_i = sum_j |m_ij| |t_j|, slope_i = the inverse curve's derivative at v_i):
 * lcms2: 4 u S_i (Rec.2020 target), 4 u (slope_i S_i + |w_i|) (sRGB target).  Measured on 400 000 pixels per profile and target
   (tests/test_truth64_icc.py): at most 1.96 and 1.29 of those units -- the float between its stages and the float it returns -- so
   the 4 is a margin of 2x.
 * the kernels, from their arithmetic as it stands in csrc/write_kernels.hip:
     - the 3x3 in float32 (AG_ICC_MATRIX_F32; icc_apply_f, icc_apply_sampled, the streaming kernels): each coefficient is rounded
       once on the host, the first product and the two FMAs round once each, every one of them bounded by u S_i: 4 u S_i.  (The
       generic icc = 1 kernel accumulates in double and rounds once: inside this.)
     - a linear channel (gamma 1) is skipped and a sampled channel is the tabulated float itself (LDS and memory forms return
       curve[][] bit for bit, tests/test_gpu_icc.py): no error of their own.
     - a parametric channel, icc_trc_f / icc_trc_simple with AG_ICC_FASTPOW: lin = fma(a, R, b) on the rounded a and b -- u |a R|,
       u |b| (each only where the float copy is inexact) and u |lin| for the operation, which x^g multiplies by g -- then
       exp2(g * log2(lin)): with e = g log2(lin), the error of v_log_f32, the rounded g and the rounded product act on e, the error
       of v_exp_f32 on the result: relative ((L + [g inexact] + 1) |e| ln 2 + E) u.  A function of the sample, not a constant: for
       |e| = 30 it is 7e-6.  The "+ add" of types 3 and 5 adds u |add| and u |t|; the linear segment c R + f adds u for each
       inexact coefficient and one for the FMA.  These reach v_i through the matrix as sum_j |m_ij| err_j.
     - icc_inv4_f, the sRGB target: slope_i times all of the above, then the same pow bound on v^(1/g), u |b| and u |pow - b| for
       the subtraction, divided by a, and 2 u |w| for the rounded 1/a and its product; below the break 2 u |w|.
   L and E: neither this repository nor the hardware guides state the accuracy of v_log_f32 / v_exp_f32.  The source comments of
   write_kernels.hip assume 1 ulp each, i.e. 2 u relative; taken here with a margin of 2x, L = E = 4.  This is an ASSUMPTION, held by
   the measurement of tests/test_gpu_icc_determined.py::test_icc_write_mismatches_use_at_most_the_band (the share of the band the
   kernels use on undrawn sources, profiles/icc_truth/band_usage.txt), not a measured bound.
 The kernels compare R with the float copy of a curve's break point and the truth with the double: they differ for the one float
 between the two at most, where both segments agree to 1e-8 (far inside BAND_ABS).
"""
from __future__ import annotations

import numpy as np

import harness

pkg = harness.pkg

f32 = np.float32
U32 = 2.0 ** -24                                   # unit roundoff of float32

# ColorTransfer.cpp:73-77, :150-152 (the reference's float32 constants, exponents rounded to float as it rounds them)
M1, M2 = f32(2610.0) / f32(16384.0), f32(2523.0) / f32(4096.0) * f32(128.0)
C1, C2, C3 = f32(3424.0) / f32(4096.0), f32(2413.0) / f32(4096.0) * f32(32.0), f32(2392.0) / f32(4096.0) * f32(32.0)
HA, HB, HC = f32(0.17883277), f32(0.28466892), f32(0.55991073)

PQ_BAND_REL = 2e-5
HLG_BAND_REL = 2e-6
SMPTE428_BAND_REL = 2e-6
BAND_ABS = 1e-3

# read direction: relative EOTF error bars (kernel: tests/test_gpu_t2_truth.py; oracle: measured on a dense sweep of [0, 1],
# PQ 5.9e-5 -- the float32 evaluation of c2 - c3*x cancels -- HLG 2.3e-7, SMPTE 428 1.1e-7)
KERNEL_EOTF_EPS = {pkg.TRANSFER_PQ: 1e-5, pkg.TRANSFER_HLG: 2e-6, pkg.TRANSFER_SMPTE428: 2e-6}
ORACLE_EOTF_EPS = {pkg.TRANSFER_PQ: 7e-5, pkg.TRANSFER_HLG: 2e-6, pkg.TRANSFER_SMPTE428: 2e-6}


class _Ops:
    """The handful of elementwise operations the curves need, for numpy arrays and torch tensors alike."""
    def __init__(self, x):
        self.t = not isinstance(x, np.ndarray)
        if self.t:
            import torch
            self.m = torch

    def where(self, c, a, b):
        return self.m.where(c, a, b) if self.t else np.where(c, a, b)

    def pow(self, x, e):
        return self.m.pow(x, e) if self.t else np.power(x, e)

    def relu(self, x):
        return x.clamp_min(0.0) if self.t else np.maximum(x, 0.0)

    def f64(self, x):
        return x.to(self.m.float64) if self.t else np.asarray(x).astype(np.float64)

    def log(self, x):
        return self.m.log(x) if self.t else np.log(x)

    def exp(self, x):
        return self.m.exp(x) if self.t else np.exp(x)

    def sqrt(self, x):
        return self.m.sqrt(x) if self.t else np.sqrt(x)

    def abs(self, x):
        return x.abs() if self.t else np.abs(x)

    def log2(self, x):
        return self.m.log2(x) if self.t else np.log2(x)

    def floor(self, x):
        return x.floor() if self.t else np.floor(x)

    def clip(self, x, lo, hi):
        return x.clamp(lo, hi) if self.t else np.clip(x, lo, hi)

    def max2(self, a, b):
        return self.m.maximum(a, b) if self.t else np.maximum(a, b)

    def f32(self, x):
        return x.to(self.m.float32) if self.t else np.asarray(x).astype(np.float32)

    def stack(self, xs):
        return self.m.stack(xs, -1) if self.t else np.stack(xs, -1)

    def lookup(self, table, idx):
        """table[idx] for a numpy table and an integer-valued float index array of either kind."""
        if self.t:
            return self.m.from_numpy(np.ascontiguousarray(table)).to(idx.device)[idx.to(self.m.int64)]
        return table[idx.astype(np.int64)]


# ---- OETFs (write direction) -------------------------------------------------------------------------------------------------
def linear_to_pq64(x, peak):                      # ColorTransfer.cpp:69-92
    o = _Ops(x)
    x = o.f64(x)
    mult = float(f32(peak) / f32(10000.0))
    X = o.pow(o.relu(x) * mult, float(M1))
    return o.where(x < 0, 0.0 * x, o.pow((float(C1) + float(C2) * X) / (1.0 + float(C3) * X), float(M2)))


def linear_to_hlg64(x):                           # :141-164
    o = _Ops(x)
    x = o.f64(x)
    hi = float(HA) * o.log(o.relu(x * 12.0 - float(HB)) + 1e-300) + float(HC)
    lo = o.sqrt(o.relu(x) * 3.0)
    return o.where(x < 0, 0.0 * x, o.where(x > float(f32(1.0) / f32(12.0)), hi, lo))


def linear_to_smpte428_64(x):                     # :119-127
    o = _Ops(x)
    x = o.f64(x)
    return o.where(x < 0, 0.0 * x, o.pow(o.relu(x) * 48.0 / float(f32(52.37)), float(f32(1.0) / f32(2.6))))


# ---- EOTFs and the HLG OOTF (read direction) -----------------------------------------------------------------------------------
def pq_to_linear64(v, peak):                      # :94-117
    v = np.asarray(v, dtype=np.float64)
    e2, e1 = float(f32(1.0) / M2), float(f32(1.0) / M1)
    mult = float(f32(10000.0) / f32(peak))
    x = np.power(np.maximum(v, 0.0), e2)
    t = np.maximum(x - float(C1), 0.0) / (float(C2) - float(C3) * x)
    return np.where(v < 0, 0.0, np.power(t, e1) * mult)


def hlg_to_linear64(v):                           # :166-190
    v = np.asarray(v, dtype=np.float64)
    hi = (np.exp((v - float(HC)) / float(HA)) + float(HB)) / 12.0
    lo = v * v * float(f32(1.0) / f32(3.0))
    return np.where(v < 0, 0.0, np.where(v > 0.5, hi, lo))


def smpte428_to_linear64(v):                      # :129-139
    v = np.asarray(v, dtype=np.float64)
    return np.where(v < 0, 0.0, np.power(np.maximum(v, 0.0), float(f32(2.6))) * float(f32(52.37) / f32(48.0)))


def hlg_ootf64(rgb, luma, gamma, peak):           # :192-205; rgb (..., 3) float64, luma the float32 weights
    l = rgb[..., 0] * float(luma[0]) + rgb[..., 1] * float(luma[1]) + rgb[..., 2] * float(luma[2])
    with np.errstate(divide="ignore"):
        factor = float(peak) * np.power(l, float(f32(gamma)) - 1.0)
    return rgb * factor[..., None]


# ---- write stage A -------------------------------------------------------------------------------------------------------------
def oetf64(desc, v):
    """The curve of a save, in float64 (float input: numpy array or torch tensor)."""
    if desc.transfer == pkg.TRANSFER_PQ:
        return linear_to_pq64(v, desc.peak_nits)
    if desc.transfer == pkg.TRANSFER_HLG:
        return linear_to_hlg64(v)
    if desc.transfer == pkg.TRANSFER_SMPTE428:
        return linear_to_smpte428_64(v)
    raise ValueError("float-tier truth covers the PQ, HLG and SMPTE 428 curves")


def band_rel(desc):
    return {pkg.TRANSFER_PQ: PQ_BAND_REL, pkg.TRANSFER_HLG: HLG_BAND_REL, pkg.TRANSFER_SMPTE428: SMPTE428_BAND_REL}[desc.transfer]


def _ncol(desc):
    return 3 if desc.planes >= 3 else 1


def _has_alpha(desc):
    return desc.planes in (2, 4)


def stage_a_values(desc, src):
    """(H, W, ncol) float32: the values the curve sees, with the oracle's float32 pre-curve operations (avif_oracle.c:346-361,
    WriteHeifImage.cpp:558-602, :1047-1066): premultiply clamp(c) * a when a < 1 (a = clamp(alpha, 0, 1); a == 0 -> 0), the
    gray-without-alpha clamp, nothing else.  src: (H, W*planes) float32, numpy array or torch tensor."""
    o = _Ops(src)
    H = src.shape[0]
    px = src.reshape(H, desc.width, desc.planes)
    col = px[..., :_ncol(desc)]
    if _has_alpha(desc):
        a = px[..., -1:].clamp(0.0, 1.0) if o.t else np.clip(px[..., -1:], f32(0.0), f32(1.0))
        if desc.alpha_state == pkg.ALPHA_PREMULTIPLIED:
            cc = col.clamp(0.0, 1.0) if o.t else np.clip(col, f32(0.0), f32(1.0))
            pre = cc * a                                           # float32 product; / 1.0f is exact
            pre = o.where(a == 0, 0.0 * pre, pre)
            col = o.where(a < 1.0, pre, col)
    elif _ncol(desc) == 1:
        col = col.clamp(0.0, 1.0) if o.t else np.clip(col, f32(0.0), f32(1.0))
    return col


def alpha_codes(desc, src):
    """(H, W) alpha codes: clamp(alpha) * max truncated, float32 arithmetic without a curve (:1093-1095)."""
    maxf = f32((1 << desc.bit_depth) - 1)
    a = np.clip(src.reshape(src.shape[0], desc.width, desc.planes)[..., -1], f32(0.0), f32(1.0))
    return np.clip(a * maxf, f32(0.0), maxf).astype(np.int64)


def codes_from_values(desc, v):
    """(codes, mask) of float32 pre-curve values (numpy or torch): the truncated float64 code, and whether it is determined."""
    o = _Ops(v)
    maxv = float((1 << desc.bit_depth) - 1)
    t = oetf64(desc, v) * maxv
    w = band_rel(desc) * o.relu(t) + BAND_ABS

    def q(x):
        x = x.clamp(0.0, maxv) if o.t else np.clip(x, 0.0, maxv)
        return x.floor() if o.t else np.floor(x)
    lo, hi = q(t - w), q(t + w)
    top = t >= maxv                                                # clamped end: at or above maxv gives maxv
    mask = (lo == hi) | top
    codes = o.where(top, 0.0 * t + maxv, lo)
    return codes, mask


def determined_codes(desc, src):
    """(codes, mask), both (H, W, ncol): the float64 code of every colour sample and whether it is determined."""
    codes, mask = codes_from_values(desc, stage_a_values(desc, src))
    return codes.astype(np.int64), mask


# ---- sources -------------------------------------------------------------------------------------------------------------------
def _draw_colour(rng, n):
    """Colour samples with harness.make_write_source's distribution: ~90 % in [0, 1), ~10 % highlights (1, 12.5], ~0.1 % small
    negatives."""
    a = rng.random(n, dtype=np.float32)
    m = rng.random(n)
    hi = (1.0 + 11.5 * rng.random(n)).astype(np.float32)
    a = np.where(m < 0.10, hi, a)
    neg = (-0.01 * rng.random(n)).astype(np.float32)
    return np.where(m > 0.999, neg, a).astype(np.float32)


def make_determined_source(desc, seed=harness.SEED, max_rounds=200):
    """harness.make_write_source (highlights, small negatives, alpha at 0, at 1 and outside [0, 1], the special values), with
    every colour sample whose code is not determined drawn again until all are.  Returns (src, replaced)."""
    src = harness.make_write_source(desc, seed=seed)
    rng = np.random.default_rng(seed + 0x5EED)
    px = src.reshape(desc.height, desc.width, desc.planes)
    replaced = 0
    for _ in range(max_rounds):
        _, mask = determined_codes(desc, src)
        bad = np.nonzero(~mask)
        if bad[0].size == 0:
            return src, replaced
        replaced += bad[0].size
        px[bad] = _draw_colour(rng, bad[0].size)
    raise AssertionError(f"{desc.width}x{desc.height}: colour samples still undetermined after {max_rounds} rounds")


# ---- which output samples are determined --------------------------------------------------------------------------------------
def output_masks(desc, pix, xp=np):
    """{plane: bool mask} of the output samples whose whole footprint is determined.  pix: (H, W) bool (or torch bool tensor) --
    every colour sample of the pixel determined.  Alpha samples carry no curve and are always determined."""
    H, W = pix.shape
    ones = (lambda shape: xp.ones(shape, dtype=bool)) if xp is np else (lambda shape: xp.ones(shape, dtype=xp.bool, device=pix.device))
    if desc.output == pkg.OUT_REFERENCE:
        if desc.planes >= 3:
            m = pix[:, :, None].repeat(1, 1, desc.planes) if xp is not np else np.repeat(pix[:, :, None], desc.planes, axis=2)
            m[..., 3:] = True                                      # interleaved alpha
            return {0: m.reshape(H, W * desc.planes)}
        out = {0: pix}
        if _has_alpha(desc):
            out[3] = ones((H, W))
        return out
    xs, ys = harness.chroma_shift(desc.chroma)
    out = {0: pix}
    if _has_alpha(desc):
        out[3] = ones((H, W))
    if desc.matrix_coefficients == pkg.MATRIX_RGB_GBR or (xs == 0 and ys == 0):
        c = pix
    elif desc.chroma_downsampling == pkg.DOWNSAMPLE_NEAREST:
        c = pix[::1 << ys, ::1 << xs]
    else:                                                          # edge-replicated box: the image edge decides replication
        cat = np.concatenate if xp is np else xp.cat
        if xs and W % 2:
            pix = cat([pix, pix[:, -1:]], 1)
        if ys and H % 2:
            pix = cat([pix, pix[-1:, :]], 0)
        c = pix[::1 << ys, 0::2] & pix[::1 << ys, 1::2]
        if ys:
            c = c & pix[1::2, 0::2] & pix[1::2, 1::2]
    out[1] = c
    out[2] = c
    return out


# ---- the ICC stage of a 32-bit save behind a document profile (docstring: "Behind a document profile") -----------------------------
ICC_LCMS_UNITS = 4.0          # lcms2's float pipeline: measured <= 1.93 (Rec.2020 target) and <= 1.33 (sRGB target) units, doubled
ICC_MATRIX_UNITS = 4.0        # the kernels' fp32 3x3: one rounded coefficient and three rounded operations per row, on sum |m||t|
ICC_LOG_UNITS = 4.0           # v_log_f32: 1 ulp = 2 units of 2^-24 relative (ASSUMED, see the docstring), doubled
ICC_EXP_UNITS = 4.0           # v_exp_f32: likewise
ICC_TOL = 0.0001              # lcms2's MATRIX_DET_TOLERANCE, as DefaultEvalParametricFn uses it
_QUICK_FLOOR_MAGIC = 68719476736.0 * 1.5


def _icc_base(xf):
    return xf.base if hasattr(xf, "parametric_mask") else xf


def _inexact(x):
    """1.0 where the kernels' float copy of a double parameter is a rounded one, else 0.0."""
    return 0.0 if float(f32(x)) == float(x) else 1.0


def icc_channel_is_sampled(xf, c):
    return hasattr(xf, "parametric_mask") and not (xf.parametric_mask >> c) & 1


def icc_has_nonlinear_parametric(xf):
    b = _icc_base(xf)
    return any(not icc_channel_is_sampled(xf, c) and not (b.trc_type[c] == 1 and b.trc_params[c][0] == 1.0) for c in range(3))


def quick_saturate_word64(v):
    """lcms2's _cmsQuickSaturateWord(v * 65535.0) of float32 samples (cmsgamma.c: the word a sampled curve is entered with), as an
    integer-valued float64 array: the product and the + 0.5 in double, the magic-number floor of _cmsQuickFloor -- the addition of
    1.5 * 2^36 rounds the value to 2^-16, the library then shifts the low word right by 16, i.e. takes the floor -- and the two
    saturation tests."""
    o = _Ops(v)
    d = o.f64(v) * 65535.0 + 0.5
    x = o.clip(d, 0.0, 65535.0) - 32767.0
    w = o.floor((x + _QUICK_FLOOR_MAGIC) - _QUICK_FLOOR_MAGIC) + 32767.0
    return o.where(d <= 0.0, 0.0 * d, o.where(d >= 65535.0, 0.0 * d + 65535.0, w))


def _pow_units(o, ex, inexact_g):
    """Relative error, in units of 2^-24, of exp2(g * log2(x)) as icc_pow32 evaluates it (AG_ICC_FASTPOW), ex = g log2 x: the
    error of v_log_f32, the rounded exponent g and the rounded product all act on ex, v_exp_f32 on the result."""
    return (ICC_LOG_UNITS + inexact_g + 1.0) * o.abs(ex) * float(np.log(2.0)) + ICC_EXP_UNITS


def _trc64(o, typ, P, R):
    """(t, err): one lcms2 parametric curve (types 1-5, DefaultEvalParametricFn as eval_parametric in csrc/icc_profile.cpp restates
    it) of the float64 samples R, and the bound of icc_trc_f's / icc_trc_simple's absolute error on it in units of 2^-24."""
    g, a, b, c, d, e, f = (float(P[k]) for k in range(7))
    zero = 0.0 * R
    if typ == 1:
        if g == 1.0:                                               # the kernels skip the curve (icc_trc_linear): t = R, exactly
            return R + zero, zero
        up, a, b, add, nonpos = R >= 0, 1.0, 0.0, 0.0, 0.0
        lc, lf = (1.0 if abs(g - 1.0) < ICC_TOL else 0.0), 0.0
    elif typ in (2, 3):
        if abs(a) < ICC_TOL:
            return zero, zero
        disc = -b / a
        add, nonpos = (c, 0.0) if typ == 3 else (0.0, 0.0)
        up = R >= (max(disc, 0.0) if typ == 3 else disc)
        lc, lf = 0.0, add
    elif typ == 4:
        up, add, nonpos, lc, lf = R >= d, 0.0, 0.0, c, 0.0
    elif typ == 5:
        up, add, nonpos, lc, lf = R >= d, e, e, c, f
    else:
        raise ValueError(f"parametric curve type {typ}")
    lin = a * R + b
    pos = lin > 0
    safe = o.where(pos, lin, zero + 1.0)
    pw = o.where(pos, o.pow(safe, g), zero)
    hi = o.where(pos, pw + add, zero + nonpos)
    low = lc * R + lf
    # lin = fma(a, R, b) on the rounded a and b: one unit each where they are rounded, one for the operation; x^g multiplies it by g
    lin_units = (_inexact(a) * o.abs(a * R) + _inexact(b) * abs(b)) / o.abs(safe) + (0.0 if (a == 1.0 and b == 0.0) else 1.0)
    hi_err = pw * (abs(g) * lin_units + _pow_units(o, g * o.log2(safe), _inexact(g)))
    if add != 0.0:
        hi_err = hi_err + _inexact(add) * abs(add) + o.abs(hi)
    low_err = _inexact(lc) * o.abs(lc * R) + _inexact(lf) * abs(lf)
    if not (lc in (0.0, 1.0) and lf == 0.0):
        low_err = low_err + o.abs(low)
    return o.where(up, hi, low), o.where(up, o.where(pos, hi_err, zero), low_err + zero)


def _inv4_64(o, P, v):
    """(w, slope, err): the inverse of lcms2's parametric type 4 (type -4, the curve in front of an sRGB destination), its
    derivative, and the bound of icc_inv4_f's absolute error in units of 2^-24.  P = out_params."""
    g, a, b, c, brk, ig = float(P[0]), float(P[1]), float(P[2]), float(P[3]), float(P[5]), float(P[6])
    zero = 0.0 * v
    up = v >= brk
    safe = o.where(up, v, zero + 1.0)
    if abs(g) < ICC_TOL or abs(a) < ICC_TOL:
        hi, hs, he = zero, zero, zero
    else:
        pw = o.pow(safe, 1.0 / g)
        hi = (pw - b) / a
        hs = pw / (g * a * safe)
        # pow, the subtraction of the rounded b, the product with the rounded 1/a
        he = (pw * _pow_units(o, ig * o.log2(safe), _inexact(ig)) + _inexact(b) * abs(b) + o.abs(pw - b)) / abs(a) + 2.0 * o.abs(hi)
    if abs(c) < ICC_TOL:
        lo, ls, le = zero, zero, zero
    else:
        lo, ls = v / c, zero + 1.0 / c
        le = 2.0 * o.abs(lo)                                       # the rounded 1/c and the product
    return o.where(up, hi, lo), o.where(up, hs, ls), o.where(up, he, le)


def _icc_eval(xf, col):
    """Everything of the stage at once.  col: (..., 3) float32 samples (numpy or torch).  Returns a dict of (..., 3) float64 arrays:
    value (the stage's output), mag (sum_j |m_ij| |t_j|), slope (of the inverse curve; ones for the Rec.2020 target), lcms and kernel
    (the two evaluations' error bounds, in units of 2^-24)."""
    o = _Ops(col)
    base = _icc_base(xf)
    R = o.f64(col)
    ts, es = [], []
    for ch in range(3):
        if icc_channel_is_sampled(xf, ch):
            word = quick_saturate_word64(col[..., ch])
            ts.append(o.f64(o.lookup(np.ctypeslib.as_array(xf.curve)[ch], word)))      # the tabulated float, exactly: no error of its own
            es.append(0.0 * R[..., ch])
        else:
            t, e = _trc64(o, int(base.trc_type[ch]), base.trc_params[ch], R[..., ch])
            ts.append(t)
            es.append(e)
    m = [float(x) for x in base.matrix]
    v, mag, prop = [], [], []
    for i in range(3):
        v.append(sum(m[3 * i + j] * ts[j] for j in range(3)))
        mag.append(sum(abs(m[3 * i + j]) * o.abs(ts[j]) for j in range(3)))
        prop.append(sum(abs(m[3 * i + j]) * es[j] for j in range(3)))
    v, mag, prop = o.stack(v), o.stack(mag), o.stack(prop)
    kernel = ICC_MATRIX_UNITS * mag + prop
    if base.out_curve == 4:
        w, slope, inv_err = _inv4_64(o, base.out_params, v)
        return dict(value=w, mag=mag, slope=slope, lcms=ICC_LCMS_UNITS * (slope * mag + o.abs(w)), kernel=slope * kernel + inv_err)
    return dict(value=v, mag=mag, slope=0.0 * v + 1.0, lcms=ICC_LCMS_UNITS * mag, kernel=kernel)


def icc_stage64(xf, col):
    """(value, mag, slope): float64 truth of the ICC stage -- avifgpu_icc_transform (parametric types 1-5, both targets) and
    avifgpu_icc_sampled32 (sampled channels through the exact 16-bit word and curve[c][word]; mixed profiles by parametric_mask) --
    of (..., 3) float32 samples; mag = sum_j |m_ij| |t_j|; slope = the inverse curve's derivative at the matrix output (sRGB target),
    None for the Rec.2020 target."""
    r = _icc_eval(xf, col)
    return r["value"], r["mag"], (r["slope"] if _icc_base(xf).out_curve == 4 else None)


def icc_lcms_unit(xf, col):
    """The unit lcms2's deviation is measured in: 2^-24 * sum |m||t| (Rec.2020 target), 2^-24 * (slope * sum |m||t| + |w|) (sRGB)."""
    r = _icc_eval(xf, col)
    return U32 * r["lcms"] / ICC_LCMS_UNITS


def icc_band(xf, col):
    """Per-sample half-width dv of the stage's output: both judged evaluations -- lcms2's float pipeline and the kernels' -- lie
    within value +- dv (docstring)."""
    r = _icc_eval(xf, col)
    return U32 * _Ops(col).max2(r["lcms"], r["kernel"])


def icc_truth_rows(desc, xf, src):
    """src with every pixel's R, G, B replaced by float32(truth): what lcms2's in-place row conversion leaves, alpha untouched."""
    px = src.reshape(src.shape[0], desc.width, desc.planes).copy()
    px[..., :3] = icc_stage64(xf, px[..., :3])[0].astype(np.float32)
    return np.ascontiguousarray(px.reshape(src.shape))


def _curve_codes64(desc, x):
    """(t, w): float64 code of float32 pre-curve values and the curve band's half-width there.  Clip has no curve: BAND_ABS alone."""
    o = _Ops(x)
    maxv = float((1 << desc.bit_depth) - 1)
    if desc.transfer == pkg.TRANSFER_CLIP:
        t = o.f64(x) * maxv
        return t, 0.0 * t + BAND_ABS
    t = oetf64(desc, x) * maxv
    return t, band_rel(desc) * o.relu(t) + BAND_ABS


def icc_code_interval(desc, xf, px, parts=False):
    """(t, lo, hi), each (..., 3) float64 codes (unclamped): the truth and the ends of everything either evaluation may give.  px:
    (..., planes) float32 pixels, 3 or 4 planes.  The reference converts the row first and runs the pixel loop on the converted row,
    so the premultiply clamp(c) * a acts on the stage's float32 output: any float32 inside [v - dv, v + dv] lies between the two
    rounded ends, and clamp, the float32 product and the curves are monotone, so the interval goes through them end by end.
    parts: also the two ends before the curve's band widens them, i.e. what dv alone makes of the interval."""
    o = _Ops(px)
    col = px[..., :3]
    r = _icc_eval(xf, col)
    dv = U32 * o.max2(r["lcms"], r["kernel"])
    ends = [o.f32(r["value"]), o.f32(r["value"] - dv), o.f32(r["value"] + dv)]
    if desc.planes == 4 and desc.alpha_state == pkg.ALPHA_PREMULTIPLIED:
        a = o.clip(px[..., 3:], 0.0, 1.0)                          # float32, as stage_a_values
        for k, x in enumerate(ends):
            pre = o.clip(x, 0.0, 1.0) * a
            pre = o.where(a == 0, 0.0 * pre, pre)
            ends[k] = o.where(a < 1.0, pre, x)
    (t, _), (tl, wl), (th, wh) = (_curve_codes64(desc, x) for x in ends)
    return (t, tl - wl, th + wh, tl, th) if parts else (t, tl - wl, th + wh)


def determined_codes_icc(desc, xf, src):
    """(codes, mask), both (H, W, 3): the float64 code of every colour sample of a 32-bit save behind the ICC stage xf
    (avifgpu_icc_transform or avifgpu_icc_sampled32), and whether it is determined: both ends of the interval truncate to the same
    code, or both sit at or beyond the same clamped end.  Alpha is copied by the transform: alpha_codes() as before."""
    o = _Ops(src)
    maxv = float((1 << desc.bit_depth) - 1)
    t, lo, hi = icc_code_interval(desc, xf, src.reshape(src.shape[0], desc.width, desc.planes))
    ql, qh = o.floor(o.clip(lo, 0.0, maxv)), o.floor(o.clip(hi, 0.0, maxv))
    codes = o.floor(o.clip(t, 0.0, maxv))
    return (codes if o.t else codes.astype(np.int64)), ql == qh


def make_determined_source_icc(desc, xf, seed=harness.SEED, max_rounds=400):
    """harness.make_write_source -- with abs() where the profile has a non-linear parametric channel, as the ICC tests draw it: no
    lcms2 build is asked about negative inputs of a power law -- with every PIXEL that has an undetermined colour sample drawn again
    (the matrix mixes the channels) until none is left.  Returns (src, replaced), replaced counting pixels, with repeats."""
    nonneg = icc_has_nonlinear_parametric(xf)
    src = harness.make_write_source(desc, seed=seed)
    px = src.reshape(desc.height, desc.width, desc.planes)
    if nonneg:
        px[..., :3] = np.abs(px[..., :3])
    rng = np.random.default_rng(seed + 0x1CC)
    maxv = float((1 << desc.bit_depth) - 1)
    flat = px.reshape(-1, desc.planes)
    todo = np.arange(flat.shape[0])
    replaced = 0
    for _ in range(max_rounds):
        _, lo, hi = icc_code_interval(desc, xf, flat[todo])
        bad = ~(np.floor(np.clip(lo, 0.0, maxv)) == np.floor(np.clip(hi, 0.0, maxv))).all(axis=-1)
        todo = todo[bad]
        if todo.size == 0:
            return src, replaced
        replaced += todo.size
        c = _draw_colour(rng, todo.size * 3).reshape(-1, 3)
        flat[todo, :3] = np.abs(c) if nonneg else c
    raise AssertionError(f"{desc.width}x{desc.height}: pixels still undetermined after {max_rounds} rounds")
