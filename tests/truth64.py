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
