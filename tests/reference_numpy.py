"""A third opinion on the integer colour paths: the reference's 8-bit open and the 8-bit 4:4:4 save restated in numpy float32,
operation by operation and in the reference's order.  Test-only; nothing here is used by the library or by the oracle.

Why a third opinion: oracle/avif_oracle.c is C compiled by whatever compiler builds it (a contracted multiply-add would change single
roundings) and is pinned to the reference by known-answer values only.  numpy's float32 operations are IEEE-754 single precision,
one rounding per operation, never contracted -- what the reference's MSVC /fp:precise build computes.

Every operation is elementwise, so a result is a function of its input CODES alone: the functions below evaluate each expression
once per distinct input (256 table entries, 256^2 pairs, 256^3 triples) and return tables indexed by code.  Lines cited:
  table entry        reference YuvLookupTables.cpp:52-66 (limited -> full), :157-190
  kr, kg, kb         reference YUVCoefficiants.cpp:58-70, :94-106, :110-151, :154-188
  R, G, B, the code  reference YuvDecode.cpp:312-326
  8 -> n bit rescale reference WriteHeifImage.cpp:87-112
  RGB -> YCbCr       libheif 1.14.0's RGB -> YCbCr operation as oracle/avif_oracle.c:425-456, :527-566 restates it
"""
from __future__ import annotations

import numpy as np

F = np.float32

# matrix_coefficients (ISO/IEC 23091-2) -> kr, kb: the rows of YUVCoefficiants.cpp:94-106
GBR, BT709, FCC, BT470BG, BT601, SMPTE240M, BT2020_NCL, CHROMA_DERIVED_NCL = 0, 1, 4, 5, 6, 7, 9, 12
_KR_KB = {BT709: (0.2126, 0.0722), FCC: (0.30, 0.11), BT470BG: (0.299, 0.114), BT601: (0.299, 0.114),
          SMPTE240M: (0.212, 0.087), BT2020_NCL: (0.2627, 0.0593)}
# colour_primaries -> rX, rY, gX, gY, bX, bY, wX, wY: the rows of YUVCoefficiants.cpp:58-70 that the tests use
_PRIMARIES = {1: (0.64, 0.33, 0.3, 0.6, 0.15, 0.06, 0.3127, 0.329),
              9: (0.708, 0.292, 0.170, 0.797, 0.131, 0.046, 0.3127, 0.3290),
              12: (0.680, 0.320, 0.265, 0.690, 0.150, 0.060, 0.3127, 0.3290)}


def coefficients(matrix, primaries=1):
    """(kr, kg, kb) as float32.  A matrix without a row -- GBR among them -- keeps BT.601's (YUVCoefficiants.cpp:171-183)."""
    one = F(1)
    if matrix == CHROMA_DERIVED_NCL:                                     # YUVCoefficiants.cpp:112-136
        rX, rY, gX, gY, bX, bY, wX, wY = (F(v) for v in _PRIMARIES.get(primaries, _PRIMARIES[1]))
        rZ, gZ, bZ, wZ = one - (rX + rY), one - (gX + gY), one - (bX + bY), one - (wX + wY)
        den = wY * (rX * (gY * bZ - bY * gZ) + gX * (bY * rZ - rY * bZ) + bX * (rY * gZ - gY * rZ))
        kr = (rY * (wX * (gY * bZ - bY * gZ) + wY * (bX * gZ - gX * bZ) + wZ * (gX * bY - bX * gY))) / den
        kb = (bY * (wX * (rY * gZ - gY * rZ) + wY * (gX * rZ - rX * gZ) + wZ * (rX * gY - gX * rY))) / den
    else:
        kr, kb = (F(v) for v in _KR_KB.get(matrix, _KR_KB[BT601]))
    kg = one - kr - kb
    assert all(type(v) is np.float32 for v in (kr, kg, kb))
    return kr, kg, kb


def _c_div(num, den):
    """C's integer division (truncation towards zero) on int64 arrays."""
    return np.sign(num) * (np.abs(num) // den)


def limited_to_full(v, lo, hi, full):                                   # YuvLookupTables.cpp:64-66
    v = _c_div((v - lo) * full + (hi - lo) // 2, hi - lo)
    return np.clip(v, 0, full)


def read8_tables(matrix, full_range):
    """(table Y, table UV): 256 float32 entries each (YuvLookupTables.cpp:157-190)."""
    i = np.arange(256, dtype=np.int64)
    uy, uuv = i, i
    if not full_range:
        uy = limited_to_full(i, 16, 235, 255)                           # :72-73
        uuv = limited_to_full(i, 16, 240, 255)                          # :93-94
    ty = uy.astype(F) / F(255)                                          # :173
    tuv = ty if matrix == GBR else uuv.astype(F) / F(255) - F(0.5)      # :177-184
    assert ty.dtype == np.float32 and tuv.dtype == np.float32
    return ty, tuv


def _code8(v):
    """std::clamp(v, 0, 1), then static_cast<uint8_t>(0.5f + (v * 255.0f))  (YuvDecode.cpp:316-322)."""
    v = np.minimum(np.maximum(v, F(0)), F(1))
    c = F(0.5) + (v * F(255))
    assert c.dtype == np.float32
    return c.astype(np.uint8)                                           # 0.5 <= c <= 255.5: the cast truncates


def read8_code_tables(matrix, full_range, primaries=1):
    """The 8-bit YCbCr -> RGB8 open of YuvDecode.cpp:312-322 for EVERY input: R[y, cr], G[y, cb, cr], B[y, cb] as u8 tables."""
    kr, kg, kb = coefficients(matrix, primaries)
    ty, tuv = read8_tables(matrix, full_range)
    one, two = F(1), F(2)
    r = ty[:, None] + (two * (one - kr)) * tuv[None, :]                 # :312  R = Y + (2 * (1 - kr)) * Cr
    b = ty[:, None] + (two * (one - kb)) * tuv[None, :]                 # :313  B = Y + (2 * (1 - kb)) * Cb
    term = (two * ((kr * (one - kr) * tuv[None, :]) + (kb * (one - kb) * tuv[:, None]))) / kg      # :314, indexed [cb, cr]
    g = ty[:, None, None] - term[None, :, :]                            # :314  G = Y - term
    assert r.dtype == np.float32 and g.dtype == np.float32 and term.dtype == np.float32
    return _code8(r), _code8(g), _code8(b)


def read8_rgb(planes, matrix, full_range, primaries=1):
    """(H, W * 3) u8 rows of a 4:4:4 open of `planes` ({0: Y, 1: Cb, 2: Cr}, same shape), from the tables above."""
    rt, gt, bt = read8_code_tables(matrix, full_range, primaries)
    y, cb, cr = planes[0], planes[1], planes[2]
    out = np.empty(y.shape + (3,), dtype=np.uint8)
    out[..., 0] = rt[y, cr]
    out[..., 1] = gt[y, cb, cr]
    out[..., 2] = bt[y, cb]
    return out.reshape(y.shape[0], -1)


def rescale8_lut(bits):
    """8-bit document code -> `bits`-bit code (WriteHeifImage.cpp:87-112); at 8 bit the reference stores the byte itself."""
    i = np.arange(256)
    if bits == 8:
        return i.astype(np.int64)
    dst_max = (1 << bits) - 1
    v = ((i.astype(F) / F(255)) * F(dst_max)) + F(0.5)
    assert v.dtype == np.float32
    return np.clip(v.astype(np.int64), 0, dst_max)


def _clip_round(v, maxi):
    """clip_round of oracle/avif_oracle.c:450-456: (long)(v + 0.5f), clamped."""
    x = v + F(0.5)
    assert x.dtype == np.float32
    return np.clip(x.astype(np.int64), 0, maxi)                         # the cast truncates towards zero, like C's


def stage_b_rows(kr, kb):
    """The three rows of the RGB -> YCbCr matrix as float32, each coefficient rounded as oracle/avif_oracle.c:442-446 rounds it."""
    kr, kb = F(kr), F(kb)
    kg = F(1) - kr - kb
    rows = {"y": (kr, kg, kb),
            "cb": (-kr / (F(1) - kb) / F(2), -kg / (F(1) - kb) / F(2), F(0.5)),
            "cr": (F(0.5), -kg / (F(1) - kr) / F(2), -kb / (F(1) - kr) / F(2))}
    assert all(type(c) is np.float32 for r in rows.values() for c in r)
    return rows


def write8_code_tables(matrix, bits, primaries=1):
    """The 8-bit RGB -> Y, Cb, Cr 4:4:4 save for EVERY (r, g, b): three (256, 256, 256) tables of `bits`-bit codes indexed [r, g, b]
    (full range, libheif's chroma zero point 2^(bits-1): oracle/avif_oracle.c:427-448, :530-565)."""
    maxi = (1 << bits) - 1
    q = rescale8_lut(bits)
    dt = np.uint8 if bits == 8 else np.uint16
    if matrix == GBR:                                                   # Y <- G, Cb <- B, Cr <- R
        shape = (256, 256, 256)
        return (np.broadcast_to(q[None, :, None], shape).astype(dt), np.broadcast_to(q[None, None, :], shape).astype(dt),
                np.broadcast_to(q[:, None, None], shape).astype(dt))
    kr, kg, kb = coefficients(matrix, primaries)
    half = F(1 << (bits - 1))
    rows = stage_b_rows(kr, kb)
    qf = q.astype(F)
    out = []
    for name in ("y", "cb", "cr"):
        c0, c1, c2 = rows[name]
        assert all(type(c) is np.float32 for c in (c0, c1, c2))
        s = ((qf * c0)[:, None] + (qf * c1)[None, :])[:, :, None] + (qf * c2)[None, None, :]      # (R c0 + G c1) + B c2
        if name != "y":
            s = s + half
        assert s.dtype == np.float32
        out.append(_clip_round(s, maxi).astype(dt))
    return tuple(out)


# ---- 10- / 12-bit planes: the open to 16-bit host rows and the save of code triples, elementwise -------------------------------------
# The tables above enumerate 8-bit inputs; 2^30 and 2^36 triples cannot be enumerated, so these two evaluate the same float32 lines on
# the pixels they are given.  `mutant` names ONE deliberate departure from the reference's operations (tests/test_tie_inputs.py counts
# what each changes); None is the reference.
_LIMITED = {8: ((16, 235), (16, 240)), 10: ((64, 940), (64, 960)), 12: ((256, 3760), (256, 3840))}      # YuvLookupTables.cpp:69-109


def read_tables(bits, full_range, identity=False):
    """(table Y, table UV, table A): 2^bits float32 entries each (YuvLookupTables.cpp:157-190)."""
    full = (1 << bits) - 1
    i = np.arange(full + 1, dtype=np.int64)
    uy, uuv = i, i
    if not full_range:
        (ylo, yhi), (clo, chi) = _LIMITED[bits]
        uy = limited_to_full(i, ylo, yhi, full)
        uuv = limited_to_full(i, clo, chi, full)
    ty = uy.astype(F) / F(full)
    tuv = ty if identity else uuv.astype(F) / F(full) - F(0.5)
    ta = i.astype(F) / F(full)
    assert ty.dtype == tuv.dtype == ta.dtype == np.float32
    return ty, tuv, ta


def fused(a, b, c):
    """a * b + c with ONE rounding, as a contracted multiply-add gives it: the product of two float32 is exact in float64 and the
    sum is rounded to float64 before it is rounded to float32 (a double rounding that differs from the fused result on about one
    input in 2^29: this is a mutant, not a model of anything)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def read16_rgb(planes, bits, matrix, full_range, primaries=1, alpha=None, shifts=(0, 0), mutant=None):
    """(H, W * channels) u16 rows of a YCbCr open to the 16-bit host (YuvDecode.cpp:312-326, :369-388, :515 as
    oracle/avif_oracle.c:751-782 restates them).  `planes`: {0: Y, 1: Cb, 2: Cr[, 3: A]}, chroma sub-sampled by `shifts` = (xs, ys)
    and taken nearest; alpha: None, 'straight' or 'premultiplied'.  mutant: 'reciprocal' (x * (1 / kg) for x / kg) or 'fma' (the
    chroma sum of G as one contracted multiply-add)."""
    assert mutant in (None, "reciprocal", "fma") and alpha in (None, "straight", "premultiplied")
    kr, kg, kb = coefficients(matrix, primaries)
    ty, tuv, ta = read_tables(bits, full_range, identity=(matrix == GBR))
    maxc = (1 << bits) - 1
    xs, ys = shifts
    up = lambda a: np.repeat(np.repeat(a, 1 << ys, axis=0), 1 << xs, axis=1) if (xs or ys) else a
    y, cb, cr = ty[np.minimum(planes[0], maxc)], tuv[np.minimum(up(planes[1]), maxc)], tuv[np.minimum(up(planes[2]), maxc)]
    one, two = F(1), F(2)
    r = y + (two * (one - kr)) * cr                                     # :312
    b = y + (two * (one - kb)) * cb                                     # :313
    t_r = (kr * (one - kr)) * cr
    s = fused(kb * (one - kb), cb, t_r) if mutant == "fma" else t_r + (kb * (one - kb)) * cb
    num = two * s
    g = y - (num * (one / kg) if mutant == "reciprocal" else num / kg)  # :314
    out = np.empty(y.shape + (3 if alpha is None else 4,), dtype=np.uint16)
    if alpha is not None:
        ua = np.minimum(planes[3], maxc)
        av = ta[ua]
    for k, v in enumerate((r, g, b)):
        v = np.minimum(np.maximum(v, F(0)), one)                        # std::clamp
        if alpha == "premultiplied":                                    # :369-388: min(v * 1 / A, 1) under a translucent alpha, 0 under alpha 0
            with np.errstate(divide="ignore", invalid="ignore"):
                u = np.minimum((v * one) / av, one)
            v = np.where(ua < maxc, np.where(ua == 0, F(0), u), v)
        c = F(0.5) + (v * F(32768))
        assert c.dtype == np.float32
        out[..., k] = c.astype(np.uint16)                               # 0.5 <= c <= 32768.5: the cast truncates
    if alpha is not None:
        out[..., 3] = (F(0.5) + (av * F(32768))).astype(np.uint16)      # :515
    return out.reshape(y.shape[0], -1)


def write_codes_ycbcr(r, g, b, bits, matrix, primaries=1, mutant=None):
    """(Y, Cb, Cr) codes of the `bits`-bit code planes r, g, b at full resolution (oracle/avif_oracle.c:534, :561-564; full range,
    chroma zero point 2^(bits-1)).  mutant: 'fma' (the last product of each sum contracted into the addition) or 'reassociated'
    (R c0 + (G c1 + B c2) for (R c0 + G c1) + B c2)."""
    assert mutant in (None, "fma", "reassociated")
    maxi = (1 << bits) - 1
    kr, kg, kb = coefficients(matrix, primaries)
    rows = stage_b_rows(kr, kb)
    rf, gf, bf = (np.asarray(v).astype(F) for v in (r, g, b))
    half = F(1 << (bits - 1))
    out = []
    for name in ("y", "cb", "cr"):
        c0, c1, c2 = rows[name]
        if mutant == "fma":
            s = fused(bf, c2, rf * c0 + gf * c1)
        elif mutant == "reassociated":
            s = rf * c0 + (gf * c1 + bf * c2)
        else:
            s = (rf * c0 + gf * c1) + bf * c2
        if name != "y":
            s = s + half
        assert s.dtype == np.float32
        out.append(_clip_round(s, maxi).astype(np.uint16))
    return tuple(out)
