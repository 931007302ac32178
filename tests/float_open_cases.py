"""The cases and inputs of the whole-code-domain float opens, shared by tests/test_whole_float_opens.py (CPU: the oracle inside its
own bar, the inputs counted) and tests/test_zz_gpu_whole_float_opens.py (GPU: the kernels inside theirs).  Numpy only.

  A  YCbCr at 10 bit on the Latin square of tests/exhaustive_inputs.py: every (Y, Cb), (Y, Cr), (Cb, Cr) pair
  B  YCbCr at 12 bit, the same square in row bands: a band of a Latin square is itself an image, and the bands together are the square
  C  planar RGB and gray with alpha on every (code, alpha) pair
"""
import functools

import numpy as np

import exhaustive_inputs as xi
import harness

pkg = harness.pkg

ODD_PAD = 3                       # samples behind every plane row: 6 bytes at 16 bit -- never a multiple of 16 (the unaligned instantiation)
CHAIN_BAR_PIXELS = 1 << 21        # the float64-chain bar (seven curve evaluations per sample) applies up to this many pixels
CHROMA = {"444": pkg.CHROMA_444, "422": pkg.CHROMA_422, "420": pkg.CHROMA_420}
NONE, STRAIGHT, PREMUL = pkg.ALPHA_NONE, pkg.ALPHA_STRAIGHT, pkg.ALPHA_PREMULTIPLIED
ALPHA_NAME = {NONE: "opaque", STRAIGHT: "straight", PREMUL: "premul"}

MATRICES = {"bt2020ncl": dict(matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020),
            "bt601": dict(matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709),
            "bt709": dict(matrix_coefficients=pkg.MATRIX_BT709, color_primaries=pkg.PRIMARIES_BT709),
            "chromaderived432": dict(matrix_coefficients=pkg.MATRIX_CHROMA_DERIVED_NCL, color_primaries=pkg.PRIMARIES_SMPTE432)}
CURVES = {"pq80": dict(transfer_characteristics=pkg.TC_PQ, pq_peak_nits=80),
          "pq10000": dict(transfer_characteristics=pkg.TC_PQ, pq_peak_nits=10000),              # log2(10000 / peak) = 0
          "hlg": dict(transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=0),
          "hlg-ootf": dict(transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=1, hlg_display_gamma=1.2, hlg_peak_nits=1000),
          "hlg-ootf-g1": dict(transfer_characteristics=pkg.TC_HLG, hlg_apply_ootf=1, hlg_display_gamma=1.0, hlg_peak_nits=1000),
          "smpte428": dict(transfer_characteristics=pkg.TC_SMPTE428)}
ONE_VALUE_CURVES = ("pq80", "pq10000", "hlg", "smpte428")        # functions of one float: no OOTF behind them


def case_id(curve, chroma, fr, alpha, matrix="bt2020ncl"):
    return f"{curve}-{chroma}-{('limited', 'full')[fr]}-{ALPHA_NAME[alpha]}" + ("" if matrix == "bt2020ncl" else f"-{matrix}")


def cases_a():
    """(curve, chroma, full_range, alpha_state, matrix) of section A, in a fixed order."""
    out = [("pq80", chroma, fr, a, "bt2020ncl") for chroma in ("444", "422", "420") for fr in (1, 0) for a in (NONE, STRAIGHT, PREMUL)]
    for curve in ("pq10000", "hlg", "hlg-ootf", "smpte428"):
        out += [(curve, "444", fr, a, "bt2020ncl") for fr in (1, 0) for a in (NONE, PREMUL)]
        out += [(curve, "422", 1, NONE, "bt2020ncl"), (curve, "420", 1, PREMUL, "bt2020ncl")]
    # gamma 1.0: powf(luma, 0) is 1 also for a black pixel.  The square without alpha holds no black pixel (no 10-bit chroma code is
    # exactly neutral, in either range: one of R, G, B stays above 0), so the open also runs with premultiplied alpha (alpha 0: black).
    out += [("hlg-ootf-g1", "444", 1, a, "bt2020ncl") for a in (NONE, PREMUL)]
    out += [("pq80", "444", 1, NONE, m) for m in ("bt601", "bt709", "chromaderived432")]
    return out


# 12 bit: (chroma, full_range, alpha_state, chroma rows per band).  No band holds more than 2^22 pixels: 4096 x 512 (4:4:4),
# 8192 x 512 (4:2:2), 8192 x 512 luma rows over 256 chroma rows (4:2:0).
FAMILIES_B = {"444-full-opaque": ("444", 1, NONE, 512), "422-full-opaque": ("422", 1, NONE, 512), "420-limited-premul": ("420", 0, PREMUL, 256)}
CURVE_B, BITS_B = "pq80", 12


def bands_b(family):
    """The (first chroma row, chroma rows) of every band of a family."""
    rows = FAMILIES_B[family][3]
    return [(r, rows) for r in range(0, 1 << BITS_B, rows)]


def cases_b():
    return [(family, r, rows) for family in FAMILIES_B for r, rows in bands_b(family)]


@functools.lru_cache(maxsize=2)
def _square(bits, chroma):
    return xi.latin_square(bits, chroma)


def release_inputs():
    _square.cache_clear()


def ycc_planes(bits, chroma, alpha, band=None):
    """The Latin square (under latin_alpha where the case has alpha), or the band (first chroma row, chroma rows) of it."""
    planes = dict(_square(bits, chroma))
    if alpha != NONE:
        planes[3] = xi.latin_alpha(bits, planes[0].shape)
    if band is not None:
        ys = xi.sub_shifts(chroma)[1] if chroma != "444" else 0
        r, rows = band
        planes = {pl: np.ascontiguousarray(a[r:r + rows] if pl in (1, 2) else a[r << ys:(r + rows) << ys]) for pl, a in planes.items()}
    return planes


# The HLG select `value > 0.5f`: 10-bit codes reach the floats next to 0.5 almost nowhere (Y + c Cr over a / 1023 lives on a lattice that
# misses them).  The 4:4:4 full-range premultiplied square holds one sample within 2 ulp ABOVE 0.5; a search over (Y, Cr, alpha) under
# three Cb codes found samples within 2 ulp BELOW it in the G channel under (Cb, Cr) = (700, 753), none at 0.5 itself.  select_planes() is
# every (Y, alpha) pair under that chroma; tests/test_whole_float_opens.py counts both.
HLG_SELECT = (700, 753)


def select_planes(bits=10):
    y, alpha = xi.pairs(bits)
    return {0: y, 1: np.full_like(y, HLG_SELECT[0]), 2: np.full_like(y, HLG_SELECT[1]), 3: alpha}


def near_half(V32):
    """(samples 1 or 2 float32 steps below 0.5, samples equal to 0.5, samples 1 or 2 steps above)."""
    off = np.ascontiguousarray(V32.astype(np.float32)).view(np.uint32).astype(np.int64) - int(np.array(0.5, np.float32).view(np.uint32))
    return int(((off >= -2) & (off < 0)).sum()), int((off == 0).sum()), int(((off > 0) & (off <= 2)).sum())


def ycc_desc(planes, bits, curve, chroma, fr, alpha, matrix="bt2020ncl"):
    h, w = planes[0].shape
    return pkg.ReadDesc(width=w, height=h, colorspace=pkg.COLORSPACE_YCBCR, chroma=CHROMA[chroma], bit_depth=bits, depth=32,
                        alpha_state=alpha, full_range_flag=fr, **MATRICES[matrix], **CURVES[curve])


# ---- C: every (code, alpha) pair -------------------------------------------------------------------------------------------------------
def cases_c10():
    """(colourspace, curve, alpha_state, full_range) at 10 bit."""
    out = [("rgb", curve, a, 1) for curve in ("pq80", "hlg", "hlg-ootf", "smpte428") for a in (STRAIGHT, PREMUL)]
    out += [("gray", "pq80", a, fr) for fr in (1, 0) for a in (STRAIGHT, PREMUL)]       # gray opens are PQ; full range decodes without tables
    return out


BAND_C12 = 512                    # alpha rows per 12-bit band


def pair_planes(bits, cs, band=None):
    """alpha = row, code = col (xi.pairs); planar RGB: G and B are col shifted by n / 3 and 2 n / 3, so along a row every channel takes
    every code.  A band (first alpha row, rows) that does not hold the opaque row gets it appended: the opaque pixels of the SAME open
    are what the bitwise comparison reads a code's own colour from."""
    code, alpha = xi.pairs(bits)
    n = 1 << bits
    shift = lambda k: ((code.astype(np.uint32) + k * (n // 3)) % n).astype(code.dtype)
    planes = {0: code, 3: alpha} if cs == "gray" else {0: code, 1: shift(1), 2: shift(2), 3: alpha}
    if band is not None:
        r, rows = band
        keep = np.r_[r:r + rows] if r + rows == n else np.r_[r:r + rows, n - 1]
        planes = {pl: np.ascontiguousarray(a[keep]) for pl, a in planes.items()}
    return planes


def pair_desc(planes, bits, cs, curve, alpha, fr=1):
    h, w = planes[0].shape
    if cs == "gray":
        return pkg.ReadDesc(width=w, height=h, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, bit_depth=bits, depth=32,
                            alpha_state=alpha, full_range_flag=fr, **CURVES[curve])
    return pkg.ReadDesc(width=w, height=h, colorspace=pkg.COLORSPACE_RGB, chroma=pkg.CHROMA_444, bit_depth=bits, depth=32, alpha_state=alpha,
                        matrix_coefficients=pkg.MATRIX_RGB_GBR, color_primaries=pkg.PRIMARIES_BT2020, **CURVES[curve])


def small_window(V32, bits):
    """The samples whose curve argument lies strictly between 0 and the first code value, the float32 quotient 1 / max -- where no
    table value falls (planar RGB and gray have none)."""
    return (V32 > 0) & (V32 < float(np.float32(1) / np.float32((1 << bits) - 1)))
