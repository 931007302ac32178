"""The definition of the cropped open (include/avifgpu.h "cropped open"), as numpy on an (H, W, C) array, and the ISO 14496-12 clean
aperture rule with exact fractions: shared by the CPU and the GPU tests."""
from fractions import Fraction
import math

from orientation_truth import orient


def crop(a, rect):
    x0, y0, w, h = rect
    return a[y0:y0 + h, x0:x0 + w]


def cropped(a, rect, code):
    """orient(code, F[y0 : y0 + h, x0 : x0 + w])"""
    return orient(code, crop(a, rect))


def view_size(rect, code):
    return (rect[2], rect[3]) if code <= 4 else (rect[3], rect[2])


def _edges(size, ap_n, ap_d, off_n, off_d):
    """first and last sample of one direction, rounded half up; None for a non-positive denominator or aperture"""
    if ap_d <= 0 or off_d <= 0 or ap_n <= 0:
        return None
    centre = Fraction(off_n, off_d) + Fraction(size - 1, 2)
    half = (Fraction(ap_n, ap_d) - 1) / 2
    return math.floor(centre - half + Fraction(1, 2)), math.floor(centre + half + Fraction(1, 2))


def clap_to_rect(width, height, clap):
    """(x0, y0, w, h), or None where the library must answer formatBadParameters."""
    ex = _edges(width, clap[0], clap[1], clap[4], clap[5])
    ey = _edges(height, clap[2], clap[3], clap[6], clap[7])
    if ex is None or ey is None:
        return None
    left, right = max(ex[0], 0), min(ex[1], width - 1)
    top, bottom = max(ey[0], 0), min(ey[1], height - 1)
    if right < left or bottom < top:
        return None
    return left, top, right - left + 1, bottom - top + 1
