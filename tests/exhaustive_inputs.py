"""Inputs that cover a whole CODE DOMAIN instead of sampling it (numpy only; no oracle, no GPU, no file is read).

The integer tiers are bit-exact claims about a finite set of codes.  A random 67 x 21 frame holds 1407 pixels; a kernel that is one
rounding off on 1 sample in 5000 passes it nine times out of ten.  The generators below enumerate instead:

  all_triples_444()        every 8-bit (Y, Cb, Cr) -- or (R, G, B) -- triple exactly once, 4096 x 4096
  all_triples_sub(chroma)  the same 2^24 triples in a 4:2:2 / 4:2:0 image (each chroma sample serves its whole footprint)
  latin_square(bits)       n x n, n = 2^bits: every (Y, Cb), (Y, Cr) and (Cb, Cr) PAIR exactly once -- all that R, B and the chroma term
                           of G (with its division by kg) depend on -- where n^3 triples are out of reach (10 and 12 bit)
  pairs(bits)              every (code, alpha) pair once: gray + alpha, one channel of planar RGB + alpha, the integer premultiply
  latin_alpha(bits)        an alpha plane for the Latin square that takes every code in every row and every column
  interleaved(planes)      the planes as the channels of an interleaved document (the save direction)
  code_preimages(codes)    for a monotonic rescale sampled on a ramp: the smallest and the largest source value of every output code

tests/test_exhaustive_inputs.py verifies every claim made here with np.unique; the GPU tests rely on those checks.
Planes come back as {plane index: 2-D array}, the layout of harness.make_read_source (0 = Y, 1 = Cb, 2 = Cr, 3 = alpha), C-contiguous.
"""
from __future__ import annotations

import numpy as np

SIDE8 = 4096                      # 4096 x 4096 = 2^24 = every 8-bit triple once


def _dtype(bits):
    return np.uint8 if bits <= 8 else np.uint16


def all_triples_444(bits=8):
    """{0, 1, 2: (4096, 4096) u8}: pixel k (raster order) holds plane0 = k >> 16, plane1 = k & 255, plane2 = (k >> 8) & 255."""
    if bits != 8:
        raise ValueError("all triples fit an image at 8 bit only (2^24); use latin_square for 10 and 12 bit")
    k = np.arange(1 << 24, dtype=np.uint32).reshape(SIDE8, SIDE8)
    return {0: (k >> 16).astype(np.uint8), 1: (k & 255).astype(np.uint8), 2: ((k >> 8) & 255).astype(np.uint8)}


def sub_shifts(chroma):
    """(xs, ys) of '422' / '420'."""
    return {"422": (1, 0), "420": (1, 1)}[chroma]


def all_triples_sub(chroma, phase=0):
    """A 4096 x 4096 image with 4:2:2 ('422') or 4:2:0 ('420') chroma planes that still holds every 8-bit (Y, Cb, Cr) triple once.
    Chroma sample k (raster order over the chroma plane): Cb = k & 255, Cr = (k >> 8) & 255, s = k >> 16.  Pixel j of its footprint
    (j = 2 * dy + dx) gets Y = 4 s + j (4:2:0, s < 64) or Y = 2 s + j (4:2:2, s < 128).  phase 1 mirrors j inside the footprint
    (Y = 4 s + (3 - j) / 2 s + (1 - j)), so that the position inside a footprint is not tied to the low bits of Y."""
    xs, ys = sub_shifts(chroma)
    cw, ch = SIDE8 >> xs, SIDE8 >> ys
    k = np.arange(cw * ch, dtype=np.uint32).reshape(ch, cw)
    cb = (k & 255).astype(np.uint8)
    cr = ((k >> 8) & 255).astype(np.uint8)
    s = (k >> 16).astype(np.uint8)
    nj = 1 << (xs + ys)
    assert int(s.max()) == 256 // nj - 1
    y = np.empty((SIDE8, SIDE8), dtype=np.uint8)
    for dy in range(1 << ys):
        for dx in range(1 << xs):
            j = 2 * dy + dx
            if phase:
                j = nj - 1 - j
            y[dy::1 << ys, dx::1 << xs] = s * nj + j
    return {0: y, 1: cb, 2: cr}


LATIN_STEP = 1365                 # the fixed odd c of the sub-sampled Latin square: Y = (ccol + c * j) mod n, far from a small stride


def latin_square(bits, chroma="444"):
    """n = 2^bits.  Chroma planes n x n with Cb = row, Cr = (row + col) mod n; 4:4:4: Y = col.  Every (Y, Cb), (Y, Cr) and (Cb, Cr)
    pair occurs exactly once.  Sub-sampled ('422' / '420'): the square lives at chroma resolution and pixel j of a footprint gets
    Y = (ccol + LATIN_STEP * j) mod n -- a bijection of ccol for each j, so every position of the footprint is itself exhaustive
    in (Y, Cb) and (Y, Cr)."""
    n = 1 << bits
    dt = _dtype(bits)
    row = np.arange(n, dtype=np.uint32)[:, None]
    col = np.arange(n, dtype=np.uint32)[None, :]
    cb = np.ascontiguousarray(np.broadcast_to(row, (n, n)), dtype=dt)
    cr = np.ascontiguousarray((row + col) % n, dtype=dt)
    if chroma == "444":
        return {0: np.ascontiguousarray(np.broadcast_to(col, (n, n)), dtype=dt), 1: cb, 2: cr}
    xs, ys = sub_shifts(chroma)
    y = np.empty((n << ys, n << xs), dtype=dt)
    for dy in range(1 << ys):
        for dx in range(1 << xs):
            y[dy::1 << ys, dx::1 << xs] = np.broadcast_to((col + LATIN_STEP * (2 * dy + dx)) % n, (n, n))
    return {0: y, 1: cb, 2: cr}


def latin_alpha(bits, shape=None):
    """(3 row + 5 col + 1) mod n over `shape` (default n x n): 3 and 5 are odd, so every row and every column of an n x n window
    takes every code once -- in particular 0 (the 'alpha == 0' branch) and n - 1 (opaque) meet every Y column and every Cb row."""
    n = 1 << bits
    h, w = shape or (n, n)
    row = np.arange(h, dtype=np.uint32)[:, None]
    col = np.arange(w, dtype=np.uint32)[None, :]
    return np.ascontiguousarray((3 * row + 5 * col + 1) % n, dtype=_dtype(bits))


def pairs(bits):
    """(code, alpha): two n x n planes, code = col, alpha = row."""
    n = 1 << bits
    dt = _dtype(bits)
    a = np.arange(n, dtype=dt)
    return np.ascontiguousarray(np.broadcast_to(a[None, :], (n, n))), np.ascontiguousarray(np.broadcast_to(a[:, None], (n, n)))


def code_preimages(codes, bits):
    """codes[v] = the output code of source value v, v = 0 .. len(codes) - 1, non-decreasing.  Returns (lo, hi), 2^bits entries each:
    the smallest and the largest v of every output code.  Raises if a code has no preimage or the map is not monotonic."""
    codes = np.asarray(codes).astype(np.int64).reshape(-1)
    n = 1 << bits
    if np.any(np.diff(codes) < 0) or codes[0] != 0 or codes[-1] != n - 1:
        raise ValueError("not a monotonic rescale onto 0 .. 2^bits - 1")
    lo = np.searchsorted(codes, np.arange(n), side="left")
    hi = np.searchsorted(codes, np.arange(n), side="right") - 1
    if np.any(hi < lo):
        raise ValueError("an output code without a source value")
    return lo.astype(np.uint16), hi.astype(np.uint16)


def ends_for_triples(r, g, b, phase=0):
    """Which end of its preimage each channel of the triple (r, g, b) takes (0 = smallest, 1 = largest source value): the parity of
    the OTHER two codes, complemented in phase 1 -- over both phases every triple is seen with each channel at both ends, and inside
    one phase every code of a channel meets both ends."""
    r, g, b = (np.asarray(v).astype(np.uint32) for v in (r, g, b))
    return ((g + b + phase) & 1, (r + b + phase) & 1, (r + g + phase) & 1)


def every_u16_in_each_channel(planes):
    """(256, 256 * planes) u16, interleaved: pixel v (raster order) holds (v, 3 v + 1, 5 v + 2, 7 v + 3) mod 2^16 in its first
    `planes` channels.  Multiplying by an odd number permutes 0 .. 65535, so EVERY channel position takes every 16-bit value once
    (the values above 32768 are the over-range ones the save clamps)."""
    v = np.arange(1 << 16, dtype=np.uint32)
    px = np.stack([(v * m + a) & 0xFFFF for m, a in ((1, 0), (3, 1), (5, 2), (7, 3))[:planes]], axis=1).astype(np.uint16)
    return np.ascontiguousarray(px.reshape(256, 256 * planes))


def interleaved(planes, order=(0, 1, 2)):
    """(H, W * len(order)) array, C-contiguous: the planes as the interleaved channels of a document (alpha last, as FormatRecord has it)."""
    h, w = planes[order[0]].shape
    return np.ascontiguousarray(np.stack([planes[k] for k in order], axis=-1).reshape(h, w * len(order)))


def lattice64():
    """The 64^3 lattice of tests/test_gpu_read.py::test_read_exhaustive_8bit_yuv (64 evenly spaced codes per channel) as 512 x 512 planes."""
    v = np.linspace(0, 255, 64).round().astype(np.uint8)
    y, u, w = np.meshgrid(v, v, v, indexing="ij")
    return {0: y.reshape(512, 512).copy(), 1: u.reshape(512, 512).copy(), 2: w.reshape(512, 512).copy()}


def with_stride_pad(planes, pad):
    """The same planes with `pad` unused samples behind every row (an odd pad makes every row start unaligned)."""
    out = {}
    for pl, a in planes.items():
        b = np.zeros((a.shape[0], a.shape[1] + pad), dtype=a.dtype)
        b[:, :a.shape[1]] = a
        out[pl] = b
    return out
