"""Inputs that cover the whole FLOAT domain of a float-tier save instead of sampling it (numpy for the oracle side, torch for the
device side: both produce the same bits; no file is read).

A write curve is a function of one float, and there are 2^32 of them.  The generators below enumerate:

  chunks()                       the 2^32 float32 bit patterns in order of the bit pattern, as (first pattern, count) with count = 2^26
  patterns(first, count)         the floats whose bit patterns are first .. first + count - 1
  window(desc)                   (e0, e1): the whole binades [2^e0, 2^e1) between "the code is still 0" and "the code is saturated" of
                                 the curve, the peak and the depth of `desc`, derived from tests/truth64.py:
                                     curve64(2^e0) * max < 0.5          (e0 the largest such exponent)
                                     curve64(2^e1) >= 1 + band          (e1 the smallest such exponent; Clip: 2^e1 >= 2)
                                 with band = the curve's relative band + BAND_ABS / max
  window_groups(e0, e1)          the window as (first pattern, count) groups of at most 8 binades (2^26 floats)
  document(first, count, shift)  an OUT_REFERENCE, planes = 3, 4096-pixel-wide document whose consecutive samples are the consecutive
                                 floats: sample shift + i holds pattern first + i, so each channel slot sees a third of the floats;
                                 shift = 1 puts every float in another slot.  Unused samples (the shift, the tail of the last row) are +0.
  sparse_patterns(step, ...)     every step-th pattern outside a window, finite ones only; document_of(vals) lays given floats out
  gray_document / pair_document  the same floats as a planes = 1 document, and as the LAST channel of a planes = 2 / 4 document

Positive floats are ordered as their bit patterns are, so a binade is the 2^23 patterns (e + 127) << 23 .. and a window is one run.
tests/test_exhaustive_floats.py counts these claims; the GPU tests rely on those checks.
"""
from __future__ import annotations

import numpy as np

import truth64

pkg = truth64.pkg

CHUNK = 1 << 26
BINADE = 1 << 23
WIDTH = 4096
ROW = WIDTH * 3                    # samples per row of the planes = 3 document
INF_BITS, NEG_ZERO_BITS, NEG_INF_BITS = 0x7F800000, 0x80000000, 0xFF800000


def chunks():
    return [(k * CHUNK, CHUNK) for k in range((1 << 32) // CHUNK)]


def binade_first(e):
    """Bit pattern of 2^e (a normal float32)."""
    assert -126 <= e <= 127
    return (e + 127) << 23


def patterns(first, count, device=None):
    """float32 array (device None: numpy; else a torch tensor there) of the bit patterns first .. first + count - 1."""
    assert 0 <= first and first + count <= 1 << 32
    if device is None:
        if first + count < 1 << 32:
            return np.arange(first, first + count, dtype=np.uint32).view(np.float32)
        return np.arange(first, first + count, dtype=np.int64).astype(np.uint32).view(np.float32)
    import torch
    b = torch.arange(first, first + count, dtype=torch.int64, device=device)
    b = b - ((b >> 31) << 32)                                      # patterns from 2^31 on are the negative int32 of the same bits
    return b.to(torch.int32).view(torch.float32)


def bits_of(x):
    """The bit patterns (0 .. 2^32 - 1, int64) of a float32 numpy array or torch tensor."""
    if isinstance(x, np.ndarray):
        return x.view(np.uint32).astype(np.int64)
    import torch
    return x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _rows(samples, row):
    return (samples + row - 1) // row


def _layout(vals, rows, row, shift, device):
    n = vals.shape[0]
    if device is None:
        doc = np.zeros(rows * row, dtype=np.float32)
    else:
        import torch
        doc = torch.zeros(rows * row, dtype=torch.float32, device=device)
    doc[shift:shift + n] = vals
    return doc.reshape(rows, row)


def document(first, count, shift=0, device=None):
    """(rows, 4096 * 3) float32: sample shift + i (raster order) holds pattern first + i; everything else is +0."""
    return _layout(patterns(first, count, device), _rows(count + shift, ROW), ROW, shift, device)


def document_desc(rows, bits, transfer, peak=80, pq_evaluation=0, planes=3, **kw):
    """The save of a document() / gray_document() / pair_document(): 4096 pixels wide, 32-bit, hand-off output unless said otherwise."""
    kw.setdefault("output", pkg.OUT_REFERENCE)
    kw.setdefault("alpha_state", pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE)
    return pkg.WriteDesc(width=WIDTH, height=rows, depth=32, planes=planes, bit_depth=bits, transfer=transfer, peak_nits=peak,
                         pq_evaluation=pq_evaluation, **kw)


def gray_document(first, count, device=None):
    """(rows, 4096) float32, planes = 1: pixel i holds pattern first + i."""
    return _layout(patterns(first, count, device), _rows(count, WIDTH), WIDTH, 0, device)


def pair_document(first, count, planes, colour=0.5, device=None):
    """(rows, 4096 * planes) float32, planes = 2 or 4: pixel i has `colour` in every colour channel and pattern first + i as its
    alpha.  The unused pixels of the last row are all +0."""
    rows = _rows(count, WIDTH)
    vals = patterns(first, count, device)
    if device is None:
        px = np.zeros((rows * WIDTH, planes), dtype=np.float32)
    else:
        import torch
        px = torch.zeros((rows * WIDTH, planes), dtype=torch.float32, device=device)
    px[:count, :planes - 1] = colour
    px[:count, planes - 1] = vals
    return px.reshape(rows, WIDTH * planes)


# ---- the window of a curve --------------------------------------------------------------------------------------------------------
def curve64_scalar(desc, x):
    """The float64 curve of `desc` at one value (Clip: the value itself)."""
    if desc.transfer == pkg.TRANSFER_CLIP:
        return float(x)
    return float(truth64.oetf64(desc, np.array([x], dtype=np.float32))[0])


def band(desc):
    """The band of a saturated code, relative to max: the curve's relative band plus BAND_ABS codes (Clip: BAND_ABS alone)."""
    maxv = float((1 << desc.bit_depth) - 1)
    rel = 0.0 if desc.transfer == pkg.TRANSFER_CLIP else truth64.band_rel(desc)
    return rel + truth64.BAND_ABS / maxv


def window(desc):
    """(e0, e1), see the module docstring.  The curves rise with the sample, so each edge is found by walking the exponents."""
    maxv = float((1 << desc.bit_depth) - 1)
    e0 = max(e for e in range(-126, 0) if curve64_scalar(desc, 2.0 ** e) * maxv < 0.5)
    if desc.transfer == pkg.TRANSFER_CLIP:
        e1 = 1
    else:
        e1 = min(e for e in range(e0 + 1, 128) if curve64_scalar(desc, 2.0 ** e) >= 1.0 + band(desc))
    return e0, e1


def window_groups(e0, e1, binades=CHUNK // BINADE):
    """[(first pattern, count, first exponent)] covering [2^e0, 2^e1) in groups of at most `binades` whole binades."""
    return [(binade_first(e), (min(e + binades, e1) - e) * BINADE, e) for e in range(e0, e1, binades)]


# ---- float64 truth of a code ------------------------------------------------------------------------------------------------------
def truth_codes(desc, x):
    """T = clip(curve64(x) * max, 0, max), float64 (numpy or torch, as the float32 x)."""
    maxv = float((1 << desc.bit_depth) - 1)
    return truth64._Ops(x).clip(truth64.oetf64(desc, x) * maxv, 0.0, maxv)


def truth_interval(desc, x, t=None):
    """(lo, hi) integer-valued float64 (numpy or torch, as x): a code inside the project's band lies in
    [floor(T (1 - rel) - abs), floor(T (1 + rel) + abs)], T = truth_codes(desc, x), rel / abs the bands of tests/truth64.py."""
    o = truth64._Ops(x)
    maxv = float((1 << desc.bit_depth) - 1)
    t = truth_codes(desc, x) if t is None else t
    rel = truth64.band_rel(desc)
    lo = o.floor(o.clip(t * (1.0 - rel) - truth64.BAND_ABS, 0.0, maxv))
    hi = o.floor(o.clip(t * (1.0 + rel) + truth64.BAND_ABS, 0.0, maxv))
    return lo, hi


def band_needed(desc, x, codes, t=None):
    """The relative band a code sequence actually needs, as a float64 array like x: 0 where the code is inside
    [floor(T - abs), floor(T + abs)], else the smallest rel with code in [floor(T (1 - rel) - abs), floor(T (1 + rel) + abs)]
    (code below the truth: T (1 - rel) - abs < code + 1; code above it: T (1 + rel) + abs >= code)."""
    o = truth64._Ops(x)
    t = truth_codes(desc, x) if t is None else t
    c = o.f64(codes)
    tt = o.max2(t, 0.0 * t + 1e-300)
    return o.relu(o.max2(1.0 - (c + 1.0 + truth64.BAND_ABS) / tt, (c - truth64.BAND_ABS) / tt - 1.0))


def sparse_patterns(step, skip_first, skip_count, device=None):
    """The finite floats among the patterns 0, step, 2 step, ... that lie outside the run [skip_first, skip_first + skip_count)."""
    if device is None:
        b = np.arange(0, 1 << 32, step, dtype=np.int64)
    else:
        import torch
        b = torch.arange(0, 1 << 32, step, dtype=torch.int64, device=device)
    keep = ((b & 0x7F800000) != 0x7F800000) & ((b < skip_first) | (b >= skip_first + skip_count))
    b = b[keep]
    if device is None:
        return b.astype(np.uint32).view(np.float32)
    import torch
    return (b - ((b >> 31) << 32)).to(torch.int32).view(torch.float32)


def document_of(vals, shift=0):
    """document() for given floats (numpy array or torch tensor) in place of a run of patterns."""
    device = None if isinstance(vals, np.ndarray) else vals.device
    return _layout(vals, _rows(vals.shape[0] + shift, ROW), ROW, shift, device)


def clip_codes(x, bits):
    """trunc(clamp(x * maxf, 0, maxf)) in float32 (numpy or torch float32 in, int64 out): the Clip 'curve' and every alpha plane
    after clamp(a, 0, 1).  NaN is not handled here."""
    maxf = float((1 << bits) - 1)
    if isinstance(x, np.ndarray):
        return np.clip(x * np.float32(maxf), np.float32(0.0), np.float32(maxf)).astype(np.int64)
    import torch
    return (x * maxf).clamp(0.0, maxf).to(torch.int64)


def alpha_codes(a, bits):
    """trunc(clamp(a, 0, 1) * max) in float32 (numpy or torch float32 in, int64 out); NaN is not handled here."""
    maxf = float((1 << bits) - 1)
    if isinstance(a, np.ndarray):
        return (np.clip(a, np.float32(0.0), np.float32(1.0)) * np.float32(maxf)).astype(np.int64)
    import torch
    return (a.clamp(0.0, 1.0) * maxf).to(torch.int64)


# ---- the oracle on a whole document -----------------------------------------------------------------------------------------------
def oracle_planes(desc, src):
    """{plane: u16 array} of the oracle's save of the numpy document `src`, converted on all host cores
    (oracle_write_image_all_cores; tests/test_oracle_properties.py holds it to the plain whole-frame conversion)."""
    import ctypes

    import harness
    import oracle_binding
    L = oracle_binding.load()
    bufs = harness._alloc_write_out(desc, desc.height)
    ptrs = pkg.planes4([bufs[i].ctypes.data if i in bufs else None for i in range(4)])
    strides = pkg.strides4([bufs[i].strides[0] if i in bufs else 0 for i in range(4)])
    n = ctypes.c_int32(0)
    rc = L.oracle_write_image_all_cores(ctypes.byref(desc), src.ctypes.data, src.strides[0], ctypes.byref(ptrs), ctypes.byref(strides),
                                        ctypes.byref(n))
    if rc != 0:
        raise pkg.AvifGpuError(rc, "oracle_write_image_all_cores")
    return {pl: b[:, :harness.write_planes(desc)[pl][0]] for pl, b in bufs.items()}
