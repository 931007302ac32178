"""Inputs HUNTED for rounding ties, where the code domain is too large to enumerate (numpy and float64 only; no oracle, no GPU, no
file is read; deterministic).

A kernel that reaches the oracle's bits by another route (x / kg as three FMAs, packed luma, clamp + floor + cast in one step) may be
one ulp off in an intermediate float.  That changes a CODE only where the exact value lies within about one float32 spacing of the
point at which the final truncation jumps: 0.5 + 32768 G an integer (opens to the 16-bit host), the matrix sum + 0.5 an integer
(saves).  A random 10- / 12-bit triple is that close once in a few hundred pixels; the Latin square of tests/exhaustive_inputs.py
shows every (Cb, Cr) pair, but under ONE Y per pair.  Here the third code is chosen per pair so that the pixel sits next to a tie:

  open_ties(bits, kr, kb, full_range, chroma)   the Latin square's chroma planes; for every (Cb, Cr) pair the Y whose exact
                                                0.5 + 32768 G is nearest an integer, among the Y with 0 < G < 1
  save_ties(bits, kr, kb, target)               R = row, B = col; the G that puts the exact pre-truncation value of `target`
                                                (Y, Cb or Cr) nearest an integer, inside the unclipped range
  save_document(bits, kr, kb, chroma)           the three targets side by side, each pixel replicated over its chroma footprint

"Exact" is the float64 value of the reference's per-pixel expression on ITS float32 inputs: the float32 table entries and the float32
constants as the reference rounds them once per image (kr (1 - kr), kg, the matrix rows; tests/reference_numpy.py states them from the
CICP definitions).  Only the per-pixel operations -- the ones a kernel may perform by another route -- are exact here.  Products of a
float32 and a code or a table entry are exact in float64 and the sums are good to 1e-12 code.

tie_distance_* measure how near the ties the result is (float64 alone); tests/test_tie_inputs.py counts every claim made here.
"""
from __future__ import annotations

import concurrent.futures
import functools

import numpy as np

import exhaustive_inputs as xi
import reference_numpy as rn

F = np.float32
TARGETS = ("y", "cb", "cr")
OPEN_SPACING = 2.0 ** -9          # float32 spacing of 32768 G in [16384, 32768)
SAVE_SPACING = {10: 2.0 ** -14, 12: 2.0 ** -12}       # float32 spacing of a matrix sum in [512, 1024) and in [2048, 4096)


def _circular(a, b):
    """|a - b| on the circle of circumference 1."""
    return np.abs(np.mod(a - b + 0.5, 1.0) - 0.5)


THREADS = 8


def _nearest_valid(points, want, lo, hi, k, budget=1 << 20):
    """For every query j: the indices of the k points p whose frac(p) is nearest want[j] on the circle, among the points with
    lo[j] < p < hi[j]; nearest first, ties towards the earlier position in (frac, index) order.  Returns (len(want), k) indices
    into `points`; raises where a query has fewer than k valid points.

    frac(points) is sorted ONCE; a query looks at a window of sorted positions around its insertion point (searchsorted) and the
    window is accepted when the k-th chosen distance does not exceed the distance of either end of the window -- every point outside
    is then at least as far.  The others go round again with a window eight times as wide, the whole circle at the end."""
    m = len(points)
    fr = np.mod(points, 1.0)
    order = np.argsort(fr, kind="stable")
    fs, ps = fr[order], points[order]
    out = np.empty((len(want), k), dtype=np.int64)
    todo = np.arange(len(want))
    half = 2 * k + 2
    while todo.size:
        whole = 2 * half >= m
        width = m if whole else 2 * half
        offsets = np.arange(m) if whole else np.arange(-half, half)
        step = max(1, budget // width)

        def piece(c0):
            q = todo[c0:c0 + step]
            cand = (np.searchsorted(fs, want[q])[:, None] + offsets[None, :]) % m
            raw = _circular(fs[cand], want[q][:, None])
            d = np.where((ps[cand] > lo[q][:, None]) & (ps[cand] < hi[q][:, None]), raw, np.inf)
            pick = np.argsort(d, axis=1, kind="stable")[:, :k]
            dk = np.take_along_axis(d, pick[:, -1:], axis=1)[:, 0]
            if whole:
                if not np.isfinite(dk).all():
                    raise ValueError("a query with fewer than k points inside its range")
                done = np.ones(q.size, dtype=bool)
            else:
                done = dk <= np.minimum(raw[:, 0], raw[:, -1])
            out[q[done]] = order[np.take_along_axis(cand, pick, axis=1)[done]]
            return q[~done]

        # the pieces are independent and write disjoint rows of `out`; numpy releases the interpreter lock inside each operation
        with concurrent.futures.ThreadPoolExecutor(max_workers=THREADS) as pool:
            todo = np.concatenate(list(pool.map(piece, range(0, todo.size, step))))
        half *= 8
    return out


# ---- opens ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _open_terms(bits, kr, kb, full_range):
    """(ty, t): the float32 luma table as float64, and the exact chroma term of G for every (Cb, Cr) pair of the Latin square's
    layout (Cb = row, Cr = (row + col) mod n) from the float32 constants kr (1 - kr), kb (1 - kb) and kg."""
    kr, kb = F(kr), F(kb)
    one = F(1)
    kg = one - kr - kb
    c_r, c_b = kr * (one - kr), kb * (one - kb)
    assert all(type(v) is np.float32 for v in (kg, c_r, c_b))
    ty, tuv, _ = rn.read_tables(bits, full_range)
    sq = xi.latin_square(bits)
    cb, cr = tuv.astype(np.float64)[sq[1]], tuv.astype(np.float64)[sq[2]]
    return ty.astype(np.float64), 2.0 * (float(c_r) * cr + float(c_b) * cb) / float(kg)


@functools.lru_cache(maxsize=2)
def _hunted_luma(bits, kr, kb, full_range, k):
    """(k, n, n) luma codes: for every pair the k nearest-tie Y, nearest first, of DIFFERENT table values (a limited-range table
    repeats its ends: one code stands for each value)."""
    n = 1 << bits
    ty, t = _open_terms(bits, kr, kb, full_range)                        # (called with the float32 values of kr, kb as Python floats)
    values, code = np.unique(ty, return_index=True)                       # the smallest code of every table value
    t = t.reshape(-1)
    # 0.5 + 32768 (ty - t) is an integer  <=>  frac(32768 ty) = frac(32768 t - 0.5);   0 < G < 1  <=>  t < ty < 1 + t
    pick = _nearest_valid(32768.0 * values, np.mod(32768.0 * t - 0.5, 1.0), 32768.0 * t, 32768.0 * (1.0 + t), k)
    return np.ascontiguousarray(code[pick].T.reshape(k, n, n).astype(np.uint16))


def open_ties(bits, kr, kb, full_range, chroma="444"):
    """{0: Y, 1: Cb, 2: Cr}: the chroma planes of xi.latin_square(bits) -- every (Cb, Cr) pair once, so xi.latin_alpha and the
    footprint helpers apply -- under the luma that puts G next to a tie.  4:2:2 / 4:2:0: the luma plane is (n << ys) x (n << xs) and
    position j = 2 dy + dx of a footprint takes the (j + 1)-th nearest Y, so each position is a near-tie of its own."""
    if bits not in (10, 12):
        raise ValueError("8-bit triples are enumerated (exhaustive_inputs.all_triples_444); 16-bit planes have no 16-bit-host tie hunt")
    n = 1 << bits
    sq = xi.latin_square(bits)
    xs, ys = (0, 0) if chroma == "444" else xi.sub_shifts(chroma)
    k = 1 << (xs + ys)
    near = _hunted_luma(bits, float(F(kr)), float(F(kb)), bool(full_range), 4)       # one hunt serves the three chroma forms
    if chroma == "444":
        return {0: near[0].copy(), 1: sq[1], 2: sq[2]}
    y = np.empty((n << ys, n << xs), dtype=np.uint16)
    for dy in range(1 << ys):
        for dx in range(1 << xs):
            y[dy::1 << ys, dx::1 << xs] = near[2 * dy + dx]
    return {0: y, 1: sq[1], 2: sq[2]}


def open_g_exact(planes, bits, kr, kb, full_range, chroma="444", rows=None):
    """The exact (float64, unclamped) G of every pixel of `planes` (rows = (r0, r1): of those luma rows, whole footprints)."""
    xs, ys = (0, 0) if chroma == "444" else xi.sub_shifts(chroma)
    ty, t = _open_terms(bits, float(F(kr)), float(F(kb)), bool(full_range))
    r0, r1 = rows or (0, planes[0].shape[0])
    t = t[r0 >> ys:r1 >> ys]
    if xs or ys:
        t = np.repeat(np.repeat(t, 1 << ys, axis=0), 1 << xs, axis=1)
    return ty[planes[0][r0:r1]] - t


def tie_distance_open(planes, bits, kr, kb, full_range, chroma="444", rows=None):
    """Per pixel: how far 0.5 + 32768 G is from an integer, in codes of the 16-bit host."""
    return _circular(0.5 + 32768.0 * open_g_exact(planes, bits, kr, kb, full_range, chroma, rows), 0.0)


# ---- saves ------------------------------------------------------------------------------------------------------------------------
def save_sum_exact(r, g, b, bits, kr, kb, target):
    """The exact value that clip_round truncates after adding 0.5: R c0 + G c1 + B c2 (+ 2^(bits-1) for Cb and Cr), float64, from
    the float32 matrix row."""
    c0, c1, c2 = (float(c) for c in rn.stage_b_rows(kr, kb)[target])
    s = np.asarray(r, np.float64) * c0 + np.asarray(g, np.float64) * c1 + np.asarray(b, np.float64) * c2
    return s if target == "y" else s + float(1 << (bits - 1))


def save_ties(bits, kr, kb, target, row_step=1):
    """(R, G, B): code planes of n / row_step x n samples with R = row_step * row, B = col and the G that puts save_sum_exact + 0.5
    nearest an integer while the sum stays inside (0, 2^bits - 1): both codes the tie separates are codes the clip leaves alone."""
    if bits not in (10, 12) or target not in TARGETS:
        raise ValueError("10- and 12-bit saves; target 'y', 'cb' or 'cr'")
    n = 1 << bits
    c0, c1, c2 = (float(c) for c in rn.stage_b_rows(kr, kb)[target])
    r = np.broadcast_to(np.arange(0, n, row_step, dtype=np.float64)[:, None], (n // row_step, n))
    b = np.broadcast_to(np.arange(n, dtype=np.float64)[None, :], (n // row_step, n))
    rest = (r * c0 + b * c2 + (0.0 if target == "y" else float(1 << (bits - 1)))).reshape(-1)
    # rest + G c1 + 0.5 is an integer  <=>  frac(G c1) = frac(-(rest + 0.5));   0 < rest + G c1 < n - 1
    pick = _nearest_valid(np.arange(n, dtype=np.float64) * c1, np.mod(-(rest + 0.5), 1.0), -rest, (n - 1.0) - rest, 1)
    g = pick[:, 0].reshape(n // row_step, n).astype(np.uint16)
    return np.ascontiguousarray(r.astype(np.uint16)), g, np.ascontiguousarray(b.astype(np.uint16))


def tie_distance_save(r, g, b, bits, kr, kb, target):
    """Per pixel: how far the value that is truncated (sum + 0.5) is from an integer, in codes."""
    return _circular(save_sum_exact(r, g, b, bits, kr, kb, target) + 0.5, 0.0)


def save_row_step(bits, chroma):
    """12-bit sub-sampled documents keep every 4th R row (n^2 / 4 triples per target); all others keep all n^2."""
    return 4 if (bits == 12 and chroma != "444") else 1


@functools.lru_cache(maxsize=2)
def _save_targets(bits, kr, kb, row_step):
    return tuple(save_ties(bits, kr, kb, t, row_step) for t in TARGETS)


def save_targets(bits, kr, kb, row_step=1):
    """The three hunts of save_document, in the order of TARGETS (shared with it: computed once)."""
    return _save_targets(bits, float(F(kr)), float(F(kb)), row_step)


def save_document(bits, kr, kb, chroma="444"):
    """(R, G, B) code planes of the document that holds the three hunts side by side (the 'y' hunt in the left third, 'cb', 'cr').
    Sub-sampled: every pixel is replicated over its 2 x 1 (4:2:2) or 2 x 2 (4:2:0) footprint, so the box average of a footprint is
    the triple itself (four equal codes below 2^12 sum and scale exactly) and box and nearest both see it."""
    xs, ys = (0, 0) if chroma == "444" else xi.sub_shifts(chroma)
    parts = _save_targets(bits, float(F(kr)), float(F(kb)), save_row_step(bits, chroma))
    rep = lambda a: np.repeat(np.repeat(a, 1 << ys, axis=0), 1 << xs, axis=1) if (xs or ys) else a
    return tuple(np.ascontiguousarray(np.concatenate([rep(p[ch]) for p in parts], axis=1)) for ch in range(3))


def pq_source_for_codes(codes, bits, inverse):
    """One float32 per code for a 32-bit document: the curve's inverse (`inverse`, float64 -> float64) at the middle of the code's
    interval, (code + 0.5) / (2^bits - 1) -- as far from both truncation points of stage A as a float can be."""
    maxc = (1 << bits) - 1
    table = np.asarray(inverse((np.arange(maxc + 1, dtype=np.float64) + 0.5) / maxc), dtype=np.float64).astype(np.float32)
    return table[codes]
