"""Hand-built stage programs of avifgpu_icc_pipeline32 (include/avifgpu.h) and a plain numpy restatement of every stage kind.

A program is described by a SPEC, a list of stage tuples:
    ("tables", [t0, t1, t2], gap)      16-bit table curves (uint16 arrays of 2..4096 entries); `gap` filler words in front of each table
    ("param", [(type, [P0, ...])] * 3) lcms2 parametric curves, type +-1..+-5
    ("matrix", m9, bias3 or None)
    ("clut", nodes, gap)               nodes: uint16 array (n0, n1, n2, 3), input 0 slowest; `gap` filler words in front of the grid
    ("lab2xyz",) / ("xyz2lab",)
    ("fill", n)                        n filler words, no stage (brings words[] to a chosen size)
    ("tail",)                          the Rec.2020-linear destination curves: parametric type -1, gamma 1
build() fills pkg.IccPipeline32 from a spec, stamp() has the library stamp it (the callback is the library's own host evaluation: the
stamp the write entry demands, not evidence), eval_host() is avifgpu_icc_pipeline32_eval and eval_numpy() the restatement:
integer stages on int64 wrapped to 32 bits where lcms2's int32 arithmetic wraps, float stages in float64 with a cast to float32 where
lcms2 casts.  Nothing here needs lcms2 except lut_profile()."""
import ctypes

import numpy as np

import harness

pkg = harness.pkg

F32_1E22 = np.float64(np.float32(1e22))                     # lcms2's PLUS_INF / MINUS_INF are float literals
DET_TOL = 1e-4                                              # MATRIX_DET_TOLERANCE
MAX_XYZ = 1.0 + 32767.0 / 32768.0
D50 = (0.9642, 1.0, 0.8249)
TAIL = ("tail",)


# ---- builders --------------------------------------------------------------------------------------------------------------------
def build(spec, target=None):
    p = pkg.IccPipeline32()
    p.target = pkg.ICC_TARGET_REC2020_LINEAR if target is None else target
    words = []
    filler = 0x5a5a
    i = 0
    for st in spec:
        if st[0] == "fill":
            words += [filler] * st[1]
            continue
        s = p.stages[i]
        i += 1
        if st[0] == "tables":
            s.kind = pkg.ICC_STAGE_CURVES
            for c, t in enumerate(st[1]):
                words += [filler] * st[2]
                s.curve_type[c], s.entries[c], s.offset[c] = 0, len(t), len(words)
                words += [int(x) for x in t]
        elif st[0] in ("param", "tail"):
            s.kind = pkg.ICC_STAGE_CURVES
            curves = [(-1, [1.0])] * 3 if st[0] == "tail" else st[1]
            for c, (typ, params) in enumerate(curves):
                s.curve_type[c] = typ
                for k, v in enumerate(params):
                    s.params[c][k] = v
        elif st[0] == "matrix":
            s.kind = pkg.ICC_STAGE_MATRIX
            for k in range(9):
                s.matrix[k] = st[1][k]
            if st[2] is not None:
                s.has_bias = 1
                for k in range(3):
                    s.bias[k] = st[2][k]
        elif st[0] == "clut":
            s.kind = pkg.ICC_STAGE_CLUT16
            nodes = st[1]
            words += [filler] * st[2]
            s.offset[0] = len(words)
            for k in range(3):
                s.entries[k] = nodes.shape[k]
            words += nodes.reshape(-1).tolist()
        elif st[0] == "lab2xyz":
            s.kind = pkg.ICC_STAGE_LAB_TO_XYZ
        elif st[0] == "xyz2lab":
            s.kind = pkg.ICC_STAGE_XYZ_TO_LAB
        else:
            raise ValueError(st[0])
    p.stage_count, p.word_count = i, len(words)
    if words:
        np.ctypeslib.as_array(p.words)[:len(words)] = np.asarray(words, dtype=np.uint16)
    return p


def fill_into(p, spec):
    """Write another program into the SAME struct (what a caller does between two saves)."""
    q = build(spec)
    ctypes.memmove(ctypes.byref(p), ctypes.byref(q), ctypes.sizeof(q))
    return p


def eval_host(prog, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.empty_like(rgb)
    rc = pkg.load().avifgpu_icc_pipeline32_eval(ctypes.byref(prog), rgb.ctypes.data, out.ctypes.data, rgb.shape[0])
    assert rc == 0, pkg.load().avifgpu_last_error()
    return out


def stamp(prog):
    lib = pkg.load()

    def run(user, pin, pout, n):
        assert lib.avifgpu_icc_pipeline32_eval(ctypes.byref(prog), pin, pout, n) == 0
    cb = pkg.TransformF32Fn(run)
    rc = lib.avifgpu_icc_pipeline32_prove(ctypes.byref(prog), ctypes.cast(cb, ctypes.c_void_p), None)
    assert rc == 0 and prog.proof != 0, lib.avifgpu_last_error()
    return prog


# ---- integer stages: int64, wrapped where lcms2 wraps -----------------------------------------------------------------------------
def _i32(x):
    """The int32 an int64 sum wraps to."""
    return ((x + (1 << 31)) & 0xffffffff) - (1 << 31)


def sat_word(v):
    """_cmsQuickSaturateWord(v * 65535.0) of float32 v: the saturations, then _cmsQuickFloorWord -- the low word of the double
    (d - 32767) + 1.5 * 2^36, shifted.  A NaN takes neither saturation; its word comes from the low bits of its payload."""
    with np.errstate(all="ignore"):
        d = np.asarray(v, dtype=np.float32).astype(np.float64) * 65535.0 + 0.5
        t = (d - 32767.0) + 68719476736.0 * 1.5
    low = (t.view(np.uint64) & 0xffffffff).astype(np.int64)
    w = ((_i32(low) >> 16) + 32767) & 0xffff
    return np.where(d <= 0, 0, np.where(d >= 65535.0, 0xffff, w)).astype(np.int64)


def to_fixed_domain(a):
    return a + (a + 0x7fff) // 0xffff


def lin_lerp_1d(table, w):
    """LinLerp1D of cmsEvalToneCurve16 on a sampled curve of len(table) entries, w: int64 words."""
    T = np.asarray(table, dtype=np.int64)
    n = len(T)
    val3 = to_fixed_domain((n - 1) * w)
    cell0, rest = val3 >> 16, val3 & 0xffff
    y0, y1 = T[cell0], T[np.minimum(cell0 + 1, n - 1)]
    dif = (((y1 - y0) * rest) & 0xffffffff) + 0x8000             # the product as uint32, as the library forms it
    out = (((dif & 0xffffffff) >> 16) + y0) & 0xffff
    return np.where(w == 0xffff, T[n - 1], out)                  # the library returns the last entry for 0xffff outright


def tetrahedral(nodes, w):
    """TetrahedralInterp16 on an n0 x n1 x n2 grid (nodes: (n0, n1, n2, 3) words, input 0 slowest), lcms2's own if-tree, its int32
    Rest wrapped.  w: (N, 3) int64 words."""
    T = np.asarray(nodes, dtype=np.int64)
    n = np.array(T.shape[:3], dtype=np.int64)
    f = to_fixed_domain(w * (n - 1))
    c0, r = f >> 16, f & 0xffff
    c1 = np.where(w == 0xffff, c0, c0 + 1)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    conds = [(rx >= ry) & (ry >= rz), (rx >= ry) & (ry < rz) & (rz >= rx), (rx >= ry) & (ry < rz) & (rz < rx),
             (rx < ry) & (rx >= rz), (rx < ry) & (rx < rz) & (ry >= rz), (rx < ry) & (rx < rz) & (ry < rz)]
    orders = [(0, 1, 2), (2, 0, 1), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 1, 0)]
    base = T[c0[:, 0], c0[:, 1], c0[:, 2]]
    out = np.zeros_like(base)
    for cond, order in zip(conds, orders):
        pos = [c0[:, 0], c0[:, 1], c0[:, 2]]
        prev, rest = base, np.zeros_like(base)
        for ax in order:
            pos = list(pos)
            pos[ax] = c1[:, ax]
            v = T[pos[0], pos[1], pos[2]]
            rest = rest + (v - prev) * r[:, ax][:, None]
            prev = v
        t = _i32(rest + 0x8001)
        o = (base + (_i32(t + (t >> 16)) >> 16)) & 0xffff
        out[cond] = o[cond]
    return out


# ---- float stages: float64, cast where lcms2 casts --------------------------------------------------------------------------------
def _f64(v):
    with np.errstate(all="ignore"):                          # (a signalling NaN raises 'invalid' when it is widened)
        return v.astype(np.float64)


def _pow(x, e):
    with np.errstate(all="ignore"):
        return np.power(x, e)


def _inv(p):
    with np.errstate(all="ignore"):
        return np.float64(1.0) / np.float64(p)


def parametric(typ, P, R):
    """DefaultEvalParametricFn behind EvalSegmentedFn's one segment (-1e22, 1e22]: whatever is not inside it -- a NaN included -- gives
    -1e22.  R float64."""
    P = list(P) + [0.0] * (10 - len(P))
    R = np.asarray(R, dtype=np.float64)
    Rp = np.where(R >= 0, R, 0.0)                                # pow() arguments of branches that are not taken stay harmless
    zero = np.zeros_like(R)

    def posval(e, g):
        return _pow(np.where(e > 0, e, 1.0), g)
    with np.errstate(all="ignore"):
        if typ == 1:
            val = np.where(R < 0, R if abs(P[0] - 1.0) < DET_TOL else zero, _pow(Rp, P[0]))
        elif typ == -1:
            inv = F32_1E22 if abs(P[0]) < DET_TOL else _pow(Rp, _inv(P[0]))
            val = np.where(R < 0, R if abs(P[0] - 1.0) < DET_TOL else zero, inv)
        elif typ == 2:
            if abs(P[1]) < DET_TOL:
                val = zero
            else:
                e = P[1] * R + P[2]
                val = np.where((R >= -P[2] / P[1]) & (e > 0), posval(e, P[0]), 0.0)
        elif typ == -2:
            if abs(P[0]) < DET_TOL or abs(P[1]) < DET_TOL:
                val = zero
            else:
                val = np.where(R < 0, 0.0, (_pow(Rp, 1.0 / P[0]) - P[2]) / P[1])
                val = np.where(val < 0, 0.0, val)
        elif typ == 3:
            if abs(P[1]) < DET_TOL:
                val = zero
            else:
                disc = max(-P[2] / P[1], 0.0)
                e = P[1] * R + P[2]
                val = np.where(R >= disc, np.where(e > 0, posval(e, P[0]) + P[3], 0.0), P[3])
        elif typ == -3:
            if abs(P[1]) < DET_TOL:
                val = zero
            else:
                e = R - P[3]
                val = np.where(R >= P[3], np.where(e > 0, (posval(e, _inv(P[0])) - P[2]) / P[1], 0.0), -P[2] / P[1])
        elif typ == 4:
            e = P[1] * R + P[2]
            val = np.where(R >= P[4], np.where(e > 0, posval(e, P[0]), 0.0), R * P[3])
        elif typ == -4:
            e = P[1] * P[4] + P[2]
            disc = 0.0 if e < 0 else float(_pow(np.float64(e), P[0]))
            hi = zero if (abs(P[0]) < DET_TOL or abs(P[1]) < DET_TOL) else (_pow(Rp, 1.0 / P[0]) - P[2]) / P[1]
            lo = zero if abs(P[3]) < DET_TOL else R / P[3]
            val = np.where(R >= disc, hi, lo)
        elif typ == 5:
            e = P[1] * R + P[2]
            val = np.where(R >= P[4], np.where(e > 0, posval(e, P[0]) + P[5], P[5]), R * P[3] + P[6])
        elif typ == -5:
            disc = P[3] * P[4] + P[6]
            e = R - P[5]
            degenerate = abs(P[0]) < DET_TOL or abs(P[1]) < DET_TOL
            inner = zero if degenerate else (_pow(np.where(e >= 0, e, 1.0), 1.0 / P[0]) - P[2]) / P[1]
            lo = zero if abs(P[3]) < DET_TOL else (R - P[6]) / P[3]
            val = np.where(R >= disc, np.where(e < 0, 0.0, inner), lo)
        else:
            raise ValueError(typ)
        val = np.where(np.isinf(val), np.where(val > 0, F32_1E22, -F32_1E22), val)
        inside = (R > -F32_1E22) & (R <= F32_1E22)
        return np.where(inside, val, -F32_1E22)


def word_to_float(w):
    return (np.asarray(w, dtype=np.float64) / 65535.0).astype(np.float32)


def matrix_stage(m, bias, v):
    v = _f64(v)
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for i in range(3):
            t = 0.0 + v[:, 0] * m[3 * i]
            t = t + v[:, 1] * m[3 * i + 1]
            t = t + v[:, 2] * m[3 * i + 2]
            if bias is not None:
                t = t + bias[i]
            out[:, i] = t
        return out.astype(np.float32)


def lab_to_xyz(v):
    v = _f64(v)

    def f1(t):
        return np.where(t <= 24.0 / 116.0, (108.0 / 841.0) * (t - 16.0 / 116.0), t * t * t)
    with np.errstate(all="ignore"):
        L, a, b = v[:, 0] * 100.0, v[:, 1] * 255.0 - 128.0, v[:, 2] * 255.0 - 128.0
        y = (L + 16.0) / 116.0
        x, z = y + 0.002 * a, y - 0.005 * b
        out = np.stack([f1(x) * D50[0] / MAX_XYZ, f1(y) * D50[1] / MAX_XYZ, f1(z) * D50[2] / MAX_XYZ], axis=1)
        return out.astype(np.float32)


def xyz_to_lab(v):
    v = _f64(v)
    lim = (24.0 / 116.0) * (24.0 / 116.0) * (24.0 / 116.0)

    def f(t):
        return np.where(t <= lim, (841.0 / 108.0) * t + 16.0 / 116.0, _pow(np.where(t <= lim, 1.0, t), 1.0 / 3.0))     # (a NaN is not <= the limit)
    with np.errstate(all="ignore"):
        fx, fy, fz = (f(v[:, k] * MAX_XYZ / D50[k]) for k in range(3))
        L, a, b = 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)
        return np.stack([L / 100.0, (a + 128.0) / 255.0, (b + 128.0) / 255.0], axis=1).astype(np.float32)


def eval_numpy(spec, rgb):
    v = np.ascontiguousarray(rgb, dtype=np.float32).copy()
    for st in spec:
        if st[0] == "tables":
            v = np.stack([word_to_float(lin_lerp_1d(st[1][c], sat_word(v[:, c]))) for c in range(3)], axis=1)
        elif st[0] in ("param", "tail"):
            curves = [(-1, [1.0])] * 3 if st[0] == "tail" else st[1]
            with np.errstate(all="ignore"):
                v = np.stack([parametric(t, P, v[:, c].astype(np.float64)).astype(np.float32) for c, (t, P) in enumerate(curves)], axis=1)
        elif st[0] == "matrix":
            v = matrix_stage(st[1], st[2], v)
        elif st[0] == "clut":
            o = tetrahedral(st[1], np.stack([sat_word(v[:, c]) for c in range(3)], axis=1))
            v = o.astype(np.float32) / np.float32(65535.0)          # EvaluateCLUTfloatIn16's From16ToFloat: a float division
        elif st[0] == "lab2xyz":
            v = lab_to_xyz(v)
        elif st[0] == "xyz2lab":
            v = xyz_to_lab(v)
    return v


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
NAN_PATTERNS = (0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc00005, 0x7fffffff, 0x7fc00004, 0xffc00003, 0x7fc00002)
SPECIALS = np.concatenate([
    np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-39, -1e-39, 1.0 - 2.0 ** -16, 1.0 + 2.0 ** -16, 1.0, 0.5, 1e4, 1e20, -1e20, 3e38, -3e38,
              np.inf, -np.inf], dtype=np.float32),
    np.array(NAN_PATTERNS, dtype=np.uint32).view(np.float32)])


def node_words(n, which=None):
    """For an axis (or table) of n nodes: the word nearest every node (or the nodes `which`), and that word - 1 and + 1."""
    i = np.arange(n, dtype=np.int64) if which is None else np.asarray(which, dtype=np.int64)
    w = (i * 65535 + (n - 1) // 2) // (n - 1)
    return np.unique(np.clip(np.concatenate([w - 1, w, w + 1]), 0, 65535))


def fraction(n, w):
    return to_fixed_domain(np.asarray(w, dtype=np.int64) * (n - 1)) & 0xffff


def _word_with_fraction(n, want, rng):
    """For each wanted fraction a word of an n-node axis that has it (or the nearest fraction there is)."""
    fr = fraction(n, np.arange(65536))
    order = np.argsort(fr, kind="stable")
    pos = np.clip(np.searchsorted(fr[order], want), 0, 65535)
    return order[pos]


def make_inputs(axes=(17, 17, 17), count=1024 * 48, seed=1):
    """(count, 3) float32 triples for a program whose three channels meet axes of axes[k] nodes (grid points or table entries): see
    tests/test_icc32_programs.py for what they are counted to hold."""
    rng = np.random.default_rng(seed)
    parts = []
    w2f = lambda w: (np.asarray(w, dtype=np.float64) / 65535.0).astype(np.float32)
    # specials: every pair (a, b) as (a, b, a), (b, a, a) and (a, a, b)
    a, b = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    parts += [np.stack([a, b, a], 1), np.stack([b, a, a], 1), np.stack([a, a, b], 1)]
    # every node word and its neighbours on every axis, the other channels on random words; then triples of node words
    nw = [node_words(n, None if n <= 256 else np.unique(np.concatenate([[0, 1, n - 2, n - 1], rng.choice(n, 400, replace=False)]))) for n in axes]
    for k in range(3):
        for rep in range(4):
            t = rng.integers(0, 65536, size=(len(nw[k]), 3))
            t[:, k] = nw[k]
            parts.append(w2f(t))
    parts.append(w2f(np.stack([rng.choice(nw[k], 3000) for k in range(3)], 1)))
    # word 0xffff in every subset of the channels
    for mask in range(1, 8):
        t = rng.integers(0, 65536, size=(48, 3))
        for k in range(3):
            if mask >> k & 1:
                t[:, k] = 0xffff
        parts.append(w2f(t))
    # neutrals; pairwise-tied VALUES; pairwise-tied FRACTIONS (another word where the axes differ); all three fractions tied
    g = rng.integers(0, 65536, size=2000)
    parts.append(w2f(np.stack([g, g, g], 1)))
    for i, j in ((0, 1), (0, 2), (1, 2)):
        t = rng.integers(0, 65536, size=(600, 3))
        t[:, j] = t[:, i]
        parts.append(w2f(t))
        t = rng.integers(0, 65536, size=(600, 3))
        t[:, j] = _word_with_fraction(axes[j], fraction(axes[i], t[:, i]), rng)
        parts.append(w2f(t))
    t = rng.integers(0, 65536, size=(600, 3))
    for j in (1, 2):
        t[:, j] = _word_with_fraction(axes[j], fraction(axes[0], t[:, 0]), rng)
    parts.append(w2f(t))
    # random words, and the floats on either side of a word
    t = w2f(rng.integers(0, 65536, size=(6000, 3)))
    parts += [t, np.nextafter(t[:3000], np.float32(-np.inf)), np.nextafter(t[3000:], np.float32(np.inf))]
    have = sum(len(p) for p in parts)
    assert have < count - 8000, (have, count)
    u = rng.uniform(-0.25, 4.0, size=(count - have, 3)).astype(np.float32)
    u[::3] = rng.uniform(0.0, 1.0, size=u[::3].shape).astype(np.float32)
    parts.append(u)
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


# ---- seeded tables and grids --------------------------------------------------------------------------------------------------------
def seeded_table(n, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=n).astype(np.uint16)


def seeded_grid(shape, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=tuple(shape) + (3,)).astype(np.uint16)


# Sixteen windows of gain 16 show 4096 words each on the 4095 code steps of a 12-bit Clip save: one adjacent pair per window shares its
# code (and words 0 and 1 both give code 0).  Seventeen windows shifted by half a window split those pairs
# (tests/test_icc32_programs.py counts it).
MAGNIFIER_BIASES = [float(j) for j in range(16)] + [j + 0.5 for j in range(-1, 16)]


def magnifier(j):
    """The window stage: gain 16, bias -j.  Under Clip at 12 bit the words of window j land on codes of their own (all but one pair)."""
    return ("matrix", [16.0, 0, 0, 0, 16.0, 0, 0, 0, 16.0], [-float(j)] * 3)


# ---- profiles built with lcms2 (only where it is present) ---------------------------------------------------------------------------
def _sig(s):
    return int.from_bytes(s.encode(), "big")


def _lcms2_lib(L):
    """The liblcms2 the ICC oracle links (already loaded with it)."""
    C = ctypes.CDLL("liblcms2.so.2")
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for name, res, args in [("cmsCreateContext", vp, [vp, vp]), ("cmsDeleteContext", None, [vp]),
                            ("cmsCreateProfilePlaceholder", vp, [vp]), ("cmsCloseProfile", ctypes.c_int, [vp]),
                            ("cmsSetProfileVersion", None, [vp, ctypes.c_double]), ("cmsSetDeviceClass", None, [vp, u32]),
                            ("cmsSetColorSpace", None, [vp, u32]), ("cmsSetPCS", None, [vp, u32]),
                            ("cmsPipelineAlloc", vp, [vp, u32, u32]), ("cmsPipelineFree", None, [vp]),
                            ("cmsPipelineInsertStage", ctypes.c_int, [vp, ctypes.c_int, vp]),
                            ("cmsStageAllocToneCurves", vp, [vp, u32, vp]),
                            ("cmsStageAllocCLut16bit", vp, [vp, u32, u32, u32, vp]),
                            ("cmsStageAllocCLutFloat", vp, [vp, u32, u32, u32, vp]),
                            ("cmsBuildTabulatedToneCurve16", vp, [vp, u32, vp]), ("cmsFreeToneCurve", None, [vp]),
                            ("cmsWriteTag", ctypes.c_int, [vp, u32, vp]), ("cmsD50_XYZ", vp, []),
                            ("cmsSaveProfileToMem", ctypes.c_int, [vp, vp, ctypes.POINTER(u32)])]:
        fn = getattr(C, name)
        fn.restype, fn.argtypes = res, args
    return C


def lut_profile(L, tag, grid, float_clut=False, table_curves=0, twisted=None):
    """A v4 RGB display profile (PCS Lab) holding one LUT tag: [curves] -> CLUT (grid^3, 16-bit or float) -> [curves].  The CLUT maps
    device RGB to a Lab ramp so that the transform exists; table_curves > 0 makes the curves 16-bit tables of that many entries;
    twisted = a seed takes the CLUT's nodes from that generator instead of the ramp."""
    C = _lcms2_lib(L)
    ctx = C.cmsCreateContext(None, None)
    h = C.cmsCreateProfilePlaceholder(ctx)
    C.cmsSetProfileVersion(h, 4.3)
    C.cmsSetDeviceClass(h, _sig("mntr"))
    C.cmsSetColorSpace(h, _sig("RGB "))
    C.cmsSetPCS(h, _sig("Lab "))
    lut = C.cmsPipelineAlloc(ctx, 3, 3)
    g = np.linspace(0.0, 1.0, grid)
    r, gg, b = np.meshgrid(g, g, g, indexing="ij")
    lab = np.stack([0.05 + 0.9 * (0.3 * r + 0.6 * gg + 0.1 * b), 0.5 + 0.2 * (r - gg), 0.5 + 0.2 * (gg - b)], axis=-1).reshape(-1)
    if twisted is not None:
        lab = np.random.default_rng(twisted).random(lab.shape)
    curves = None
    if table_curves:
        t = np.round(np.linspace(0.0, 1.0, table_curves) ** 1.1 * 65535).astype(np.uint16)
        c = C.cmsBuildTabulatedToneCurve16(ctx, table_curves, t.ctypes.data)
        curves = (ctypes.c_void_p * 3)(c, c, c)
    if not float_clut:                                      # (a multi-process-element tag holds segmented curves only: none there)
        C.cmsPipelineInsertStage(lut, 1, C.cmsStageAllocToneCurves(ctx, 3, curves))
    if float_clut:
        tab = lab.astype(np.float32)
        clut = C.cmsStageAllocCLutFloat(ctx, grid, 3, 3, tab.ctypes.data)
    else:
        tab = np.round(lab * 65535).astype(np.uint16)
        clut = C.cmsStageAllocCLut16bit(ctx, grid, 3, 3, tab.ctypes.data)
    assert clut
    C.cmsPipelineInsertStage(lut, 1, clut)
    if not float_clut:
        C.cmsPipelineInsertStage(lut, 1, C.cmsStageAllocToneCurves(ctx, 3, None))
    assert C.cmsWriteTag(h, _sig(tag), lut) and C.cmsWriteTag(h, _sig("wtpt"), C.cmsD50_XYZ())
    if tag != "A2B0":                                       # a float LUT tag goes WITH an A2B0 (which lcms2 then ignores)
        lut16 = C.cmsPipelineAlloc(ctx, 3, 3)
        C.cmsPipelineInsertStage(lut16, 1, C.cmsStageAllocToneCurves(ctx, 3, None))
        C.cmsPipelineInsertStage(lut16, 1, C.cmsStageAllocCLut16bit(ctx, 2, 3, 3, None))
        C.cmsPipelineInsertStage(lut16, 1, C.cmsStageAllocToneCurves(ctx, 3, None))
        assert C.cmsWriteTag(h, _sig("A2B0"), lut16)
        C.cmsPipelineFree(lut16)
    n = ctypes.c_uint32(0)
    assert C.cmsSaveProfileToMem(h, None, ctypes.byref(n))
    buf = ctypes.create_string_buffer(n.value)
    assert C.cmsSaveProfileToMem(h, buf, ctypes.byref(n))
    if table_curves:
        C.cmsFreeToneCurve(c)
    C.cmsPipelineFree(lut)
    C.cmsCloseProfile(h)
    C.cmsDeleteContext(ctx)
    return buf.raw[:n.value]


# ---- the program families both test files run --------------------------------------------------------------------------------------
def _tables(counts, seed):
    return [seeded_table(n, seed + 7 * c) for c, n in enumerate(counts)]


M_PLAIN = [3.5, -2.25, -0.75, -100.0, 100.5, 0.25, 0.001, -0.002, 1.0]
M_SMALL = [0.6, 0.3, 0.1, -0.2, 1.1, 0.1, 0.05, -0.15, 1.1]
M_XYZ = [1.6, -0.4, -0.2, -0.5, 1.4, 0.1, 0.02, -0.1, 1.1]


def composition():
    """Table curves -> CLUT -> table curves -> LAB_TO_XYZ -> MATRIX -> MATRIX -> tail (the shape of a real A2B program)."""
    return [("tables", _tables((256, 1024, 33), 40), 1), ("clut", seeded_grid((9, 9, 9), 41), 3), ("tables", _tables((3, 4096, 255), 42), 0),
            ("lab2xyz",), ("matrix", M_XYZ, None), ("matrix", M_SMALL, [0.01, -0.02, 0.03]), TAIL]


def sixteen_stages():
    spec = [("tables", _tables((17, 256, 2), 50), 0), ("matrix", M_SMALL, None), ("clut", seeded_grid((5, 4, 3), 51), 1)]
    for i in range(6):
        spec += [("matrix", M_SMALL, [0.001 * i, 0.0, -0.001 * i]), ("tables", _tables((64 + i, 2 + i, 300), 52 + i), i & 1)]
    return spec + [TAIL]


def tier_a_programs():
    """{name: (spec, axes the three inputs meet first, ' lds' expected (words[] in use and at most 48 KiB), tuning word or None)}"""
    P = {}
    for name, counts, gap in (("tables 2/3/255 even and odd offsets", (2, 3, 255), 0), ("tables 256/1024/4096 gaps 1", (256, 1024, 4096), 1),
                              ("tables 4096/2/256 gaps 3", (4096, 2, 256), 3)):
        P[name] = ([("tables", _tables(counts, 10 + gap), gap), TAIL], counts, True, None)
    for shape in ((2, 2, 2), (2, 33, 3), (33, 2, 17), (9, 9, 9), (17, 17, 17)):
        P["clut %dx%dx%d" % shape] = ([("clut", seeded_grid(shape, 20 + shape[1]), 5), TAIL], shape, True, None)
    fit = [("tables", _tables((190, 190, 190), 30), 2), ("clut", seeded_grid((20, 20, 20), 31), 0)]     # 3 * 192 + 24000 words = 48 KiB
    P["clut 20^3 + tables = 49152 bytes"] = (fit + [TAIL], (190, 190, 190), True, None)
    P["clut 20^3 + tables = 49154 bytes"] = (fit + [("fill", 1), TAIL], (190, 190, 190), False, None)
    P["clut 21^3"] = ([("clut", seeded_grid((21, 21, 21), 32), 1), TAIL], (21, 21, 21), False, None)
    P["clut 33^3"] = ([("clut", seeded_grid((33, 33, 33), 33), 7), TAIL], (33, 33, 33), False, None)
    P["clut 17^3 from device memory (tuning bit 6)"] = ([("clut", seeded_grid((17, 17, 17), 34), 5), TAIL], (17, 17, 17), False, 1 | 2 | 4 | 64)
    P["matrix without bias"] = ([("matrix", M_PLAIN, None), TAIL], (17, 17, 17), False, None)
    P["matrix with bias"] = ([("matrix", M_PLAIN, [-0.5, 1e-3, 250.0]), TAIL], (17, 17, 17), False, None)
    P["lab to xyz"] = ([("lab2xyz",), TAIL], (17, 17, 17), False, None)
    # a NaN through the curve segment gives -1e22 (and only there): the gain turns that into 1.25, everything finite into ~0.25
    P["nan through the segment"] = ([("param", [(1, [1.0]), (-1, [1.0]), (1, [1.0])]), ("matrix", [-1e-22, 0, 0, 0, -1e-22, 0, 0, 0, -1e-22],
                                                                                       [0.25, 0.25, 0.25]), TAIL], (17, 17, 17), False, None)
    P["composition"] = (composition(), (256, 1024, 33), True, None)
    P["16 stages"] = (sixteen_stages(), (17, 256, 2), True, None)
    P["the tail alone"] = ([TAIL], (17, 17, 17), False, None)
    return P


MAGNIFIED = {"tables": ("tables 256/1024/4096 gaps 1", (256, 1024, 4096)), "clut": ("clut 9x9x9", (9, 9, 9))}

SRGB = [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045]
EPS = 5e-5                                                   # below lcms2's 1e-4 degeneracy bound


def tier_b_programs():
    """{name: spec}: one stage with pow() (or the cube root) in front of the tail.  Three curves per program, one per channel."""
    ordinary = [(1, [2.2]), (-1, [2.2]), (2, [2.4, 0.9, 0.1]), (-2, [2.4, 0.9, 0.1]), (3, [2.4, 0.9, 0.1, 0.05]), (-3, [2.4, 0.9, 0.1, 0.05]),
                (4, SRGB), (-4, SRGB), (5, SRGB + [0.01, 0.02]), (-5, SRGB + [0.01, 0.02]), (1, [0.45]), (-1, [0.45])]
    degenerate = [(1, [1.00005]), (1, [1.0]), (-1, [EPS]),                         # negative R with gamma ~ 1 / gamma 1; |P0| < 1e-4
                  (-1, [1.00005]), (2, [2.4, EPS, 0.1]), (2, [2.4, -0.9, 0.5]),    # |P1| < 1e-4; e <= 0 above the breakpoint
                  (-2, [EPS, 0.9, 0.1]), (-2, [2.4, EPS, 0.1]), (-2, [2.4, 0.9, 0.5]),     # ...; a negative value clamped
                  (3, [2.4, EPS, 0.1, 0.05]), (3, [2.4, -0.9, 0.5, 0.05]), (3, [2.4, 0.9, -0.3, 0.05]),   # ...; R below a positive breakpoint
                  (-3, [2.4, EPS, 0.1, 0.05]), (-3, [2.4, 0.9, 0.1, 0.5]), (-3, [-2.4, 0.9, 0.1, 0.05]),
                  (4, [2.4, -0.9, 0.5, 0.1, 0.2]), (4, [2.4, 0.9, 0.1, 0.1, 0.6]), (-4, [EPS, 0.9, 0.1, 0.1, 0.2]),
                  (-4, [2.4, EPS, 0.1, 0.1, 0.2]), (-4, [2.4, 0.9, 0.1, EPS, 0.2]), (-4, [2.4, 0.9, -0.5, 0.1, 0.2]),
                  (5, [2.4, -0.9, 0.5, 0.1, 0.2, 0.01, 0.02]), (5, [2.4, 0.9, 0.1, 0.1, 0.6, 0.01, 0.02]), (-5, [EPS, 0.9, 0.1, 0.1, 0.2, 0.01, 0.02]),
                  (-5, [2.4, EPS, 0.1, 0.1, 0.2, 0.01, 0.02]), (-5, [2.4, 0.9, 0.1, EPS, 0.2, 0.01, 0.02]), (-5, [2.4, 0.9, 0.1, 0.1, 0.2, 0.3, 0.02])]
    P = {}
    for kind, curves in (("ordinary", ordinary), ("degenerate", degenerate)):
        for i in range(0, len(curves), 3):
            three = curves[i:i + 3]
            P["%s %s" % (kind, " ".join("%+d" % t for t, _ in three))] = [("param", three), TAIL]
    P["xyz to lab"] = [("xyz2lab",), TAIL]
    return P


def tier_c_program():
    """Parametric A-curves -> twisted CLUT -> tail: (the whole spec, the curve stage alone)."""
    curves = ("param", [(4, SRGB), (1, [2.2]), (3, [2.4, 0.9, 0.1, 0.0])])
    return [curves, ("clut", seeded_grid((9, 9, 9), 60), 0), TAIL], [curves]


def neighbours(h):
    h = np.asarray(h, dtype=np.float32)
    return np.nextafter(h, np.float32(-np.inf)), np.nextafter(h, np.float32(np.inf))
