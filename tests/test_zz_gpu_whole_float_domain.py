"""The float-tier save curves held to float64 truth on EVERY float32, and to the oracle on every float between the first non-zero code
and saturation.

A write curve is a function of one float and there are 2^32 of them; tests/test_gpu_t2_truth.py sweeps 900 000.  Here, per curve case
(PQ close at 80 / 1000 / 10 000 nits x 10 / 12 bit, PQ compact, HLG, SMPTE 428, Clip) and for BOTH evaluations -- the scalar one of the
generic write_px (tuning word 0) and the packed one of write_f32_ref_stream, each asserted from the launch label:

  all 2^32 patterns (no oracle)   every non-negative finite float's code lies in [floor(T (1 - rel) - abs), floor(T (1 + rel) + abs)],
                                  T = clip(curve64(x) * max), the bands of tests/truth64.py unchanged (Clip: equality with
                                  trunc(clamp(x * maxf, 0, maxf)) in float32); negative floats and -0 give 0; every NaN pattern gives 0;
                                  +-Inf give a code in [0, max]; the places where the code falls as the float rises are counted
                                  (asserted zero for the forms of MONOTONE, where the enumeration found none)
  the window (against the oracle) |code - oracle| <= 1 on every float of the whole binades between "code still 0" and "saturated"
                                  (tests/exhaustive_floats.py: window); Clip equals the oracle; outside the window every 251st
                                  finite pattern equals the oracle.  Exact rates (pooled, worst binade) are recorded, not barred: a
                                  uniform walk over floats is not the distribution the bars of DESIGN section 4 were measured on.
  same bits from every form       on the window, the codes of write_px equal those of write_rgb32_ycbcr444_hot (both lane widths) and
                                  write_rgba32_ycbcra444_hot (alpha 1) under the GBR matrix (planes = stage-A codes), of
                                  write_f32_ref_stream on the source shifted by one float (every float in another channel slot), of the
                                  gray save (PQ and Clip; source clamped to [0, 1], WriteHeifImage.cpp:602), and the bins of
                                  write_hist_px equal the bincount of the per-pixel maximum of those codes.
                                  LEFT OUT: write_rgb32_ycbcr_sub_hot (4:2:2 nearest) -- the library refuses a GBR save that is not
                                  4:4:4 ("identity (GBR) matrix requires 4:4:4"), so the dispatcher offers no such kernel whose planes
                                  are the stage-A codes.  write_hist_px is launched by avifgpu_probe_histogram (twin 0), which is that
                                  kernel's own entry point and writes no launch label.
  alpha                           every float as straight alpha of an RGBA and of a gray + alpha save (write_rgba32_ycbcra444_hot,
                                  write_ga_stream, write_px): trunc(clamp(a, 0, 1) * max) for every non-NaN float, the oracle's plane on
                                  [2^-13, 2); a NaN alpha gives a code in [0, max] (no rule beyond the range exists for it).

Sources are generated on the device (tests/exhaustive_floats.py; tests/test_exhaustive_floats.py holds the numpy and the torch
generators to the same bits) in chunks of 2^26 floats, the float64 truth is computed there in slices of 2^24, the oracle's codes are
uploaded group by group.  With AVIFGPU_FLOAT_DOMAIN_RECORD=<directory> every test appends what it measured (band needed, per-binade
exact rates, descents, +-Inf codes, SHA-256 of the window's code sequence) to text files there: profiles/float_domain/ was written so.
The file is named to be collected after tests/test_zz_gpu_whole_domain_write.py: every earlier GPU test keeps its place.
"""
import ctypes
import hashlib
import os
import time

import numpy as np
import pytest

import exhaustive_floats as xf
import harness
import truth64

pkg = harness.pkg
pytestmark = pytest.mark.gpu

PQ, HLG, S428, CLIP = pkg.TRANSFER_PQ, pkg.TRANSFER_HLG, pkg.TRANSFER_SMPTE428, pkg.TRANSFER_CLIP
DEFAULT_VARIANT = 1 | 2 | 4
STREAMING = 1 | 2 | 4 | 8
STREAMING_PXL4 = 1 | 4 | 8          # bit 1 clear: write_rgb32_ycbcr444_hot with 4 pixels per lane
GENERIC = 0
GBR = dict(matrix_coefficients=pkg.MATRIX_RGB_GBR, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444)
SLICE = 1 << 24
FILL = 0x5A5A                       # what an output sample holds before the kernel writes it: above every code
RECORD = os.environ.get("AVIFGPU_FLOAT_DOMAIN_RECORD")

CASES = [(f"pq{peak}-close-b{bits}", PQ, peak, bits, pkg.PQ_AUTO) for peak in (80, 1000, 10000) for bits in (10, 12)]
CASES += [(f"pq{peak}-compact-b{bits}", PQ, peak, bits, pkg.PQ_COMPACT) for peak, bits in ((80, 10), (80, 12), (10000, 12))]
CASES += [(f"{name}-b{bits}", tr, 80, bits, pkg.PQ_AUTO) for name, tr in (("hlg", HLG), ("smpte428", S428), ("clip", CLIP)) for bits in (10, 12)]
FORMS = (("write_px", GENERIC), ("write_f32_ref_stream", STREAMING))

# (case, form) whose code sequence the enumeration found non-decreasing over ALL non-negative finite floats: asserted from now on
# (profiles/float_domain/README.md holds the counts of the others).
MONOTONE = {(f"{name}-b{bits}", form) for name in ("hlg", "smpte428", "clip") for bits in (10, 12) for form, _ in FORMS}


def _record(name, lines):
    for line in lines:
        print(line)
    if RECORD:
        os.makedirs(RECORD, exist_ok=True)
        with open(os.path.join(RECORD, name + ".txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


def _dev(gpu):
    return f"cuda:{gpu.device}"


def _save(gpu, d, src, word, kernel):
    """A device document through avifgpu_write_rows under the tuning word `word`; the launch label must begin with `kernel`.
    Returns {plane: (rows, samples) int16 device tensor} -- codes are at most 4095, FILL marks a sample nothing wrote."""
    import torch
    dev = _dev(gpu)
    out = {pl: torch.full((max((d.height + ys) >> ys, 1), w), FILL, dtype=torch.int16, device=dev) for pl, (w, xs, ys) in harness.write_planes(d).items()}
    ptrs = [out[i].data_ptr() if i in out else None for i in range(4)]
    strides = [out[i].stride(0) * 2 if i in out else 0 for i in range(4)]
    gpu.lib.avifgpu_set_hot_variant(word)
    try:
        gpu.write_rows(d, 0, d.height, src.data_ptr(), src.stride(0) * 4, ptrs, strides, mem=pkg.MEM_DEVICE,
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    finally:
        gpu.lib.avifgpu_set_hot_variant(DEFAULT_VARIANT)
    label = gpu.last_kernel()
    begin, part = kernel if isinstance(kernel, tuple) else (kernel, "")
    assert label.startswith(begin + "<") and part in label, (label, kernel)
    return out


def _codes(gpu, d, src, word, kernel, count, shift=0):
    """The first `count` codes (behind `shift`) of the hand-off plane, int32."""
    import torch
    return _save(gpu, d, src, word, kernel)[0].reshape(-1)[shift:shift + count].to(torch.int32)


def _desc(case, rows, **kw):
    _, tr, peak, bits, ev = case
    return xf.document_desc(rows, bits, tr, peak, ev, **kw)


def _tag(case, form="write_f32_ref_stream"):
    """The transfer a launch label shows: the descriptor's, except that write_px names its template argument, which is 4 for the
    close PQ evaluation (kTransferPqHi, csrc/write_kernels.hip) -- so the label also tells the two PQ evaluations apart."""
    _, tr, _, _, ev = case
    return f"transfer={4 if form == 'write_px' and tr == PQ and ev != pkg.PQ_COMPACT else tr}"


def _floats(bits):
    """The floats of a tensor of bit patterns, for messages."""
    return [float(v) for v in np.asarray(bits, dtype=np.int64).astype(np.uint32).view(np.float32)]


# ---- all 2^32 patterns against float64 truth -------------------------------------------------------------------------------------------
class _Tally:
    """What one form accumulates over the patterns, all on the device: nothing is read back before the walk is over."""

    def __init__(self, dev):
        import torch
        z = lambda dt=torch.int64: torch.zeros((), dtype=dt, device=dev)
        self.outside, self.neg_nonzero, self.nan_nonzero, self.descents, self.max_fall = z(), z(), z(), z(), z()
        self.need, self.need_bits, self.worst_bits = z(torch.float64), z(), torch.full((), -1, dtype=torch.int64, device=dev)
        self.last = z(torch.int32)
        self.inf = {}


def _walk_nonneg(case, d, x, first, codes, tallies):
    """Non-negative finite floats x (patterns first ..) and each form's codes: the truth interval, the band needed, the descents."""
    import torch
    tr = case[1]
    for s in range(0, x.shape[0], SLICE):
        xs = x[s:s + SLICE]
        if tr == CLIP:
            want = xf.clip_codes(xs, d.bit_depth)
        else:
            t = xf.truth_codes(d, xs)
            lo, hi = xf.truth_interval(d, xs, t)
        for name, c in codes.items():
            ty, cs = tallies[name], c[s:s + SLICE]
            if tr == CLIP:
                bad = cs != want
            else:
                cf = cs.to(torch.float64)
                bad = (cf < lo) | (cf > hi)
                need = xf.band_needed(d, xs, cs, t)
                m, i = need.max(0)
                better = m > ty.need
                ty.need = torch.where(better, m, ty.need)
                ty.need_bits = torch.where(better, i + (first + s), ty.need_bits)
            nbad = bad.sum()
            ty.worst_bits = torch.where((ty.worst_bits < 0) & (nbad > 0), bad.to(torch.int8).argmax() + (first + s), ty.worst_bits)
            ty.outside += nbad
            seq = torch.cat([ty.last.reshape(1), cs])
            fall = seq[:-1] - seq[1:]
            ty.descents += (fall > 0).sum()
            ty.max_fall = torch.maximum(ty.max_fall, fall.max().to(torch.int64))
            ty.last = cs[-1].clone()
        del xs


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_float32_pattern_against_float64_truth(gpu, case):
    import torch
    dev = _dev(gpu)
    name, tr, peak, bits, ev = case
    maxv = (1 << bits) - 1
    tallies = {form: _Tally(dev) for form, _ in FORMS}
    t0 = time.perf_counter()
    for first, count in xf.chunks():
        src = xf.document(first, count, device=dev)
        d = _desc(case, src.shape[0])
        codes = {form: _codes(gpu, d, src, word, (form, _tag(case, form) + ","), count) for form, word in FORMS}
        x = src.reshape(-1)[:count]
        end = first + count
        fin = min(end, xf.INF_BITS)
        if first < fin:                                                     # +0 and the positive finite floats, in float order
            _walk_nonneg(case, d, x[:fin - first], first, {k: c[:fin - first] for k, c in codes.items()}, tallies)
        for form, c in codes.items():
            ty = tallies[form]
            if first <= xf.INF_BITS < end:                                   # +Inf, then the positive NaNs
                ty.inf["+inf"] = c[xf.INF_BITS - first]
                ty.nan_nonzero += (c[xf.INF_BITS + 1 - first:] != 0).sum()
            if first >= xf.NEG_ZERO_BITS:                                    # -0 and the negative finite floats, -Inf, the negative NaNs
                nfin = min(end, xf.NEG_INF_BITS) - first
                ty.neg_nonzero += (c[:nfin] != 0).sum()
                if first <= xf.NEG_INF_BITS < end:
                    ty.inf["-inf"] = c[xf.NEG_INF_BITS - first]
                    ty.nan_nonzero += (c[xf.NEG_INF_BITS + 1 - first:] != 0).sum()
        del src, codes, x
    torch.cuda.synchronize(dev)
    seconds = time.perf_counter() - t0
    lines, failures = [], []
    for form, _ in FORMS:
        ty = tallies[form]
        inf = {k: int(v) for k, v in ty.inf.items()}
        need, need_at = float(ty.need), _floats([int(ty.need_bits)])[0]
        descents, max_fall = int(ty.descents), int(ty.max_fall)
        lines.append(f"{name} {form}: all 2^32 patterns: outside the truth interval {int(ty.outside)}; relative band needed {need:.3e} at {need_at!r}; "
                     f"descents over the non-negative finite floats {descents}, largest fall {max(max_fall, 0)}; negative floats with a non-zero code "
                     f"{int(ty.neg_nonzero)}; NaN patterns with a non-zero code {int(ty.nan_nonzero)}; +Inf -> {inf['+inf']}, -Inf -> {inf['-inf']}")
        if int(ty.outside):
            w = int(ty.worst_bits)
            failures.append(f"{form}: {int(ty.outside)} floats outside the truth interval, the first is pattern {w:#x} = {_floats([w])[0]!r}")
        if int(ty.neg_nonzero) or int(ty.nan_nonzero):
            failures.append(f"{form}: {int(ty.neg_nonzero)} negative floats and {int(ty.nan_nonzero)} NaN patterns with a non-zero code")
        if not all(0 <= v <= maxv for v in inf.values()):
            failures.append(f"{form}: +-Inf out of range: {inf}")
        if tr != CLIP and need > truth64.band_rel(d):
            failures.append(f"{form}: needs a relative band of {need:.3e} at {need_at!r}")
        if (name, form) in MONOTONE and descents:
            failures.append(f"{form}: {descents} descents (largest {max_fall}) where the enumeration had found none")
    lines.append(f"{name}: {seconds:.2f} s")
    _record("all_patterns", lines)
    assert not failures, failures


# ---- the window against the oracle ---------------------------------------------------------------------------------------------------------
def _oracle_codes(d, src_np, count, dev):
    import torch
    plane = np.ascontiguousarray(xf.oracle_planes(d, src_np)[0]).reshape(-1)[:count]
    return torch.from_numpy(plane.view(np.int16)).to(dev).to(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_float_of_the_window_against_the_oracle(gpu, case):
    import torch
    dev = _dev(gpu)
    name, tr, peak, bits, ev = case
    e0, e1 = xf.window(_desc(case, 1))
    t0 = time.perf_counter()
    t_oracle = 0.0
    far = {form: torch.zeros((), dtype=torch.int64, device=dev) for form, _ in FORMS}
    first_far = {form: torch.full((), -1, dtype=torch.int64, device=dev) for form, _ in FORMS}
    exact = {form: [] for form, _ in FORMS}
    sha = {form: hashlib.sha256() for form, _ in FORMS}
    for first, count, e in xf.window_groups(e0, e1):
        src_np = xf.document(first, count)
        d = _desc(case, src_np.shape[0])
        t1 = time.perf_counter()
        want = _oracle_codes(d, src_np, count, dev)
        t_oracle += time.perf_counter() - t1
        del src_np
        src = xf.document(first, count, device=dev)
        for form, word in FORMS:
            got = _codes(gpu, d, src, word, (form, _tag(case, form) + ","), count)
            diff = (got - want).abs()
            nfar = (diff > 1).sum()
            first_far[form] = torch.where((first_far[form] < 0) & (nfar > 0), (diff > 1).to(torch.int8).argmax() + first, first_far[form])
            far[form] += nfar
            exact[form].append((diff == 0).reshape(-1, xf.BINADE).sum(1))
            if RECORD:
                sha[form].update(got.to(torch.int16).cpu().numpy().tobytes())
        del src, want
    # outside the window: every 251st pattern, finite ones only, must equal the oracle
    skip = (xf.binade_first(e0), (e1 - e0) * xf.BINADE)
    vals_np, vals = xf.sparse_patterns(251, *skip), xf.sparse_patterns(251, *skip, device=dev)
    n = vals_np.shape[0]
    assert n == vals.shape[0] and n > 15_000_000
    src_np = xf.document_of(vals_np)
    d = _desc(case, src_np.shape[0])
    want = _oracle_codes(d, src_np, n, dev)
    src = xf.document_of(vals)
    outside = {form: int((_codes(gpu, d, src, word, (form, _tag(case, form) + ","), n) != want).sum()) for form, word in FORMS}
    seconds = time.perf_counter() - t0
    lines, failures = [], []
    for form, _ in FORMS:
        per = torch.cat(exact[form]).cpu().numpy().astype(np.float64) / xf.BINADE
        worst = int(per.argmin())
        pooled = float(per.mean())
        lines.append(f"{name} {form}: window [2^{e0}, 2^{e1}), {(e1 - e0) * xf.BINADE} floats: more than one code from the oracle {int(far[form])}; exact "
                     f"pooled {pooled:.6f}, worst binade 2^{e0 + worst} {per[worst]:.6f}; outside the window {outside[form]} of {n} sampled floats differ"
                     + (f"; sha256 {sha[form].hexdigest()}" if RECORD else ""))
        lines.append(f"{name} {form}: exact rate per binade from 2^{e0}: " + " ".join(f"{v:.5f}" for v in per))
        if int(far[form]):
            w = int(first_far[form])
            failures.append(f"{form}: {int(far[form])} floats more than one code from the oracle, the first is pattern {w:#x} = {_floats([w])[0]!r}")
        if tr == CLIP and pooled != 1.0:
            failures.append(f"{form}: Clip differs from the oracle (exact {pooled:.9f})")
        if outside[form]:
            failures.append(f"{form}: {outside[form]} sampled floats outside the window differ from the oracle")
    lines.append(f"{name}: {seconds:.2f} s, {t_oracle:.2f} s of them the oracle")
    _record("window", lines)
    assert not failures, failures


# ---- same bits from every form --------------------------------------------------------------------------------------------------------------
SAME_BITS = [c for c in CASES if c[0] in ("pq80-close-b12", "hlg-b10", "smpte428-b12")]


def _with_alpha_one(src):
    """The planes = 3 document as a planes = 4 one with alpha 1."""
    import torch
    px = src.reshape(-1, 3)
    return torch.cat([px, torch.ones((px.shape[0], 1), dtype=torch.float32, device=src.device)], 1).reshape(src.shape[0], xf.WIDTH * 4)


def _probe_hist(gpu, d, src):
    import torch
    dev = _dev(gpu)
    bins = torch.zeros(1 << d.bit_depth, dtype=torch.int64, device=dev)
    rc = gpu.lib.avifgpu_probe_histogram(ctypes.byref(d), 0, src.data_ptr(), src.stride(0) * 4, bins.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, gpu.lib.avifgpu_last_error().decode()
    return bins


@pytest.mark.parametrize("case", SAME_BITS, ids=[c[0] for c in SAME_BITS])
def test_every_form_gives_the_same_bits_on_the_window(gpu, case):
    import torch
    dev = _dev(gpu)
    name, tr, peak, bits, ev = case
    e0, e1 = xf.window(_desc(case, 1))
    tag, tag_px = _tag(case), _tag(case, "write_px") + ","
    differ = {}
    t0 = time.perf_counter()

    def judge(what, got, ref, first):
        n = int((got != ref).sum())
        if n and what not in differ:
            differ[what] = (n, hex(int((got != ref).to(torch.int8).argmax()) + first))
        elif n:
            differ[what] = (differ[what][0] + n, differ[what][1])

    for first, count, e in xf.window_groups(e0, e1):
        src = xf.document(first, count, device=dev)
        rows = src.shape[0]
        d = _desc(case, rows)
        ref_plane = _save(gpu, d, src, GENERIC, ("write_px", tag_px))[0]
        ref = ref_plane.reshape(-1, 3)                                      # every pixel of the document, the +0 tail included
        for word, part in ((STREAMING, "pxl=8"), (STREAMING_PXL4, "pxl=4")):
            got = _save(gpu, _desc(case, rows, **GBR), src, word, ("write_rgb32_ycbcr444_hot", part))
            for pl, ch in ((0, 1), (1, 2), (2, 0)):                          # Y <- G, Cb <- B, Cr <- R
                judge(f"write_rgb32_ycbcr444_hot {part} plane {pl}", got[pl].reshape(-1), ref[:, ch], first)
            del got
        got = _save(gpu, _desc(case, rows, planes=4, **GBR), _with_alpha_one(src), STREAMING, ("write_rgba32_ycbcra444_hot", tag))
        for pl, ch in ((0, 1), (1, 2), (2, 0)):
            judge(f"write_rgba32_ycbcra444_hot plane {pl}", got[pl].reshape(-1), ref[:, ch], first)
        assert bool((got[3] == (1 << bits) - 1).all())
        del got
        shifted = xf.document(first, count, shift=1, device=dev)
        got = _save(gpu, _desc(case, shifted.shape[0]), shifted, STREAMING, ("write_f32_ref_stream", tag + ","))[0].reshape(-1)
        judge("write_f32_ref_stream, shifted by one float", got[1:1 + count], ref_plane.reshape(-1)[:count], first)
        del got, shifted
        bins = _probe_hist(gpu, d, src)
        want = torch.bincount(ref.max(1).values.to(torch.int64), minlength=1 << bits)
        assert torch.equal(bins, want), (name, "write_hist_px", hex(first), int((bins != want).sum()))
        if tr == PQ:                                                        # gray saves: PQ or Clip
            gsrc = xf.gray_document(first, count, device=dev)
            dg = _desc(case, gsrc.shape[0], planes=1)
            csrc = xf.document_of(gsrc.reshape(-1)[:count].clamp(0.0, 1.0))
            cref = _codes(gpu, _desc(case, csrc.shape[0]), csrc, GENERIC, ("write_px", tag_px), count)
            for word, kernel in ((STREAMING, ("write_f32_ref_stream", "planes=1")), (GENERIC, ("write_px", "planes=1,"))):
                judge(f"gray {kernel[0]}", _codes(gpu, dg, gsrc, word, kernel, count), cref, first)
            del gsrc, csrc, cref
        del src, ref, ref_plane
    _record("same_bits", [f"{name}: window [2^{e0}, 2^{e1}): forms that differ from write_px: {differ or 'none'}; {time.perf_counter() - t0:.2f} s"])
    assert not differ, differ


@pytest.mark.parametrize("bits", [10, 12])
def test_clip_gray_save_gives_the_same_bits_on_the_window(gpu, bits):
    """The gray save under Clip: write_f32_ref_stream<planes=1> and write_px<planes=1> against write_px of the RGB document."""
    case = (f"clip-b{bits}", CLIP, 80, bits, pkg.PQ_AUTO)
    e0, e1 = xf.window(_desc(case, 1))
    t0 = time.perf_counter()
    for first, count, e in xf.window_groups(e0, e1):
        gsrc = xf.gray_document(first, count, device=_dev(gpu))
        csrc = xf.document_of(gsrc.reshape(-1)[:count].clamp(0.0, 1.0))
        cref = _codes(gpu, _desc(case, csrc.shape[0]), csrc, GENERIC, ("write_px", f"transfer={CLIP},"), count)
        for word, kernel in ((STREAMING, ("write_f32_ref_stream", "planes=1")), (GENERIC, ("write_px", "planes=1,"))):
            got = _codes(gpu, _desc(case, gsrc.shape[0], planes=1), gsrc, word, kernel, count)
            assert bool((got == cref).all()), (kernel, hex(first), int((got != cref).sum()))
    _record("same_bits", [f"clip-b{bits} gray save: window [2^{e0}, 2^{e1}): both gray kernels equal write_px of the RGB document; {time.perf_counter() - t0:.3f} s"])


# ---- alpha: every float as straight alpha ---------------------------------------------------------------------------------------------------
ALPHA_FORMS = (("rgba", 4, GBR, STREAMING, "write_rgba32_ycbcra444_hot"), ("rgba", 4, GBR, GENERIC, "write_px"),
               ("gray+alpha", 2, {}, STREAMING, "write_ga_stream"), ("gray+alpha", 2, {}, GENERIC, "write_px"))


@pytest.mark.parametrize("tr,bits", [(PQ, 12), (CLIP, 10)], ids=["pq-b12", "clip-b10"])
def test_every_float32_pattern_as_straight_alpha(gpu, tr, bits):
    import torch
    dev = _dev(gpu)
    maxv = (1 << bits) - 1
    case = ("alpha", tr, 80, bits, pkg.PQ_AUTO)
    wrong = {f"{doc} {kernel}": 0 for doc, _, _, _, kernel in ALPHA_FORMS}
    nan_codes = {k: set() for k in wrong}
    t0 = time.perf_counter()
    lo_w, hi_w = xf.binade_first(-13), xf.binade_first(1)
    for first, count in xf.chunks():
        a = xf.patterns(first, count, device=dev)
        nan = torch.isnan(a)
        want = torch.where(nan, torch.zeros((), dtype=torch.int64, device=dev), xf.alpha_codes(a, bits)).to(torch.int16)
        in_window = lo_w < first + count and first < hi_w
        for planes in (4, 2):
            src = xf.pair_document(first, count, planes, device=dev)
            rows = src.shape[0]
            for doc, pl, kw, word, kernel in ALPHA_FORMS:
                if pl != planes:
                    continue
                d = _desc(case, rows, planes=planes, **kw)
                got = _save(gpu, d, src, word, kernel)[3].reshape(-1)[:count]
                key = f"{doc} {kernel}"
                wrong[key] += int(((got != want) & ~nan).sum())
                if bool(nan.any()):
                    nan_codes[key] |= set(int(v) for v in torch.unique(got[nan]).cpu())
            if in_window and planes == 2:                                    # the oracle's alpha plane on [2^-13, 2): the chunks that hold it
                orc = np.ascontiguousarray(xf.oracle_planes(_desc(case, rows, planes=2), xf.pair_document(first, count, 2))[3]).reshape(-1)[:count]
                s0, s1 = max(lo_w - first, 0), min(hi_w - first, count)
                assert torch.equal(torch.from_numpy(orc.view(np.int16)).to(dev)[s0:s1], want[s0:s1]), hex(first)
            del src
        del a, want, nan
    _record("alpha", [f"alpha {('clip', 'pq')[tr == PQ]} {bits} bit: floats whose alpha code is not trunc(clamp(a, 0, 1) * max): {wrong}; "
                      f"codes of NaN alphas: {({k: sorted(v) for k, v in nan_codes.items()})}; {time.perf_counter() - t0:.2f} s"])
    assert not any(wrong.values()), wrong
    assert all(0 <= c <= maxv for v in nan_codes.values() for c in v), nan_codes
