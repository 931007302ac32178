"""The box-average thumbnail of a save, the host side (include/avifgpu.h "thumbnail of a save"): avifgpu_thumbnail_from_sums against a
numpy restatement of its definition, avifgpu_thumbnail_fit enumerated against a Python restatement, arming and disarming without a
device.  CPU only: none of these calls touches a device.  box_sums / thumb_codes are the reference the GPU tests use too."""
import ctypes

import numpy as np
import pytest

import harness

pkg = harness.pkg

CHROMAS = (pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420)


# ---- the reference: integer sums over planes with the cell rule, and the rounded mean --------------------------------------------------
def channels(desc, planes):
    """[(plane index, 2-D array of one channel)] of trimmed write planes, in the sums' channel order R,G,B[,A] | Y[,A] | Y,Cb,Cr[,A]."""
    if desc.output == pkg.OUT_REFERENCE and desc.planes >= 3:
        p0 = planes[0]
        return [(0, p0.reshape(p0.shape[0], -1, desc.planes)[..., c]) for c in range(desc.planes)]
    if desc.output == pkg.OUT_REFERENCE:
        return [(0, planes[0])] + ([(3, planes[3])] if desc.planes == 2 else [])
    return [(c, planes[c]) for c in range(desc.planes)]


def cell_index(n, t):
    return (np.arange(n, dtype=np.int64) * t) // n


def box_sums(planes, desc, tw, th):
    """sums[ty, tx, c] = sum of the codes of channel c whose sample (x, y) has floor(x tw / pw) == tx and floor(y th / ph) == ty."""
    sums = np.zeros((th, tw, desc.planes), dtype=np.int64)
    for c, (_, a) in enumerate(channels(desc, planes)):
        ph, pw = a.shape
        np.add.at(sums[:, :, c], (cell_index(ph, th)[:, None], cell_index(pw, tw)[None, :]), a.astype(np.int64))
    return sums


def channel_sizes(desc):
    xs, ys = harness.chroma_shift(desc.chroma) if desc.output == pkg.OUT_YCBCR else (0, 0)
    out = []
    for c in range(desc.planes):
        chroma = desc.output == pkg.OUT_YCBCR and c in (1, 2)
        out.append(((desc.width + xs) >> xs, (desc.height + ys) >> ys) if chroma else (desc.width, desc.height))
    return out


def cell_counts(desc, tw, th):
    """n[ty, tx, c]: the samples of each cell, COUNTED (the library takes them from the ceil formula)."""
    n = np.zeros((th, tw, desc.planes), dtype=np.int64)
    for c, (pw, ph) in enumerate(channel_sizes(desc)):
        n[:, :, c] = np.bincount(cell_index(ph, th), minlength=th)[:, None] * np.bincount(cell_index(pw, tw), minlength=tw)[None, :]
    return n


def thumb_codes(sums, desc, tw, th):
    """{plane: array} of floor((2 sum + n) / (2 n)) in the form of the main output (YCBCR: every plane tw x th)."""
    n = cell_counts(desc, tw, th)
    code = (2 * sums.astype(np.int64).reshape(th, tw, desc.planes) + n) // (2 * n)
    dt = np.uint16 if desc.bit_depth > 8 else np.uint8
    if desc.output == pkg.OUT_REFERENCE and desc.planes >= 3:
        return {0: code.reshape(th, tw * desc.planes).astype(dt)}
    if desc.output == pkg.OUT_REFERENCE:
        out = {0: code[:, :, 0].astype(dt)}
        if desc.planes == 2:
            out[3] = code[:, :, 1].astype(dt)
        return out
    return {c: code[:, :, c].astype(dt) for c in range(desc.planes)}


def make_desc(width, height, planes, bits, output=pkg.OUT_REFERENCE, chroma=pkg.CHROMA_444, depth=16, alpha=None, **kw):
    if alpha is None:
        alpha = pkg.ALPHA_STRAIGHT if planes in (2, 4) else pkg.ALPHA_NONE
    return pkg.WriteDesc(width=width, height=height, depth=depth, planes=planes, bit_depth=bits, alpha_state=alpha,
                         output=output if planes >= 3 else pkg.OUT_REFERENCE, chroma=chroma, **kw)


# ---- 1. avifgpu_thumbnail_from_sums -----------------------------------------------------------------------------------------------------
def _from_sums_cases():
    out = []
    for planes in (1, 2, 3, 4):
        for bits in (8, 10, 12):
            outs = [(pkg.OUT_REFERENCE, pkg.CHROMA_444)]
            if planes >= 3:
                outs += [(pkg.OUT_YCBCR, c) for c in CHROMAS]
            for output, chroma in outs:
                out.append((planes, bits, output, chroma))
    return out


@pytest.mark.parametrize("planes,bits,output,chroma", _from_sums_cases())
def test_from_sums_is_the_rounded_mean(planes, bits, output, chroma):
    rng = np.random.default_rng(planes * 100 + bits + chroma)
    maxcode = (1 << bits) - 1
    for (w, h) in ((97, 41), (41, 97), (16384, 3)):
        d = make_desc(w, h, planes, bits, output, chroma)
        mw, mh = min(s[0] for s in channel_sizes(d)), min(s[1] for s in channel_sizes(d))
        for tw, th in ((13, 7), (7, 13), (1, 1), (mw, mh), (mw, 1), (1, mh)):
            tw, th = min(tw, mw, 1024), min(th, mh, 1024)
            n = cell_counts(d, tw, th)
            assert n.min() >= 1
            for c, (pw, ph) in enumerate(channel_sizes(d)):
                assert int(n[:, :, c].sum()) == pw * ph
            sums = (rng.integers(0, maxcode + 1, size=n.shape, dtype=np.int64) * n)                     # means that are codes ...
            frac = rng.integers(0, n + 1, size=n.shape, dtype=np.int64)                                  # ... and everything between, up to n * maxcode
            sums = np.minimum(sums + frac, n * maxcode)
            sums[0, 0, :] = n[0, 0, :] * maxcode
            sums[-1, -1, :] = 0
            flat = np.ascontiguousarray(sums.reshape(-1)).astype(np.uint64)
            want = thumb_codes(sums, d, tw, th)
            for pad in (0, 3):
                got = pkg.thumbnail_from_sums(d, tw, th, flat, stride_pad=pad)
                assert sorted(got) == sorted(want)
                for pl in want:
                    ncol = want[pl].shape[1]
                    assert got[pl].dtype == want[pl].dtype
                    assert np.array_equal(got[pl][:, :ncol], want[pl]), (w, h, tw, th, pl, pad)
                    assert (got[pl][:, ncol:] == (0xA5A5 if bits > 8 else 0xA5)).all()                   # the padding is left alone
            if tw == mw and th == mh and output == pkg.OUT_REFERENCE:                                   # identity: the codes are the sums
                assert (n == 1).all()


def test_from_sums_rounds_half_up_and_refuses_a_sum_out_of_range():
    d = make_desc(4, 2, 1, 10)
    # one cell of 8 samples: floor((2 S + 8) / 16)
    for s, want in ((0, 0), (3, 0), (4, 1), (11, 1), (12, 2), (8 * 1023, 1023), (8 * 1023 - 4, 1023), (8 * 1023 - 5, 1022)):
        got = pkg.thumbnail_from_sums(d, 1, 1, np.array([s], dtype=np.uint64))
        assert int(got[0][0, 0]) == want, (s, want)
    with pytest.raises(pkg.AvifGpuError) as e:
        pkg.thumbnail_from_sums(d, 1, 1, np.array([8 * 1023 + 1], dtype=np.uint64))
    assert e.value.code == pkg.formatBadParameters and "exactly once" in e.value.message
    # a frame fed twice is caught in whichever cell it shows, and then nothing is written
    d3 = make_desc(97, 41, 3, 8, pkg.OUT_YCBCR, pkg.CHROMA_420)
    n = cell_counts(d3, 13, 7)
    sums = (n * 255).astype(np.uint64)
    assert pkg.thumbnail_from_sums(d3, 13, 7, sums.reshape(-1))[1].min() == 255
    sums[6, 12, 2] += 1
    lib = pkg.load()
    bufs = [np.full((7, 13), 0xA5, dtype=np.uint8) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 4)(*[b.ctypes.data for b in bufs], None)
    strides = (ctypes.c_int64 * 4)(13, 13, 13, 0)
    rc = lib.avifgpu_thumbnail_from_sums(ctypes.byref(d3), 13, 7, sums.ctypes.data, ctypes.byref(ptrs), ctypes.byref(strides))
    assert rc == pkg.formatBadParameters
    assert all((b == 0xA5).all() for b in bufs)


def test_from_sums_argument_errors():
    lib = pkg.load()
    d = make_desc(97, 41, 3, 8, pkg.OUT_YCBCR, pkg.CHROMA_420)
    sums = np.zeros(49 * 21 * 3 + 16, dtype=np.uint64)
    bufs = [np.zeros((64, 128), dtype=np.uint8) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 4)(*[b.ctypes.data for b in bufs], None)
    strides = (ctypes.c_int64 * 4)(128, 128, 128, 0)

    def call(desc=d, tw=13, th=7, s=sums.ctypes.data, p=ptrs, st=strides):
        return lib.avifgpu_thumbnail_from_sums(ctypes.byref(desc) if desc is not None else None, tw, th, s,
                                               ctypes.byref(p) if p is not None else None, ctypes.byref(st) if st is not None else None)
    assert call() == 0
    assert call(tw=49, th=21) == 0                                                     # the chroma planes' own size
    for kw in (dict(tw=50), dict(th=22), dict(tw=0), dict(th=0), dict(tw=-1), dict(s=None), dict(p=None), dict(st=None), dict(desc=None)):
        assert call(**kw) == pkg.formatBadParameters, kw
    assert call(p=(ctypes.c_void_p * 4)(bufs[0].ctypes.data, None, bufs[2].ctypes.data, None)) == pkg.formatBadParameters
    assert call(st=(ctypes.c_int64 * 4)(128, 12, 128, 0)) == pkg.formatBadParameters
    bad = make_desc(97, 41, 3, 8, pkg.OUT_YCBCR, pkg.CHROMA_420)
    bad.planes = 5
    assert call(desc=bad) == pkg.formatBadParameters
    wide = make_desc(4000, 3000, 3, 8)
    assert call(desc=wide, tw=1025, th=7) == pkg.formatBadParameters                  # 1024 is the limit


# ---- 2. avifgpu_thumbnail_fit -------------------------------------------------------------------------------------------------------------
def fit(w, h, bbox, mw, mh):
    tw, th = w, h
    if max(w, h) > bbox:
        if w >= h:
            tw, th = bbox, max(1, (2 * h * bbox + w) // (2 * w))
        else:
            tw, th = max(1, (2 * w * bbox + h) // (2 * h)), bbox
    return min(tw, mw, 1024), min(th, mh, 1024)


def test_fit_enumerated():
    lib = pkg.load()
    tw, th = ctypes.c_int32(), ctypes.c_int32()
    ptw, pth = ctypes.byref(tw), ctypes.byref(th)
    call = lib.avifgpu_thumbnail_fit
    bad = []
    for chroma in CHROMAS:
        xs, ys = harness.chroma_shift(chroma)
        d = make_desc(1, 1, 3, 8, pkg.OUT_YCBCR, chroma, full_range=1)
        pd = ctypes.byref(d)
        for w in range(1, 65):
            d.width = w
            mw = (w + xs) >> xs
            for h in range(1, 65):
                d.height = h
                mh = (h + ys) >> ys
                for bbox in range(1, 71):
                    rc = call(pd, bbox, ptw, pth)
                    got = (tw.value, th.value)
                    if rc != 0 or got != fit(w, h, bbox, mw, mh) or not (1 <= got[0] <= mw and 1 <= got[1] <= mh):
                        bad.append((chroma, w, h, bbox, rc, got))
    assert not bad, bad[:10]


@pytest.mark.parametrize("w,h,bbox,want", [(16384, 9001, 256, (256, 141)), (5, 16384, 1024, (1, 1024)), (16384, 16384, 4096, (1024, 1024)),
                                           (300, 200, 64, (64, 43)), (97, 41, 1000, (97, 41))])
def test_fit_large(w, h, bbox, want):
    for planes, output in ((3, pkg.OUT_REFERENCE), (1, pkg.OUT_REFERENCE), (4, pkg.OUT_YCBCR)):
        d = make_desc(w, h, planes, 10, output, pkg.CHROMA_444, full_range=1)
        assert pkg.thumbnail_fit(d, bbox) == want
    # (16384, 9001, 256): 9001 * 256 / 16384 = 140.64 -> 141;  (5, 16384, 1024): 5 * 1024 / 16384 = 0.31 -> max(1, 0)
    d = make_desc(w, h, 3, 10, pkg.OUT_YCBCR, pkg.CHROMA_420, full_range=1)
    assert pkg.thumbnail_fit(d, bbox) == fit(w, h, bbox, (w + 1) >> 1, (h + 1) >> 1)


def test_fit_argument_errors():
    lib = pkg.load()
    d = make_desc(97, 41, 3, 8)
    tw, th = ctypes.c_int32(), ctypes.c_int32()
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), 13, ctypes.byref(tw), ctypes.byref(th)) == 0
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), 0, ctypes.byref(tw), ctypes.byref(th)) == pkg.formatBadParameters
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), -5, ctypes.byref(tw), ctypes.byref(th)) == pkg.formatBadParameters
    assert lib.avifgpu_thumbnail_fit(None, 13, ctypes.byref(tw), ctypes.byref(th)) == pkg.formatBadParameters
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), 13, None, ctypes.byref(th)) == pkg.formatBadParameters
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), 13, ctypes.byref(tw), None) == pkg.formatBadParameters
    d.width = 0
    assert lib.avifgpu_thumbnail_fit(ctypes.byref(d), 13, ctypes.byref(tw), ctypes.byref(th)) == pkg.formatBadParameters
    with pytest.raises(pkg.AvifGpuError):
        pkg.thumbnail_fit(d, 13)


# ---- 3. arming ---------------------------------------------------------------------------------------------------------------------------
def test_attach_argument_errors_and_disarming():
    lib = pkg.load()
    sums = np.zeros(4 * 16, dtype=np.uint64)
    for tw, th, kind in ((0, 4, pkg.MEM_HOST), (4, 0, pkg.MEM_HOST), (1025, 4, pkg.MEM_HOST), (4, 1025, pkg.MEM_DEVICE), (-1, 4, pkg.MEM_HOST),
                         (4, 4, 2), (4, 4, -1)):
        assert lib.avifgpu_thumbnail_attach(sums.ctypes.data, tw, th, kind) == pkg.formatBadParameters, (tw, th, kind)
        assert b"avifgpu_thumbnail_attach" in lib.avifgpu_last_error()
    for tw, th, kind in ((1, 1, pkg.MEM_HOST), (1024, 1024, pkg.MEM_DEVICE), (4, 4, pkg.MEM_HOST)):
        assert lib.avifgpu_thumbnail_attach(sums.ctypes.data, tw, th, kind) == 0
    # disarming always succeeds, whatever the other arguments say, and twice in a row
    assert lib.avifgpu_thumbnail_attach(None, 0, 0, pkg.MEM_HOST) == 0
    assert lib.avifgpu_thumbnail_attach(None, 5000, -3, 77) == 0
    assert not sums.any()
    with pytest.raises(ValueError):
        with pkg.thumbnail_sums(np.zeros(3, dtype=np.uint64), 2, 2):
            pass
    with pytest.raises(ValueError):
        with pkg.thumbnail_sums(np.zeros(16, dtype=np.uint32), 2, 2):
            pass
    with pytest.raises(pkg.AvifGpuError):
        with pkg.thumbnail_sums(sums.ctypes.data, 4, 2000):                       # a raw address: the library's own check
            pass
    with pkg.thumbnail_sums(sums, 4, 4) as t:
        assert t.tw == 4


def test_reference_box_sums_on_a_worked_example():
    """The reference itself on numbers small enough to check by hand: 5 x 3 -> 2 x 2, cells x: {0,1,2 | 3,4}, y: {0,1 | 2}."""
    d = make_desc(5, 3, 1, 8)
    a = np.arange(15, dtype=np.uint8).reshape(3, 5)
    s = box_sums({0: a}, d, 2, 2)
    assert s[:, :, 0].tolist() == [[0 + 1 + 2 + 5 + 6 + 7, 3 + 4 + 8 + 9], [10 + 11 + 12, 13 + 14]]
    assert cell_counts(d, 2, 2)[:, :, 0].tolist() == [[6, 4], [3, 2]]
    got = pkg.thumbnail_from_sums(d, 2, 2, s.reshape(-1).astype(np.uint64))
    assert got[0].tolist() == [[(2 * 21 + 6) // 12, (2 * 24 + 4) // 8], [(2 * 33 + 3) // 6, (2 * 27 + 2) // 4]]
