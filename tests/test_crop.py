"""Host-only half of the cropped open (include/avifgpu.h "cropped open"): the clean-aperture rule against exact fractions, folding a crop
into an oriented view, geometry, the tile helper, the scratch formula and every rejected argument.  No device is needed: everything here
returns before anything would be launched."""
import ctypes
import itertools
import random

import numpy as np
import pytest

import crop_truth
import harness
from orientation_truth import orient

pkg = harness.pkg

CODES = range(1, 9)
BAD = pkg.formatBadParameters


def desc_for(width, height, chroma=pkg.CHROMA_444, **kw):
    base = dict(width=width, height=height, colorspace=pkg.COLORSPACE_YCBCR, chroma=chroma, bit_depth=8, depth=8, alpha_state=pkg.ALPHA_NONE)
    base.update(kw)
    return pkg.ReadDesc(**base)


def lib_clap(width, height, clap):
    """(x0, y0, w, h), or None for formatBadParameters"""
    out = pkg.CropRect()
    rc = pkg.load().avifgpu_clap_to_rect(width, height, ctypes.byref((ctypes.c_int32 * 8)(*clap)), ctypes.byref(out))
    assert rc in (0, BAD), rc
    return out.astuple() if rc == 0 else None


# ---- avifgpu_clap_to_rect ----------------------------------------------------------------------------------------------------------------
def test_clap_hand_checked_cases():
    # each row worked out by hand from ISO 14496-12 (pc = off + (size - 1) / 2, edges pc -+ (ap - 1) / 2, rounded half up, clamped); the
    # Fraction rule is asserted against the same numbers before it is trusted for the sweep below
    table = [
        ((100, 80), (50, 1, 40, 1, 0, 1, 0, 1), (25, 20, 50, 40)),
        ((101, 80), (50, 1, 40, 1, 0, 1, 0, 1), (26, 20, 50, 40)),          # 25.5 .. 74.5 -> left 26, right 75
        ((100, 80), (50, 1, 40, 1, -1, 2, 0, 1), (25, 20, 50, 40)),         # 24.5 .. 73.5 -> left 25, right 74
        ((10, 80), (20, 1, 40, 1, 0, 1, 0, 1), (0, 20, 10, 40)),            # -5 .. 14 -> the whole width
    ]
    for (w, h), clap, want in table:
        assert crop_truth.clap_to_rect(w, h, clap) == want, (w, h, clap)
        assert lib_clap(w, h, clap) == want, (w, h, clap)
    assert lib_clap(101, 80, (50, 1, 40, 1, 0, 1, 0, 1))[0] + 50 - 1 == 75
    assert lib_clap(100, 80, (50, 1, 40, 1, -1, 2, 0, 1))[0] + 50 - 1 == 74


def test_clap_rejections():
    good = [50, 1, 40, 1, 0, 1, 0, 1]
    assert lib_clap(100, 80, good) is not None
    # an aperture lying outside the image: to the right, to the left, below
    for clap in ((10, 1, 10, 1, 200, 1, 0, 1), (10, 1, 10, 1, -200, 1, 0, 1), (10, 1, 10, 1, 0, 1, 500, 1), (10, 1, 10, 1, 0, 1, -500, 1)):
        assert crop_truth.clap_to_rect(100, 80, clap) is None
        assert lib_clap(100, 80, clap) is None, clap
    # zero or negative denominators, zero or negative aperture
    for i in (1, 3, 5, 7):
        for v in (0, -1, -(2 ** 31)):
            clap = list(good); clap[i] = v
            assert crop_truth.clap_to_rect(100, 80, clap) is None
            assert lib_clap(100, 80, clap) is None, clap
    for i in (0, 2):
        for v in (0, -3):
            clap = list(good); clap[i] = v
            assert lib_clap(100, 80, clap) is None, clap
    # operands that overflow 32- and 64-bit intermediates, lying outside the image
    big = 2 ** 31 - 1
    for clap in ((big, 1, 40, 1, big, 1, 0, 1), (big, 1, 40, 1, -big - 1, 1, 0, 1), (50, 1, big, 1, 0, 1, big, 1), (big, big - 1, 40, 1, big, 1, 0, 1),
                 (big, 1, big, 1, -big - 1, 1, -big - 1, 1)):
        assert crop_truth.clap_to_rect(100, 80, clap) is None
        assert lib_clap(100, 80, clap) is None, clap
    # ... while huge operands whose result is inside the image are computed exactly
    for clap in ((big, 1, big, 1, 0, 1, 0, 1), (big - 1, big, 40, 1, 7, big, 0, 1), (50 * (big // 50), big // 50, 40, 1, -big, big, 3 * (big // 4), big // 4 * 4)):
        want = crop_truth.clap_to_rect(100, 80, clap)
        assert want is not None and lib_clap(100, 80, clap) == want, clap
    lib = pkg.load()
    out = pkg.CropRect()
    arr = (ctypes.c_int32 * 8)(*good)
    assert lib.avifgpu_clap_to_rect(0, 80, ctypes.byref(arr), ctypes.byref(out)) == BAD
    assert lib.avifgpu_clap_to_rect(100, 80, None, ctypes.byref(out)) == BAD
    assert lib.avifgpu_clap_to_rect(100, 80, ctypes.byref(arr), None) == BAD


def test_clap_seeded_sweep_against_fractions():
    rng = random.Random(20261019)
    hits = 0
    for i in range(6000):
        w, h = rng.choice((1, 2, 7, 64, 101, 4096, 65535, 2 ** 31 - 1)), rng.choice((1, 3, 80, 1001, 2 ** 30))
        def rat(scale):
            kind = rng.randrange(4)
            if kind == 0:
                return rng.randint(1, max(1, 2 * scale)), 1
            if kind == 1:
                d = rng.randint(1, 64)
                return rng.randint(-d * scale, 2 * d * scale), d
            if kind == 2:
                return rng.randint(-(2 ** 31), 2 ** 31 - 1), rng.randint(1, 2 ** 31 - 1)
            d = rng.choice((2, 3, 4, 1000, 65536))
            return rng.randint(0, d * scale), d
        def off(scale):
            d = rng.choice((1, 2, 3, 4, 7, 1000))
            return rng.randint(-d * scale // 2, d * scale // 2), d
        an, ad = rat(min(w, 2 ** 30)); bn, bd = rat(min(h, 2 ** 30))
        hn, hd = off(min(w, 2 ** 30)); vn, vd = off(min(h, 2 ** 30))
        if i % 17 == 0:
            hd = rng.choice((0, -1))
        clap = tuple(max(-(2 ** 31), min(2 ** 31 - 1, v)) for v in (an, ad, bn, bd, hn, hd, vn, vd))      # the fields are int32
        want = crop_truth.clap_to_rect(w, h, clap)
        assert lib_clap(w, h, clap) == want, (w, h, clap)
        hits += want is not None
    assert hits > 1000                                          # the sweep is not all rejections


# ---- avifgpu_crop_compose ------------------------------------------------------------------------------------------------------------------
def all_rects(w, h):
    for x0, y0 in itertools.product(range(w), range(h)):
        for cw, ch in itertools.product(range(1, w - x0 + 1), range(1, h - y0 + 1)):
            yield (x0, y0, cw, ch)


def test_crop_compose_brute_force():
    L = np.arange(7 * 6).reshape(6, 7, 1)                       # the stored label array, 7 wide, 6 high
    current = (1, 2, 5, 4)                                      # a 5 x 4 current rectangle inside it
    n = 0
    for code in CODES:
        view = orient(code, crop_truth.crop(L, current))
        vw, vh = crop_truth.view_size(current, code)
        assert view.shape[:2] == (vh, vw)
        for v in all_rects(vw, vh):
            out = pkg.crop_compose(current, code, v)
            assert np.array_equal(orient(code, crop_truth.crop(L, out)), crop_truth.crop(view, v)), (code, v, out)
            n += 1
    assert n == 8 * 150


def test_crop_compose_two_crops_with_a_turn_between():
    L = np.arange(23 * 17).reshape(17, 23, 1)
    for turn, second_turn in itertools.product((6, 8, 3, 2, 5), (1, 4, 7)):
        # numpy, step by step: crop, turn, crop, turn
        a = crop_truth.crop(L, (3, 2, 17, 12))
        a = orient(turn, a)
        c2 = (2, 1, a.shape[1] - 5, a.shape[0] - 3)
        a = crop_truth.crop(a, c2)
        a = orient(second_turn, a)
        # the adapter's fold, starting from (whole image, 1)
        rect, code = (0, 0, 23, 17), 1
        rect = pkg.crop_compose(rect, code, (3, 2, 17, 12))
        code = pkg.orientation_compose(code, turn)
        rect = pkg.crop_compose(rect, code, c2)
        code = pkg.orientation_compose(code, second_turn)
        assert np.array_equal(crop_truth.cropped(L, rect, code), a), (turn, second_turn, rect, code)


def test_crop_compose_rejections():
    lib = pkg.load()
    out = pkg.CropRect()
    def rc(cur, code, v):
        return lib.avifgpu_crop_compose(ctypes.byref(pkg.CropRect(*cur)), code, ctypes.byref(pkg.CropRect(*v)), ctypes.byref(out))
    assert rc((1, 2, 5, 4), 6, (0, 0, 4, 5)) == 0
    for cur, code, v in (((1, 2, 5, 4), 0, (0, 0, 1, 1)), ((1, 2, 5, 4), 9, (0, 0, 1, 1)), ((1, 2, 5, 4), 1, (0, 0, 6, 1)), ((1, 2, 5, 4), 6, (0, 0, 5, 4)),
                         ((1, 2, 5, 4), 1, (-1, 0, 2, 2)), ((1, 2, 5, 4), 1, (0, 0, 0, 2)), ((-1, 2, 5, 4), 1, (0, 0, 1, 1)), ((1, 2, 0, 4), 1, (0, 0, 1, 1)),
                         ((2 ** 31 - 3, 0, 5, 4), 1, (0, 0, 1, 1))):
        assert rc(cur, code, v) == BAD, (cur, code, v)
    assert lib.avifgpu_crop_compose(None, 1, ctypes.byref(out), ctypes.byref(out)) == BAD


# ---- geometry, tiles, scratch --------------------------------------------------------------------------------------------------------------
def test_geometry():
    d = desc_for(67, 35, pkg.CHROMA_420)
    for code in CODES:
        assert pkg.read_cropped_geometry(d, (3, 5, 40, 20), code) == ((40, 20) if code <= 4 else (20, 40))
    lib = pkg.load()
    w, h = ctypes.c_int32(), ctypes.c_int32()
    r = pkg.CropRect(3, 5, 40, 20)
    for code in (0, 9):
        assert lib.avifgpu_read_cropped_geometry(ctypes.byref(d), ctypes.byref(r), code, ctypes.byref(w), ctypes.byref(h)) == BAD
    for bad in ((-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 68, 4), (60, 0, 8, 4), (0, 30, 4, 6), (0, 0, 4, -1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)):
        assert lib.avifgpu_read_cropped_geometry(ctypes.byref(d), ctypes.byref(pkg.CropRect(*bad)), 1, ctypes.byref(w), ctypes.byref(h)) == BAD, bad
    assert lib.avifgpu_read_cropped_geometry(ctypes.byref(d), None, 1, ctypes.byref(w), ctypes.byref(h)) == BAD
    assert lib.avifgpu_read_cropped_geometry(ctypes.byref(d), ctypes.byref(r), 1, None, ctypes.byref(h)) == BAD


def cut_rule(d, rect, upsampling, code):
    """(extent of the cut direction, absolute start of it, flipped, whether the rule applies) -- restated from the definition"""
    xs, ys = harness.chroma_shift(d.chroma) if d.colorspace == pkg.COLORSPACE_YCBCR else (0, 0)
    turned = code >= 5
    flipped = code in ((7, 8) if turned else (3, 4))
    interpolated = upsampling != pkg.UPSAMPLE_NEAREST and xs
    applies = bool(xs if turned else ys) and not interpolated
    return (rect[2] if turned else rect[3]), (rect[0] if turned else rect[1]), flipped, applies


@pytest.mark.parametrize("chroma", [pkg.CHROMA_444, pkg.CHROMA_422, pkg.CHROMA_420])
def test_next_tile_partitions_every_rect(chroma):
    d = desc_for(9, 8, chroma)
    applied = 0
    for rect in all_rects(9, 8):
        if rect[0] > 3 or rect[1] > 3:
            continue                                            # both parities of every start are in
        for code, max_rows, ups in itertools.product(CODES, (1, 2, 7), (pkg.UPSAMPLE_NEAREST, pkg.UPSAMPLE_BILINEAR_CENTER)):
            out_h, a0, flipped, applies = cut_rule(d, rect, ups, code)
            o = 0
            while o < out_h:
                n = pkg.read_cropped_next_tile(d, rect, ups, code, o, max_rows)
                assert 0 < n <= max_rows and o + n <= out_h, (rect, code, max_rows, o, n)
                rest = out_h - o
                if not applies:
                    assert n == min(max_rows, rest)
                elif n < rest and n > 1:
                    # the cut falls on an even absolute source index: the next tile's start (forwards) or this tile's (backwards)
                    edge = a0 + out_h - o - n if flipped else a0 + o + n
                    assert edge % 2 == 0, (rect, code, max_rows, o, n)
                    assert n >= min(max_rows, rest) - 1                 # and no more than one row was given up for it
                    applied += 1
                elif n < rest:
                    assert min(max_rows, rest) <= 2                      # a single row only where nothing larger could end even
                o += n
            assert o == out_h
    assert (applied > 0) == (chroma != pkg.CHROMA_444)


def test_next_tile_rejections():
    lib = pkg.load()
    d = desc_for(9, 8, pkg.CHROMA_420)
    r = pkg.CropRect(1, 1, 6, 5)
    def rc(rect, ups, code, o, m):
        return lib.avifgpu_read_cropped_next_tile(ctypes.byref(d), ctypes.byref(rect), ups, code, o, m)
    assert rc(r, 0, 1, 0, 4) > 0
    assert rc(r, 0, 1, 5, 4) == BAD and rc(r, 0, 6, 6, 4) == BAD and rc(r, 0, 6, 5, 4) == 1
    assert rc(r, 0, 1, -1, 4) == BAD and rc(r, 0, 1, 0, 0) == BAD
    assert rc(r, 3, 1, 0, 4) == BAD and rc(r, -1, 1, 0, 4) == BAD and rc(r, 0, 0, 0, 4) == BAD and rc(r, 0, 9, 0, 4) == BAD
    assert rc(pkg.CropRect(1, 1, 9, 5), 0, 1, 0, 4) == BAD


def align256(v):
    return (v + 255) // 256 * 256


def scratch_formula(d, rect, ups, code, onrows):
    """the formula as the header states it"""
    xs, ys = harness.chroma_shift(d.chroma) if d.colorspace == pkg.COLORSPACE_YCBCR else (0, 0)
    s = 2 if d.bit_depth > 8 else 1
    nch = (1 if d.colorspace == pkg.COLORSPACE_MONOCHROME else 3) + (1 if d.alpha_state != pkg.ALPHA_NONE else 0)
    b = nch * d.depth // 8
    turned = code >= 5
    sw, sh = (onrows, rect[3]) if turned else (rect[2], onrows)
    if sw < 1 or sh < 1:
        return 0
    if ups != pkg.UPSAMPLE_NEAREST and xs:
        return 2 * align256(sw * s) * sh + (0 if code == 1 else align256(sw * b) * sh)
    px = 1 if xs and sw > 1 and (turned or rect[0] % 2) else 0
    py = 1 if ys and sh > 1 and (not turned or rect[1] % 2) else 0
    if code == 1 and not px and not py:
        return 0
    return align256((sw + px) * b) * (sh + py)


def test_scratch_bytes_formula():
    cases = [desc_for(37, 21, pkg.CHROMA_420), desc_for(38, 22, pkg.CHROMA_422), desc_for(37, 21, pkg.CHROMA_444),
             desc_for(37, 21, pkg.CHROMA_420, bit_depth=12, depth=16), desc_for(37, 21, pkg.CHROMA_420, bit_depth=10, depth=32, has_nclx=1,
                                                                               transfer_characteristics=pkg.TC_PQ, pq_peak_nits=1000),
             desc_for(37, 21, colorspace=pkg.COLORSPACE_RGB, alpha_state=pkg.ALPHA_STRAIGHT),
             desc_for(37, 21, colorspace=pkg.COLORSPACE_MONOCHROME, chroma=pkg.CHROMA_MONOCHROME, alpha_state=pkg.ALPHA_STRAIGHT)]
    nonzero = 0
    for d, rect, ups, code in itertools.product(cases, ((0, 0, 20, 10), (1, 0, 20, 10), (0, 1, 20, 10), (3, 3, 1, 1), (3, 3, 30, 1), (3, 3, 1, 15), (0, 0, 37, 21)),
                                                (pkg.UPSAMPLE_NEAREST, pkg.UPSAMPLE_BILINEAR_CENTER, pkg.UPSAMPLE_BILINEAR_LEFT), CODES):
        rect = (rect[0], rect[1], min(rect[2], d.width - rect[0]), min(rect[3], d.height - rect[1]))
        out_h = crop_truth.view_size(rect, code)[1]
        for onrows in {0, 1, min(2, out_h), out_h}:
            got = pkg.read_cropped_scratch_bytes(d, rect, ups, code, onrows)
            assert got == scratch_formula(d, rect, ups, code, onrows), (rect, ups, code, onrows)
            nonzero += got > 0
    assert nonzero > 100
    lib = pkg.load()
    d = cases[0]
    r = pkg.CropRect(1, 1, 20, 10)
    assert lib.avifgpu_read_cropped_scratch_bytes(ctypes.byref(d), ctypes.byref(r), 0, 1, 11) == BAD
    assert lib.avifgpu_read_cropped_scratch_bytes(ctypes.byref(d), ctypes.byref(r), 0, 6, 21) == BAD
    assert lib.avifgpu_read_cropped_scratch_bytes(ctypes.byref(d), ctypes.byref(r), 5, 1, 1) == BAD
    assert lib.avifgpu_read_cropped_scratch_bytes(ctypes.byref(d), ctypes.byref(pkg.CropRect(30, 1, 20, 10)), 0, 1, 1) == BAD


# ---- avifgpu_read_rows_cropped / avifgpu_probe_crop: every rejection that returns before a device is looked for ----------------------------------
def test_read_rows_cropped_rejections_before_any_device():
    lib = pkg.load()
    P4, S4 = ctypes.c_void_p * 4, ctypes.c_int64 * 4
    buf = ctypes.create_string_buffer(1 << 16)
    ptrs = P4(*[ctypes.addressof(buf)] * 4)
    strides = S4(64, 64, 64, 64)
    d = desc_for(37, 21, pkg.CHROMA_420)

    def rc(rect=(1, 1, 20, 10), ups=0, code=1, o=0, n=10, src=ptrs, st=strides, dst=buf, drb=64, scratch=None, sb=0, mem=pkg.MEM_DEVICE, desc=d):
        return lib.avifgpu_read_rows_cropped(ctypes.byref(desc), ctypes.byref(pkg.CropRect(*rect)), ups, code, o, n,
                                             ctypes.byref(src) if src is not None else None, ctypes.byref(st), dst, drb, scratch, sb, mem, None)

    def msg():
        return lib.avifgpu_last_error()

    for kw, text in ((dict(rect=(1, 1, 37, 10)), b"not inside"), (dict(rect=(-1, 1, 5, 5)), b"not inside"), (dict(rect=(1, 1, 0, 5)), b"not inside"),
                     (dict(rect=(1, 20, 5, 2)), b"not inside"), (dict(ups=3), b"upsampling"), (dict(ups=-1), b"upsampling"), (dict(code=0), b"1..8"), (dict(code=9), b"1..8"),
                     (dict(o=-1), b"outside"), (dict(o=5, n=6), b"outside"), (dict(n=-1), b"outside"), (dict(code=6, o=0, n=21), b"outside"),
                     (dict(mem=7), b"mem_kind"), (dict(src=None), b"null buffer"), (dict(dst=None), b"null buffer"),
                     (dict(drb=59), b"dst_row_bytes"), (dict(code=6, drb=29), b"dst_row_bytes"),
                     (dict(st=S4(36, 18, 64, 64)), b"src_stride"),
                     (dict(), b"scratch"),                                             # odd start: the covering rectangle needs scratch
                     (dict(scratch=ctypes.addressof(buf), sb=255), b"scratch"),
                     (dict(rect=(2, 2, 20, 10), code=3), b"scratch"),
                     (dict(rect=(2, 2, 20, 10), ups=1), b"scratch")):
        assert rc(**kw) == BAD, kw
        assert text in msg(), (kw, msg())
    assert rc(desc=desc_for(37, 21, pkg.CHROMA_420, bit_depth=9)) == pkg.readErr
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the missing device, and no further
        assert rc(rect=(2, 2, 20, 10)) == BAD and b"no CPU fallback" in msg()
        assert rc(scratch=ctypes.addressof(buf), sb=1 << 16) == BAD and b"no CPU fallback" in msg()
        assert rc(mem=pkg.MEM_HOST) == BAD and b"no CPU fallback" in msg()
    assert lib.avifgpu_probe_crop(None, 64, buf, 64, 16, 1, None) == BAD
    assert lib.avifgpu_probe_crop(buf, 64, buf, 64, 0, 1, None) == BAD
    assert lib.avifgpu_probe_crop(buf, 64, buf, 64, 16, 0, None) == BAD
    assert lib.avifgpu_probe_crop(buf, 15, buf, 64, 16, 1, None) == BAD and lib.avifgpu_probe_crop(buf, 64, buf, 15, 16, 1, None) == BAD
