"""CPU checks behind the exhaustive GPU tests (tests/test_zz_gpu_whole_domain_read.py, tests/test_zz_gpu_whole_domain_write.py):

1. every generator of tests/exhaustive_inputs.py covers what it says it covers -- counted, not argued;
2. the oracle agrees with a numpy float32 restatement of the reference (tests/reference_numpy.py) on EVERY 8-bit triple, both ways.
   The oracle is otherwise pinned to known-answer values only; this is the comparison that decides who is right when a GPU test fails.

No GPU.  Bit for bit throughout.
"""
import numpy as np
import pytest

import exhaustive_inputs as xi
import harness
import reference_numpy as rn

pkg = harness.pkg


def _each_exactly_once(keys, domain):
    """Every value of 0 .. domain - 1 occurs exactly once in `keys` (np.unique up to 2^20 keys, its counting equivalent above)."""
    keys = np.asarray(keys).reshape(-1)
    if keys.size != domain:
        return False
    if domain <= 1 << 20:
        u, c = np.unique(keys, return_counts=True)
        return u.size == domain and int(u[0]) == 0 and int(u[-1]) == domain - 1 and bool((c == 1).all())
    return bool((np.bincount(keys, minlength=domain) == 1).all()) and int(keys.max()) == domain - 1


def _key(*codes, bits):
    k = np.zeros(np.broadcast(*codes).shape, dtype=np.int64)
    for c in codes:
        k = (k << bits) | c.astype(np.int64)
    return k


def _upsampled(planes, chroma):
    xs, ys = xi.sub_shifts(chroma)
    up = lambda a: np.repeat(np.repeat(a, 1 << ys, axis=0), 1 << xs, axis=1)
    return planes[0], up(planes[1]), up(planes[2])


# ---- 1. coverage claims ---------------------------------------------------------------------------------------------------------
def test_all_triples_444_holds_every_triple_once():
    p = xi.all_triples_444()
    assert all(p[i].shape == (4096, 4096) and p[i].dtype == np.uint8 and p[i].flags.c_contiguous for i in range(3))
    assert _each_exactly_once(_key(p[0], p[1], p[2], bits=8), 1 << 24)
    with pytest.raises(ValueError):
        xi.all_triples_444(10)


@pytest.mark.parametrize("chroma", ["422", "420"])
@pytest.mark.parametrize("phase", [0, 1])
def test_all_triples_sub_holds_every_triple_once(chroma, phase):
    p = xi.all_triples_sub(chroma, phase)
    xs, ys = xi.sub_shifts(chroma)
    assert p[0].shape == (4096, 4096) and p[1].shape == p[2].shape == (4096 >> ys, 4096 >> xs) and all(p[i].flags.c_contiguous for i in range(3))
    y, cb, cr = _upsampled(p, chroma)                       # what a nearest-neighbour open pairs every luma sample with
    assert _each_exactly_once(_key(y, cb, cr, bits=8), 1 << 24)
    # the position inside the footprint is not tied to Y's low bits: the two phases put different low bits at every position
    q = xi.all_triples_sub(chroma, 1 - phase)
    nj = 1 << (xs + ys)
    assert np.all((p[0] % nj) + (q[0] % nj) == nj - 1)
    assert np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2])


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_latin_square_holds_every_pair_once(bits):
    n = 1 << bits
    p = xi.latin_square(bits)
    assert all(p[i].shape == (n, n) and p[i].dtype == (np.uint8 if bits == 8 else np.uint16) and p[i].flags.c_contiguous for i in range(3))
    for a, b in ((0, 1), (0, 2), (1, 2)):                   # (Y, Cb), (Y, Cr), (Cb, Cr)
        assert _each_exactly_once(_key(p[a], p[b], bits=bits), n * n), (a, b)


@pytest.mark.parametrize("bits", [10, 12])
@pytest.mark.parametrize("chroma", ["422", "420"])
def test_sub_sampled_latin_square_is_exhaustive_at_every_footprint_position(bits, chroma):
    n = 1 << bits
    xs, ys = xi.sub_shifts(chroma)
    p = xi.latin_square(bits, chroma)
    assert p[0].shape == (n << ys, n << xs) and p[1].shape == p[2].shape == (n, n) and all(p[i].flags.c_contiguous for i in range(3))
    assert xi.LATIN_STEP % 2 == 1
    assert _each_exactly_once(_key(p[1], p[2], bits=bits), n * n)
    seen = set()
    for dy in range(1 << ys):
        for dx in range(1 << xs):
            y = p[0][dy::1 << ys, dx::1 << xs]
            assert _each_exactly_once(_key(y, p[1], bits=bits), n * n), (dy, dx)
            assert _each_exactly_once(_key(y, p[2], bits=bits), n * n), (dy, dx)
            seen.add(int(y[0, 0]))
    assert len(seen) == 1 << (xs + ys)                      # the positions of a footprint hold different luma codes


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_pairs_and_latin_alpha(bits):
    n = 1 << bits
    code, alpha = xi.pairs(bits)
    assert code.flags.c_contiguous and alpha.flags.c_contiguous
    assert _each_exactly_once(_key(code, alpha, bits=bits), n * n)
    a = xi.latin_alpha(bits)
    assert a.flags.c_contiguous and a.dtype == code.dtype
    want = np.arange(n)
    assert np.array_equal(np.sort(a, axis=0), np.broadcast_to(want[:, None], (n, n)))       # every column holds every code
    assert np.array_equal(np.sort(a, axis=1), np.broadcast_to(want[None, :], (n, n)))       # every row too
    big = xi.latin_alpha(bits, (2 * n, 2 * n))                                             # at luma resolution: any n x n window does
    assert np.array_equal(np.sort(big[5:5 + n, 3:3 + n], axis=1), np.broadcast_to(want[None, :], (n, n)))


def _oracle_rescale16(bits):
    """The oracle's 16 -> `bits` rescale of every Photoshop 16-bit value 0 .. 32768, read off a one-plane ramp."""
    d = pkg.WriteDesc(width=32769, height=1, depth=16, planes=1, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    ramp = np.arange(32769, dtype=np.uint16).reshape(1, -1)
    return harness.oracle_write(d, ramp)[0].reshape(-1)


@pytest.mark.parametrize("bits", [8, 10, 12])
def test_code_preimages_are_the_ends_of_each_code(bits):
    codes = _oracle_rescale16(bits)
    lo, hi = xi.code_preimages(codes, bits)
    n = 1 << bits
    assert lo.shape == hi.shape == (n,) and lo[0] == 0 and hi[-1] == 32768
    assert np.array_equal(codes[lo], np.arange(n)) and np.array_equal(codes[hi], np.arange(n))
    assert np.array_equal(lo[1:].astype(np.int64), hi[:-1].astype(np.int64) + 1)            # the preimages tile 0 .. 32768
    assert (hi > lo).all()                                                                  # two different ends for every code
    with pytest.raises(ValueError):
        xi.code_preimages(codes[::-1], bits)
    with pytest.raises(ValueError):
        xi.code_preimages(codes[::16], 16)


def test_ends_for_triples_show_both_ends_of_every_code():
    c = np.arange(256)
    r, g, b = np.meshgrid(c, c, c, indexing="ij")
    e0, e1 = xi.ends_for_triples(r, g, b, 0), xi.ends_for_triples(r, g, b, 1)
    for k, code in enumerate((r, g, b)):
        assert np.all(e0[k] + e1[k] == 1)                                                   # over both phases: each triple, both ends
        assert _each_exactly_once(np.unique(_key(code, e0[k], bits=1)), 512)                # inside one phase: each code, both ends


@pytest.mark.parametrize("planes", [3, 4])
def test_every_u16_in_each_channel(planes):
    a = xi.every_u16_in_each_channel(planes)
    assert a.shape == (256, 256 * planes) and a.dtype == np.uint16
    px = a.reshape(-1, planes)
    for k in range(planes):
        assert _each_exactly_once(px[:, k], 1 << 16), k


def test_lattice64_is_the_old_tests_lattice():
    p = xi.lattice64()
    assert all(np.unique(p[i]).size == 64 for i in range(3))
    assert np.unique(_key(p[0], p[1], p[2], bits=8)).size == 64 ** 3       # 1.6 % of the 2^24 triples


def test_interleaved_puts_plane_k_into_channel_k():
    p = {0: np.full((2, 3), 1, np.uint8), 1: np.full((2, 3), 2, np.uint8), 3: np.full((2, 3), 9, np.uint8)}
    a = xi.interleaved(p, (0, 1, 3))
    assert a.shape == (2, 9) and a.flags.c_contiguous and np.array_equal(a.reshape(2, 3, 3)[0, 0], [1, 2, 9])


def test_with_stride_pad_keeps_the_samples():
    p = {0: np.arange(12, dtype=np.uint8).reshape(3, 4)}
    q = xi.with_stride_pad(p, 3)
    assert q[0].shape == (3, 7) and q[0].strides[0] == 7 and np.array_equal(q[0][:, :4], p[0]) and not q[0][:, 4:].any()


# ---- 2. the oracle against the numpy restatement of the reference -----------------------------------------------------------------
READ_MATRICES = [("bt601", pkg.MATRIX_BT601), ("bt709", pkg.MATRIX_BT709), ("bt2020ncl", pkg.MATRIX_BT2020_NCL), ("fcc", pkg.MATRIX_FCC),
                 ("smpte240m", pkg.MATRIX_SMPTE240M)]


def _read_desc(planes, matrix, fr):
    h, w = planes[0].shape
    return pkg.ReadDesc(width=w, height=h, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_444, bit_depth=8, depth=8,
                        alpha_state=pkg.ALPHA_NONE, matrix_coefficients=matrix, full_range_flag=fr)


def test_restatement_constants_match_the_oracles():
    """kr, kg, kb of every matrix the tests use (and of the rows the oracle falls back on) are the same floats on both sides."""
    for m, pr in [(m, 1) for _, m in READ_MATRICES] + [(pkg.MATRIX_RGB_GBR, 1), (pkg.MATRIX_BT470BG, 1), (pkg.MATRIX_YCGCO, 1),
                                                       (pkg.MATRIX_CHROMA_DERIVED_NCL, pkg.PRIMARIES_BT709),
                                                       (pkg.MATRIX_CHROMA_DERIVED_NCL, pkg.PRIMARIES_BT2020),
                                                       (pkg.MATRIX_CHROMA_DERIVED_NCL, pkg.PRIMARIES_SMPTE432)]:
        want = np.array(pkg.yuv_coefficients(1, m, pr), dtype=np.float32)
        got = np.array(rn.coefficients(m, pr), dtype=np.float32)
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (m, pr, want, got)


@pytest.mark.parametrize("name,matrix", READ_MATRICES, ids=[n for n, _ in READ_MATRICES])
def test_oracle_open_equals_numpy_restatement_on_all_triples(name, matrix):
    """8-bit YCbCr 4:4:4 -> RGB8, all 2^24 triples, both ranges: oracle_read_rows against YuvLookupTables.cpp:157-190 and
    YuvDecode.cpp:312-326 restated in numpy float32."""
    planes = xi.all_triples_444()
    for fr in (1, 0):
        want = rn.read8_rgb(planes, matrix, bool(fr))
        got = harness.oracle_read(_read_desc(planes, matrix, fr), planes)
        bad = np.argwhere(want != got)
        assert len(bad) == 0, (name, fr, len(bad), bad[:5].tolist())


def test_oracle_open_equals_numpy_restatement_gbr_lattice():
    """The GBR identity matrix in a YCbCr image (identity chroma table, BT.601 coefficients: YuvLookupTables.cpp:177-180,
    YUVCoefficiants.cpp:171-183) on the 64^3 lattice, both ranges."""
    planes = xi.lattice64()
    for fr in (1, 0):
        want = rn.read8_rgb(planes, pkg.MATRIX_RGB_GBR, bool(fr))
        got = harness.oracle_read(_read_desc(planes, pkg.MATRIX_RGB_GBR, fr), planes)
        assert np.array_equal(want, got), fr


WRITE_MATRICES = [("bt601", pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), ("bt709", pkg.MATRIX_BT709, pkg.PRIMARIES_BT709),
                  ("bt2020ncl", pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020),
                  ("chromaderived432", pkg.MATRIX_CHROMA_DERIVED_NCL, pkg.PRIMARIES_SMPTE432), ("gbr", pkg.MATRIX_RGB_GBR, pkg.PRIMARIES_BT709)]


@pytest.mark.parametrize("bits", [8, 10, 12])
@pytest.mark.parametrize("name,matrix,primaries", WRITE_MATRICES, ids=[n for n, _, _ in WRITE_MATRICES])
def test_oracle_save_equals_numpy_restatement_on_all_triples(name, matrix, primaries, bits):
    """RGB8, all 2^24 triples -> Y, Cb, Cr 4:4:4 at 8, 10 and 12 bit: oracle_write_rows against the rescale table of
    WriteHeifImage.cpp:87-112 and libheif's RGB -> YCbCr restated in numpy float32."""
    src = xi.interleaved(xi.all_triples_444())               # R = plane 0, G = plane 1, B = plane 2
    d = pkg.WriteDesc(width=4096, height=4096, depth=8, planes=3, bit_depth=bits, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR,
                      chroma=pkg.CHROMA_444, matrix_coefficients=matrix, color_primaries=primaries)
    got = harness.oracle_write(d, src)
    tables = rn.write8_code_tables(matrix, bits, primaries)
    p = xi.all_triples_444()
    for pl in range(3):
        want = tables[pl][p[0], p[1], p[2]]                  # the [r, g, b] tables, indexed with the document's own channels
        assert np.array_equal(want, got[pl]), (name, bits, pl, int((want != got[pl]).sum()))
