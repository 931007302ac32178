"""Documents that carry the hunted code triples of tests/tie_inputs.py into a save, and the matrices the tie tests run under.  Shared
by tests/test_zzzzzzzz_tie_inputs.py (CPU: the claims, the oracle against numpy) and tests/test_zzzzzzzzz_gpu_tie_triples.py.

A save's stage A turns the document's samples into codes; what is hunted is stage B, on codes.  So every document here is built FROM
its codes -- a 16-bit document takes an end of each code's source interval (the two complementary phases of
exhaustive_inputs.ends_for_triples), a 32-bit document the float in the middle of it -- and stage_a_codes() asserts that the
oracle's interleaved hand-off (OUT_REFERENCE) returns exactly those codes.
"""
import functools

import numpy as np

import exhaustive_inputs as xi
import harness
import reference_numpy as rn
import tie_inputs as ti
import truth64
from test_zz_gpu_whole_domain_write import _source16

pkg = harness.pkg

# the four non-identity matrices of the whole-domain tests (MATRICES16 of the opens, MATRICES without GBR of the saves)
MATRICES = [("bt601", pkg.MATRIX_BT601, pkg.PRIMARIES_BT709), ("bt709", pkg.MATRIX_BT709, pkg.PRIMARIES_BT709),
            ("bt2020ncl", pkg.MATRIX_BT2020_NCL, pkg.PRIMARIES_BT2020),
            ("chromaderived432", pkg.MATRIX_CHROMA_DERIVED_NCL, pkg.PRIMARIES_SMPTE432)]
MATRIX_IDS = [m[0] for m in MATRICES]
PQ_PEAK = 1000


def kr_kb(matrix, primaries):
    kr, _, kb = rn.coefficients(matrix, primaries)
    return kr, kb


def open_document(bits, matrix, primaries, full_range, chroma):
    return ti.open_ties(bits, *kr_kb(matrix, primaries), full_range, chroma)


def save_codes(bits, matrix, primaries, chroma):
    """(R, G, B) code planes of the side-by-side document, uint16."""
    return ti.save_document(bits, *kr_kb(matrix, primaries), chroma)


def rgb16_document(codes, bits, phase, alpha=None):
    """Interleaved RGB16 / RGBA16 (straight alpha): each colour code at the smallest or the largest 16-bit value that rescales to it,
    the end chosen from the other two codes' parity (phase 1: the other end); an alpha code at the end its pixel's R + G + B parity
    picks."""
    r, g, b = codes
    ends = xi.ends_for_triples(r, g, b, phase)
    chans = {k: _source16(codes[k], ends[k], bits) for k in range(3)}
    if alpha is not None:
        chans[3] = _source16(alpha, (r.astype(np.uint32) + g + b + phase) & 1, bits)
    return xi.interleaved(chans, tuple(range(len(chans))))


@functools.lru_cache(maxsize=None)
def _float_for_code(bits, transfer):
    codes = np.arange(1 << bits)
    if transfer == pkg.TRANSFER_PQ:
        return ti.pq_source_for_codes(codes, bits, lambda v: truth64.pq_to_linear64(v, PQ_PEAK))
    assert transfer == pkg.TRANSFER_CLIP
    return ti.pq_source_for_codes(codes, bits, lambda v: v)


def f32_document(codes, bits, transfer, alpha=None):
    """Interleaved RGB / RGBA float32 (straight alpha): per colour code the float whose curve value (PQ at PQ_PEAK nits by the float64
    inverse of tests/truth64.py, or Clip) is the middle of the code's interval; alpha (code + 0.5) / max, opaque exactly 1."""
    table = _float_for_code(bits, transfer)
    chans = {k: table[codes[k]] for k in range(3)}
    if alpha is not None:
        maxc = (1 << bits) - 1
        chans[3] = np.minimum((alpha.astype(np.float32) + np.float32(0.5)) / np.float32(maxc), np.float32(1))
    return xi.interleaved(chans, tuple(range(len(chans))))


def stage_a_codes(d, src, codes, alpha=None):
    """Assert that the ORACLE's stage A (its OUT_REFERENCE save of the same document) gives exactly the intended codes."""
    ref = pkg.WriteDesc(width=d.width, height=d.height, depth=d.depth, planes=d.planes, bit_depth=d.bit_depth, transfer=d.transfer,
                        peak_nits=d.peak_nits, alpha_state=d.alpha_state, output=pkg.OUT_REFERENCE)
    got = harness.oracle_write(ref, src)[0].reshape(d.height, d.width, d.planes)
    for k, want in enumerate(tuple(codes) + (() if alpha is None else (alpha,))):
        assert np.array_equal(got[..., k], want), (k, int((got[..., k] != want).sum()))
