"""The device copies of a save's ICC tables (csrc/icc_tables.cpp): one cache record per HIP device and table kind, brought up to date by
one primitive.  These tests hold what a caller can see of it, on device pointers and tiles of 256 x 16 -- the code under test is host
code in front of the launch:

  * two tables alternating, for each of the six entry kinds: a save never sees the other table;
  * a table rewritten in place: the kinds verified once per device and epoch (33^3 table: tests/test_icc16.py; sampled curves: here) keep
    the old result in a call that continues the previous one and see the new one in any other; the kinds compared on every call
    (8-bit shaper, stage program) see it at once;
  * the 16-bit and the 8-bit-LUT saves share one record; the records are per device; a rejected table costs no upload and harms nothing.

Every "differs" is first established on the CPU, with the checkers the suite already has (truth64.icc_stage64, the numpy tetrahedral of
tests/test_icc16.py, MatShaperEval16 as in tests/test_icc8.py, icc32_programs.eval_host)."""
import ctypes

import numpy as np
import pytest

import harness
import icc32_programs as ip
import icc_profiles
import truth64
from test_icc16 import _tetrahedral

pkg = harness.pkg
pytestmark = pytest.mark.gpu

W, H, TILE = 256, 64, 16
KINDS = ["parametric", "sampled", "clut16", "clut8", "shaper8", "program"]
GREY = {32: np.float32(0.5), 16: np.uint16(16384), 8: np.uint8(128)}
DTYPE = {32: np.float32, 16: np.uint16, 8: np.uint8}
PROFILE_A, PROFILE_B = "adobergb-gamma2.2", "p3-para-gamma1.8"
SAMPLED_A, SAMPLED_B = "p3-sampled-srgb-1024", "adobergb-sampled-per-channel-256"
TIER_A = ip.tier_a_programs()


def _desc(kind):
    depth = {"parametric": 32, "sampled": 32, "program": 32, "clut16": 16}.get(kind, 8)
    kw = dict(transfer=pkg.TRANSFER_CLIP, peak_nits=1000) if depth == 32 else {}
    return pkg.WriteDesc(width=W, height=H, depth=depth, planes=3, bit_depth=8 if depth == 8 else 12, alpha_state=pkg.ALPHA_NONE,
                         output=pkg.OUT_REFERENCE, **kw)


def _copy(t):
    """The same contents at another address."""
    return type(t).from_buffer_copy(t)


@pytest.fixture(scope="module")
def tables(gpu):
    """kind -> (A, B): two different tables of that kind, each at an address of its own and private to this module."""
    icc = {n: icc_profiles.profile_bytes(n) for n in (PROFILE_A, PROFILE_B)}
    t = {"parametric": tuple(_copy(icc_profiles.prepared(n, icc_profiles.REC2020)) for n in (PROFILE_A, PROFILE_B)),
         "sampled": tuple(_copy(icc_profiles.prepared(n, icc_profiles.REC2020)) for n in (SAMPLED_A, SAMPLED_B)),
         "clut16": tuple(gpu.icc_prepare_clut16(icc[n]) for n in (PROFILE_A, PROFILE_B)),
         "shaper8": tuple(gpu.icc_prepare_shaper8(icc[n]) for n in (PROFILE_A, PROFILE_B)),
         "program": (ip.stamp(ip.build(TIER_A["clut 9x9x9"][0])), ip.stamp(ip.build(ip.composition())))}
    t["clut8"] = tuple(_copy(x) for x in t["clut16"])      # an 8-bit document behind a LUT-based profile takes the same kind of table
    return t


def _grey_reference(kind, table):
    """What the CPU checkers give for the grey pixel of the tile, in units of the output code."""
    if kind in ("parametric", "sampled"):
        return truth64.icc_stage64(table, np.full((1, 3), GREY[32]))[0].reshape(3) * 4095.0
    if kind == "program":
        return ip.eval_host(table, np.full((1, 3), GREY[32])).reshape(3).astype(np.float64) * 4095.0
    if kind in ("clut16", "clut8"):
        nodes = np.ctypeslib.as_array(table.table).reshape(33, 33, 33, 4)[..., :3]
        word = 128 * 257 if kind == "clut8" else 32768          # the grey sample as the 16-bit word the interpolation is entered with
        return _tetrahedral(nodes, np.full((1, 3), word)).reshape(3) / (257.0 if kind == "clut8" else 16.0)
    s1, M, s2 = np.array(table.shaper1, dtype=np.int64), np.array(table.matrix, dtype=np.int64), np.array(table.shaper2, dtype=np.uint8)
    lin = s1[:, int(GREY[8])]                                   # MatShaperEval16, as tests/test_icc8.py restates it
    return np.array([s2[i][np.clip((M[i] @ lin + 0x2000) >> 14, 0, 16384)] for i in range(3)], dtype=np.float64)


def _differ_on_the_cpu(kind, a, b):
    ra, rb = _grey_reference(kind, a), _grey_reference(kind, b)
    assert np.abs(ra - rb).max() >= 2.0, (kind, ra, rb)         # two codes: more than any rounding of either evaluation


class Saver:
    """Saves of rows [row0, row0 + nrows) of a constant grey document of `kind` on device pointers of one device."""

    def __init__(self, gpu, kind, device=None):
        import torch
        self.torch, self.gpu, self.d = torch, gpu, _desc(kind)
        self.device = gpu.device if device is None else device
        self.dev = f"cuda:{self.device}"
        row = np.full((H, W * 3), GREY[self.d.depth], dtype=DTYPE[self.d.depth])
        self.src = torch.from_numpy(row.view(np.uint8)).to(self.dev)
        self.out_dtype = np.uint8 if self.d.bit_depth == 8 else np.uint16
        self.out_row_bytes = W * 3 * np.dtype(self.out_dtype).itemsize

    def __call__(self, table, row0=0, nrows=TILE):
        torch = self.torch
        with torch.cuda.device(self.device):                    # the cache is keyed by the calling thread's current device
            out = torch.zeros((H, self.out_row_bytes), dtype=torch.uint8, device=self.dev)
            self.gpu.write_rows(self.d, row0, nrows, self.src[row0].data_ptr(), self.src.stride(0), [out[row0].data_ptr(), None, None, None],
                                [self.out_row_bytes, 0, 0, 0], mem=pkg.MEM_DEVICE, stream=torch.cuda.current_stream(self.dev).cuda_stream, icc=table)
            torch.cuda.synchronize(self.dev)
        return out[row0:row0 + nrows].cpu().numpy().view(self.out_dtype)


# ---- 1: two tables alternating ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_tables_alternating(gpu, tables, kind):
    a, b = tables[kind]
    _differ_on_the_cpu(kind, a, b)
    save = Saver(gpu, kind)
    o = [save(t) for t in (a, b, a, b)]                         # every save starts at row 0
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])
    assert not np.array_equal(o[0], o[1])
    assert (o[0] == o[0][0, :3].tolist() * W).all()             # a constant tile stays constant


# ---- 2: sampled curves rewritten in place: verified once per device and epoch ----------------------------------------------------------------
def _rewrite_sampled_grey(t):
    """Change what channel 0 of a sampled table gives the grey sample, at words the strided fingerprint does not read: curve[0][32768]
    (the memory path's lookup) and table16[0][511..512] (the entries the LDS path interpolates between for a 1024-entry curve)."""
    assert t.entries[0] == 1024
    words = (ctypes.sizeof(t.curve) + ctypes.sizeof(t.table16)) // 4     # the span the library fingerprints: curve[] and table16[]
    step = words // 4096
    assert step == 49                                           # table_fingerprint: words 0, 49, 98, ... and the last (tools/icc_tables_check.cpp)
    curve_words = ctypes.sizeof(t.curve) // 4
    for word in (32768, curve_words + 511 // 2, curve_words + 512 // 2):
        assert word % step != 0 and word != words - 1, word
    t.curve[0][32768] += 0.25
    t.table16[0][511] = (t.table16[0][511] + 0x2000) & 0xffff
    t.table16[0][512] = (t.table16[0][512] + 0x2000) & 0xffff


def test_sampled_curves_rewritten_in_place_between_two_tile_calls_are_seen(gpu, tables):
    """tests/test_icc16.py::test_gpu_table_rewritten_in_place_between_two_tile_calls_is_seen for avifgpu_icc_sampled32: a tile at row0 = 16
    converted twice with the SAME struct, rewritten in between where the fingerprint does not look, comes out like a fresh struct."""
    t = _copy(tables["sampled"][0])
    save = Saver(gpu, "sampled")
    first = save(t, 16, 32)
    _rewrite_sampled_grey(t)
    second = save(t, 16, 32)                                    # same address, same fingerprint, not a continuation
    third = save(_copy(t), 16, 32)
    assert not np.array_equal(first, third), "the rewrite must change the output of a grey tile"
    assert np.array_equal(second, third), "stale device copy of curves rewritten in place"


def test_sampled_curves_only_a_continuing_call_keeps_its_epoch(gpu, tables):
    """The epoch rule itself (tests/test_icc16.py has it for the 33^3 table): the next tile of the same save trusts the fingerprint, a call
    further down re-verifies the curves and sees a rewrite the fingerprint misses."""
    original = tables["sampled"][0]
    changed = _copy(original)
    _rewrite_sampled_grey(changed)
    save = Saver(gpu, "sampled")
    old, new = save(_copy(original), 8, 8), save(changed, 8, 8)               # fresh structs: what each contents give
    assert not np.array_equal(old, new), "the rewrite must change the output of a grey tile"
    t = _copy(original)
    assert np.array_equal(save(t, 8, 8), old)                   # rows [8, 16)
    _rewrite_sampled_grey(t)
    assert np.array_equal(save(t, 16, 8), old)                  # rows [16, 24): the contract says the table is immutable here, the cheap check runs
    assert np.array_equal(save(t, 40, 8), new), "a call that does not continue the previous one must re-verify the curves"


# ---- 3: the 8-bit shaper and the stage program are compared on every call ------------------------------------------------------------------------
def _rewrite_shaper(t):
    t.shaper1[0][int(GREY[8])] = t.shaper1[0][int(GREY[8])] // 2                # what the red of the grey sample enters the matrix with


def _rewrite_program(t):
    # another proven program at the same address, of the same size (stages and words): other nodes in the 9 x 9 x 9 grid of tables["program"][0]
    n = (t.stage_count, t.word_count)
    ip.stamp(ip.fill_into(t, [("clut", ip.seeded_grid((9, 9, 9), 99), 5), ip.TAIL]))
    assert (t.stage_count, t.word_count) == n


@pytest.mark.parametrize("kind,rewrite", [("shaper8", _rewrite_shaper), ("program", _rewrite_program)])
def test_rewrite_in_place_is_seen_by_a_continuing_call(gpu, tables, kind, rewrite):
    t = _copy(tables[kind][0])
    changed = _copy(t)
    rewrite(changed)
    _differ_on_the_cpu(kind, t, changed)
    save = Saver(gpu, kind)
    old, new = save(_copy(t), TILE, TILE), save(_copy(changed), TILE, TILE)   # fresh structs: what each contents give
    assert not np.array_equal(old, new)
    assert np.array_equal(save(t, 0, TILE), old)
    rewrite(t)                                                  # same address
    assert np.array_equal(save(t, TILE, TILE), new), "stale device copy: row0 continues the previous call, and these kinds are compared on every call"


# ---- 4: the 16-bit and the 8-bit-LUT saves share one device buffer ---------------------------------------------------------------------------
def test_16bit_and_8bit_lut_saves_share_one_record(gpu, tables):
    t, t8 = tables["clut16"][0], tables["clut8"][1]              # T and T': different contents
    _differ_on_the_cpu("clut8", tables["clut8"][0], t8)
    save16, save8 = Saver(gpu, "clut16"), Saver(gpu, "clut8")
    alone = save8(t8)                                           # on its own sequence
    assert not np.array_equal(alone, save8(tables["clut8"][0]))
    o1, o2, o3 = save16(t), save8(t8), save16(t)
    assert np.array_equal(o1, o3)
    assert np.array_equal(o2, alone), "the 8-bit-LUT save ran on the table the 16-bit save left in the shared buffer"


# ---- 5: the records are per device ---------------------------------------------------------------------------------------------------------------
def test_caches_are_per_device(gpu, tables):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    for kind in ("clut16", "sampled", "program"):
        a, b = tables[kind]
        first, second = Saver(gpu, kind, 0), Saver(gpu, kind, 1)
        on0 = first(a)
        other = second(b)
        on1 = second(a)                                         # device 1 holds B; a record keyed by kind alone would call A current
        assert np.array_equal(on1, on0) and not np.array_equal(on1, other), kind


# ---- 6: validation comes before the upload -----------------------------------------------------------------------------------------------------
def test_a_rejected_sampled_table_is_refused_as_ever_and_harms_nothing(gpu, tables):
    a, b = tables["sampled"]
    save = Saver(gpu, "sampled")
    want = save(_copy(b))
    save(a)
    bad = _copy(a)
    bad.parametric_mask = 7
    with pytest.raises(pkg.AvifGpuError) as err:
        save(bad)
    assert err.value.code == pkg.formatBadParameters
    assert "sampled ICC curves: parametric_mask must leave at least one sampled channel" in str(err.value)
    assert np.array_equal(save(b), want)                        # a different table than the rejected one and than the one before it


