"""The 256-entry PQ exponent tables (csrc/device_math.h): same codes as the 512-entry tables they replace, on every exponent field and
sign, and a table fill and barrier that hold at every workgroup geometry.

Exponent-field sweep.  The close PQ form indexes its tables with the exponent field of t = sample * mult alone; a set sign bit no
longer selects an entry (F = 0, N = -100 -> code 0) but reaches v_log_f32, whose NaN the clamp of the last v_exp_f32 turns into
code 0.  All 512 sign + exponent fields x 5 mantissas (tests/pq_exponent_fields.py: 2 560 floats, each in every channel slot of a
512 x 15 RGB document) go through every kernel that evaluates the form and can show stage-A codes, at 10 and 12 bit, 80 nits, and
must give the codes recorded from the 512-entry build (tests/golden/pq_exponent_fields_codes.npz, written by
tests/golden/make_pq_exponent_fields_codes.py) -- and the rule itself: sign bit set or NaN => code 0.

Workgroup geometry.  The headline kernel's workgroup copies the tables once, under its first span's loads, and meets at one barrier
(none for a single-wave workgroup).  The launcher has two workgroups for it: two waves where every span lies on 128-byte lines, four
waves where rows start inside a line; each shape runs in both layouts -- "tight" (rows padded to 16 bytes plus guard samples) and
"lines" (source and plane rows padded to 128 bytes) -- and the capped launch's label shows which workgroup took it.  Widths
{1, 7, 511, 512, 513, 1025} x rows {1, 2, 3, 5, 9} at 10 bit give 1 ... 27 spans: fewer spans than a workgroup has waves (waves
beyond the tile must still fill their share and reach the barrier), ragged last spans, and
-- with the tuning word's grid cap at ONE workgroup -- span loops of three and more trips whose last trip leaves some waves of the
workgroup inside the tile and others beyond it.  Planes are pre-filled with a sentinel above every code, with a guard row before
and after and guard samples behind every row.  The codes equal those of write_px (tuning word 0) on the same input, lie within the
float-tier rule against the oracle (|delta code| <= 1, harness.T2_MIN_EXACT or a handful of samples), and nothing outside the image
is written.

(The file's name makes it the last one collected, after tests/test_zzzzz_gpu_icc_table_cache.py: every earlier test of the suite keeps
its place in the collection order.)"""
import os
import re

import numpy as np
import pytest

import harness
import pq_exponent_fields as pf

pkg = harness.pkg
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pq_exponent_fields_codes.npz")


# ---- exponent-field sweep ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k].astype(np.int32) for k in z.files}


def _must_be_zero(planes):
    """(7 680, channels) bool: the samples whose sign bit is set or that are NaN."""
    px = pf.gray() if planes == 1 else pf.rgb()
    return np.signbit(px) | np.isnan(px)


def test_the_sweep_holds_every_field_and_sign():
    v = pf.floats()
    bits = v.view(np.uint32)
    assert v.shape == (2560,) and len(set(bits.tolist())) == 2560
    assert set((bits >> 23).tolist()) == set(range(512))
    for special in (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xFF7FFFFF):
        assert special in bits, hex(special)
    px = pf.rgb()
    assert px.shape == (pf.WIDTH * pf.HEIGHT, 3)
    for c in range(3):                                                   # every float in every channel slot
        assert np.array_equal(px[c::3, c].view(np.uint32), bits)
    assert int(_must_be_zero(3).sum()) == 3 * (1280 + 4) and int(_must_be_zero(1).sum()) == 3 * (1280 + 4)


@pytest.mark.parametrize("bits", pf.DEPTHS)
@pytest.mark.parametrize("form", pf.FORMS, ids=[f[0] for f in pf.FORMS])
def test_exponent_fields_give_the_recorded_codes(gpu, recorded, form, bits):
    name, planes = form[0], form[1]
    got = pf.run(gpu, form, bits)
    want = recorded[f"{name}_b{bits}"]
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    print(f"{gpu.last_kernel()}: {bad.shape[0]} of {got.size} codes differ from the record")
    src = pf.gray() if planes == 1 else pf.rgb()
    assert bad.shape[0] == 0, [(int(p), int(c), hex(int(src[p, c].view(np.uint32))), int(got[p, c]), int(want[p, c])) for p, c in bad[:6]]
    zero = _must_be_zero(planes)
    assert (got[zero] == 0).all(), (name, bits, "sign bit set or NaN must give code 0",
                                    [hex(int(b)) for b in src[zero][got[zero] != 0][:6].view(np.uint32)])


# ---- workgroup geometry --------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 7, 511, 512, 513, 1025)
ROWS = (1, 2, 3, 5, 9)
SPAN_PX = 512
GUARD = 8                                # samples (at least) behind every row, and one whole row before and after each plane
WAVES = {"tight": 4, "lines": 2}         # waves of the workgroup the launcher picks for the layout (csrc/write_kernels.hip: AG_HOT444_BLOCK, _LINES)


def _geometry_desc(width, rows):
    return pkg.WriteDesc(width=width, height=rows, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=80,
                         alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444,
                         matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)


def _guarded_save(gpu, d, src_np, word, kernel, layout="tight"):
    """The whole frame into guarded planes; returns ({plane: (rows, width) codes}, label) after asserting that every guard sample
    kept its fill.  layout "lines": source rows and plane rows are multiples of 128 bytes from 128-byte aligned bases."""
    import torch
    dev = f"cuda:{gpu.device}"
    if layout == "lines":
        src = torch.zeros((d.height, harness.align(src_np.shape[1], 32)), dtype=torch.float32, device=dev)
        src[:, :src_np.shape[1]] = torch.from_numpy(src_np).to(dev)
        stride = harness.align(d.width + GUARD, 64)
    else:
        src = torch.from_numpy(src_np).to(dev)
        stride = harness.align(d.width * 2, 16) // 2 + GUARD
    out = {pl: torch.full((d.height + 2, stride), pf.FILL, dtype=torch.int16, device=dev) for pl in range(3)}
    ptrs = [out[pl][1].data_ptr() for pl in range(3)] + [None]
    assert layout != "lines" or all(v % 128 == 0 for v in ptrs[:3] + [src.data_ptr(), src.stride(0) * 4, stride * 2])
    strides = [stride * 2] * 3 + [0]
    gpu.lib.avifgpu_set_hot_variant(word)
    try:
        gpu.write_rows(d, 0, d.height, src.data_ptr(), src.stride(0) * 4, ptrs, strides, mem=pkg.MEM_DEVICE,
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    finally:
        gpu.lib.avifgpu_set_hot_variant(pf.DEFAULT_WORD)
    label = gpu.last_kernel()
    assert label.startswith(kernel + "<"), (label, kernel)
    torch.cuda.synchronize(dev)
    codes = {}
    for pl in range(3):
        a = out[pl].cpu().numpy().astype(np.int32)
        assert (a[0] == pf.FILL).all() and (a[-1] == pf.FILL).all(), (label, pl, "a row outside the image was written")
        assert (a[1:-1, d.width:] == pf.FILL).all(), (label, pl, "samples behind a row were written")
        codes[pl] = a[1:-1, :d.width]
        assert (codes[pl] != pf.FILL).all(), (label, pl, "samples of the image were left unwritten")
    return codes, label


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", WIDTHS)
def test_every_workgroup_geometry_fills_its_table(gpu, width, rows):
    d = _geometry_desc(width, rows)
    src = harness.make_write_source(d, seed=77)
    src.reshape(-1)[1::7] *= np.float32(-1.0)                            # negatives among the few samples of the tiny frames too
    spans = -(-width // SPAN_PX) * rows
    ref, _ = _guarded_save(gpu, d, src, pf.GENERIC, "write_px")
    want = harness.oracle_write(d, src)
    st = harness.compare_write(d, want, {pl: ref[pl].astype(np.uint16) for pl in ref})
    print(f"{width} x {rows}: {spans} spans; write_px against the oracle: exact {st['exact_frac']:.5f} max {st['max_abs']}")
    assert st["max_abs"] <= 1 and harness.t2_exact_ok(st, harness.T2_MIN_EXACT[10]), st
    for layout, waves in WAVES.items():
        for word in (pf.DEFAULT_WORD, pf.DEFAULT_WORD | (1 << 8)):       # as dispatched; then ONE workgroup walks the whole tile
            got, label = _guarded_save(gpu, d, src, word, "write_rgb32_ycbcr444_hot", layout)
            assert "pxl=8" in label, label
            m = re.search(r" cap=(\d+)/(\d+)", label)
            trips = -(-spans // waves)                                   # of the one workgroup: it stands in for `trips` workgroups
            if word >> 8 and trips > 1:
                # From 9 spans on that is three trips and more, and an odd span count leaves the last trip with waves of the
                # workgroup on both sides of the tile's end.
                assert m is not None and (int(m.group(1)), int(m.group(2))) == (1, trips), (label, layout, spans)
            else:
                assert m is None, label
            for pl in range(3):
                bad = np.argwhere(got[pl] != ref[pl])
                assert bad.shape[0] == 0, (label, layout, pl, bad[:4].tolist())
            print(f"{layout}: {label}: equal to write_px")
    assert spans < 9 or -(-spans // max(WAVES.values())) >= 3
