"""The one pool of staging slots behind the host-pointer calls of the oriented, upsampled and cropped opens (csrc/staged_open.cpp).

A slot's buffers grown by one feature are reused by the next: the sequence below makes every buffer change hands -- a crop's staged
rectangle, then the whole image's planes (larger: they grow), then the upsampled open's chroma WINDOWS where planes were, then a 1 x 1
crop that asks for nothing (the 256-byte floor), then the first call again -- in one process, and each result must be byte-equal to the
SAME entry called with device pointers, which uses no pool at all.  Padding and guard rows of every destination must come back untouched
(the openers of the three features' own test files check that).  After a shutdown the pool has to come back.

130 x 66, 4:2:0 with alpha: odd in chroma, rows that end off the 16-byte grid.

The file sorts behind the three features' own test files (and all the others), as the suite's other late additions do: in a run of the
whole suite the pool it meets has already been grown and shrunk by every one of them, and no earlier test's place in the run moves."""
import pytest

import harness
from test_gpu_crop import open_cropped, same
from test_gpu_orientation import open_oriented
from test_gpu_upsample import open_upsampled
from upsample_truth import CENTER, NEAREST

pkg = harness.pkg
pytestmark = pytest.mark.gpu

W, H = 130, 66
ODD_RECT, ONE_PIXEL = (3, 5, 120, 55), (7, 9, 1, 1)            # (7, 9): every plane's host pointer is off the 16-byte grid, so the call is staged

FORMATS = {
    "8 bit": dict(bit_depth=8, depth=8, matrix_coefficients=pkg.MATRIX_BT601),
    "12 bit to f32": dict(bit_depth=12, depth=32, transfer_characteristics=pkg.TC_PQ, color_primaries=pkg.PRIMARIES_BT2020,
                          matrix_coefficients=pkg.MATRIX_BT2020_NCL, pq_peak_nits=1000),
}


def _calls(g, desc, planes, **kw):
    """The sequence, as (name, opener); kw: the memory kind and the destination's padding."""
    return [
        ("cropped, odd origin, code 6", lambda: open_cropped(g, desc, planes, ODD_RECT, NEAREST, 6, **kw)),
        ("oriented, code 3, whole image", lambda: open_oriented(g, desc, planes, 3, **kw)),
        ("upsampled CENTER, code 8", lambda: open_upsampled(g, desc, planes, CENTER, 8, **kw)),
        ("cropped, 1 x 1, code 1", lambda: open_cropped(g, desc, planes, ONE_PIXEL, NEAREST, 1, **kw)),
        ("cropped, odd origin, code 6, again", lambda: open_cropped(g, desc, planes, ODD_RECT, NEAREST, 6, **kw)),
    ]


@pytest.mark.parametrize("name", list(FORMATS))
def test_buffers_change_hands_between_features(gpu, name):
    desc = pkg.ReadDesc(width=W, height=H, colorspace=pkg.COLORSPACE_YCBCR, chroma=pkg.CHROMA_420, alpha_state=pkg.ALPHA_STRAIGHT, **FORMATS[name])
    planes = harness.make_read_source(desc, seed=77)
    device = [(what, run()) for what, run in _calls(gpu, desc, planes, mem="device")]
    host = dict(mem="host", pad=5, guard_rows=2)
    for (what, run), (_, want) in zip(_calls(gpu, desc, planes, **host), device):
        assert same(run(), want), (name, what)
    try:
        gpu.lib.avifgpu_shutdown()                             # releases the pool
        g = pkg.AvifGpu(gpu.device)
        what, run = _calls(g, desc, planes, **host)[0]
        assert same(run(), device[0][1]), (name, what, "after shutdown and a new init")
    finally:
        pkg.AvifGpu(gpu.device)                                # the session's binding
