"""avifgpu_cli write --thumbnail BBOX THUMB.planes: the thumbnail of a save through the FormatRecord shim, armed around the shim's call,
written in the raw form of the main planes.  The file equals avifgpu_thumbnail_from_sums of the numpy box sums of the ORACLE's planes."""
import os
import subprocess

import numpy as np
import pytest

import harness
from test_thumbnail import box_sums, thumb_codes

pkg = harness.pkg
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "avif-format_amd", "avifgpu_cli")


def _run(tmp_path, d, src, extra, thumb=("--thumbnail", "64")):
    (tmp_path / "in.raw").write_bytes(src.tobytes())
    args = [CLI, "write", "--width", str(d.width), "--height", str(d.height), "--depth", str(d.depth), "--planes", str(d.planes),
            "--bits", str(d.bit_depth), *extra]
    if thumb:
        args += [*thumb, str(tmp_path / "thumb.planes")]
    return subprocess.run(args + [str(tmp_path / "in.raw"), str(tmp_path / "out.planes")], capture_output=True, text=True, timeout=300)


def test_cli_thumbnail_of_an_rgb8_save(tmp_path):
    d = pkg.WriteDesc(width=300, height=200, depth=8, planes=3, bit_depth=8, alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_REFERENCE)
    src = harness.make_write_source(d, seed=64)
    want = harness.oracle_write(d, src)
    r = _run(tmp_path, d, src, [])
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["thumbnail 64x43"], r.stdout
    assert pkg.thumbnail_fit(d, 64) == (64, 43)
    sums = box_sums(want, d, 64, 43)
    ref = pkg.thumbnail_from_sums(d, 64, 43, np.ascontiguousarray(sums.reshape(-1)).astype(np.uint64))
    assert np.array_equal(ref[0], thumb_codes(sums, d, 64, 43)[0])
    assert (tmp_path / "thumb.planes").read_bytes() == ref[0].tobytes()
    assert (tmp_path / "out.planes").read_bytes() == want[0].tobytes()              # the main planes are what they are without the option
    # without the option: nothing on stdout, no file
    os.remove(tmp_path / "thumb.planes")
    r = _run(tmp_path, d, src, [], thumb=None)
    assert r.returncode == 0 and r.stdout == "" and not (tmp_path / "thumb.planes").exists()
    assert (tmp_path / "out.planes").read_bytes() == want[0].tobytes()


def test_cli_thumbnail_of_a_tiled_ycbcr_save_with_alpha(tmp_path):
    d = pkg.WriteDesc(width=301, height=230, depth=16, planes=4, bit_depth=10, alpha_state=pkg.ALPHA_STRAIGHT, output=pkg.OUT_YCBCR,
                      chroma=pkg.CHROMA_420, matrix_coefficients=pkg.MATRIX_BT601, color_primaries=pkg.PRIMARIES_BT709, full_range=1,
                      chroma_downsampling=pkg.DOWNSAMPLE_NEAREST)
    src = harness.make_write_source(d, seed=65)
    want = harness.oracle_write(d, src)
    r = _run(tmp_path, d, src, ["--alpha", "straight", "--ycbcr", "420", "--maxdata", str(src.strides[0] * 6)], thumb=("--thumbnail", "100"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["thumbnail 100x76"], r.stdout
    assert int(r.stderr.split(" tiles")[0].split()[-1]) >= 24, r.stderr
    ref = thumb_codes(box_sums(want, d, 100, 76), d, 100, 76)
    assert (tmp_path / "thumb.planes").read_bytes() == b"".join(ref[pl].tobytes() for pl in range(4))
    # a bounding box the geometry clamps: 4:2:0 chroma is 151 x 115
    r = _run(tmp_path, d, src, ["--alpha", "straight", "--ycbcr", "420"], thumb=("--thumbnail", "4000"))
    assert r.returncode == 0 and r.stdout.splitlines() == ["thumbnail 151x115"], r.stdout + r.stderr


def test_cli_usage_names_the_option(tmp_path):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--thumbnail BBOX THUMB.planes" in r.stderr
    r = subprocess.run([CLI, "write", "--width", "8", "--height", "8", "--thumbnail", "0", "t", "a", "b"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "bounding box" in r.stderr
