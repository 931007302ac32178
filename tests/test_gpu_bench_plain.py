"""bench.py's PLAIN run (no --full): it times exactly --steps steps and prints the headline line without the diagnostics of --full, and
--dump-outputs writes what the last timed step computed -- checked here against the CPU oracle on the same seeded frame."""
import glob
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = harness.pkg
FULL_ONLY = ("c2", "c3", "c5", "d12", "d8", "open_d12", "open_d8", "pcie_inclusive", "cpu_baseline", "cold_launch")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_plain(tmp_path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out), *extra], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert key in d, key
    assert d["steps"] == 7 and d["warmup"] == 2 and d["profile_window"]["timed_launches"] == 7
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    assert "peak_measured" not in d["roofline"] and "same_buffers" not in d["roofline"]
    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / "*.npy"))}
    assert sum(os.path.getsize(f) for f in glob.glob(str(out / "*.npy"))) <= 64e6
    assert all(a.dtype == np.float32 for a in files.values())
    return d, files


def _oracle(width, height, rows=None):
    """The bench's seeded frame (bench.make_frame, same device and seed) through the CPU oracle: {plane: codes}, optionally rows only."""
    import torch
    bench = _bench_module()
    frame = bench.make_frame(torch, torch.device("cuda", 0), width, height, 3, 1234).cpu().numpy()
    desc = pkg.WriteDesc(width=width, height=height, depth=32, planes=3, bit_depth=10, transfer=pkg.TRANSFER_PQ, peak_nits=80,
                         alpha_state=pkg.ALPHA_NONE, output=pkg.OUT_YCBCR, chroma=pkg.CHROMA_444,
                         matrix_coefficients=pkg.MATRIX_BT2020_NCL, color_primaries=pkg.PRIMARIES_BT2020)
    if rows is None:
        return harness.oracle_write(desc, frame)
    got = [harness.oracle_write(desc, frame, row0=int(r), nrows=1) for r in rows]      # 4:4:4: every row stands alone
    return {pl: np.concatenate([g[pl] for g in got]) for pl in got[0]}


def test_plain_run_small_frame_dumps_whole_planes(tmp_path):
    _, files = _run_plain(tmp_path, "--width", "1024", "--height", "256", "--clock-ramp-ms", "20")
    assert sorted(files) == ["cb", "cr", "y"], sorted(files)
    want = _oracle(1024, 256)
    got = {i: files[n].astype(np.int64) for i, n in enumerate(("y", "cb", "cr"))}
    stats = harness.compare_write(pkg.WriteDesc(width=1024, height=256, depth=32, planes=3, bit_depth=10), want, got)
    assert stats["max_abs"] <= 1, stats


def test_plain_run_headline_size_dumps_a_seeded_sample(tmp_path):
    d, files = _run_plain(tmp_path)
    assert d["n_gpus"] == 1 and d["config"]["rows_per_gpu"] == 8192
    assert sorted(files) == ["cb_points", "cb_rows", "cr_points", "cr_rows", "y_points", "y_rows"], sorted(files)
    bench = _bench_module()
    rows, points = bench.dump_positions(8192, 8192, bench.DUMP_SAMPLES, 0)
    assert files["y_rows"].shape == (len(rows), 8192) and files["y_points"].shape == points.shape
    assert rows[0] == 0 and rows[-1] == 8191
    picks = {}                                                    # plane -> (positions in its _rows file, frame rows): first and last 8
    for i in range(3):
        r_i, _ = bench.dump_positions(8192, 8192, bench.DUMP_SAMPLES, i)
        at = np.concatenate([np.arange(8), np.arange(len(r_i) - 8, len(r_i))])
        picks[i] = (at, r_i[at])
    check = np.unique(np.concatenate([r for _, r in picks.values()]))
    want = _oracle(8192, 8192, rows=check)
    for i, n in enumerate(("y", "cb", "cr")):
        at, r = picks[i]
        got = files[n + "_rows"][at].astype(np.int64)
        assert np.abs(got - want[i][np.searchsorted(check, r)].astype(np.int64)).max() <= 1, n
