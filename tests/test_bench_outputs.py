"""bench.py --dump-outputs and --full.  The dump is the last timed step's frame
(accum.npy float32, ids.npy float64), the same from run to run and equal to the
frame --dump-frame saves; an output above the size limit is cut to a fixed,
seeded pixel sample.  A plain run leaves out what takes runs of its own (the
counting-instantiation step, the CPU baseline); --full reports them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

W, H, SPP = 72, 40, 2   # 9 x 5 tiles


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench_module()
    rng = np.random.default_rng(1)
    acc = rng.random((10, 13, 4), dtype=np.float32)
    ids = rng.integers(0, 2**32, size=(10, 13), dtype=np.uint32).view(np.int32)
    bench.dump_outputs(str(tmp_path / "whole"), acc, ids)
    a, i = np.load(tmp_path / "whole" / "accum.npy"), np.load(tmp_path / "whole" / "ids.npy")
    assert a.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(a, acc.reshape(-1, 4)) and np.array_equal(i, ids.view(np.uint32).reshape(-1))
    assert not os.path.exists(tmp_path / "whole" / "pixels.npy")
    # above the limit: the same seeded sample every time, within the limit in all
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 32 * 50 + 3 * 128)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), acc, ids)
    px = np.load(tmp_path / "s1" / "pixels.npy")
    assert np.array_equal(px, np.load(tmp_path / "s2" / "pixels.npy"))
    assert len(px) == 50 and len(set(px)) == 50 and np.all(np.diff(px) > 0)
    sel = px.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s1" / "accum.npy"), acc.reshape(-1, 4)[sel])
    assert np.array_equal(np.load(tmp_path / "s1" / "ids.npy"), ids.view(np.uint32).reshape(-1)[sel])
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= 32 * 50 + 3 * 128


def _run(*extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "2", "--spp",
           str(SPP), "--width", str(W), "--height", str(H)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_frame(tmp_path):
    plain, err = _run("--dump-outputs", str(tmp_path / "a"), "--dump-frame", str(tmp_path / "a.npz"))
    full, err_full = _run("--full", "--cpu-budget", "0.2", "--dump-outputs", str(tmp_path / "b"))
    # the plain run: the headline and the timed steps' own figures, no run of its own beside them
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["cpu_baseline"] is None and plain["traversal_per_step"] is None and plain["simd_lane_util"] is None
    assert plain["roofline"]["algorithmic"] is None and plain["roofline"]["kernel_ms"] > 0
    assert "counting-instantiation" not in err and "counting-instantiation" in err_full
    assert full["cpu_baseline"]["value"] > 0 and full["traversal_per_step"]["trips"] > 0
    assert 0 < full["simd_lane_util"] <= 1 and full["roofline"]["algorithmic"]["bytes_per_launch"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "rays_per_step"):
        assert plain[k] == full[k]
    # the dump: the frame --dump-frame saves, bit for bit, and the same in both runs
    a, i = np.load(tmp_path / "a" / "accum.npy"), np.load(tmp_path / "a" / "ids.npy")
    assert a.dtype == np.float32 and a.shape == (W * H, 4) and i.dtype == np.float64 and i.shape == (W * H,)
    f = np.load(tmp_path / "a.npz")
    assert np.array_equal(a.view(np.uint32), f["accum"].reshape(-1, 4).view(np.uint32))
    assert np.array_equal(i, f["ids"].reshape(-1))
    assert np.array_equal(a.view(np.uint32), np.load(tmp_path / "b" / "accum.npy").view(np.uint32))
    assert np.array_equal(i, np.load(tmp_path / "b" / "ids.npy"))
