"""bench.py's plain run (one timed block of exactly --steps steps, nothing measured beside it) and --dump-outputs (what the
last timed step returned, the same arrays run after run for the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _same_arrays(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def _check_plain(d, steps):
    assert d["steps"] == steps and d["repeats"] == 1 and len(d["blocks_ms_per_step"]) == 1 and d["full"] is False
    assert d["ms_per_step"] == d["first_block_ms_per_step"] == d["blocks_ms_per_step"][0] > 0
    assert abs(d["value"] - d["config"]["K"] * steps / (d["ms_per_step"] * steps / 1e3)) < 1e-6 * d["value"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["cold"] is None and d["per_solve_ms"] is None and d["sustained"] is None
    assert "roofline" not in d and "stage_ms" not in d and "cpu_baseline" not in d


def test_plain_selftest_run_times_one_block_and_dumps_the_same_outputs(tmp_path):
    args = ["--gpus", "1", "--selftest-cpu", "--steps", "4", "--warmup", "2", "--K", "128", "--T", "20"]
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    _check_plain(a, 4)
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    oa, ob = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(oa) == {"control_seq", "control_hist"} and oa["control_seq"].shape == (20, 2)
    _same_arrays(oa, ob)


def test_dump_samples_long_vectors_with_a_fixed_seed(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_MAX_PER_ARRAY + 1000
    v = np.arange(n, dtype=np.float32)
    outs = {"costs": v, "weights": 2 * v, "U": np.ones((7, 2), np.float32), "traj_cost": np.array([3.0], np.float32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    _same_arrays(a, b)
    idx = a["sample_index_%d" % n]
    assert idx.dtype == np.float64 and idx.size == bench.DUMP_MAX_PER_ARRAY and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["costs"], v[idx.astype(np.int64)])
    np.testing.assert_array_equal(a["weights"], 2 * v[idx.astype(np.int64)])
    np.testing.assert_array_equal(a["U"], outs["U"])
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) < 64 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step_and_full_computes_the_same(tmp_path):
    """Two plain runs and a --full run with one block: the same bits in every array the last timed step returned (the
    priming pass runs for a wall-clock time, the handle is reset behind it; --full's passes come after the dump)."""
    args = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--prime-ms", "50"]
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    _check_plain(a, 20)
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    f = _bench(args + ["--full", "--repeats", "1", "--latency-solves", "0", "--event-solves", "4", "--sustained-s", "0",
                       "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "f")])
    assert f["full"] is True and f["roofline"]["kernel_ms"] > 0 and f["cold"]["ms_per_step"] > 0
    oa, ob, of = (_load(str(tmp_path / x)) for x in "abf")
    assert set(oa) == {"U", "traj_cost", "costs", "weights", "control_seq", "control_hist"}
    assert oa["U"].shape == (100, 2) and oa["costs"].shape == (4096,) and oa["weights"].shape == (4096,)
    assert all(np.all(np.isfinite(v)) for v in oa.values())
    _same_arrays(oa, ob)
    _same_arrays(oa, of)
