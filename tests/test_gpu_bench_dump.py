"""bench.py --dump-outputs DIR: a plain run writes what its last timed tick left as DIR/<name>.npy
(float32 / float64, < 64 MB), the same arrays on every run with the same arguments, and its result
line carries none of the --full legs. A small cluster (N = 1,024: more rows than the 48 sampled), a
few ticks."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_sample_indices_fixed_and_distinct():
    bench = _bench_module()
    a = bench.sample_indices(65536, 48, bench.DUMP_SEED)
    assert a == bench.sample_indices(65536, 48, bench.DUMP_SEED)
    assert len(set(a)) == 48 and a == sorted(a) and 0 <= a[0] and a[-1] < 65536
    assert a != bench.sample_indices(65536, 48, bench.DUMP_SEED + 1)
    assert bench.sample_indices(5, 48, 1) == [0, 1, 2, 3, 4]


def _run(args, out_dir):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "5", "--warmup", "1", "--dump-outputs",
                        str(out_dir)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays


def _check_common(out, arrays):
    assert out["steps"] == 5 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - out["config"]["n"] / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert "companion" not in out and "cpu_baseline" not in out  # the --full legs
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["tick_stats"][1] == out["config"]["live"] and arrays["tick_stats"][3] == 0


@pytest.mark.gpu
def test_scaled_dump_is_reproducible(tmp_path):
    n = 1024
    out, a = _run(["--cluster", str(n)], tmp_path / "a")
    _, b = _run(["--cluster", str(n)], tmp_path / "b")
    _check_common(out, a)
    assert sorted(a) == ["event_totals", "nodes", "table_hb", "table_rows", "table_ts", "target_counts", "targets",
                         "tick_stats"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["table_rows"].astype(int)
    assert a["table_hb"].shape == a["table_ts"].shape == (len(rows), n) and a["nodes"].shape == (n, 4)
    # the run ends with tick 25 + 1 + 5 = 31: the freshest entry of the ~48 x 5 lists the sampled
    # observers merged on that tick carries its timestamp, and nothing is newer
    failed = a["nodes"][:, 2] != 0
    assert int(failed.sum()) == out["config"]["crashed"] == 10
    assert a["table_ts"].max() == 31 and a["table_ts"].min() >= -1
    assert a["event_totals"][2] == out["check"]["removed_rank0"]
    assert a["targets"].shape == (n, 5) and a["targets"].max() < n and a["target_counts"].max() == 5

