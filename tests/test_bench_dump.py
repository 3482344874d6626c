"""bench.py --dump-outputs: the scores of the last timed step land in DIR/<name>.npy (whole, or as a fixed, seeded row
sample when larger than the budget), and the result line reports the steps it timed and ms_per_step."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_samples_the_same_rows_within_budget(tmp_path, monkeypatch):
    import torch
    bench = _bench_module()
    a = torch.arange(500 * 40, dtype=torch.float32).reshape(500, 40)
    b = torch.arange(3 * 7, dtype=torch.float64).reshape(3, 7)
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 100 * 40 * 4)   # 100 rows of `a` per array
    info = bench.dump_outputs(str(tmp_path / "one"), {"scores": a, "small": b})
    bench.dump_outputs(str(tmp_path / "two"), {"scores": a, "small": b})
    got = np.load(tmp_path / "one" / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (100, 40)
    rows = got[:, 0].astype(np.int64) // 40
    assert (np.diff(rows) > 0).all() and rows.max() < 500
    np.testing.assert_array_equal(got, a.numpy()[rows])
    np.testing.assert_array_equal(got, np.load(tmp_path / "two" / "scores.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "one" / "small.npy"), b.numpy())
    assert info["scores"] == {"shape": [500, 40], "rows_written": 100, "row_sample_seed": bench.DUMP_SEED}
    assert info["small"] == {"shape": [3, 7], "rows_written": 3, "row_sample_seed": None}


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_scores_of_its_timed_path(tmp_path):
    bench = _bench_module()
    from oracle import simspread_oracle as O
    nq, n, steps = 200, 600, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--nq", str(nq), "--n", str(n), "--no-sweep", "--no-cpu-baseline", "--no-c3", "--no-c5",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["ms_per_step"] > 0
    assert res["dumped_outputs"]["scores"] == {"shape": [nq, n], "rows_written": nq, "row_sample_seed": None}
    got = np.load(tmp_path / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (nq, n)
    Xq, Xs, Ys = bench.synth_c2(nq, n, n, n, 0.05, 0.01, seed=20250222 + 2, rank=0)
    want = O.predict_factored(Xq.astype(np.float64), Xs.astype(np.float64), Ys.astype(np.float64), "query")
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-5
