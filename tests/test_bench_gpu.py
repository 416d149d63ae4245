"""bench.py end to end on the MI355X: what a plain run does and prints, `--dump-outputs`, and
the legs behind `--full`.  Small configurations only (`small`: 200K × 50K, 10M signals,
k = 128, the default workload's code path with sampled factor files; `c1`: the ML-100K shape)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from helpers import ROOT

pytestmark = pytest.mark.gpu


def run_bench(*flags):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(flags),
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain run prints the headline fields and none of the `--full` legs; `--steps` sets the
    timed steps; two runs with the same arguments write the same outputs (fp64: the parity
    bar of the GPU tests, 1e-9 of the largest entry), float64, under 64 MB in all."""
    dumps = []
    for name in ("a", "b"):
        d = run_bench("--config", "small", "--steps", "2", "--warmup", "1",
                      "--dump-outputs", str(tmp_path / name))
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert abs(d["value"] - 250_000 / (d["ms_per_step"] / 1e3)) <= 1e-3 * d["value"]
        assert "metric" in d and "parity" not in d and "cpu_baseline" not in d
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["item_factors.npy", "loss.npy", "user_factors.npy"]
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64 << 20
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert a["user_factors.npy"].shape == (len(bench.dump_rows(200_000, 128, 0)), 128)
    assert a["item_factors.npy"].shape == (len(bench.dump_rows(50_000, 128, 0)), 128)
    for f in a:
        assert a[f].dtype == np.float64 and a[f].shape == b[f].shape
        assert np.all(np.isfinite(a[f])) and np.any(a[f] != 0)
        assert np.max(np.abs(a[f] - b[f])) <= 1e-9 * np.max(np.abs(a[f])), f
    # the loss in the file is the raw loss the last half returned; the line's is per cell
    assert abs(a["loss.npy"][0] / 200_000 / 50_000 - d["loss"]) <= 1e-12 * abs(d["loss"])


def test_full_run_adds_parity_and_cpu_baseline():
    """`--full` on C1: the 10-epoch run against the port (parity) and the port's time."""
    d = run_bench("--config", "c1", "--steps", "2", "--warmup", "1", "--full")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["parity"]["pass"] is True
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0
