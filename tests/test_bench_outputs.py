"""bench.py --dump-outputs / --full on the CPU: dump_outputs' formats, budget and sampling as a unit,
and the plain / --full lines of a one-rank CPU rehearsal of the metric config (tests/rehearsal_engine.py's
oracle reductions injected; the product engine is HIP-only)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_whole_arrays_and_dtypes(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    arrs = {"w": torch.randn(3, 5, generator=g), "h": torch.randn(7, generator=g).bfloat16(),
            "n/b": torch.arange(4, dtype=torch.int64) + (1 << 40), "d": torch.randn(2, generator=g).double(),
            "none": None}
    done = bench.dump_outputs(str(tmp_path), arrs)
    assert done == {"w.npy": 15, "h.npy": 7, "n_b.npy": 4, "d.npy": 2}
    w, h, n, d = (np.load(tmp_path / f) for f in ("w.npy", "h.npy", "n_b.npy", "d.npy"))
    assert w.dtype == np.float32 and np.array_equal(w, arrs["w"].reshape(-1).numpy())
    assert h.dtype == np.float32 and np.array_equal(h, arrs["h"].float().numpy())
    assert n.dtype == np.float64 and np.array_equal(n, arrs["n/b"].numpy().astype(np.float64))
    assert d.dtype == np.float64 and np.array_equal(d, arrs["d"].numpy())


def test_dump_outputs_samples_past_the_budget(tmp_path):
    """Past the budget every array gets an equal share; a larger one is written as whole tiles chosen
    by its size and a fixed seed only: the same elements on every run, in ascending order."""
    import bench
    E, n = 16, 16 * 40 + 5  # 41 tiles, the last one ragged
    big = torch.arange(n, dtype=torch.float32)
    small = torch.ones(8)
    budget = 2 * 10 * E * 4  # two arrays: a share of 10 tiles each
    a, b = tmp_path / "a", tmp_path / "b"
    done = bench.dump_outputs(str(a), {"big": big, "small": small}, budget=budget, E=E)
    bench.dump_outputs(str(b), {"big": big * 2, "small": small}, budget=budget, E=E)
    got, got2 = np.load(a / "big.npy"), np.load(b / "big.npy")
    assert np.load(a / "small.npy").size == 8
    tiles = bench.sample_tiles(n, 10, 2024, E)
    assert len(tiles) == 10 == len(set(tiles)) and tiles == sorted(tiles)
    exp = np.concatenate([np.arange(t * E, min((t + 1) * E, n)) for t in tiles]).astype(np.float32)
    assert np.array_equal(got, exp) and np.array_equal(got2, 2 * exp)
    assert done["big.npy"] == exp.size and got.nbytes + 32 <= budget


def _bench(args, timeout=240):
    env = dict(os.environ, FEDML_AMD_BENCH_REHEARSAL="cpu", FEDML_AMD_BENCH_ENGINE="rehearsal_engine:make",
               PYTHONPATH=os.path.join(ROOT, "tests") + os.pathsep + os.environ.get("PYTHONPATH", ""),
               WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", OMP_NUM_THREADS="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--clients", "8", "--params", "5000"]
                       + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_and_full_lines_and_dumps(tmp_path):
    plain = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--steps", "2", "--warmup", "0", "--full", "--soak-seconds", "0", "--no-cpu-baseline",
                   "--dump-outputs", str(tmp_path / "full")])
    for d, steps, warm in ((plain, 3, 1), (full, 2, 0)):
        assert d["steps"] == steps and d["warmup"] == warm
        assert d["metric"] and d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
        assert d["ms_per_step"] > 0
        # value = algorithmic bytes of one step / the time one timed step took
        nbytes = (8 + 1) * 5000 * 4
        assert abs(d["value"] - nbytes / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.05 * d["value"] + 0.01
        assert d["outputs"]["arrays"] == 1 and d["outputs"]["elements"] == 5000
    assert plain["full"] is False and plain["parity"] is None and plain["cpu_baseline"] is None
    assert "sustained" not in plain and "cold" not in plain and "clock" not in plain
    assert full["full"] is True and full["parity"].startswith("bit-exact"), full["parity"]
    a, b = np.load(tmp_path / "plain" / "global_model.npy"), np.load(tmp_path / "full" / "global_model.npy")
    assert a.dtype == np.float32 and a.shape == (5000,) and np.array_equal(a, b) and np.isfinite(a).all()
