"""bench.py's multi-rank launch contract, rehearsed on CPU (gloo, NLOSGR_BENCH_STUB=1).

`python bench.py --gpus N` without a launcher must start N ranks itself, and a
launcher whose WORLD_SIZE differs from --gpus must be refused rather than reported as N GPUs.
"""
import json
import os
import subprocess
import sys

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(NLOSGR_BENCH_STUB="1", NLOSGR_DIST_BACKEND="gloo", OMP_NUM_THREADS="1", **kw)
    return env


def _run(args, env, timeout=180):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT)


def test_gpus2_spawns_two_ranks():
    p = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"], _env())
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout           # rank 0 alone prints the job line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3
    assert out["dist"] == {"backend": "gloo", "world_size": 2}
    assert sorted(r["rank"] for r in out["ranks"]) == [0, 1]
    # the job time is the max over ranks
    assert out["ms_per_step"] >= max(r["ms_per_step"] for r in out["ranks"]) - 1e-6


def test_single_rank_default():
    p = _run(["--steps", "2", "--warmup", "0"], _env())
    assert p.returncode == 0, p.stderr
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and len(out["ranks"]) == 1


def test_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's arrays as float32 .npy files, the same from run to run
    (seeded inputs), and --steps is the number of timed steps the line reports."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        p = _run(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)], _env())
        assert p.returncode == 0, p.stderr
        out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        got.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert list(got[0]) == ["grad.npy", "y.npy"] == list(got[1])
    for f in got[0]:
        assert got[0][f].dtype == np.float32 and np.isfinite(got[0][f]).all()
        assert np.array_equal(got[0][f], got[1][f])


def test_dump_outputs_sample_is_bounded_and_fixed():
    """Arrays over the budget keep a fixed (seeded) sorted sample of their rows, within the budget."""
    import numpy as np
    import tempfile
    import torch
    sys.path.insert(0, ROOT)
    import bench
    arrays = {"a": torch.arange(4000, dtype=torch.float32).reshape(1000, 4), "b": torch.arange(500.0),
              "s": torch.tensor(3.0)}
    outs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench.dump_outputs(d, arrays, budget=4096)
            outs.append({n: np.load(os.path.join(d, n + ".npy")) for n in arrays})
    a, b = outs[0]["a"], outs[0]["b"]
    assert sum(v.nbytes for v in outs[0].values()) <= 4096 + 4      # the scalar rides along
    assert a.shape[1] == 4 and 0 < a.shape[0] < 1000 and (np.diff(a[:, 0]) > 0).all()
    assert (a[:, 1] == a[:, 0] + 1).all() and (np.diff(b) > 0).all()   # whole rows, in order
    assert outs[0]["s"] == 3.0
    for n in arrays:
        assert np.array_equal(outs[0][n], outs[1][n])


def test_world_size_mismatch_refused():
    p = _run(["--gpus", "4", "--steps", "1", "--warmup", "0"],
             _env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert p.returncode != 0
    assert "WORLD_SIZE=1" in p.stderr and not p.stdout.strip()


def test_failing_rank_ends_the_job():
    """A rank that dies must not leave the others waiting at the barrier: the launcher ends them
    and exits non-zero."""
    p = _run(["--gpus", "2", "--steps", "2", "--warmup", "0"], _env(NLOSGR_BENCH_STUB_FAIL_RANK="1"),
             timeout=120)
    assert p.returncode != 0
