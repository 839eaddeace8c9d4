"""bench.py on the GPU at its smallest config: a plain run does only the timed steps, --full adds the
support count and the CPU baseline, --dump-outputs writes the last step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
BENCH = os.path.join(ROOT, "bench.py")
GROUPS = {"mu": 3, "f_dc": 1, "f_rest": 15, "opacity": 1, "scaling": 3, "rotation": 4}   # floats per Gaussian (SH degree 3)


def _bench(args, **extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NLOSGR_BENCH_STUB")}
    env.update(extra)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "C1"] + args, env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_last_step(tmp_path):
    out = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["unit"] == "volumes/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert abs(out["value"] - 1000.0 / out["ms_per_step"]) <= 1e-9 * out["value"]
    # nothing that takes a run of its own
    assert "cpu_baseline" not in out and "cpu_baseline_c1" not in out and out["compute"]["evaluations"] is None
    names = ["loss"] + list(GROUPS) + ["adam_m_" + g for g in GROUPS]
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    arr = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arr.values())
    assert arr["loss"].shape == (2,) and arr["loss"][0] > 0
    for g, k in GROUPS.items():
        assert arr[g].size == 1000 * k and arr["adam_m_" + g].shape == arr[g].shape
    # the step moved the parameters: first moments = 0.1 x the step's gradients, not all zero
    assert np.abs(arr["adam_m_mu"]).max() > 0 and np.abs(arr["adam_m_f_dc"]).max() > 0


def test_full_run_adds_count_and_cpu_baseline():
    # a smaller CPU sample: the leg is checked, not its figure
    out = _bench(["--steps", "1", "--warmup", "0", "--full"], NLOSGR_CPU_SAMPLE_G="8")
    assert out["compute"]["evaluations"] > 0 and out["compute"]["pairs"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "volumes/s"
