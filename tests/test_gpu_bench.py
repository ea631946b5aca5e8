"""A plain `bench.py --gpus 1 --steps N --warmup W` run on the GPU: one JSON line with the headline only (what
--full adds is absent), --steps timed steps, and --dump-outputs writing the last step's outputs as float32 / float64
.npy files, the same in two runs.  A small agent count: the benchmark's own process and set-up are what is tested."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("kernels", "roofline", "roofline_secondary", "cpu_baseline", "micro", "workloads",
             "ms_per_step_timed_pass")
N, STEPS, WARMUP = 8, 2, 1


def _bench(dump):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--agents_per_gpu", str(N), "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    out = _bench(tmp_path / "a")
    for k in HEADLINE:
        assert k in out, k
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["n_gpus"] == 1
    assert out["unit"] == "agent-env-steps/sec" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    # value is the inner-rollout agent-env-steps of one step (N W T K) over ms_per_step
    c = out["config"]
    per_step = c["num_agents"] * c["env_workers"] * c["train_rollout_len"] * c["num_agent_updates"]
    assert c["num_agents"] == N
    assert out["value"] == pytest.approx(per_step / (out["ms_per_step"] * 1e-3), rel=1e-3)
    files = sorted((tmp_path / "a").glob("*.npy"))
    names = {f.stem for f in files}
    assert {"eta", "adam_m", "adam_v", "meta_grad", "agents_theta", "agents_phi", "agents_vcrit", "agents_step",
            "agents_state", "agents_levels", "metrics_lpg_loss", "metrics_lpg_agent_return"} <= names
    arrs = {f.stem: np.load(f) for f in files}
    assert sum(x.nbytes for x in arrs.values()) <= 64 << 20
    for name, x in arrs.items():
        assert x.dtype in (np.float32, np.float64), (name, x.dtype)
        assert x.size and np.isfinite(x).all(), name
    # the Adam count is the number of meta-steps the run made; the last step moved eta
    assert arrs["adam_count"][0] == STEPS + WARMUP
    assert arrs["agents_theta"].shape[0] == N and arrs["metrics_lpg_loss"].shape == (N,)
    assert np.abs(arrs["meta_grad"]).max() > 0 and np.abs(arrs["adam_m"]).max() > 0
    # same arguments, same inputs: a second run writes the same arrays
    _bench(tmp_path / "b")
    for name, x in arrs.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / f"{name}.npy")), name
