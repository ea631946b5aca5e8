"""Timings of the value-loss PLR scores (toued_value_loss_scores) and of the C3 regret round scored with them:

    python3 tools/bench_vscore.py [--reps 20] [--rounds 5] [--out profiles/vscore/bench_vscore.json]

Each measurement step runs in a child process of its own under `timeout`; a step that fails ends the run (no later
step is started).

  * kernel: the fused kernel alone at N = 512 agents, W = 64 workers, T = 750 (`all`'s eval length and critic row) and
    T = 2000 (`tabular`'s), against the composed path it replaces on the same tensors: a torch gather of the values,
    toued_gae, then torch relu / abs / mean.  Both are warmed up, then timed alternately with device events, `reps`
    times each, in one process; medians.  Beside the fused time the fraction of HBM bandwidth it reaches at the 13
    algorithmic bytes per (worker, step): idx 4, time 4, reward 4, done 1.  The gate: the fused median must not exceed
    the composed one (exit status 1 otherwise).
  * rounds: the C3 regret round (all_shortlife, 512 agents, every agent terminated) with --score_function
    positive_value_loss, l1_value_loss, alg_regret and optimal_regret, timed the way bench.py's workload_c3 times it
    (a host clock around `rounds` rounds ending in a device synchronise, after one warm-up round), the four alternated
    in one process.

Prints one JSON line and writes it to --out."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

HBM_SPEC_TBS = 8.0          # MI355X HBM3E peak, datasheet
HBM_COPY_TBS = 6.29         # what a float4 copy reaches
BYTES_PER_PAIR = 13
STEP_TIMEOUT_S = {"kernel": 240, "rounds": 420}


def step_kernel(reps: int) -> dict:
    import numpy as np
    import torch
    from toued import _lib
    from toued.metrics import gae
    from toued.rollout import RolloutWrapper
    gamma, lam = 0.99, 0.95
    gl = float(np.float32(gamma * lam))
    N, W = 512, 64
    out = []
    for mode, T in (("all", 750), ("tabular", 2000)):
        D = RolloutWrapper(mode, 20).obs_dim
        g = torch.Generator(device="cuda").manual_seed(T)
        vcrit = torch.randn((N, D), device="cuda", generator=g)
        idx = torch.randint(0, D - 1, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
        tm = torch.randint(0, 2000, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
        rew = torch.randn((N, T, W), device="cuda", generator=g)
        done = (torch.rand((N, T, W), device="cuda", generator=g) < 0.05).to(torch.uint8)
        pvl, l1 = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")

        def fused():
            _lib.call("toued_value_loss_scores", N, W, T, D, _lib.ptr(vcrit), _lib.ptr(idx), _lib.ptr(tm),
                      _lib.ptr(rew), _lib.ptr(done), gamma, gl, _lib.ptr(pvl), _lib.ptr(l1), None, _lib.stream_ptr())
            return pvl, l1

        def composed():
            v = vcrit.gather(1, idx.view(N, -1).long()).view(N, T + 1, W)
            v = v + (tm.float() * 0.001) * vcrit[:, -1].view(N, 1, 1)
            adv, _ = gae(v, rew, done, gamma, lam)
            return torch.relu(adv).mean(dim=(1, 2)), adv.abs().mean(dim=(1, 2))

        for _ in range(3):                                   # warm-up: code objects, allocator pools
            f_out = [x.clone() for x in fused()]
            c_out = composed()
        torch.cuda.synchronize()
        # the two paths agree (the composed means are float32 sums)
        for a, b in zip(f_out, c_out):
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), (a[:4], b[:4])
        times = {"fused": [], "composed": []}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(reps):
            for name, fn in (("fused", fused), ("composed", composed)):
                ev0.record()
                fn()
                ev1.record()
                torch.cuda.synchronize()
                times[name].append(ev0.elapsed_time(ev1))
        f_ms, c_ms = statistics.median(times["fused"]), statistics.median(times["composed"])
        nbytes = BYTES_PER_PAIR * N * T * W
        tbs = nbytes / (f_ms * 1e-3) / 1e12
        out.append({"mode": mode, "N": N, "W": W, "T": T, "D": D, "reps": reps,
                    "fused_ms_median": round(f_ms, 4), "fused_ms_min": round(min(times["fused"]), 4),
                    "fused_ms_max": round(max(times["fused"]), 4),
                    "composed_ms_median": round(c_ms, 4), "composed_ms_min": round(min(times["composed"]), 4),
                    "composed_ms_max": round(max(times["composed"]), 4),
                    "composed_over_fused": round(c_ms / f_ms, 2),
                    "algorithmic_bytes": nbytes, "fused_TB_per_s": round(tbs, 3),
                    "fraction_of_hbm_spec_8.0": round(tbs / HBM_SPEC_TBS, 3),
                    "fraction_of_hbm_copy_6.29": round(tbs / HBM_COPY_TBS, 3),
                    "gate_fused_not_slower": bool(f_ms <= c_ms)})
    return {"kernel": out}


def step_rounds(rounds: int) -> dict:
    import torch
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    trs = {}
    for sf in ("positive_value_loss", "l1_value_loss", "alg_regret", "optimal_regret"):
        args = parse_args(["--env_mode", "all_shortlife", "--num_agents", "512", "--num_mini_batches", "1",
                           "--score_function", sf])
        trs[sf] = Trainer(args)

    def one_round(tr):
        tr.agents.step = tr.agents.levels[:, L_LIFETIME].clone()     # every agent terminated: all are scored
        tr.buffer, tr.agents = tr.sampler.sample(tr.rng, tr.buffer, tr.agents)

    times = {sf: [] for sf in trs}
    for sf, tr in trs.items():
        one_round(tr)                                                  # warm-up
    for _ in range(3):                                                 # alternated
        for sf, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                one_round(tr)
            torch.cuda.synchronize()
            times[sf].append((time.perf_counter() - t0) / rounds * 1e3)
    return {"c3_regret_round": {sf: {"regret_round_ms": [round(x, 3) for x in v],
                                     "regret_round_ms_median": round(statistics.median(v), 3)}
                                for sf, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "vscore" / "bench_vscore.json"))
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT_S), default=None, help="run one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_vscore: needs the GPU (no CPU fallback)")
        res = step_kernel(a.reps) if a.step == "kernel" else step_rounds(a.rounds)
        print("BENCH_VSCORE_STEP " + json.dumps(res), flush=True)
        return 0
    out = {}
    for step in ("kernel", "rounds"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, str(Path(__file__).resolve()),
               "--step", step, "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("BENCH_VSCORE_STEP ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"bench_vscore: step {step} failed (exit status {r.returncode}); nothing more is run")
        out.update(json.loads(lines[-1][len("BENCH_VSCORE_STEP "):]))
    line = json.dumps(out)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 0 if all(k["gate_fused_not_slower"] for k in out["kernel"]) else 1


if __name__ == "__main__":
    sys.exit(main())
