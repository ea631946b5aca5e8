"""Timings of the policy PLR scores (toued_policy_scores) and of the C3 regret round scored with one of them:

    python3 tools/bench_polscore.py [--reps 20] [--rounds 5] [--out profiles/polscore/bench_polscore.json]

Each measurement step runs in a child process of its own under `timeout`; a step that fails ends the run (no later
step is started).

  * kernel: toued_policy_scores alone at N = 512 agents, W = 64 workers, T = 750 / D = 3201 (`all`'s eval length and
    table) and T = 2000 / D = 5409 (`tabular`'s), against two references on the same trajectory buffers:
    toued_value_loss_scores, the closest existing kernel, which reads 13 bytes per (worker, step) -- idx 4, time 4,
    reward 4, done 1 -- where this one reads 8, and a composition of torch ops of the same definition
    (``composed_policy_scores``: a gather of the table rows, softmax and log_softmax, the entropy, the two largest
    probabilities, float64 means).  All three are warmed up, then timed alternately with device events, `reps` times
    each, in one process; medians with the range.  Beside the kernel's time the algorithmic bytes (8 per pair) over
    it.  The gate: the kernel's median must not exceed the composed one (exit status 1 otherwise); its ratio to
    toued_value_loss_scores is reported, not gated.
  * rounds: the C3 regret round (all_shortlife, 512 agents, every agent terminated) with --score_function
    policy_entropy and positive_value_loss, timed the way bench.py's workload_c3 times it (a host clock around `rounds`
    rounds ending in a device synchronise, after one warm-up round), the two alternated in one process.

Prints one JSON line and writes it to --out."""
import argparse
import json
import math
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

HBM_SPEC_TBS = 8.0          # MI355X HBM3E peak, datasheet
HBM_COPY_TBS = 6.29         # what a float4 copy reaches
BYTES_PER_PAIR = 8
STEP_TIMEOUT_S = {"kernel": 240, "rounds": 300}


def composed_policy_scores(theta, idx, tm):
    """(entropy, least confidence, min margin) f32 [N] of the definition from torch ops: the kernel's results up to
    rounding."""
    import torch
    N, D, _ = theta.shape
    T, W = idx.shape[1] - 1, idx.shape[2]
    rows = theta.gather(1, idx[:, :T].reshape(N, -1, 1).long().expand(-1, -1, 5))
    logits = rows + (tm[:, :T].reshape(N, -1, 1).float() * 0.001) * theta[:, D - 1].view(N, 1, 5)
    logp = torch.log_softmax(logits, dim=-1)
    p = logp.exp()
    ent = -(p * logp).sum(dim=-1).double().mean(dim=1) / math.log(5)
    top = p.topk(2, dim=-1).values
    lc = (1.0 - top[..., 0]).double().mean(dim=1)
    mm = (1.0 - (top[..., 0] - top[..., 1])).double().mean(dim=1)
    return ent.float(), lc.float(), mm.float()


def step_kernel(reps: int) -> dict:
    import numpy as np
    import torch
    from toued import _lib
    from toued.rollout import RolloutWrapper
    gamma, lam = 0.99, 0.95
    gl = float(np.float32(gamma * lam))
    N, W = 512, 64
    out = []
    for mode, T in (("all", 750), ("tabular", 2000)):
        D = RolloutWrapper(mode, 20).obs_dim
        g = torch.Generator(device="cuda").manual_seed(T)
        theta = torch.randn((N, D, 5), device="cuda", generator=g)
        vcrit = torch.randn((N, D), device="cuda", generator=g)
        idx = torch.randint(0, D - 1, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
        tm = torch.randint(0, 2000, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
        rew = torch.randn((N, T, W), device="cuda", generator=g)
        done = (torch.rand((N, T, W), device="cuda", generator=g) < 0.05).to(torch.uint8)
        ent, lc, mm = (torch.empty(N, device="cuda") for _ in range(3))
        pvl, l1 = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")

        def polscore():
            _lib.call("toued_policy_scores", N, W, T, D, _lib.ptr(theta), _lib.ptr(idx), _lib.ptr(tm), _lib.ptr(ent),
                      _lib.ptr(lc), _lib.ptr(mm), None, _lib.stream_ptr())
            return ent, lc, mm

        def vscore():
            _lib.call("toued_value_loss_scores", N, W, T, D, _lib.ptr(vcrit), _lib.ptr(idx), _lib.ptr(tm),
                      _lib.ptr(rew), _lib.ptr(done), gamma, gl, _lib.ptr(pvl), _lib.ptr(l1), None, _lib.stream_ptr())

        def composed():
            return composed_policy_scores(theta, idx, tm)

        for _ in range(3):                                   # warm-up: code objects, allocator pools
            k_out = [x.clone() for x in polscore()]
            vscore()
            c_out = composed()
        torch.cuda.synchronize()
        for a, b in zip(k_out, c_out):                       # the two paths agree
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), (a[:4], b[:4])
        fns = (("polscore", polscore), ("vscore", vscore), ("composed", composed))
        times = {name: [] for name, _ in fns}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(reps):
            for name, fn in fns:
                ev0.record()
                fn()
                ev1.record()
                torch.cuda.synchronize()
                times[name].append(ev0.elapsed_time(ev1))
        med = {name: statistics.median(v) for name, v in times.items()}
        nbytes = BYTES_PER_PAIR * N * T * W
        tbs = nbytes / (med["polscore"] * 1e-3) / 1e12
        row = {"mode": mode, "N": N, "W": W, "T": T, "D": D, "reps": reps}
        for name, v in times.items():
            row.update({f"{name}_ms_median": round(med[name], 4), f"{name}_ms_min": round(min(v), 4),
                        f"{name}_ms_max": round(max(v), 4)})
        row.update({"polscore_over_vscore": round(med["polscore"] / med["vscore"], 3),
                    "composed_over_polscore": round(med["composed"] / med["polscore"], 2),
                    "algorithmic_bytes": nbytes, "polscore_TB_per_s": round(tbs, 3),
                    "pairs_per_us": round(N * T * W / (med["polscore"] * 1e3), 1),
                    "fraction_of_hbm_spec_8.0": round(tbs / HBM_SPEC_TBS, 3),
                    "fraction_of_hbm_copy_6.29": round(tbs / HBM_COPY_TBS, 3),
                    "gate_polscore_not_slower_than_composed": bool(med["polscore"] <= med["composed"])})
        out.append(row)
    return {"kernel": out}


def step_rounds(rounds: int) -> dict:
    import torch
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    trs = {}
    for sf in ("policy_entropy", "positive_value_loss"):
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
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "polscore" / "bench_polscore.json"))
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT_S), default=None, help="run one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_polscore: needs the GPU (no CPU fallback)")
        res = step_kernel(a.reps) if a.step == "kernel" else step_rounds(a.rounds)
        print("BENCH_POLSCORE_STEP " + json.dumps(res), flush=True)
        return 0
    out = {}
    for step in ("kernel", "rounds"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, str(Path(__file__).resolve()),
               "--step", step, "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("BENCH_POLSCORE_STEP ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"bench_polscore: step {step} failed (exit status {r.returncode}); nothing more is run")
        out.update(json.loads(lines[-1][len("BENCH_POLSCORE_STEP "):]))
    line = json.dumps(out)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 0 if all(k["gate_polscore_not_slower_than_composed"] for k in out["kernel"]) else 1


if __name__ == "__main__":
    sys.exit(main())
