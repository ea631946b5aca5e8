"""Timings of the exact optimal return (toued_optimal_return) and of the C3 regret round scored with it:

    python3 tools/bench_optret.py [--reps 5] [--rounds 5] [--out FILE.json]

  * toued_optimal_return on generated levels: 512 and 4000 `all` levels at L = 750, 512 `tabular` levels at
    L = 2000.  Device events around `reps` back-to-back calls after a warm-up call; beside each time the count of
    state-action-outcome updates (per level and step: valid cells x 5 actions x 3^n_objs outcome terms, the sum over
    the existence masks e of 2^|absent(e)|; times H = min(max_steps, L) steps) and the rate they give.
  * the C3 regret round (all_shortlife, 512 agents, every agent terminated) with --score_function optimal_regret and
    with alg_regret, timed the way bench.py's workload_c3 times it (a host clock around `rounds` rounds ending in a
    device synchronise, after one warm-up round), the two alternated.

Prints one JSON line.  tools/bench_polret.py and tools/bench_polvar.py take their levels, tables, timing and regret
rounds from here."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def updates_per_level(levels: np.ndarray, spec, L: int) -> np.ndarray:
    """State-action-outcome updates of each packed level's recursion."""
    from toued.env import L_MAX_STEPS, L_NOBJS, unpack_levels
    params, _, _ = unpack_levels(levels, spec)
    g2 = params["grid_size"].astype(np.int64) ** 2
    cells = np.arange(spec.g2)[None, :]
    ncell = ((cells < g2[:, None]) & ~params["walls"]).sum(axis=1)
    H = np.minimum(np.maximum(levels[:, L_MAX_STEPS], 0), L).astype(np.int64)
    return ncell * 5 * 3 ** levels[:, L_NOBJS].astype(np.int64) * H


def timed(fn, reps: int) -> float:
    """ms per call: device events around `reps` back-to-back calls."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def levels_and_tables(mode: str, n: int, L: int, tables: bool = True):
    """The wrapper, n generated levels and (``tables``) the agents' tables from create_agents scaled by 10 (the
    regret tests' tables) of one timed shape; the keys depend on n + L."""
    from toued import prng
    from toued.agents import create_agents
    from toued.env import LevelGenerator
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper(mode, 20)
    levels = LevelGenerator(mode)(prng.split(prng.PRNGKey(n + L, "cuda"), n))
    if not tables:
        return ro, levels, None
    theta, _ = create_agents(prng.split(prng.PRNGKey(n + L + 1, "cuda"), n), ro.obs_dim, 8)
    theta.mul_(10.0)
    return ro, levels, theta


def time_optimal_return(mode: str, n: int, L: int, reps: int) -> dict:
    ro, levels, _ = levels_and_tables(mode, n, L, tables=False)
    v = ro.optimal_return(levels, L)        # warm-up: code object, LDS attribute
    torch.cuda.synchronize()
    ms = timed(lambda: ro.optimal_return(levels, L), reps)
    upd = updates_per_level(levels.cpu().numpy(), ro.spec, L)
    return {"mode": mode, "levels": n, "L": L, "ms": round(ms, 3), "updates_total": int(upd.sum()),
            "updates_per_level_mean": float(upd.mean()), "updates_per_level_max": int(upd.max()),
            "updates_per_sec": round(float(upd.sum()) / (ms * 1e-3), 1),
            "per_level_updates_per_sec": round(float(upd.sum()) / (ms * 1e-3) / n, 1),
            "v0_mean": round(float(v.mean()), 6)}


def regret_rounds(rounds: int, variants: dict) -> dict:
    """The C3 regret round (all_shortlife, 512 agents, every agent terminated) of each variant, name -> its extra
    command-line flags: a host clock around `rounds` rounds ending in a device synchronise, after one warm-up round,
    the variants alternated, twice."""
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    trs = {k: Trainer(parse_args(["--env_mode", "all_shortlife", "--num_agents", "512", "--num_mini_batches", "1"]
                                 + flags)) for k, flags in variants.items()}

    def one_round(tr):
        tr.agents.step = tr.agents.levels[:, L_LIFETIME].clone()     # every agent terminated: all are scored
        tr.buffer, tr.agents = tr.sampler.sample(tr.rng, tr.buffer, tr.agents)

    times = {k: [] for k in trs}
    for tr in trs.values():
        one_round(tr)                                                  # warm-up
    for _ in range(2):                                                 # alternated
        for k, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                one_round(tr)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / rounds * 1e3)
    return {k: {"regret_round_ms": [round(x, 3) for x in v]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optret: needs the GPU (no CPU fallback)")
    out = {"optimal_return": [time_optimal_return("all", 512, 750, a.reps),
                              time_optimal_return("all", 4000, 750, a.reps),
                              time_optimal_return("tabular", 512, 2000, a.reps)],
           "c3_regret_round": regret_rounds(a.rounds, {sf: ["--score_function", sf]
                                                       for sf in ("alg_regret", "optimal_regret")})}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
