"""Timings of the state occupancy kernel (toued_policy_occupancy) and of the policy scores built on it:

    python3 tools/bench_occupancy.py [--reps 20] [--trials 5] [--out FILE.json]

  * ``kernel``: RolloutWrapper.policy_occupancy (output allocation included) beside RolloutWrapper.policy_return, the
    backward recursion over the same tables, on the same buffers: 512 ``all_shortlife`` levels and 4000 ``all`` levels
    at the eval rollout length, N(0, 2^2) actor tables with the time row scaled by 30.  The two are alternated within a
    trial.  ``occ_all`` is timed once more on the 512 levels.  Before timing, the occupancy's return is compared with
    policy_return's and two runs with one another (bit for bit).
  * ``round``: the policy scores of the C3 regret round (512 ``all_shortlife`` agents, 64 eval workers,
    ``--score_function policy_entropy``) with ``--policy_score_eval sampled`` (the eval rollout and
    toued_policy_scores; the code path of the commit before the flag, unchanged) and ``exact``
    (toued.plr.exact_policy_scores), alternated, and how far the two scores are apart.

Device events around ``reps`` back-to-back calls after a warm-up call of each variant; medians over ``trials``.
Prints one JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
import torch  # noqa: E402

N, MODE = 512, "all_shortlife"


def _timed(fn, reps: int) -> float:
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def _tables(n, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    th = torch.randn((n, D, 5), device="cuda", generator=g) * 2.0
    th[:, -1] *= 30.0
    return th


def _medians(t):
    return {k: statistics.median(v) for k, v in t.items()}


def bench_kernel(a):
    from toued import prng
    from toued.env import LevelGenerator
    from toued.rollout import RolloutWrapper
    out = {}
    for mode, n in ((MODE, N), ("all", 4000)):
        ro = RolloutWrapper(mode, 20)
        L = ro.eval_rollout_len
        levels = LevelGenerator(mode)(prng.split(prng.PRNGKey(7, "cuda"), n))
        theta = _tables(n, ro.obs_dim, 11)
        occ, again = ro.policy_occupancy(levels, theta, L), ro.policy_occupancy(levels, theta, L)
        assert all(torch.equal(x, y) for x, y in zip(occ[:10], again[:10]))
        vpi = ro.policy_return(levels, theta, L)
        gap = float(((occ.ret - vpi).abs() / occ.ret_abs.clamp(min=1.0)).max())
        variants = {"occupancy": lambda: ro.policy_occupancy(levels, theta, L),
                    "policy_return": lambda: ro.policy_return(levels, theta, L)}
        if n == N:
            variants["occupancy_occ_all"] = lambda: ro.policy_occupancy(levels, theta, L, return_all=True)
        t = {k: [] for k in variants}
        for _ in range(a.trials):
            for k, fn in variants.items():
                t[k].append(_timed(fn, a.reps if n == N else max(1, a.reps // 4)))
        med = _medians(t)
        out[f"{mode}_{n}"] = {"max_rollout_len": L, **{k + "_ms": round(v, 4) for k, v in med.items()},
                              "occupancy_over_policy_return": round(med["occupancy"] / med["policy_return"], 3),
                              "mean_length": round(float(occ.length.mean()), 2),
                              "max_ret_gap_over_ret_abs": gap,
                              "trials_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}
    return out


def bench_round(a):
    from toued import plr, prng
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    base = ["--env_mode", MODE, "--num_agents", str(N), "--num_mini_batches", "1", "--score_function",
            "policy_entropy", "--buffer_size", "4000"]
    sampled = LevelSampler(parse_args(base))
    exact = LevelSampler(parse_args(base + ["--policy_score_eval", "exact"]))
    buf = sampled.initialize_buffer(prng.PRNGKey(0, "cuda"))
    _, agents = sampled.initial_sample(prng.PRNGKey(2, "cuda"), buf, N, False)
    theta = agents.theta * 10.0      # fresh tables are near uniform: scaled, the policies differ from state to state
    keys = prng.split(prng.PRNGKey(3, "cuda"), N)
    variants = {"sampled": lambda: plr.policy_scores(sampled, keys, agents.levels, theta),
                "exact": lambda: plr.policy_scores(exact, keys, agents.levels, theta)}
    got = {k: fn() for k, fn in variants.items()}
    t = {k: [] for k in variants}
    for _ in range(a.trials):
        for k, fn in variants.items():
            t[k].append(_timed(fn, a.reps))
    med = _medians(t)
    diff = [float((s - e).abs().mean()) for s, e in zip(got["sampled"], got["exact"])]
    return {"shape": {"env_mode": MODE, "agents": N, "env_workers": sampled.env_workers,
                      "eval_rollout_len": sampled.rollout_manager.eval_rollout_len},
            "sampled_ms": round(med["sampled"], 4), "exact_ms": round(med["exact"], 4),
            "exact_over_sampled": round(med["exact"] / med["sampled"], 3),
            "mean_abs_sampled_minus_exact": dict(zip(("policy_entropy", "least_confidence", "min_margin"), diff)),
            "trials_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy: needs the GPU (no CPU fallback)")
    out = {"kernel": bench_kernel(a), "round": bench_round(a), "reps": a.reps, "trials": a.trials}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
