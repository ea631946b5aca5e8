"""Timings of the exact return moments (toued_policy_return_moments) beside the exact policy return, and of the C3
regret round with --score_function return_variance beside optimal_regret:

    python3 tools/bench_polvar.py [--reps 20] [--trials 5] [--rounds 5] [--out FILE.json]

  * toued_policy_return_moments and toued_policy_return on the same generated levels and tables, alternated in one
    process: tools/bench_polret.py's shapes (512 and 4000 `all` levels at L = 750, 512 `tabular` levels at
    L = 2000), levels, tables and method.  Per trial, device events around `reps` back-to-back calls of one kernel,
    then of the other, after a warm-up call of each; the medians over `trials` trials and the ratio of the two
    medians.  Beside them the count of state-action-outcome updates (tools/bench_optret.py) and the rate the moments
    kernel gives.
  * the C3 regret round (all_shortlife, 512 agents, every agent terminated) for return_variance and for
    optimal_regret with --regret_eval sampled and exact, timed the way tools/bench_optret.py times it (a host clock
    around `rounds` rounds ending in a device synchronise, after one warm-up round), the three alternated.

Prints one JSON line."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

from bench_optret import levels_and_tables, regret_rounds, timed, updates_per_level  # noqa: E402


def time_moments(mode: str, n: int, L: int, reps: int, trials: int) -> dict:
    ro, levels, theta = levels_and_tables(mode, n, L)
    mom = lambda: ro.policy_return_moments(levels, theta, L)
    pol = lambda: ro.policy_return(levels, theta, L)
    (mean, var), vpi = mom(), pol()          # warm-up: code objects, LDS attributes
    torch.cuda.synchronize()
    if not torch.equal(mean, vpi):
        raise SystemExit("bench_polvar: the moments' mean is not toued_policy_return's")
    t_mom, t_pol = [], []
    for _ in range(trials):
        t_mom.append(timed(mom, reps))
        t_pol.append(timed(pol, reps))
    m_mom, m_pol = statistics.median(t_mom), statistics.median(t_pol)
    upd = updates_per_level(levels.cpu().numpy(), ro.spec, L)
    return {"mode": mode, "levels": n, "L": L, "moments_ms": round(m_mom, 3), "policy_return_ms": round(m_pol, 3),
            "ratio": round(m_mom / m_pol, 3), "moments_ms_trials": [round(x, 3) for x in t_mom],
            "policy_return_ms_trials": [round(x, 3) for x in t_pol], "updates_total": int(upd.sum()),
            "moments_updates_per_sec": round(float(upd.sum()) / (m_mom * 1e-3), 1),
            "v_pi_mean": round(float(mean.mean()), 6), "var_mean": round(float(var.mean()), 6),
            "var_min": round(float(var.min()), 9), "var_max": round(float(var.max()), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polvar: needs the GPU (no CPU fallback)")
    out = {"policy_return_moments": [time_moments("all", 512, 750, a.reps, a.trials),
                                     time_moments("all", 4000, 750, a.reps, a.trials),
                                     time_moments("tabular", 512, 2000, a.reps, a.trials)],
           "c3_regret_round": regret_rounds(a.rounds, {
               "return_variance": ["--score_function", "return_variance"],
               "optimal_regret_sampled": ["--score_function", "optimal_regret"],
               "optimal_regret_exact": ["--score_function", "optimal_regret", "--regret_eval", "exact"]})}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
