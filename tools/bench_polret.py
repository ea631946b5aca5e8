"""Timings of the exact policy return (toued_policy_return) beside the exact optimal return, and of the C3 regret
round with --regret_eval sampled and exact:

    python3 tools/bench_polret.py [--reps 20] [--trials 5] [--rounds 5] [--out FILE.json]

  * toued_policy_return and toued_optimal_return on generated levels, alternated in one process: 512 and 4000 `all`
    levels at L = 750, 512 `tabular` levels at L = 2000, the agents' tables from create_agents scaled by 10 (the
    regret tests' tables).  Per trial, device events around `reps` back-to-back calls of one kernel, then of the
    other, after a warm-up call of each; the medians over `trials` trials and the ratio of the two medians.  Beside
    them the count of state-action-outcome updates (tools/bench_optret.py) and the rate the policy return gives.
  * the C3 regret round (all_shortlife, 512 agents, every agent terminated) for optimal_regret and alg_regret, each
    with --regret_eval sampled and exact, timed the way tools/bench_optret.py times it (a host clock around `rounds`
    rounds ending in a device synchronise, after one warm-up round), the four alternated.

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


def time_policy_return(mode: str, n: int, L: int, reps: int, trials: int) -> dict:
    ro, levels, theta = levels_and_tables(mode, n, L)
    pol = lambda: ro.policy_return(levels, theta, L)
    opt = lambda: ro.optimal_return(levels, L)
    vpi, vst = pol(), opt()                  # warm-up: code objects, LDS attributes
    torch.cuda.synchronize()
    t_pol, t_opt = [], []
    for _ in range(trials):
        t_pol.append(timed(pol, reps))
        t_opt.append(timed(opt, reps))
    m_pol, m_opt = statistics.median(t_pol), statistics.median(t_opt)
    upd = updates_per_level(levels.cpu().numpy(), ro.spec, L)
    return {"mode": mode, "levels": n, "L": L, "policy_return_ms": round(m_pol, 3),
            "optimal_return_ms": round(m_opt, 3), "ratio": round(m_pol / m_opt, 3),
            "policy_return_ms_trials": [round(x, 3) for x in t_pol],
            "optimal_return_ms_trials": [round(x, 3) for x in t_opt], "updates_total": int(upd.sum()),
            "policy_updates_per_sec": round(float(upd.sum()) / (m_pol * 1e-3), 1),
            "v_pi_mean": round(float(vpi.mean()), 6), "v_star_mean": round(float(vst.mean()), 6),
            "regret_min": round(float((vst - vpi).min()), 9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polret: needs the GPU (no CPU fallback)")
    out = {"policy_return": [time_policy_return("all", 512, 750, a.reps, a.trials),
                             time_policy_return("all", 4000, 750, a.reps, a.trials),
                             time_policy_return("tabular", 512, 2000, a.reps, a.trials)],
           "c3_regret_round": regret_rounds(a.rounds, {f"{sf}_{ev}": ["--score_function", sf, "--regret_eval", ev]
                                                       for sf in ("optimal_regret", "alg_regret")
                                                       for ev in ("sampled", "exact")})}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
