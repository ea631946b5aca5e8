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
import sys

import bench_trajscore as bt

BYTES_PER_PAIR = 13


def step_kernel(reps: int) -> dict:
    from toued.metrics import gae
    N, W = bt.N_AGENTS, bt.N_WORKERS
    out = []
    for mode, T in bt.SHAPES:
        tr = bt.random_trajectory(mode, T)
        vcrit, idx, tm = tr["vcrit"], tr["idx"], tr["tm"]

        def composed():
            v = vcrit.gather(1, idx.view(N, -1).long()).view(N, T + 1, W)
            v = v + (tm.float() * 0.001) * vcrit[:, -1].view(N, 1, 1)
            adv, _ = gae(v, tr["rew"], tr["done"], 0.99, 0.95)
            return adv.relu().mean(dim=(1, 2)), adv.abs().mean(dim=(1, 2))

        # the two paths agree (the composed means are float32 sums)
        times = bt.time_alternated((("fused", bt.vscore_call(tr, T)), ("composed", composed)), reps,
                                   dict(rtol=1e-4, atol=1e-6))
        row, med = bt.timing_row(mode, T, tr["D"], reps, times)
        f_ms, c_ms = med["fused"], med["composed"]
        nbytes = BYTES_PER_PAIR * N * T * W
        tbs = nbytes / (f_ms * 1e-3) / 1e12
        row.update({"composed_over_fused": round(c_ms / f_ms, 2), "algorithmic_bytes": nbytes,
                    "fused_TB_per_s": round(tbs, 3), **bt.hbm_fractions(tbs),
                    "gate_fused_not_slower": bool(f_ms <= c_ms)})
        out.append(row)
    return {"kernel": out}


if __name__ == "__main__":
    sys.exit(bt.main("vscore", __file__, step_kernel,
                     ("positive_value_loss", "l1_value_loss", "alg_regret", "optimal_regret"),
                     "gate_fused_not_slower", {"kernel": 240, "rounds": 420}))
