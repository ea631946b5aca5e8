"""Timings of the MaxMC PLR score (toued_max_mc_scores) and of the C3 regret round scored with it:

    python3 tools/bench_maxmc.py [--reps 20] [--rounds 5] [--out profiles/maxmc/bench_maxmc.json]

Each measurement step runs in a child process of its own under `timeout`; a step that fails ends the run (no later
step is started).

  * kernel: toued_max_mc_scores alone at N = 512 agents, W = 64 workers, T = 750 (`all`'s eval length and critic row)
    and T = 2000 (`tabular`'s), against two references on the same tensors: toued_value_loss_scores, the closest
    existing kernel, which reads the same 13 bytes per (worker, step) -- idx 4, time 4, reward 4, done 1 -- and a
    composition of torch ops of the same definition (``composed_max_mc``: a gather of the values and their mean; the
    episode returns without a loop over time, from a float64 cumulative sum of gamma^t r_t, the episodes' first steps
    by a cumulative maximum, and a masked maximum).  All three are warmed up, then timed alternately with device
    events, `reps` times each, in one process; medians with the range.  Beside the kernel's time the fraction of HBM
    bandwidth it reaches at the 13 algorithmic bytes per pair.  The gate: the kernel's median must not exceed the
    composed one (exit status 1 otherwise); its ratio to toued_value_loss_scores is reported, not gated.
  * rounds: the C3 regret round (all_shortlife, 512 agents, every agent terminated) with --score_function max_mc and
    positive_value_loss, timed the way bench.py's workload_c3 times it (a host clock around `rounds` rounds ending in
    a device synchronise, after one warm-up round), the two alternated in one process.

Prints one JSON line and writes it to --out."""
import sys

import bench_trajscore as bt

BYTES_PER_PAIR = 13


def composed_max_mc(vcrit, idx, tm, rew, done, gamma):
    """(score, rmax) f32 [N] of the MaxMC definition from torch ops, returns in float64: the kernel's results up to
    rounding (its per-worker chains are float32 and sequential)."""
    import torch
    N, T, W = rew.shape
    dev = rew.device
    v = vcrit.gather(1, idx[:, :T].reshape(N, -1).long()).view(N, T, W)
    v = v + (tm[:, :T].float() * 0.001) * vcrit[:, -1].view(N, 1, 1)
    mean_v = v.double().mean(dim=(1, 2))
    steps = torch.arange(T, device=dev)
    pw = torch.pow(torch.tensor(float(gamma), dtype=torch.float64, device=dev), steps.double())      # gamma^t
    P = torch.cumsum(rew.double() * pw.view(1, T, 1), dim=1)
    d = done.bool()
    # first step of the episode that step t belongs to: one past the last done before t
    nxt = torch.cummax(torch.where(d, steps.view(1, T, 1) + 1, 0), dim=1).values
    start = torch.cat([torch.zeros_like(nxt[:, :1]), nxt[:, :-1]], dim=1)
    before = torch.where(start > 0, P.gather(1, (start - 1).clamp(min=0)), 0.0)
    ret = (P - before) / pw[start]
    ends = d.clone()
    ends[:, T - 1] = True                                # the episode still open at the end: its truncated return
    rmax = torch.where(ends, ret, float("-inf")).amax(dim=(1, 2))
    return (rmax - mean_v).float(), rmax.float()


def step_kernel(reps: int) -> dict:
    from toued import _lib
    N, W = bt.N_AGENTS, bt.N_WORKERS
    out = []
    for mode, T in bt.SHAPES:
        tr = bt.random_trajectory(mode, T)
        D, gamma = tr["D"], 0.99
        score, rmax = (tr["rew"].new_empty(N) for _ in range(2))

        def maxmc():
            _lib.call("toued_max_mc_scores", N, W, T, D, _lib.ptr(tr["vcrit"]), _lib.ptr(tr["idx"]), _lib.ptr(tr["tm"]),
                      _lib.ptr(tr["rew"]), _lib.ptr(tr["done"]), gamma, None, _lib.ptr(score), _lib.ptr(rmax), None,
                      _lib.stream_ptr())
            return score, rmax

        def composed():
            return composed_max_mc(tr["vcrit"], tr["idx"], tr["tm"], tr["rew"], tr["done"], gamma)

        # the two paths agree (the kernel's chains are float32, the composed returns float64)
        times = bt.time_alternated((("maxmc", maxmc), ("vscore", bt.vscore_call(tr, T)), ("composed", composed)), reps,
                                   dict(rtol=1e-4, atol=1e-4))
        row, med = bt.timing_row(mode, T, D, reps, times)
        nbytes = BYTES_PER_PAIR * N * T * W
        tbs = nbytes / (med["maxmc"] * 1e-3) / 1e12
        row.update({"maxmc_over_vscore": round(med["maxmc"] / med["vscore"], 3),
                    "composed_over_maxmc": round(med["composed"] / med["maxmc"], 2),
                    "algorithmic_bytes": nbytes, "maxmc_TB_per_s": round(tbs, 3),
                    "vscore_TB_per_s": round(nbytes / (med["vscore"] * 1e-3) / 1e12, 3), **bt.hbm_fractions(tbs),
                    "gate_maxmc_not_slower_than_composed": bool(med["maxmc"] <= med["composed"])})
        out.append(row)
    return {"kernel": out}


if __name__ == "__main__":
    sys.exit(bt.main("maxmc", __file__, step_kernel, ("max_mc", "positive_value_loss"),
                     "gate_maxmc_not_slower_than_composed", {"kernel": 240, "rounds": 300}))
