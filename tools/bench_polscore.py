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
import math
import sys

import bench_trajscore as bt

BYTES_PER_PAIR = 8


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
    from toued import _lib
    N, W = bt.N_AGENTS, bt.N_WORKERS
    out = []
    for mode, T in bt.SHAPES:
        tr = bt.random_trajectory(mode, T, with_theta=True)
        D = tr["D"]
        ent, lc, mm = (tr["rew"].new_empty(N) for _ in range(3))

        def polscore():
            _lib.call("toued_policy_scores", N, W, T, D, _lib.ptr(tr["theta"]), _lib.ptr(tr["idx"]), _lib.ptr(tr["tm"]),
                      _lib.ptr(ent), _lib.ptr(lc), _lib.ptr(mm), None, _lib.stream_ptr())
            return ent, lc, mm

        def composed():
            return composed_policy_scores(tr["theta"], tr["idx"], tr["tm"])

        times = bt.time_alternated((("polscore", polscore), ("vscore", bt.vscore_call(tr, T)), ("composed", composed)),
                                   reps, dict(rtol=1e-4, atol=1e-5))
        row, med = bt.timing_row(mode, T, D, reps, times)
        nbytes = BYTES_PER_PAIR * N * T * W
        tbs = nbytes / (med["polscore"] * 1e-3) / 1e12
        row.update({"polscore_over_vscore": round(med["polscore"] / med["vscore"], 3),
                    "composed_over_polscore": round(med["composed"] / med["polscore"], 2),
                    "algorithmic_bytes": nbytes, "polscore_TB_per_s": round(tbs, 3),
                    "pairs_per_us": round(N * T * W / (med["polscore"] * 1e3), 1), **bt.hbm_fractions(tbs),
                    "gate_polscore_not_slower_than_composed": bool(med["polscore"] <= med["composed"])})
        out.append(row)
    return {"kernel": out}


if __name__ == "__main__":
    sys.exit(bt.main("polscore", __file__, step_kernel, ("policy_entropy", "positive_value_loss"),
                     "gate_polscore_not_slower_than_composed", {"kernel": 240, "rounds": 300}))
