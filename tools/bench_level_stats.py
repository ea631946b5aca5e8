"""Timings of the level reachability statistics (toued_level_stats) and of what is built on them:

    python3 tools/bench_level_stats.py [--reps 50] [--trials 5] [--steps 10] [--out FILE.json]

  * ``kernel``: toued.env.level_stats_raw (launch and output allocation included) on 4000 ``all`` levels (a C3 buffer)
    and on 512 ``mazes`` levels, with and without the distance map, beside a torch-ops restatement of the same
    definition on the same inputs (dense frontier dilation over [n, G^2] masks, run to a fixed point, one host check
    per round); the restatement's reached counts, eccentricities and maps are compared with the kernel's first.
  * ``reset``: toued.plr.reset_lowest_scoring at the C3 shape (all_shortlife, buffer 4000, 512 reset slots) with
    ``--level_editor accel --edit_prob 1`` and the same with ``--edit_require_solvable``, alternated (each call
    preceded by the three small copies that restore the buffer's flags, as in tools/bench_level_edit.py), beside the
    regret round the reset hides behind: ``positive_value_loss`` of 512 agents, the shortest of the score functions.
  * ``train``: the C3 meta-step (512 all_shortlife agents, alg_regret) with --level_metrics off and on, alternated
    step by step in one Trainer, a host clock around meta_step and reduce_metrics.

Device events around ``reps`` back-to-back calls after a warm-up call of each variant; medians over ``trials``.
Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
import torch  # noqa: E402

B, N, MODE = 4000, 512, "all_shortlife"


def _timed(fn, reps: int) -> float:
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def torch_level_stats(levels, spec):
    """The definition in torch ops: (n_reach [n], ecc [n], dist [n, G^2], rounds)."""
    from toued.env import L_GRID, L_START, L_WALLS
    n, G2, dev = levels.shape[0], spec.g2, levels.device
    g = levels[:, L_GRID].clamp(1, spec.max_grid_size).long()[:, None]
    start = levels[:, L_START].clamp(0, G2 - 1).long()
    c = torch.arange(G2, device=dev)[None, :]
    wall = ((levels[:, L_WALLS:L_WALLS + 8][:, c[0] // 32] >> (c % 32).int()) & 1) != 0
    ingrid = c < g * g
    free = ingrid & ~wall
    col = c % g
    # cell c is entered from c - g (down), c + g (up), c - 1 (right), c + 1 (left)
    pulls = [((c - g).clamp(0, G2 - 1).expand(n, G2), c - g >= 0), ((c + g).clamp(0, G2 - 1).expand(n, G2), c + g < g * g),
             ((c - 1).clamp(0, G2 - 1).expand(n, G2), col != 0), ((c + 1).clamp(0, G2 - 1).expand(n, G2), col != g - 1)]
    rows = torch.arange(n, device=dev)
    reach = torch.zeros((n, G2), dtype=torch.bool, device=dev)
    reach[rows, start] = True
    dist = torch.full((n, G2), -1, dtype=torch.int32, device=dev)
    dist[rows, start] = torch.where(start < (g * g)[:, 0], 0, -1).int()
    r = 0
    while True:
        r += 1
        src = reach & ingrid
        new = torch.zeros_like(reach)
        for idx, ok in pulls:
            new |= torch.gather(src, 1, idx) & ok
        new &= free & ~reach
        if not bool(new.any()):
            break
        reach |= new
        dist = torch.where(new, r, dist)
    return reach.sum(1).int(), dist.amax(1), dist, r


def bench_kernel(a):
    from toued import prng
    from toued.env import LSTAT_ECC, LSTAT_N_REACH, LevelGenerator, get_env_spec, level_stats_raw
    out = {}
    for mode, n in (("all", 4000), ("mazes", 512)):
        spec, _, _ = get_env_spec(mode)
        levels = LevelGenerator(mode)(prng.split(prng.PRNGKey(7, "cuda"), n))
        dist = torch.empty((n, spec.g2), dtype=torch.int32, device="cuda")
        st = level_stats_raw(levels, spec, dist)
        nr, ecc, tdist, rounds = torch_level_stats(levels, spec)
        assert torch.equal(st[:, LSTAT_N_REACH], nr) and torch.equal(st[:, LSTAT_ECC], ecc) and torch.equal(dist, tdist)
        t = {k: [] for k in ("stats", "stats_dist", "torch")}
        for _ in range(a.trials):
            t["stats"].append(_timed(lambda: level_stats_raw(levels, spec), a.reps))
            t["stats_dist"].append(_timed(lambda: level_stats_raw(levels, spec, dist), a.reps))
            t["torch"].append(_timed(lambda: torch_level_stats(levels, spec), max(1, a.reps // 10)))
        med = {k: statistics.median(v) for k, v in t.items()}
        out[f"{mode}_{n}"] = {"stats_us": round(med["stats"] * 1e3, 2), "stats_dist_us": round(med["stats_dist"] * 1e3, 2),
                              "torch_ops_us": round(med["torch"] * 1e3, 1), "torch_rounds": rounds,
                              "max_ecc": int(ecc.max()), "torch_over_kernel": round(med["torch"] / med["stats_dist"], 1),
                              "trials_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}
    return out


def bench_reset(a):
    from toued import prng
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    from toued.plr import positive_value_loss, reset_lowest_scoring
    base = ["--env_mode", MODE, "--num_agents", str(N), "--num_mini_batches", "1", "--score_function",
            "positive_value_loss", "--buffer_size", str(B), "--level_editor", "accel", "--edit_prob", "1"]
    plain = LevelSampler(parse_args(base))
    filt = LevelSampler(parse_args(base + ["--edit_require_solvable"]))
    buf = plain.initialize_buffer(prng.PRNGKey(0, "cuda"))
    g = torch.Generator(device="cuda").manual_seed(0)
    score0 = torch.randn(B, device="cuda", generator=g)
    active0 = torch.arange(B, device="cuda") < N
    new0 = (torch.rand(B, device="cuda", generator=g) < 0.2) & ~active0
    key = prng.PRNGKey(1, "cuda")

    def restore():
        buf.score.copy_(score0)
        buf.active.copy_(active0)
        buf.new = new0.clone()

    def reset(smp):
        restore()
        return reset_lowest_scoring(smp, key, buf, N)

    reset(plain)
    reset(filt)
    torch.cuda.synchronize()
    counts = {"edited_plain": int(plain.last_edit["edited"].sum()), "edited_filtered": int(filt.last_edit["edited"].sum()),
              "rejected": int(filt.last_edit["rejected"].sum())}
    # the regret round of the same session: the scores of 512 agents on their levels
    _, agents = plain.initial_sample(prng.PRNGKey(2, "cuda"), buf, N, True)
    keys = prng.split(prng.PRNGKey(3, "cuda"), N)
    vcrit = agents.vcrit.reshape(N, plain.obs_dim)
    score = lambda: positive_value_loss(plain, keys, agents.levels, agents.theta, vcrit)
    score()
    t = {k: [] for k in ("plain", "filtered", "regret")}
    for _ in range(a.trials):
        t["plain"].append(_timed(lambda: reset(plain), a.reps))
        t["filtered"].append(_timed(lambda: reset(filt), a.reps))
        t["regret"].append(_timed(score, max(1, a.reps // 5)))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"shape": {"env_mode": MODE, "buffer_size": B, "reset_slots": N, **counts},
            "reset_accel_ms": round(med["plain"], 4), "reset_accel_require_solvable_ms": round(med["filtered"], 4),
            "filter_cost_ms": round(med["filtered"] - med["plain"], 4),
            "regret_round_positive_value_loss_ms": round(med["regret"], 4),
            "filtered_reset_inside_regret_round": bool(med["filtered"] < med["regret"]),
            "trials_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}


def bench_train(a):
    from toued.parse_args import parse_args
    from toued.train import Trainer, reduce_metrics
    args = parse_args(["--env_mode", MODE, "--num_agents", str(N), "--num_mini_batches", "1", "--score_function",
                       "alg_regret"])
    tr = Trainer(args)
    t = {False: [], True: []}
    for i in range(2 * (a.steps + 1)):
        on = bool(i % 2)
        tr.args.level_metrics = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = reduce_metrics(tr.meta_step(), tr.world)
        torch.cuda.synchronize()
        if i >= 2:                                     # one warm-up step of each
            t[on].append((time.perf_counter() - t0) * 1e3)
        assert ("levels" in m) == on
    off, onm = statistics.median(t[False]), statistics.median(t[True])
    return {"meta_step_off_ms": round(off, 3), "meta_step_level_metrics_ms": round(onm, 3),
            "difference_ms": round(onm - off, 3), "steps_each": a.steps, "last_levels": m.get("levels"),
            "steps_ms": {"off": [round(x, 3) for x in t[False]], "on": [round(x, 3) for x in t[True]]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_level_stats: needs the GPU (no CPU fallback)")
    out = {"kernel": bench_kernel(a), "reset": bench_reset(a), "train": bench_train(a), "reps": a.reps,
           "trials": a.trials}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
