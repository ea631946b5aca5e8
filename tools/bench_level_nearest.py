"""Timings of the level distance kernel (toued_level_nearest) and of what is built on it:

    python3 tools/bench_level_nearest.py [--reps 50] [--trials 5] [--steps 10] [--out FILE.json]

  * ``kernel``: toued.env.level_nearest (output allocation and the three launches included) of 512 and of 4000 ``all``
    levels against a 4000-level buffer of which they are rows (eligible "others"), beside a torch-ops restatement of
    the same definition on the same inputs (canonical records [n, 54], then != / xor-popcount over [chunk, B, 54]
    temporaries, chunked over the queries); the restatement's four outputs are compared with the kernel's first.
  * ``reset``: toued.plr.reset_lowest_scoring at the C3 shape (all_shortlife, buffer 4000, 512 reset slots) with
    ``--level_editor accel --edit_prob 1`` (the parent commit's behaviour) and the same with ``--edit_min_distance 1``,
    alternated (each call preceded by the three small copies that restore the buffer's flags, as in
    tools/bench_level_edit.py), beside the regret round the reset hides behind: ``positive_value_loss`` of 512 agents,
    the shortest of the score functions.
  * ``train``: the C3 meta-step (512 all_shortlife agents, alg_regret) with --buffer_diversity off and on, alternated
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


def torch_canonical(levels, include_lifetime=True):
    """The canonical records [n, 54] in torch ops: 46 plain words, then 8 wall words."""
    from toued.env import L_GRID, L_LIFETIME, L_NOBJS, L_OBJ_IDS, L_WALLS
    dev = levels.device
    head = levels[:, :6].clone()
    if not include_lifetime:
        head[:, L_LIFETIME] = 0
    nobj = levels[:, L_NOBJS].clamp(0, 8)[:, None]
    slot = torch.arange(40, device=dev)[None, :] % 8
    slots = torch.where(slot < nobj, levels[:, L_OBJ_IDS:L_OBJ_IDS + 40], 0)
    g2 = levels[:, L_GRID].clamp(0, 16)[:, None] ** 2
    rem = (g2 - 32 * torch.arange(8, device=dev)[None, :]).clamp(0, 32).long()
    keep = ((torch.ones((), dtype=torch.int64, device=dev) << rem) - 1).to(torch.int32)      # 2^32 - 1 wraps to -1
    return torch.cat([head, slots, levels[:, L_WALLS:L_WALLS + 8] & keep], dim=1)


def _popcount32(x):
    x = x.long() & 0xFFFFFFFF
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) >> 24) & 0xFF


def torch_level_nearest(queries, corpus, mode="others", chunk=128):
    """The definition in torch ops, chunked over the queries: (dist, idx, dist_sum, count), int32 [n] each."""
    n, b, dev = queries.shape[0], corpus.shape[0], queries.device
    q, c = torch_canonical(queries), torch_canonical(corpus)
    j = torch.arange(b, device=dev)[None, :]
    big = 2 ** 31 - 1
    outs = []
    for lo in range(0, n, chunk):
        qc = q[lo:lo + chunk]
        d = ((qc[:, None, :46] != c[None, :, :46]).sum(dim=2)
             + _popcount32(qc[:, None, 46:] ^ c[None, :, 46:]).sum(dim=2))
        i = torch.arange(lo, lo + qc.shape[0], device=dev)[:, None]
        ok = {"all": torch.ones_like(d, dtype=torch.bool), "others": j != i, "lower": j < i}[mode]
        dm = torch.where(ok, d, big)
        nn, _ = dm.min(dim=1)
        idx = torch.where(dm == nn[:, None], j, b).amin(dim=1)          # the lowest index of the minimum
        cnt = ok.sum(dim=1)
        outs.append(torch.stack([nn, torch.where(cnt > 0, idx, -1), torch.where(ok, d, 0).sum(dim=1), cnt]))
    return tuple(torch.cat(outs, dim=1).to(torch.int32))


def bench_kernel(a):
    from toued import prng
    from toued.env import L_BUFID, LevelGenerator, level_nearest
    out = {}
    levels = LevelGenerator("all")(prng.split(prng.PRNGKey(7, "cuda"), B))
    levels[B // 2:] = levels[:B // 2]                  # every level twice: duplicates, and ties at the minimum
    levels[:, L_BUFID] = torch.arange(B, dtype=torch.int32, device="cuda")
    for n in (N, B):
        q = levels[:n].contiguous()
        got = level_nearest(q, levels, eligible="others")
        want = torch_level_nearest(q, levels, "others")
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        assert bool((got.dist == 0).all())
        t = {"kernel": [], "torch": []}
        for _ in range(a.trials):
            t["kernel"].append(_timed(lambda: level_nearest(q, levels, eligible="others"), a.reps))
            t["torch"].append(_timed(lambda: torch_level_nearest(q, levels, "others"), max(1, a.reps // 25)))
        med = {k: statistics.median(v) for k, v in t.items()}
        out[f"all_{n}x{B}"] = {"kernel_us": round(med["kernel"] * 1e3, 2), "torch_ops_us": round(med["torch"] * 1e3, 1),
                               "torch_over_kernel": round(med["torch"] / med["kernel"], 1),
                               "pairs_per_us": round(n * B / (med["kernel"] * 1e3), 1),
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
    filt = LevelSampler(parse_args(base + ["--edit_min_distance", "1"]))
    buf = plain.initialize_buffer(prng.PRNGKey(0, "cuda"))
    levels0 = buf.levels.clone()
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

    # the counts on the untouched buffer (a timed call edits the buffer the one before it refilled)
    reset(plain)
    torch.cuda.synchronize()
    counts = {"edited_plain": int(plain.last_edit["edited"].sum())}
    buf.levels.copy_(levels0)
    reset(filt)
    torch.cuda.synchronize()
    counts.update(edited_filtered=int(filt.last_edit["edited"].sum()), too_close=int(filt.last_edit["too_close"].sum()))
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
            "reset_accel_ms": round(med["plain"], 4), "reset_accel_min_distance_1_ms": round(med["filtered"], 4),
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
        tr.args.buffer_diversity = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = reduce_metrics(tr.meta_step(), tr.world)
        torch.cuda.synchronize()
        if i >= 2:                                     # one warm-up step of each
            t[on].append((time.perf_counter() - t0) * 1e3)
        assert ("buffer" in m) == on
    off, onm = statistics.median(t[False]), statistics.median(t[True])
    return {"meta_step_off_ms": round(off, 3), "meta_step_buffer_diversity_ms": round(onm, 3),
            "difference_ms": round(onm - off, 3), "steps_each": a.steps, "last_buffer": m.get("buffer"),
            "steps_ms": {"off": [round(x, 3) for x in t[False]], "on": [round(x, 3) for x in t[True]]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_level_nearest: needs the GPU (no CPU fallback)")
    out = {"kernel": bench_kernel(a), "reset": bench_reset(a), "train": bench_train(a), "reps": a.reps,
           "trials": a.trials}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
