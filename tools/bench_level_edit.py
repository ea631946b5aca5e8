"""Timings of the PLR reset (toued.plr.reset_lowest_scoring) with the ACCEL level editor off and on, at the C3 shape
(all_shortlife, buffer 4000, 512 reset slots), and of the editor's two calls alone (launch and output allocation
included):

    python3 tools/bench_level_edit.py [--reps 50] [--trials 5] [--out FILE.json]

The buffer holds generated levels with random scores; 512 slots are active and a fifth of the rest is new, so the reset
takes new and low-scoring slots and about 2800 scored slots are eligible parents.  A reset changes the buffer's flags,
so every call is preceded by the same three small copies that restore them (timed alone as ``restore_ms`` and
included in both reset figures).  Per trial, device events around ``reps`` back-to-back calls on one stream, off and on
alternated, after a warm-up call of each; the medians over ``trials`` trials.  --edit_prob 1 with the default ops and
edit count: every slot is edited, the editor's worst case.

Prints one JSON line."""
import argparse
import json
import statistics
import sys
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_level_edit: needs the GPU (no CPU fallback)")
    from toued import prng
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    from toued.plr import parent_ids, reset_lowest_scoring
    base = ["--env_mode", MODE, "--num_agents", str(N), "--num_mini_batches", "1", "--score_function", "alg_regret",
            "--buffer_size", str(B)]
    off = LevelSampler(parse_args(base))
    on = LevelSampler(parse_args(base + ["--level_editor", "accel", "--edit_prob", "1"]))
    buf = off.initialize_buffer(prng.PRNGKey(0, "cuda"))
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

    ids = reset(off).clone()
    reset(on)
    torch.cuda.synchronize()
    edited = int(on.last_edit["edited"].sum())
    restore()
    n_elig = int((~buf.new).sum()) - int((~buf.new)[ids.long()].sum())
    parents = parent_ids(buf, ids)
    keys = prng.split(key, N)
    levels = off.gen(keys, buffer_ids=ids)
    t = {k: [] for k in ("restore", "off", "on", "parent_ids", "level_edit")}
    for _ in range(a.trials):
        t["restore"].append(_timed(restore, a.reps))
        t["off"].append(_timed(lambda: reset(off), a.reps))
        t["on"].append(_timed(lambda: reset(on), a.reps))
        restore()
        t["parent_ids"].append(_timed(lambda: parent_ids(buf, ids), a.reps))
        t["level_edit"].append(_timed(lambda: on.editor(buf.levels, parents, keys, levels), a.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": {"env_mode": MODE, "buffer_size": B, "reset_slots": N, "eligible_parents": n_elig,
                     "edited_slots": edited, "num_edits": on.editor.num_edits, "ops_mask": on.editor.ops_mask},
           "reset_off_ms": round(med["off"], 4), "reset_on_ms": round(med["on"], 4),
           "editor_cost_ms": round(med["on"] - med["off"], 4), "restore_ms": round(med["restore"], 4),
           "parent_ids_call_ms": round(med["parent_ids"], 4), "level_edit_call_ms": round(med["level_edit"], 4),
           "trials_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}, "reps": a.reps}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
