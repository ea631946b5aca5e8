"""Measurements of the meta-test (toued.evaluate), into profiles/metatest/bench_metatest.json.

    python tools/bench_metatest.py [--reps 20] [--levels 512] [--trials 3]

(a) ``kernel``: toued_episode_stats at 512 x 64 x 20 (a train rollout) and 512 x 64 x 750 against the torch ops of the
    same definition -- the step loop ``ret = ret + r_t; len += 1; record where done; clear where done`` with f64
    sums, T steps of elementwise launches, which is what carrying episodes across update boundaries costs without a
    kernel -- alternated in one process, device events, medians of ``--reps``; the carries are held bit-identical.
(b) ``metatest``: one whole meta-test of ``--levels`` ``mazes`` levels (2500 updates): the wall time of the run (host
    clock around a device synchronise, median of ``--trials``), alternated with a run under HIP-event timers that gives
    each per-update launch's share; and a C3 meta-step (all_shortlife, 512 agents, alg_regret) timed the same way, so
    what ``--eval_every M`` adds to it amortised over M is meta_test_ms / M.
Each step runs in a child process of its own under ``timeout``; a step that fails ends the run.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

TAG = "BENCH_METATEST_STEP "
TIMEOUTS = {"kernel": 240, "metatest": 540}
N, W = 512, 64


def torch_episode_stats(rew, done, run_ret, run_len, stats):
    """The definition in torch ops, one step at a time (in place on the carry, added to stats [N, 6] f64)."""
    import torch
    T = rew.shape[1]
    zero_f, zero_i = torch.zeros((), device=rew.device), torch.zeros((), dtype=torch.int32, device=rew.device)
    for t in range(T):
        run_ret += rew[:, t]
        run_len += 1
        d = done[:, t].bool()
        r = torch.where(d, run_ret, zero_f).double()
        stats[:, 0] += d.sum(dim=1)
        stats[:, 1] += r.sum(dim=1)
        stats[:, 2] += (r * r).sum(dim=1)
        stats[:, 3] += torch.where(d, run_len, zero_i).sum(dim=1)
        run_ret.masked_fill_(d, 0.0)
        run_len.masked_fill_(d, 0)
    stats[:, 4] += rew.double().sum(dim=(1, 2))
    stats[:, 5] += rew.shape[1] * rew.shape[2]
    return run_ret, run_len, stats


def step_kernel(reps: int) -> dict:
    import torch
    from toued import _lib
    rows = []
    for T in (20, 750):
        g = torch.Generator(device="cuda").manual_seed(T)
        rew = torch.randn((N, T, W), device="cuda", generator=g)
        done = (torch.rand((N, T, W), device="cuda", generator=g) < 0.05).to(torch.uint8)
        c0 = (torch.randn((N, W), device="cuda", generator=g), torch.randint(0, 50, (N, W), device="cuda", generator=g,
                                                                            dtype=torch.int32))

        def fresh():
            return c0[0].clone(), c0[1].clone(), torch.zeros((N, 6), dtype=torch.float64, device="cuda")

        def kernel(rr, rl, st):
            _lib.call("toued_episode_stats", N, W, T, _lib.ptr(rew), _lib.ptr(done), _lib.ptr(rr), _lib.ptr(rl),
                      _lib.ptr(st), _lib.stream_ptr())
            return rr, rl, st

        fns = (("kernel", kernel), ("torch", lambda rr, rl, st: torch_episode_stats(rew, done, rr, rl, st)))
        outs = {}
        for _ in range(2):                                  # warm-up, and the two held against each other
            for name, fn in fns:
                outs[name] = fn(*fresh())
        torch.cuda.synchronize()
        k, t = outs["kernel"], outs["torch"]
        assert torch.equal(k[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(k[1], t[1])
        assert torch.equal(k[2][:, [0, 3, 5]], t[2][:, [0, 3, 5]]) and torch.allclose(k[2], t[2], rtol=1e-12, atol=1e-9)
        times = {name: [] for name, _ in fns}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(reps):
            for name, fn in fns:
                args = fresh()
                torch.cuda.synchronize()
                ev0.record()
                fn(*args)
                ev1.record()
                torch.cuda.synchronize()
                times[name].append(ev0.elapsed_time(ev1))
        med = {name: statistics.median(v) for name, v in times.items()}
        nbytes = N * W * T * 5 + N * W * 16 + N * 96
        row = {"N": N, "W": W, "T": T, "reps": reps, "bytes": nbytes}
        for name, v in times.items():
            row.update({f"{name}_ms_median": round(med[name], 4), f"{name}_ms_min": round(min(v), 4),
                        f"{name}_ms_max": round(max(v), 4)})
        row["kernel_tb_per_s"] = round(nbytes / (med["kernel"] * 1e-3) / 1e12, 4)
        row["torch_over_kernel"] = round(med["torch"] / med["kernel"], 1)
        rows.append(row)
    return {"kernel": rows}


def step_metatest(levels: int, trials: int) -> dict:
    import torch
    from toued import evaluate as ev
    from toued.lpg import LPGLayout
    from toued.meta import KernelTimers
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = ev.parse_eval_args(["--checkpoint_dir", "unused", "--eval_mode", "mazes", "--eval_levels", str(levels)])
    lv, sub, rng = ev.draw_levels("mazes", levels, 0, "cuda")
    eta = torch.zeros(LPGLayout(5).size, device="cuda")
    mt = ev.MetaTest(args, eta, "cuda")
    tr = Trainer(parse_args(["--env_mode", "all_shortlife", "--num_agents", "512", "--num_mini_batches", "1",
                             "--score_function", "alg_regret"]))
    tr.meta_step()                                          # warm: graph capture, code objects
    mt.run(lv, rng, sub)
    torch.cuda.synchronize()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    t_plain, t_timed, t_c3, shares = [], [], [], None
    for _ in range(trials):                                 # alternated
        mt.timers = None
        ms, res = wall(lambda: mt.run(lv, rng, sub))
        t_plain.append(ms)
        mt.timers = KernelTimers()
        mt.timers.enabled = True
        ms, _ = wall(lambda: mt.run(lv, rng, sub))
        t_timed.append(ms)
        shares = mt.timers.summary()
        ms, _ = wall(lambda: [tr.meta_step() for _ in range(5)])
        t_c3.append(ms / 5)
    total = sum(v[2] for v in shares.values())
    med = statistics.median(t_plain)
    c3 = statistics.median(t_c3)
    return {"metatest": {
        "env_mode": "mazes", "levels": levels, "updates": res.updates, "points": res.points, "trials": trials,
        "meta_test_ms": [round(x, 1) for x in t_plain], "meta_test_ms_median": round(med, 1),
        "meta_test_timed_ms": [round(x, 1) for x in t_timed],
        "per_update_launch": {k: {"launches": v[0], "mean_us": round(v[1] * 1e3, 2), "share": round(v[2] / total, 4)}
                              for k, v in shares.items()},
        "per_update_ms": round(med / max(res.updates, 1), 4),
        "c3_meta_step_ms": [round(x, 2) for x in t_c3], "c3_meta_step_ms_median": round(c3, 2),
        "eval_every_added_fraction_of_c3_step": {str(M): round(med / M / c3, 4) for M in (100, 1000, 10000)}}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--levels", type=int, default=512)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "metatest" / "bench_metatest.json"))
    ap.add_argument("--step", choices=sorted(TIMEOUTS), default=None, help="run one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_metatest: needs the GPU (no CPU fallback)")
        res = step_kernel(a.reps) if a.step == "kernel" else step_metatest(a.levels, a.trials)
        print(TAG + json.dumps(res), flush=True)
        return 0
    out = {}
    for step in ("kernel", "metatest"):
        cmd = ["timeout", "-k", "10", str(TIMEOUTS[step]), sys.executable, str(Path(__file__).resolve()), "--step",
               step, "--reps", str(a.reps), "--levels", str(a.levels), "--trials", str(a.trials)]
        print(f"bench_metatest: step {step}", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"bench_metatest: step {step} failed (exit status {r.returncode}); nothing more is run")
        out.update(json.loads(lines[-1][len(TAG):]))
    line = json.dumps(out)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
