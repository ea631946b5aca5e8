"""Latency of the PLR sampler kernels with and without the prioritised replay distribution:

    python3 tools/bench_plr_replay.py [--reps 50] [--rounds 5] [--out profiles/plr_replay/bench_plr_replay.json]

The measurement runs in a child process of its own under `timeout`; if it fails nothing more is run.

At bench.py's micro_plr shape (B = 4000 buffer slots, N = 512 agents, the same random buffer) it times, with HIP events
around `reps` back-to-back launches after one warm-up launch, `rounds` times each, the variants alternated in one
process (microseconds per call; median and range over the rounds):

  * toued_plr_sample, rank and proportional (the reference's transforms);
  * toued_plr_sample_prio with (rank_sampled, rho = 0), (rank_sampled, rho = 0.1) and (proportional, rho = 0.1), and
    with (rank, rho = 0) / (proportional, rho = 0), the two calls that reproduce toued_plr_sample.

rank_sampled sorts the buffer once more than proportional (the ranks): three 8192-key bitonic sorts against two, beside
the shared serial float sum and the selection's 512-key sort; `rank_sampled_over_proportional` is the measured ratio.

Prints one JSON line and writes it to --out."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

STEP_TIMEOUT_S = 240
B, N = 4000, 512


def step_kernel(reps: int, rounds: int) -> dict:
    import torch
    from toued import _lib
    g = torch.Generator(device="cuda").manual_seed(1)
    score = torch.rand(B, device="cuda", generator=g)
    active = (torch.rand(B, device="cuda", generator=g) < 0.6).to(torch.uint8)
    new = (torch.rand(B, device="cuda", generator=g) < 0.3).to(torch.uint8)
    keys = torch.randint(0, 2 ** 31 - 1, (3, 2), dtype=torch.int32, device="cuda", generator=g)
    stamp = torch.randint(0, 500, (B,), dtype=torch.int32, device="cuda", generator=g)
    chosen, rep, rnd, use = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(4))
    p = torch.empty(B, dtype=torch.float32, device="cuda")
    st = _lib.stream_ptr()

    def old(prop):
        return lambda: _lib.call("toued_plr_sample", B, N, _lib.ptr(score), _lib.ptr(active), _lib.ptr(new),
                                 _lib.ptr(keys), prop, 1.0, 0.5, _lib.ptr(chosen), _lib.ptr(rep), _lib.ptr(rnd),
                                 _lib.ptr(use), st)

    def prio(transform, rho):
        return lambda: _lib.call("toued_plr_sample_prio", B, N, _lib.ptr(score), _lib.ptr(active), _lib.ptr(new),
                                 _lib.ptr(stamp) if rho > 0 else None, 500, _lib.ptr(keys), transform, 1.0, rho, 0.5,
                                 _lib.ptr(chosen), _lib.ptr(rep), _lib.ptr(rnd), _lib.ptr(use), _lib.ptr(p), st)

    variants = {"sample_rank": old(0), "sample_proportional": old(1),
                "prio_rank_rho0": prio(0, 0.0), "prio_proportional_rho0": prio(1, 0.0),
                "prio_rank_sampled_rho0": prio(2, 0.0), "prio_rank_sampled_rho0.1": prio(2, 0.1),
                "prio_proportional_rho0.1": prio(1, 0.1)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for fn in variants.values():        # warm-up: code objects
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            fn()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    out = {"buffer_size": B, "num_agents": N, "reps": reps, "rounds": rounds, "unit": "us per call"}
    for name, v in times.items():
        out[name] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    med = lambda k: statistics.median(times[k])
    out["rank_sampled_over_proportional"] = round(med("prio_rank_sampled_rho0") / med("sample_proportional"), 3)
    out["staleness_over_none_rank_sampled"] = round(med("prio_rank_sampled_rho0.1") / med("prio_rank_sampled_rho0"), 3)
    out["prio_over_sample_rank"] = round(med("prio_rank_rho0") / med("sample_rank"), 3)
    out["prio_over_sample_proportional"] = round(med("prio_proportional_rho0") / med("sample_proportional"), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / "plr_replay" / "bench_plr_replay.json"))
    ap.add_argument("--step", choices=["kernel"], default=None, help="run the measurement in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_plr_replay: needs the GPU (no CPU fallback)")
        print("BENCH_PLR_REPLAY_STEP " + json.dumps(step_kernel(a.reps, a.rounds)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, str(Path(__file__).resolve()), "--step",
           "kernel", "--reps", str(a.reps), "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("BENCH_PLR_REPLAY_STEP ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"bench_plr_replay: the measurement failed (exit status {r.returncode})")
    line = lines[-1][len("BENCH_PLR_REPLAY_STEP "):]
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
