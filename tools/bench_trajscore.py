"""What tools/bench_vscore.py, bench_maxmc.py and bench_polscore.py share: the random trajectory they time their
kernels on, the alternated device-event timing, the C3 regret round of a list of score functions, and the driver that
runs each measurement step in a child process of its own under `timeout` (a step that fails ends the run)."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

HBM_SPEC_TBS = 8.0          # MI355X HBM3E peak, datasheet
HBM_COPY_TBS = 6.29         # what a float4 copy reaches
N_AGENTS, N_WORKERS = 512, 64
SHAPES = (("all", 750), ("tabular", 2000))      # (mode, its eval length T); the critic row / actor table is the mode's


def random_trajectory(mode: str, T: int, with_theta: bool = False) -> dict:
    """D and a random trajectory of N_AGENTS x N_WORKERS x T on the GPU, seeded with T: theta (only when asked for,
    drawn first) f32 [N, D, 5], vcrit f32 [N, D], idx / tm int32 [N, T+1, W], rew f32 and done uint8 [N, T, W]."""
    import torch
    from toued.rollout import RolloutWrapper
    N, W = N_AGENTS, N_WORKERS
    D = RolloutWrapper(mode, 20).obs_dim
    g = torch.Generator(device="cuda").manual_seed(T)
    tr = {"D": D}
    if with_theta:
        tr["theta"] = torch.randn((N, D, 5), device="cuda", generator=g)
    tr["vcrit"] = torch.randn((N, D), device="cuda", generator=g)
    tr["idx"] = torch.randint(0, D - 1, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
    tr["tm"] = torch.randint(0, 2000, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
    tr["rew"] = torch.randn((N, T, W), device="cuda", generator=g)
    tr["done"] = (torch.rand((N, T, W), device="cuda", generator=g) < 0.05).to(torch.uint8)
    return tr


def vscore_call(tr: dict, T: int):
    """toued_value_loss_scores on the trajectory (no advantages), as a function of no arguments returning (pvl, l1)."""
    import numpy as np
    import torch
    from toued import _lib
    gamma, gl = 0.99, float(np.float32(0.99 * 0.95))
    pvl, l1 = torch.empty(N_AGENTS, device="cuda"), torch.empty(N_AGENTS, device="cuda")

    def vscore():
        _lib.call("toued_value_loss_scores", N_AGENTS, N_WORKERS, T, tr["D"], _lib.ptr(tr["vcrit"]),
                  _lib.ptr(tr["idx"]), _lib.ptr(tr["tm"]), _lib.ptr(tr["rew"]), _lib.ptr(tr["done"]), gamma, gl,
                  _lib.ptr(pvl), _lib.ptr(l1), None, _lib.stream_ptr())
        return pvl, l1
    return vscore


def time_alternated(fns, reps: int, tol: dict) -> dict:
    """``fns``: (name, function) pairs, the kernel under test first and the composed path last.  All are warmed up (code
    objects, allocator pools), the kernel's outputs are held against the composed ones with torch.allclose(**tol), then
    all are timed alternately with device events, ``reps`` times each: {name: [ms]}."""
    import torch
    for _ in range(3):
        outs = {name: fn() for name, fn in fns}
        k_out = [x.clone() for x in outs[fns[0][0]]]
    torch.cuda.synchronize()
    for a, b in zip(k_out, outs[fns[-1][0]]):
        assert torch.allclose(a, b, **tol), (a[:4], b[:4])
    times = {name: [] for name, _ in fns}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for name, fn in fns:
            ev0.record()
            fn()
            ev1.record()
            torch.cuda.synchronize()
            times[name].append(ev0.elapsed_time(ev1))
    return times


def timing_row(mode: str, T: int, D: int, reps: int, times: dict):
    """The head of a kernel row -- the shape, then median, min and max of every timed function -- and the medians."""
    med = {name: statistics.median(v) for name, v in times.items()}
    row = {"mode": mode, "N": N_AGENTS, "W": N_WORKERS, "T": T, "D": D, "reps": reps}
    for name, v in times.items():
        row.update({f"{name}_ms_median": round(med[name], 4), f"{name}_ms_min": round(min(v), 4),
                    f"{name}_ms_max": round(max(v), 4)})
    return row, med


def hbm_fractions(tbs: float) -> dict:
    return {"fraction_of_hbm_spec_8.0": round(tbs / HBM_SPEC_TBS, 3),
            "fraction_of_hbm_copy_6.29": round(tbs / HBM_COPY_TBS, 3)}


def step_rounds(score_functions, rounds: int) -> dict:
    """The C3 regret round (all_shortlife, 512 agents, every agent terminated) with each of ``score_functions``, timed
    the way bench.py's workload_c3 times it (a host clock around ``rounds`` rounds ending in a device synchronise, after
    one warm-up round), alternated three times in one process."""
    import torch
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    trs = {}
    for sf in score_functions:
        args = parse_args(["--env_mode", "all_shortlife", "--num_agents", "512", "--num_mini_batches", "1",
                           "--score_function", sf])
        trs[sf] = Trainer(args)

    def one_round(tr):
        tr.agents.step = tr.agents.levels[:, L_LIFETIME].clone()     # every agent terminated: all are scored
        tr.buffer, tr.agents = tr.sampler.sample(tr.rng, tr.buffer, tr.agents)

    times = {sf: [] for sf in trs}
    for sf, tr in trs.items():
        one_round(tr)                                                  # warm-up
    for _ in range(3):                                                 # alternated
        for sf, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(rounds):
                one_round(tr)
            torch.cuda.synchronize()
            times[sf].append((time.perf_counter() - t0) / rounds * 1e3)
    return {"c3_regret_round": {sf: {"regret_round_ms": [round(x, 3) for x in v],
                                     "regret_round_ms_median": round(statistics.median(v), 3)}
                                for sf, v in times.items()}}


def main(tool: str, script: str, step_kernel, score_functions, gate: str, timeouts: dict) -> int:
    """The tools' command line.  ``tool`` is the name (bench_<tool>, BENCH_<TOOL>_STEP, profiles/<tool>/), ``script``
    the tool's own file, ``step_kernel(reps)`` its kernel step, ``score_functions`` those of its rounds step, ``gate``
    the key of its kernel rows that decides the exit status, ``timeouts`` the steps' limits in seconds."""
    name, tag = f"bench_{tool}", f"BENCH_{tool.upper()}_STEP "
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=str(ROOT / "profiles" / tool / f"{name}.json"))
    ap.add_argument("--step", choices=sorted(timeouts), default=None, help="run one step in this process")
    a = ap.parse_args()
    if a.step is not None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit(f"{name}: needs the GPU (no CPU fallback)")
        res = step_kernel(a.reps) if a.step == "kernel" else step_rounds(score_functions, a.rounds)
        print(tag + json.dumps(res), flush=True)
        return 0
    out = {}
    for step in ("kernel", "rounds"):
        cmd = ["timeout", "-k", "10", str(timeouts[step]), sys.executable, str(Path(script).resolve()),
               "--step", step, "--reps", str(a.reps), "--rounds", str(a.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(tag)]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"{name}: step {step} failed (exit status {r.returncode}); nothing more is run")
        out.update(json.loads(lines[-1][len(tag):]))
    line = json.dumps(out)
    print(line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 0 if all(k[gate] for k in out["kernel"]) else 1
