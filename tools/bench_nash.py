"""Timings of the Nash solver (toued_nash_solve) and of the simplex projection (toued_project_simplex):

    python3 tools/bench_nash.py [--trials 5] [--torch_iters 200] [--out FILE.json]

  * toued_nash_solve at B in {8, 32, 128} x G in {1, 64} games of N(0, 1) payoffs, every slot active, 10 000
    iterations at lr 0.01 from the one-hot starts: ms per solve, the median over `trials` trials of a host clock
    around one call ending in a device synchronise (after a warm-up call), and ns per iteration.
  * beside each, the same iteration written with torch ops on the same GPU (get_nash as one would run it on this stack
    without the kernel: two batched matrix-vector products and two sort-based projections per iteration, util/
    projection.py's form, a dozen launches each), `torch_iters` iterations, timed the same way and scaled per
    iteration; and the largest difference between its averages and the kernel's at that iteration count.
  * toued_project_simplex at (R, B) = (512, 128) and (1, 4000) on N(0, 1) rows: us per call, device events around 50
    back-to-back calls.

Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

from bench_polret import _timed  # noqa: E402


def torch_project(v, mask, ind):
    """projection_simplex (util/projection.py:9-37) over the rows of v with torch ops; mask = arange(B) < nz."""
    s, _ = torch.sort(torch.where(mask, v, torch.full_like(v, float("-inf"))), dim=1, descending=True)
    vals = torch.where(mask, s, torch.zeros_like(s))
    cs = torch.cumsum(vals, dim=1)
    cond = ((1.0 / ind + (vals - cs / ind)) > 0) & mask
    k = cond.sum(dim=1, keepdim=True)
    tau = (torch.gather(cs, 1, k - 1) - 1.0) / k
    return torch.where(mask, torch.relu(v - tau), torch.zeros_like(v))


def torch_get_nash(M, nx, ny, x0, y0, iters, lr):
    B = M.shape[1]
    ar = torch.arange(B, device=M.device).unsqueeze(0)
    mx, my = ar < nx.unsqueeze(1), ar < ny.unsqueeze(1)
    ind = (ar + 1).to(torch.float32)
    x, y = x0.clone(), y0.clone()
    xs, ys = x0.double(), y0.double()
    for _ in range(iters):
        gx = torch.bmm(M, y.unsqueeze(2)).squeeze(2)
        gy = torch.bmm(x.unsqueeze(1), M).squeeze(1)
        x, y = torch_project(x - lr * gx, mx, ind), torch_project(y + lr * gy, my, ind)
        xs += x
        ys += y
    return (xs / (iters + 1)).float(), (ys / (iters + 1)).float()


def _wall_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_solve(B: int, G: int, iters: int, torch_iters: int, trials: int) -> dict:
    from toued.nash import solve_nash
    gen = torch.Generator(device="cuda").manual_seed(1000 * B + G)
    M = torch.randn((G, B, B), generator=gen, device="cuda")
    n = torch.full((G,), B, dtype=torch.int32, device="cuda")
    hot = torch.zeros((G, B), device="cuda")
    hot[:, 0] = 1.0
    kern = lambda it: solve_nash(M, n, n, hot, hot, it, 0.01)
    ref = lambda: torch_get_nash(M, n, n, hot, hot, torch_iters, 0.01)
    s, (tx, ty) = kern(torch_iters), ref()                   # warm-up of both, and their agreement
    diff = max(float((s.x - tx).abs().max()), float((s.y - ty).abs().max()))
    full = kern(iters)
    t_k = [_wall_ms(lambda: kern(iters)) for _ in range(trials)]
    t_t = [_wall_ms(ref) for _ in range(trials)]
    m_k, m_t = statistics.median(t_k), statistics.median(t_t)
    return {"B": B, "G": G, "iters": iters, "solve_ms": round(m_k, 3), "solve_ms_trials": [round(v, 3) for v in t_k],
            "kernel_ns_per_iter": round(m_k * 1e6 / iters, 1), "torch_iters": torch_iters,
            "torch_ms": round(m_t, 3), "torch_ms_trials": [round(v, 3) for v in t_t],
            "torch_ns_per_iter": round(m_t * 1e6 / torch_iters, 1),
            "torch_over_kernel_per_iter": round((m_t / torch_iters) / (m_k / iters), 1),
            "max_abs_diff_at_torch_iters": diff,
            "exploitability_mean": round(float(full.exploitability.mean()), 6)}


def time_project(R: int, B: int, trials: int) -> dict:
    from toued.nash import project_simplex
    gen = torch.Generator(device="cuda").manual_seed(R + B)
    x = torch.randn((R, B), generator=gen, device="cuda")
    nz = torch.full((R,), B, dtype=torch.int32, device="cuda")
    fn = lambda: project_simplex(x, nz)
    fn()
    t = [_timed(fn, 50) * 1e3 for _ in range(trials)]
    return {"R": R, "B": B, "project_us": round(statistics.median(t), 2), "project_us_trials": [round(v, 2) for v in t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--torch_iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nash: needs the GPU (no CPU fallback)")
    out = {"nash_solve": [time_solve(B, G, a.iters, a.torch_iters, a.trials) for B in (8, 32, 128) for G in (1, 64)],
           "project_simplex": [time_project(512, 128, a.trials), time_project(1, 4000, a.trials)]}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
