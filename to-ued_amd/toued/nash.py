"""The double-oracle level sampler's game solver (environments/nash_sampler.py, util/projection.py).

In the reference's NashSampler a train player mixes over levels to minimise algorithmic regret and an eval player mixes
over levels to maximise it; the next training distribution is the Nash equilibrium of the empirical regret matrix.
This module is the part of that sampler that stands on its own:

  ``project_simplex``      util/projection.py:9-37 ``projection_simplex`` (toued_project_simplex)
  ``solve_nash``           nash_sampler.py:39-58 ``get_nash`` (toued_nash_solve: every iteration in one launch)
  ``initial_strategies``   the random start of ``compute_nash`` (:193-198)
  ``training_level_ids``   the draw of ``get_training_levels`` (:210-211)
  ``cross_regret``         an extension, not in the reference: the exact regret of tabular agents on each other's
                           levels, a payoff matrix that needs no training run

Filling the payoff matrix by LPG training (``get_payoff_matrix``), the best-response searches (``get_train_br``,
``get_eval_br``) and a ``train_do`` driver are out of scope.

    python -m toued.nash --payoff M.npy [--nx N --ny N --iters 10000 --lr 0.01 --out sol.npz]
"""
from __future__ import annotations

import argparse
from typing import NamedTuple

import numpy as np
import torch

from . import _lib


class NashSolution(NamedTuple):
    x: torch.Tensor               # f32 [B] or [G, B]: the row (train, minimising) player's average strategy
    y: torch.Tensor               # f32 [B] or [G, B]: the column (eval, maximising) player's
    value: torch.Tensor           # f32 [] or [G]: x^T M y
    exploitability: torch.Tensor  # f32 [] or [G]: max_j (x^T M)_j - min_i (M y)_i, 0 at an equilibrium


def _counts(n, rows: int, device) -> torch.Tensor:
    """An int or an int tensor (0-d or [rows]) as int32 [rows] on the device."""
    if isinstance(n, torch.Tensor):
        return n.to(device=device, dtype=torch.int32).reshape(-1).expand(rows).contiguous()
    return torch.full((rows,), int(n), dtype=torch.int32, device=device)


def project_simplex(x: torch.Tensor, nz) -> torch.Tensor:
    """projection_simplex(x, max_nz) (util/projection.py:9-37) over the last axis: the Euclidean projection of
    ``x[..., :nz]`` onto the unit simplex, exactly 0 from index ``nz`` on.  x f32 [B] or [R, B]; nz an int or an int
    tensor (one count, or one per row; values outside [1, B] are clamped on the device).  No host synchronisation."""
    if x.dtype != torch.float32 or x.dim() not in (1, 2):
        raise ValueError(f"project_simplex: x {x.dtype} {tuple(x.shape)}, expected float32 [B] or [R, B]")
    if x.dim() == 1:
        return project_simplex(x.view(1, -1), nz)[0]
    x = x.contiguous()
    R, B = x.shape
    out = torch.empty_like(x)
    n = _counts(nz, R, x.device)
    _lib.call("toued_project_simplex", _lib.ptr(x), _lib.ptr(n), R, B, _lib.ptr(out), _lib.stream_ptr())
    return out


def solve_nash(payoff: torch.Tensor, nx, ny, x0: torch.Tensor | None = None, y0: torch.Tensor | None = None,
               iters: int = 10000, lr: float = 0.01) -> NashSolution:
    """get_nash (nash_sampler.py:39-58): ``iters`` simultaneous projected-gradient steps of the zero-sum game
    ``x^T M y`` (x over the first ``nx`` rows minimises, y over the first ``ny`` columns maximises) and the means of
    the iterates, the start included.  payoff f32 [B, B] or [G, B, B] with B <= 128; nx, ny ints or int tensors (one
    per game).  x0 / y0 f32 [B] or [G, B] are used as given; absent, the start is one-hot at slot 0 (train_do.py:17-18).
    Rows >= nx and columns >= ny of the payoff do not enter.  One launch, no host synchronisation."""
    if payoff.dtype != torch.float32 or payoff.dim() not in (2, 3) or payoff.shape[-1] != payoff.shape[-2]:
        raise ValueError(f"solve_nash: payoff {payoff.dtype} {tuple(payoff.shape)}, expected float32 [B, B] or "
                         f"[G, B, B]")
    if payoff.dim() == 2:
        s = solve_nash(payoff.unsqueeze(0), nx, ny, None if x0 is None else x0.view(1, -1),
                       None if y0 is None else y0.view(1, -1), iters, lr)
        return NashSolution(s.x[0], s.y[0], s.value[0], s.exploitability[0])
    payoff = payoff.contiguous()
    G, B = payoff.shape[0], payoff.shape[1]
    dev = payoff.device

    def start(v, name):
        if v is None:
            v = torch.zeros((G, B), dtype=torch.float32, device=dev)
            v[:, 0] = 1.0
            return v
        if v.dtype != torch.float32 or tuple(v.shape) != (G, B) or v.device != dev:
            raise ValueError(f"solve_nash: {name} {v.dtype} {tuple(v.shape)} on {v.device}, expected float32 "
                             f"{(G, B)} on {dev}")
        return v.contiguous()

    x0, y0 = start(x0, "x0"), start(y0, "y0")
    x = torch.empty((G, B), dtype=torch.float32, device=dev)
    y = torch.empty((G, B), dtype=torch.float32, device=dev)
    stats = torch.empty((G, 2), dtype=torch.float32, device=dev)
    nx, ny = _counts(nx, G, dev), _counts(ny, G, dev)     # both alive until the call is enqueued
    _lib.call("toued_nash_solve", _lib.ptr(payoff), _lib.ptr(nx), _lib.ptr(ny), _lib.ptr(x0), _lib.ptr(y0), G, B,
              int(iters), float(lr), _lib.ptr(x), _lib.ptr(y), _lib.ptr(stats), _lib.stream_ptr())
    return NashSolution(x, y, stats[:, 0], stats[:, 1])


def initial_strategies(key: torch.Tensor, B: int, nz):
    """The random start of compute_nash (nash_sampler.py:196-198) from its ``_rng``:
    ``where(arange(B) < nz, jax.random.uniform(key, (2, B)), 0)``, each row projected with ``nz``.  The reference
    projects both rows with the train buffer's count; so does this.  key int32 [2]; nz an int or a 0-d int tensor.
    Returns (x0, y0), f32 [B] each."""
    from . import prng
    u = prng.uniform(key.reshape(1, 2), 2 * int(B)).view(2, int(B))
    n = _counts(nz, 2, u.device)
    u = torch.where(torch.arange(int(B), device=u.device).unsqueeze(0) < n.unsqueeze(1), u, torch.zeros_like(u))
    s = project_simplex(u, n)
    return s[0], s[1]


def training_level_ids(key: torch.Tensor, x: torch.Tensor, n: int) -> torch.Tensor:
    """The draw of get_training_levels (nash_sampler.py:210-211) from its ``_rng``:
    ``jax.random.choice(key, arange(B), (n,), True, x)`` -> int32 [n].  The cdf of x is built on the host in jax's
    cumsum order, as LevelSampler._frozen_ids builds its own (one read-back of x)."""
    from .level_sampler import cumsum_assoc_np
    cdf = torch.from_numpy(cumsum_assoc_np(x.detach().cpu().numpy().astype(np.float32))).to(x.device)
    out = torch.empty(int(n), dtype=torch.int32, device=x.device)
    _lib.call("toued_choice_cdf", _lib.ptr(key.contiguous()), _lib.ptr(cdf), cdf.shape[0], int(n), _lib.ptr(out),
              _lib.stream_ptr())
    return out


def cross_regret(rollout_manager, levels: torch.Tensor, theta: torch.Tensor, max_rollout_len: int) -> torch.Tensor:
    """The exact regret of every tabular agent on every level: out[i, j] = V*(level j) - V^{pi_i}(level j) over
    ``max_rollout_len`` steps, f32 [n_agents, n_levels] (levels int32 [n_levels, 80], theta f32 [n_agents, obs_dim,
    5]).  One call each to RolloutWrapper.optimal_return and policy_return, the latter on the n_agents * n_levels
    (agent, level) pairs; no rollout, no keys.  A cheap, exact example of a payoff matrix for ``solve_nash``.  An
    extension: the reference fills its matrix by one LPG training per train level (get_payoff_matrix)."""
    if not rollout_manager.spec.tabular:
        raise NotImplementedError("Cross regret not implemented for non-tabular environments.")
    n_agents, n_levels = theta.shape[0], levels.shape[0]
    vst = rollout_manager.optimal_return(levels, max_rollout_len)
    lv = levels.repeat(n_agents, 1)                               # pair (i, j) at i * n_levels + j
    th = theta.repeat_interleave(n_levels, dim=0)
    vpi = rollout_manager.policy_return(lv, th, max_rollout_len)
    return vst.unsqueeze(0) - vpi.view(n_agents, n_levels)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m toued.nash",
                                 description="Solve a saved payoff matrix: the Nash equilibrium of the zero-sum game "
                                             "x^T M y (rows minimise, columns maximise) by get_nash's iteration.")
    ap.add_argument("--payoff", required=True, help=".npy file with a [B, B] or [G, B, B] matrix (B <= 128)")
    ap.add_argument("--nx", type=int, default=None, help="active rows (default: all)")
    ap.add_argument("--ny", type=int, default=None, help="active columns (default: all)")
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--out", default=None, help=".npz file for x, y, value, exploitability")
    a = ap.parse_args(argv)
    M = torch.from_numpy(np.load(a.payoff).astype(np.float32)).cuda()
    B = M.shape[-1]
    s = solve_nash(M, B if a.nx is None else a.nx, B if a.ny is None else a.ny, iters=a.iters, lr=a.lr)
    value, expl = s.value.cpu().numpy(), s.exploitability.cpu().numpy()
    for g, (v, e) in enumerate(zip(value.reshape(-1), expl.reshape(-1))):
        print(f"game {g}: value {v:.6f} exploitability {e:.6f}")
    if a.out:
        np.savez(a.out, x=s.x.cpu().numpy(), y=s.y.cpu().numpy(), value=value, exploitability=expl)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
