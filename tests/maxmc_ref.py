"""numpy restatement of the MaxMC PLR score (toued_max_mc_scores), the target the GPU tests compare with.

Values in float32 by the critic's formula (tests/vscore_ref.py ``values``); rows t = 0..T-1 enter the score.  Per
worker, forward in time, in float32 with one rounding per operation:
    cum = cum + disc * r[t];  disc = disc * gamma;  on done[t]: best = max(best, cum), cum = 0, disc = 1
from cum = 0, disc = 1, best = -inf; an episode still open after the last step counts with its truncated return, an
empty one (done on the last step) adds nothing.  rmax = max(prior, max over workers of best), and the score is
rmax - mean(v) in float64, the unclipped mean of R_max - V(s_t).
Layouts are the trajectory's: idx / time [N, T+1, W], reward / done [N, T, W], vcrit [N, D], prior [N] or None.
"""
import numpy as np

from vscore_ref import values


def worker_max(reward, done, gamma):
    """float32 [N, W]: the best episode return of each worker, all (agent, worker) chains advanced together."""
    f = np.float32
    r = np.asarray(reward, f)
    d = np.asarray(done).astype(bool)
    N, T, W = r.shape
    g = f(gamma)
    cum, disc = np.zeros((N, W), f), np.ones((N, W), f)
    best = np.full((N, W), -np.inf, f)
    is_open = np.zeros((N, W), bool)
    for t in range(T):
        cum = (cum + (disc * r[:, t]).astype(f)).astype(f)
        disc = (disc * g).astype(f)
        best = np.where(d[:, t], np.maximum(best, cum), best)
        cum = np.where(d[:, t], f(0.0), cum).astype(f)
        disc = np.where(d[:, t], f(1.0), disc).astype(f)
        is_open = ~d[:, t]
    return np.where(is_open, np.maximum(best, cum), best).astype(f)


def max_mc_scores(vcrit, idx, time, reward, done, gamma, prior=None):
    """(score float64 [N], rmax float32 [N], wmax float32 [N, W])."""
    wmax = worker_max(reward, done, gamma)
    N, T, W = np.asarray(reward).shape
    if T * W == 0:
        raise ValueError("max_mc_scores: no (worker, step) pairs")
    rmax = wmax.max(axis=1) if N else np.zeros(0, np.float32)
    if prior is not None:
        rmax = np.maximum(np.asarray(prior, np.float32), rmax)
    v = values(vcrit, idx, time)[:, :T].astype(np.float64).reshape(N, -1)
    return rmax.astype(np.float64) - v.sum(axis=1) / (float(W) * float(T)), rmax.astype(np.float32), wmax
