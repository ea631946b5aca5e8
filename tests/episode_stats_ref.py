"""Numpy restatement of toued_episode_stats (csrc/epstats.hip): the episodes a batch of workers completes in a
trajectory, with every worker's unfinished episode carried from call to call.

Per worker, first step first: ``run_ret = fl32(run_ret + r_t)``, ``run_len += 1``; on ``done_t`` the episode
``(run_ret, run_len)`` is recorded and both are cleared.  The running return is an f32 sum in time order (the
contract: it makes the carry bit-exact and a call on T1 + T2 steps equal to two calls).  The sums over episodes and
over rewards are taken with ``math.fsum`` of exact f64 terms (f32 -> f64 and the square of an f32 in f64 are exact),
so they are the correctly rounded sums the kernel's f64 sums are held to.
"""
from __future__ import annotations

import math

import numpy as np

COLUMNS = ("episodes", "ret_sum", "ret_sq_sum", "len_sum", "reward_sum", "steps")


def episode_stats(reward, done, run_ret=None, run_len=None):
    """reward f32 [N, T, W], done [N, T, W] (any integer / bool), carry run_ret f32 [N, W], run_len int32 [N, W]
    (None: zeros).  Returns (stats f64 [N, 6], run_ret, run_len, abs_terms f64 [N, 6]): the columns of COLUMNS, the new
    carry (new arrays) and per column the sum of the terms' magnitudes, the scale of an f64 summation error."""
    reward = np.asarray(reward, np.float32)
    done = np.asarray(done).astype(bool)
    N, T, W = reward.shape
    ret = np.zeros((N, W), np.float32) if run_ret is None else np.array(run_ret, np.float32)
    ln = np.zeros((N, W), np.int32) if run_len is None else np.array(run_len, np.int32)
    rets = [[] for _ in range(N)]
    lens = [[] for _ in range(N)]
    for t in range(T):
        ret = (ret + reward[:, t]).astype(np.float32)        # one f32 rounding per step
        ln = ln + 1
        d = done[:, t]
        for a, w in zip(*np.nonzero(d)):
            rets[a].append(float(ret[a, w]))
            lens[a].append(int(ln[a, w]))
        ret = np.where(d, np.float32(0.0), ret).astype(np.float32)
        ln = np.where(d, 0, ln).astype(np.int32)
    stats = np.zeros((N, 6), np.float64)
    mag = np.zeros((N, 6), np.float64)
    for a in range(N):
        rew = [float(x) for x in reward[a].ravel()]
        stats[a] = (len(rets[a]), math.fsum(rets[a]), math.fsum(x * x for x in rets[a]), sum(lens[a]),
                    math.fsum(rew), W * T)
        mag[a] = (len(rets[a]), math.fsum(abs(x) for x in rets[a]), math.fsum(x * x for x in rets[a]), sum(lens[a]),
                  math.fsum(abs(x) for x in rew), W * T)
    return stats, ret, ln, mag


def enumerate_episodes(reward, done, run_ret=None, run_len=None):
    """The plain per-worker enumeration: for agent a the list of (return, length) of the episodes completed, worker
    by worker, and the carry left.  Independent of ``episode_stats``'s vectorised walk."""
    reward = np.asarray(reward, np.float32)
    N, T, W = reward.shape
    out = []
    ret_c = np.zeros((N, W), np.float32)
    len_c = np.zeros((N, W), np.int32)
    for a in range(N):
        eps = []
        for w in range(W):
            r = np.float32(0.0) if run_ret is None else np.float32(run_ret[a][w])
            n = 0 if run_len is None else int(run_len[a][w])
            for t in range(T):
                r = np.float32(r + reward[a, t, w])
                n += 1
                if done[a][t][w]:
                    eps.append((float(r), n))
                    r, n = np.float32(0.0), 0
            ret_c[a, w], len_c[a, w] = r, n
        out.append(eps)
    return out, ret_c, len_c


def done_pattern(name: str, N: int, T: int, W: int, rng) -> np.ndarray:
    """The edge done patterns of the tests, uint8 [N, T, W]."""
    d = np.zeros((N, T, W), np.uint8)
    if name == "random":
        d = (rng.random((N, T, W)) < 0.15).astype(np.uint8)
    elif name == "never":
        pass
    elif name == "always":
        d[:] = 1
    elif name == "first":
        d[:, 0] = 1
    elif name == "last":
        d[:, T - 1] = 1
    else:
        raise ValueError(name)
    return d


PATTERNS = ("random", "never", "always", "first", "last")
