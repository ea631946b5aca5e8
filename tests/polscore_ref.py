"""numpy restatement of the policy PLR scores (toued_policy_scores), the target the GPU tests compare with.

Per (worker, step), in float32 with one rounding per operation, the operations of the rollout's actor (actor_probs5,
csrc/env_dev.h) in its order:
    c = f32(time) * 0.001;  l_j = theta[idx][j] + c * theta[D-1][j];  m = max_j l_j;  d_j = l_j - m;  e_j = exp(d_j)
    s = e_0 + e_1 + e_2 + e_3 + e_4 (left to right);  p_j = e_j / s
then
    q = e_0 d_0 + ... + e_4 d_4 (left to right);  H = max(log(s) - q / s, 0);  lc = 1 - p_max;  mm = 1 - (p_max - p_2nd)
with p_2nd the second entry of p sorted descending (two equal maxima: mm = 1).  exp and log are oracle.pmath's, the
restatements of common.h's pexp and plog (pexp_le0 equals pexp on every softmax argument).  An index outside the table
is held to row D-1.  The scores are the float64 means of the float32 terms over rows t = 0..T-1 (the end observation,
row T, does not enter), the entropy divided by log 5.
Layouts are the trajectory's: theta [N, D, 5], idx / time [N, R, W] with R = T + 1 rows (or any R when T is given).
"""
import math

import numpy as np

from oracle import pmath

f32 = np.float32


def _rows(theta, idx):
    theta = np.asarray(theta, f32)
    idx = np.asarray(idx)
    N, D = theta.shape[0], theta.shape[1]
    i = np.where((idx >= 0) & (idx < D - 1), idx, D - 1)
    a = np.arange(N).reshape(N, 1, 1)
    return theta[a, i], theta[:, D - 1][:, None, None, :]       # [N, R, W, 5], [N, 1, 1, 5]


def probs_terms(theta, idx, time):
    """(p float32 [N, R, W, 5], terms float32 [N, 3, R, W]: H, lc, mm) of every row given."""
    row, last = _rows(theta, idx)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        c = (np.asarray(time).astype(f32) * f32(0.001)).astype(f32)[..., None]
        l = (row + (c * last).astype(f32)).astype(f32)
        m = l.max(axis=-1, keepdims=True)
        d = (l - m).astype(f32)
        e = pmath.exp(d)
        s = e[..., 0]
        q = (e[..., 0] * d[..., 0]).astype(f32)
        for j in range(1, 5):
            s = (s + e[..., j]).astype(f32)
            q = (q + (e[..., j] * d[..., j]).astype(f32)).astype(f32)
        p = (e / s[..., None]).astype(f32)
        H = np.maximum((pmath.log(s) - (q / s).astype(f32)).astype(f32), f32(0.0))
        ps = np.sort(p, axis=-1)
        pmax, p2nd = ps[..., 4], ps[..., 3]
        lc = (f32(1.0) - pmax).astype(f32)
        mm = (f32(1.0) - (pmax - p2nd).astype(f32)).astype(f32)
    return p, np.stack([H, lc, mm], axis=1).astype(f32)


def policy_scores(theta, idx, time, T=None):
    """(entropy, least confidence, min margin), float64 [N] each: the means of the float32 terms of rows t < T
    (default: all rows but the last), the entropy over log 5."""
    idx, time = np.asarray(idx), np.asarray(time)
    T = idx.shape[1] - 1 if T is None else T
    if T * idx.shape[2] == 0:
        raise ValueError("policy_scores: no (worker, step) pairs")
    _, terms = probs_terms(theta, idx[:, :T], time[:, :T])
    mean = terms.astype(np.float64).reshape(terms.shape[0], 3, -1).mean(axis=2)
    return mean[:, 0] / math.log(5), mean[:, 1], mean[:, 2]


def terms_f64(theta, idx, time):
    """The three per-step terms float64 [N, 3, R, W] from a float64 softmax and log: H = -sum_j p_j log p_j with
    log p_j = d_j - log s (so p_j = 0 adds 0), lc = 1 - max p, mm = 1 - (largest p - second largest p)."""
    row, last = _rows(theta, idx)
    c = np.asarray(time).astype(np.float64)[..., None] * 0.001
    l = row.astype(np.float64) + c * last.astype(np.float64)
    d = l - l.max(axis=-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=-1, keepdims=True)
    p = e / s
    H = -(p * (d - np.log(s))).sum(axis=-1)
    ps = np.sort(p, axis=-1)
    return np.stack([H, 1.0 - ps[..., 4], 1.0 - (ps[..., 4] - ps[..., 3])], axis=1)


def policy_scores_f64(theta, idx, time, T=None):
    """policy_scores' three definitions in float64 throughout."""
    idx, time = np.asarray(idx), np.asarray(time)
    T = idx.shape[1] - 1 if T is None else T
    terms = terms_f64(theta, idx[:, :T], time[:, :T])
    mean = terms.reshape(terms.shape[0], 3, -1).mean(axis=2)
    return mean[:, 0] / math.log(5), mean[:, 1], mean[:, 2]


# --------------------------------------------------------------------------------------------------- test inputs
SCALES = (0.0, 1e-3, 1.0, 30.0, 300.0)


def make_case(N, T, W, D, first_scale=0):
    """A trajectory dict {theta [N, D, 5], idx, time [N, T+1, W]} (read-only arrays):
      * agent a's table is drawn at scale SCALES[(a + first_scale) % 5], its time row (D-1) included: 0 is the uniform
        policy, 300 makes every e_j but the largest underflow to 0 (a deterministic policy);
      * times in [0, 2000];
      * the last agent whose scale is not 0 has, on every third table row, its two largest logits equal, and a time row
        of five equal entries (so that the tie survives the time term exactly);
      * where the trajectory has room, agent 0's first pairs hold an index past the row (D + 3), a negative one and two
        equal to D - 1; all of them are read as row D - 1."""
    rs = np.random.RandomState(7919 * N + 31 * T + 7 * W + D + first_scale)
    scale = np.array([SCALES[(a + first_scale) % 5] for a in range(N)], f32)
    theta = (rs.randn(N, D, 5).astype(f32) * scale[:, None, None]).astype(f32)
    tied = [a for a in range(N) if scale[a] != 0]
    if tied:
        a = tied[-1]
        theta[a, D - 1, :] = theta[a, D - 1, 0]
        rows = np.arange(0, D - 1, 3)
        top = theta[a, rows].argmax(axis=1)
        theta[a, rows, (top + 1) % 5] = theta[a, rows, top]
    idx = rs.randint(0, max(D - 1, 1), size=(N, T + 1, W)).astype(np.int32)
    time = rs.randint(0, 2001, size=(N, T + 1, W)).astype(np.int32)
    flat = idx[0, :T].reshape(-1)          # a view: T W contiguous ints
    special = [D + 3, -1, D - 1, D - 1]
    for k, v in enumerate(special[:max(0, flat.size - 1)]):
        flat[k] = v
    out = {"theta": theta, "idx": idx, "time": time}
    for v in out.values():
        v.setflags(write=False)
    return out
