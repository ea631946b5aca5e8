"""float64 numpy restatement of the exact state occupancy of a tabular agent (RolloutWrapper.policy_occupancy) -- the
reference of tests/test_occupancy_cpu.py and tests/test_gpu_occupancy.py.

The forward counterpart of tests/polret_ref.py: with H = min(max_steps_in_episode, max_rollout_len), d_0 = 1 at the
start state (start cell, all used objects present) and, for t = 0 .. H-1,

    d_{t+1}(pos1, (e \\ c) | R) += d_t(s) * pi_t(a|s) * keep(s, a) * P[absent][R]

for every state s = (pos, e), action a (pos1 the next cell, c the objects collected there) and subset R of the absent
objects, so d_t(s) = P(the first episode is still running at step t and is in state s).  pi_t is polret_ref.policy
(float64 softmax of the rollouts' float32 logits) and keep = clip(1 - sum of the collected objects' p_terminate, 0, 1):
the env's bernoulli(p) terminates always for p >= 1, where polret_ref follows the reference's DP and does not clip.
The three policy terms are polscore_ref.terms_f64 on the step's float32 logits.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

import polret_ref as prf
import polscore_ref as psr
from optret_ref import _next_pos, invalid_states, start_index

F32 = np.float32
SUMMARY = ("ret", "length", "p_early_term", "alive_end", "entropy", "least_confidence", "min_margin", "ret_abs")


class Occupancy(NamedTuple):
    visits: np.ndarray        # float64 [S]: sum_t d_t(s)
    rows: np.ndarray          # float64 [max_rollout_len, S]: d_t, rows t >= H zero
    collected: np.ndarray     # float64 [max_n_objs]: expected collections of each object
    summary: np.ndarray       # float64 [8], SUMMARY's columns
    d_end: np.ndarray         # float64 [S]: d_H


def level_tables(spec, params, i):
    """What does not depend on time: (coll bool [S, 5, n], r [S, 5], p_term [S, 5], the p > 0 outcomes as (row = s * 5
    + a, target state, probability))."""
    G2, n, NE = spec.max_grid_size ** 2, spec.max_n_objs, 1 << spec.max_n_objs
    S = G2 * NE
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    walls = np.asarray(params["walls"][i], bool)
    static = np.asarray(params["static_obj_poss"][i], np.int64)
    ids = np.asarray(params["obj_ids"][i], np.int64)
    rew = np.asarray(params["obj_rewards"][i], np.float64)[ids]
    pterm = np.asarray(params["obj_p_terminate"][i], np.float64)[ids]
    presp = np.asarray(params["obj_p_respawn"][i], np.float64)[ids]
    s = np.arange(S)
    pos = (s % G2)[:, None]
    ex = (((s // G2)[:, None] >> np.arange(n)) & 1) == 1
    pos1 = _next_pos(pos, np.arange(5)[None, :], g, walls)
    coll = ex[:, None, :] & (static[None, None, :] == pos1[:, :, None]) & (np.arange(n) < nobj)[None, None, :]
    r = coll @ rew
    p_term = coll @ pterm
    nxt_ex = ((np.arange(NE)[:, None] >> np.arange(n)) & 1) == 1
    p_next = np.ones((S, 5, NE))
    for o in range(n):
        x = nxt_ex[None, None, :, o]
        absent_p = np.where(x, presp[o], 1.0 - presp[o])
        p_next *= np.where(o >= nobj, 1.0 - x,
                           np.where(coll[:, :, None, o], 1.0 - x, np.where(ex[:, None, None, o], 1.0 * x, absent_p)))
    tab = np.clip(pos1[:, :, None] + G2 * np.arange(NE)[None, None, :], 0, S - 1)
    nz = p_next > 0.0
    rows = np.broadcast_to(np.arange(S * 5).reshape(S, 5, 1), nz.shape)[nz]
    return coll, r, p_term, (rows, tab[nz], p_next[nz])


def collected_sets_p_terminate(spec, params, i):
    """The largest sum of p_terminate over a set of objects that one move of a valid state collects."""
    _, _, p_term, _ = level_tables(spec, params, i)
    return float(p_term[~invalid_states(spec, params, i)].max(initial=0.0))


def step_terms(theta, t):
    """float64 [3, S]: entropy (before the division by log 5), least confidence and min margin of pi_t(.|s), by
    polscore_ref.terms_f64 on the float32 logits of step t (a table whose rows are those logits, read at time 0)."""
    theta = np.asarray(theta, F32)
    c = F32(F32(t) * prf.TIME_SCALE)
    logits = (theta[:-1] + (c * theta[-1]).astype(F32)[None, :]).astype(F32)
    S = logits.shape[0]
    tab = np.concatenate([logits, np.zeros((1, 5), F32)])[None]
    return psr.terms_f64(tab, np.arange(S).reshape(1, 1, S), np.zeros((1, 1, S), np.int64))[0, :, 0, :]


def occupancy(spec, params, i, theta, max_rollout_len) -> Occupancy:
    G2, n = spec.max_grid_size ** 2, spec.max_n_objs
    S = G2 << n
    theta = np.asarray(theta, F32)
    assert theta.shape == (S + 1, 5), theta.shape
    L = int(max_rollout_len)
    H = max(0, min(int(params["max_steps_in_episode"][i]), L))
    rows_out = np.zeros((L, S))
    visits, collected, summ = np.zeros(S), np.zeros(n), np.zeros(8)
    d = np.zeros(S)
    if H == 0:
        return Occupancy(visits, rows_out, collected, summ, d)
    coll, r, p_term, (orow, oidx, op) = level_tables(spec, params, i)
    keep = np.clip(1.0 - p_term, 0.0, 1.0)
    invalid = invalid_states(spec, params, i)
    d[start_index(spec, params, i)] = 1.0
    ret = ret_abs = early = 0.0
    terms = np.zeros(3)
    for t in range(H):
        assert not d[invalid].any()
        rows_out[t] = d
        visits += d
        live = d > 0.0
        w = d[:, None] * prf.policy(theta, t)                       # [S, 5]: d pi
        w[~live] = 0.0
        ret += float((w * r).sum())
        ret_abs += float((w * np.abs(r)).sum())
        early += float((w * (1.0 - keep)).sum())
        collected += np.einsum("sa,sao->o", w, coll)
        tm = step_terms(theta, t)
        terms += (tm[:, live] * d[live]).sum(axis=1)
        d = np.bincount(oidx, weights=(w * keep).reshape(-1)[orow] * op, minlength=S)
    length = float(visits.sum())
    summ[:] = (ret, length, early, float(d.sum()), terms[0] / length / math.log(5), terms[1] / length,
               terms[2] / length, ret_abs)
    return Occupancy(visits, rows_out, collected, summ, d)
