"""float64 numpy restatement of the mean and variance of a tabular agent's first-episode return
(RolloutWrapper.policy_return_moments) — the reference of tests/test_polvar_cpu.py and tests/test_gpu_polvar.py.

tests/polret_ref.py's recursion with a second table.  With H = min(max_steps_in_episode, max_rollout_len),
v_H = u_H = 0, t = H-1 .. 0, c(s, a) = 1 - p_term(s, a) and
E[f](s, a) = sum_R P[absent][R] * f_{t+1}(pos1, (e \\ coll) | R) over the p > 0 outcomes,

    q(s, a) = r + c * E[v]
    w(s, a) = r^2 + c * (2 r E[v] + E[v^2])                  (the second moment of r + cont * v')
    v_t(s)  = sum_a pi_t(a|s) * q(s, a)                      (polret_ref's, with its pi_t)
    u_t(s)  = sum_a pi_t(a|s) * (c * E[u] + w(s, a)) - v_t(s)^2

u_t(s) = Var[G_t | s] by the law of total variance: given (s, a) the return is r + cont * G' with cont a
Bernoulli(c) draw and G' the return from the drawn next state, whose second moment given that state is u' + v'^2.
The formulas are taken literally where c < 0 (two collected objects whose p_terminate sum past 1), as q is, and nothing
is clamped: a zero variance may come out a rounding below zero.  Invalid states hold -inf in both tables and the rows
t >= max_steps are zero, as in polret_ref.policy_return_all.
"""
from __future__ import annotations

import numpy as np

from optret_ref import _next_pos, invalid_states, start_index
from polret_ref import F32, policy


def moments_all(spec, params, i, theta, max_rollout_len):
    """(v, u), float64 [max_rollout_len, S] each: row t = v_t and u_t under the policy of ``theta``."""
    G2, n, NE = spec.max_grid_size ** 2, spec.max_n_objs, 1 << spec.max_n_objs
    S = G2 * NE
    theta = np.asarray(theta, F32)
    assert theta.shape == (S + 1, 5), theta.shape
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    walls = np.asarray(params["walls"][i], bool)
    static = np.asarray(params["static_obj_poss"][i], np.int64)
    ids = np.asarray(params["obj_ids"][i], np.int64)           # jnp.take wraps a -1 id to the last type
    rew = np.asarray(params["obj_rewards"][i], np.float64)[ids]
    pterm = np.asarray(params["obj_p_terminate"][i], np.float64)[ids]
    presp = np.asarray(params["obj_p_respawn"][i], np.float64)[ids]
    max_steps = int(params["max_steps_in_episode"][i])

    s = np.arange(S)
    pos = (s % G2)[:, None]
    ex = (((s // G2)[:, None] >> np.arange(n)) & 1) == 1
    pos1 = _next_pos(pos, np.arange(5)[None, :], g, walls)
    coll = ex[:, None, :] & (static[None, None, :] == pos1[:, :, None])
    r = coll @ rew
    c = 1.0 - coll @ pterm
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
    idx, pnz = tab[nz], p_next[nz]
    invalid = invalid_states(spec, params, i)
    expect = lambda f: np.bincount(rows, weights=pnz * f[idx], minlength=S * 5).reshape(S, 5)

    out_v, out_u = np.zeros((max_rollout_len, S)), np.zeros((max_rollout_len, S))
    v_t1, u_t1 = np.zeros(S), np.zeros(S)
    with np.errstate(invalid="ignore"):
        for time in range(max_rollout_len - 1, -1, -1):
            if time >= max_steps:
                continue                                        # the rows stay 0
            ev, ev2, eu = expect(v_t1), expect(v_t1 * v_t1), expect(u_t1)
            q = r + c * ev
            w = r * r + c * (2.0 * r * ev + ev2)
            pi = policy(theta, time)
            v = (pi * q).sum(axis=1)
            u = (pi * (c * eu + w)).sum(axis=1) - v * v
            v_t1 = out_v[time] = np.where(invalid, -np.inf, v)
            u_t1 = out_u[time] = np.where(invalid, -np.inf, u)
    return out_v, out_u


def moments(spec, params, i, theta, max_rollout_len):
    """(v_0, u_0) at the start state ((0, 0) for max_rollout_len == 0)."""
    if max_rollout_len == 0:
        return 0.0, 0.0
    v, u = moments_all(spec, params, i, theta, max_rollout_len)
    si = start_index(spec, params, i)
    return float(v[0, si]), float(u[0, si])


def variance_tolerance(returns, rewards):
    """The bound on |s^2 - exact variance| of M sampled returns of one level: 5 standard errors of the sample
    variance, sqrt((m4 - s^4) / M) with m4 the sample's fourth central moment, plus 8 R^2 / M with R the level's largest
    |obj_rewards| for the levels whose reward events are rarer than 1 / M (polret_ref.mc_tolerance's second term,
    for a squared quantity).  Returns (s^2, bound)."""
    x = np.asarray(returns, np.float64)
    M = x.shape[0]
    d = x - x.mean()
    s2 = float((d * d).sum() / (M - 1))
    m4 = float((d ** 4).mean())
    R = float(np.abs(rewards).max())
    return s2, 5.0 * np.sqrt(max(m4 - s2 * s2, 0.0) / M) + 8.0 * R * R / M
