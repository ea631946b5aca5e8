"""float64 numpy restatement of the exact policy return of a tabular agent (RolloutWrapper.policy_return) — the
reference of tests/test_polret_cpu.py and tests/test_gpu_polret.py.

tests/optret_ref.py's recursion with ``sum_a pi_t(a|s) q_t(s, a)`` in place of ``max_a q_t(s, a)``: with v_H = 0 and
t = H-1 .. 0 (H = min(max_steps_in_episode, max_rollout_len)),

    l_a      = fl32(theta[s][a] + fl32(fl32(f32(t) * 0.001f) * theta[D-1][a]))     (the rollouts' logits)
    pi_t(a|s) = exp(l_a - m) / sum_a' exp(l_a' - m),  m = max_a l_a                (float64, from the f32 logits)
    q_t(s, a) = r(s, a) + (1 - p_term(s, a)) * sum_R P[absent][R] * v_{t+1}(pos1, (e \\ c) | R)
    v_t(s)   = sum_a pi_t(a|s) * q_t(s, a)

over all S = max_grid^2 * 2^max_n_objs states, the invalid ones then set to -inf and the rows t >= max_steps to 0, as
optret_ref.optimal_return_all does.  theta is the agent's actor table f32 [D, 5], D = S + 1.
"""
from __future__ import annotations

import numpy as np

from optret_ref import _next_pos, invalid_states, start_index

F32 = np.float32
TIME_SCALE = F32(0.001)


def policy(theta, t):
    """float64 [S, 5]: pi_t(.|s) of every table state."""
    theta = np.asarray(theta, F32)
    c = F32(F32(t) * TIME_SCALE)
    logits = (theta[:-1] + (c * theta[-1]).astype(F32)[None, :]).astype(F32)
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def policy_return_all(spec, params, i, theta, max_rollout_len):
    """float64 [max_rollout_len, S], row t = v_t under the policy of ``theta``."""
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
    idx, pnz = tab[nz], p_next[nz]
    invalid = invalid_states(spec, params, i)

    out = np.zeros((max_rollout_len, S))
    v_t1 = np.zeros(S)
    with np.errstate(invalid="ignore"):
        for time in range(max_rollout_len - 1, -1, -1):
            if time >= max_steps:
                continue                                        # where(time < max_steps, v, 0): the row stays 0
            ev = np.bincount(rows, weights=pnz * v_t1[idx], minlength=S * 5).reshape(S, 5)
            q = r + ev * (1.0 - p_term)
            v = np.where(invalid, -np.inf, (policy(theta, time) * q).sum(axis=1))
            out[time] = v
            v_t1 = v
    return out


def random_tables(seed, n, D):
    """n actor tables f32 [n, D, 5]: N(0, 2^2) entries, the time-feature row scaled by 30 (the time feature is at
    most 0.001 * max_steps, so its row needs large weights to move the policy over an episode)."""
    th = np.random.default_rng(seed).normal(0.0, 2.0, (n, D, 5)).astype(F32)
    th[:, -1] *= F32(30.0)
    return th


def mc_tolerance(returns, rewards):
    """The bound on |mean - exact| of M sampled returns of one level: 5 standard errors, plus 8 R / M with R the
    level's largest |obj_rewards| for the levels whose reward events are rarer than 1 / M, where the sample standard
    deviation underestimates the spread."""
    M = returns.shape[0]
    s = float(np.std(returns.astype(np.float64), ddof=1))
    return 5.0 * s / np.sqrt(M) + 8.0 * float(np.abs(rewards).max()) / M


def policy_return(spec, params, i, theta, max_rollout_len):
    """v_0 at the start state (0 for max_rollout_len == 0)."""
    if max_rollout_len == 0:
        return 0.0
    return float(policy_return_all(spec, params, i, theta, max_rollout_len)[0, start_index(spec, params, i)])
