"""float64 numpy restatement of GridWorld.optimal_return (environments/gridworld/gridworld.py:253-323) — the
reference of tests/test_optret_cpu.py and tests/test_gpu_optret.py.

A direct restatement: the scan over ``flip(arange(max_rollout_len))`` from ``zeros(S)``, every step computing the
value of ALL S = max_grid^2 * 2^max_n_objs states (invalid ones included, then set to -inf) and masking the row with
``where(time < max_steps_in_episode, v, 0)``; no horizon shortcut.  Vectorised over (state, action, next existence
state).  The quantities that do not depend on time (next cell, collected objects, reward, p_term, the next-state
probabilities) are formed once; the p > 0 outcomes are kept as a list, the others being exact zeros of the
reference's ``dot(p, where(p > 0, v_t1[idx], 0))``.

Levels are the params dicts of ``oracle.levels.reset_env_params`` (leading batch axis); ``make_params`` builds one by
hand in the same form, so both go through ``oracle.levels.pack_levels`` for the device.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def make_params(spec, grid_size, start_pos, obj_ids, static_obj_poss, obj_rewards, obj_p_terminate, obj_p_respawn,
                max_steps, walls=()):
    """A hand-built level as a batch-of-one params dict.  obj_ids lists the level's objects (n_objs = len); the
    per-type tables are padded with zeros to max_n_obj_types, the per-object arrays with -1 / 0 to max_n_objs."""
    n, t, g2 = spec.max_n_objs, spec.max_n_obj_types, spec.max_grid_size ** 2
    k = len(obj_ids)
    pad_t = lambda v: np.array([list(v) + [0.0] * (t - len(v))], F32)
    w = np.zeros((1, g2), bool)
    w[0, list(walls)] = True
    return {
        "max_steps_in_episode": np.array([max_steps], np.int32), "random_respawn": np.array([False]),
        "grid_size": np.array([grid_size], np.int32), "walls": w, "start_pos": np.array([start_pos], np.int32),
        "n_objs": np.array([k], np.int32), "obj_ids": np.array([list(obj_ids) + [-1] * (n - k)], np.int32),
        "static_obj_poss": np.array([list(static_obj_poss) + [0] * (n - k)], np.int32),
        "obj_rewards": pad_t(obj_rewards), "obj_p_terminate": pad_t(obj_p_terminate),
        "obj_p_respawn": pad_t(obj_p_respawn), "sub_mode": np.zeros(1, np.int32),
    }


def concat_params(ps):
    return {k: np.concatenate([p[k] for p in ps]) for k in ps[0]}


def _next_pos(pos, action, g, walls):
    """_get_next_pos (gridworld.py:138-146) on arrays; walls[next_pos] with jax's clamped gather."""
    top, bottom = pos < g, pos >= g * (g - 1)
    left, right = pos % g == 0, pos % g == g - 1
    step = ((action == 0) * (1 - top) * -g + (action == 1) * (1 - bottom) * g + (action == 2) * (1 - left) * -1
            + (action == 3) * (1 - right) * 1)
    nxt = pos + step
    return np.where(walls[np.clip(nxt, 0, walls.shape[0] - 1)], pos, nxt)


def invalid_states(spec, params, i):
    """bool [S]: position out of the grid or on a wall, or an unused object present (gridworld.py:299-302)."""
    G2, n = spec.max_grid_size ** 2, spec.max_n_objs
    s = np.arange(G2 << n)
    pos, k = s % G2, s // G2
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    return (pos >= g * g) | params["walls"][i][pos] | ((k >> nobj) != 0)


def start_index(spec, params, i):
    nobj = int(params["n_objs"][i])
    return int(params["start_pos"][i]) + spec.max_grid_size ** 2 * ((1 << nobj) - 1)


def optimal_return_all(spec, params, i, max_rollout_len):
    """return_all=True of level i: float64 [max_rollout_len, S], row t = v_t (the reference's output after its flip)."""
    G2, n, NE = spec.max_grid_size ** 2, spec.max_n_objs, 1 << spec.max_n_objs
    S = G2 * NE
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    walls = np.asarray(params["walls"][i], bool)
    static = np.asarray(params["static_obj_poss"][i], np.int64)
    ids = np.asarray(params["obj_ids"][i], np.int64)           # jnp.take wraps a -1 id to the last type
    rew = np.asarray(params["obj_rewards"][i], np.float64)[ids]
    pterm = np.asarray(params["obj_p_terminate"][i], np.float64)[ids]
    presp = np.asarray(params["obj_p_respawn"][i], np.float64)[ids]
    max_steps = int(params["max_steps_in_episode"][i])

    s = np.arange(S)
    pos = (s % G2)[:, None]                                     # [S, 1]
    ex = (((s // G2)[:, None] >> np.arange(n)) & 1) == 1         # [S, n]  obj_existss_t
    pos1 = _next_pos(pos, np.arange(5)[None, :], g, walls)       # [S, 5]
    coll = ex[:, None, :] & (static[None, None, :] == pos1[:, :, None])   # [S, 5, n]
    r = coll @ rew                                              # [S, 5]
    p_term = coll @ pterm
    nxt_ex = ((np.arange(NE)[:, None] >> np.arange(n)) & 1) == 1  # [NE, n]  obj_exist_states (column i = bit i)
    p_next = np.ones((S, 5, NE))
    for o in range(n):
        x = nxt_ex[None, None, :, o]
        absent_p = np.where(x, presp[o], 1.0 - presp[o])
        p_next *= np.where(o >= nobj, 1.0 - x,
                           np.where(coll[:, :, None, o], 1.0 - x, np.where(ex[:, None, None, o], 1.0 * x, absent_p)))
    tab = np.clip(pos1[:, :, None] + G2 * np.arange(NE)[None, None, :], 0, S - 1)    # _get_tabular_pos
    nz = p_next > 0.0
    rows = np.broadcast_to(np.arange(S * 5).reshape(S, 5, 1), nz.shape)[nz]
    idx, pnz = tab[nz], p_next[nz]
    invalid = invalid_states(spec, params, i)

    out = np.zeros((max_rollout_len, S))
    v_t1 = np.zeros(S)
    with np.errstate(invalid="ignore"):
        for time in range(max_rollout_len - 1, -1, -1):
            ev = np.bincount(rows, weights=pnz * v_t1[idx], minlength=S * 5).reshape(S, 5)
            q = r + ev * (1.0 - p_term)
            v = np.where(invalid, -np.inf, q.max(axis=1))
            v = np.where(time < max_steps, v, 0.0)
            out[time] = v
            v_t1 = v
    return out


def optimal_return(spec, params, i, max_rollout_len):
    """return_all=False: v_0 at the start state (zeros(S)[start] = 0 for an empty scan)."""
    if max_rollout_len == 0:
        return 0.0
    return float(optimal_return_all(spec, params, i, max_rollout_len)[0, start_index(spec, params, i)])
