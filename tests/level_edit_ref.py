"""numpy restatement of the ACCEL level editor (toued_level_edit) and of its parent selection
(toued_plr_parent_ids) -- the reference of tests/test_level_edit_cpu.py and tests/test_gpu_level_edit.py.

Written from the semantics (include/toued.h), one level at a time on the params dicts of
``oracle.levels.reset_env_params`` (leading batch axis), on top of ``oracle.jaxrand`` and ``oracle.levels.pack_levels``.

Row j of a reset round, with the slot's generator key ``keys[j]``:
    ek = fold_in(keys[j], 0x45444954); ek_use, ek_edit = split(ek); use = bernoulli(ek_use, p_edit)
    use and parent_ids[j] >= 0: the row is edit(parent, ek_edit) with the row's own buffer id; else it is untouched.
``edit`` applies ``num_edits`` edits; each one draws, whatever it ends up doing,
    rng, k_op = split(rng); rng, k_cell = split(rng); rng, k_obj = split(rng); rng, k_val = split(rng)
    op = the randint(k_op, (), 0, n_enabled)-th enabled op (ascending bit order of the mask)
    c = randint(k_cell, (), 0, grid^2); o = randint(k_obj, (), 0, max(n_objs, 1)); dv = uniform(k_val, (), -d, d)
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import jaxrand as jr
from oracle import levels as olv

F32 = np.float32
OPS = ("walls", "objects", "start", "rewards")     # bit i of the ops mask
EDIT_FOLD = 0x45444954
INHERITED = ("max_steps_in_episode", "grid_size", "n_objs", "obj_ids", "obj_p_terminate", "obj_p_respawn",
             "random_respawn")


def ops_mask(names) -> int:
    return sum(1 << OPS.index(n) for n in names)


def take(params, i):
    """Level i of a batched params dict, as a batch of one (copied)."""
    return {k: np.array(v[i:i + 1]) for k, v in params.items()}


def concat(ps):
    return {k: np.concatenate([p[k] for p in ps]) for k in ps[0]}


def unpack(rows, spec):
    """Packed rows int32 [B, 80] -> (params dict, lifetime, buffer_id): the inverse of oracle.levels.pack_levels."""
    rows = np.ascontiguousarray(rows, np.int32)
    n, t, g2 = spec.max_n_objs, spec.max_n_obj_types, spec.max_grid_size ** 2
    bits = rows[:, olv.L_WALLS:olv.L_WALLS + 8].view(np.uint32)
    c = np.arange(g2)
    f = lambda off: rows[:, off:off + t].view(F32).copy()
    params = {
        "max_steps_in_episode": rows[:, olv.L_MAX_STEPS].copy(), "random_respawn": rows[:, olv.L_RANDRESP] != 0,
        "grid_size": rows[:, olv.L_GRID].copy(), "walls": ((bits[:, c // 32] >> (c % 32).astype(np.uint32)) & 1) != 0,
        "start_pos": rows[:, olv.L_START].copy(), "n_objs": rows[:, olv.L_NOBJS].copy(),
        "obj_ids": rows[:, olv.L_OBJ_IDS:olv.L_OBJ_IDS + n].copy(),
        "static_obj_poss": rows[:, olv.L_STATIC:olv.L_STATIC + n].copy(),
        "obj_rewards": f(olv.L_TREW), "obj_p_terminate": f(olv.L_TPTERM), "obj_p_respawn": f(olv.L_TPRESP),
    }
    return params, rows[:, olv.L_LIFETIME].copy(), rows[:, olv.L_BUFID].copy()


def edit(parent, key, num_edits, mask, reward_delta, spec):
    """``num_edits`` edits of a batch-of-one params dict with key uint32[2].  Returns (child, log) with log a list of
    (op name, applied, cell drawn) per edit; the parent is left unchanged."""
    p = {k: np.array(v) for k, v in parent.items()}
    enabled = [i for i in range(4) if (mask >> i) & 1]
    g2 = int(p["grid_size"][0]) ** 2
    n_objs = int(p["n_objs"][0])
    walls, cells, rew = p["walls"][0], p["static_obj_poss"][0], p["obj_rewards"][0]
    rng = np.asarray(key, np.uint32)
    log = []
    for _ in range(num_edits):
        rng, k_op = jr.split(rng)
        rng, k_cell = jr.split(rng)
        rng, k_obj = jr.split(rng)
        rng, k_val = jr.split(rng)
        op = OPS[enabled[int(jr.randint(k_op, (), 0, len(enabled)))]]
        c = int(jr.randint(k_cell, (), 0, g2))
        o = int(jr.randint(k_obj, (), 0, max(n_objs, 1)))
        dv = jr.uniform(k_val, (), -reward_delta, reward_delta)
        occupied = c == int(p["start_pos"][0]) or c in cells.tolist()
        applied = False
        if op == "walls":
            if not occupied:
                walls[c] = not walls[c]
                applied = True
        elif op == "objects":
            if n_objs > 0 and not walls[c] and not occupied:
                cells[o] = c
                applied = True
        elif op == "start":
            if not walls[c] and not occupied:
                p["start_pos"][0] = c
                applied = True
        elif n_objs > 0:
            t = int(p["obj_ids"][0, o])
            t = t + spec.max_n_obj_types if t < 0 else t
            v = F32(rew[t]) + F32(dv)
            rew[t] = np.clip(v, F32(0.0 if t == 0 else -1.0), F32(1.0))
            applied = True
        log.append((op, applied, c))
    return p, log


def edit_rows(buf_rows, parent_ids, keys, gen_rows, spec, p_edit, num_edits, mask, reward_delta):
    """The whole of toued_level_edit on packed rows: (rows int32 [n, 80], edited bool [n], logs).  ``buf_rows`` is the
    packed buffer, ``gen_rows`` the generator's rows of the reset slots; logs[j] is None for an untouched row."""
    buf_params, buf_lt, _ = unpack(buf_rows, spec)
    out = np.array(gen_rows, np.int32)
    edited = np.zeros(len(out), bool)
    logs = [None] * len(out)
    for j in range(len(out)):
        ek = jr.fold_in(np.asarray(keys[j], np.uint32), EDIT_FOLD)
        ek_use, ek_edit = jr.split(ek)
        use = bool(jr.bernoulli(ek_use, p_edit))
        pid = int(parent_ids[j])
        if not (use and pid >= 0):
            continue
        child, logs[j] = edit(take(buf_params, pid), ek_edit, num_edits, mask, reward_delta, spec)
        out[j] = olv.pack_levels(child, buf_lt[pid:pid + 1], spec, buffer_id=gen_rows[j, olv.L_BUFID])[0]
        out[j, olv.L_AUTOC] = buf_rows[pid, olv.L_AUTOC]
        edited[j] = True
    return out, edited, logs


def parent_ids(score, fresh, reset_ids):
    """parent_ids[j] = order[j % n_elig], order the stable argsort of where(eligible, -score, +inf) with
    eligible = not fresh and not among reset_ids; all -1 when nothing is eligible."""
    score = np.asarray(score, F32)
    elig = ~np.asarray(fresh, bool)
    elig[np.asarray(reset_ids, np.int64)] = False
    key = np.where(elig, -score, F32(np.inf)).astype(F32)
    key = np.where(key == 0, F32(0.0), key)          # jax's sort puts -0 and +0 together; ties go by index
    order = np.argsort(key, kind="stable")
    n_elig = int(elig.sum())
    j = np.arange(len(reset_ids))
    return (order[j % n_elig] if n_elig else np.full(len(j), -1)).astype(np.int32)


# ---------------------------------------------------------------------------
# The kernel test's cases, shared with the CPU test (which asserts that they cover what they are meant to).
CASE_MODES = ("debug", "all", "mazes")
CASE_N, CASE_B = 65, 24
CASE_SEED = {"debug": 301, "all": 302, "mazes": 303}
REWARD_DELTA = 0.1
CASE_EDITS = (0, 1, 8)
CASE_MASKS = (1, 2, 4, 8, 15)
# (num_edits, mask, p_edit): every edit count with each op alone and with all four at p_edit = 1, then the coin
CASE_CONFIGS = tuple((e, m, 1.0) for e in CASE_EDITS for m in CASE_MASKS) + ((8, 15, 0.5), (1, 15, 0.5), (8, 15, 0.0))


@functools.lru_cache(maxsize=None)
def case(mode):
    """A buffer of CASE_B generator levels and CASE_N reset slots (generator keys and rows, buffer ids 100 + j) of
    ``mode``; slot j's parent is j % CASE_B, and -1 for j % 7 == 3."""
    spec = olv.env_spec(mode)
    bk = jr.split(jr.PRNGKey(CASE_SEED[mode]), CASE_B)
    bp, blt = olv.reset_env_params(bk, mode)
    buf_rows = olv.pack_levels(bp, blt, spec, buffer_id=np.arange(CASE_B))
    keys = jr.split(jr.PRNGKey(CASE_SEED[mode] + 1000), CASE_N)
    gp, glt = olv.reset_env_params(keys, mode)
    gen_rows = olv.pack_levels(gp, glt, spec, buffer_id=100 + np.arange(CASE_N))
    j = np.arange(CASE_N)
    pids = np.where(j % 7 == 3, -1, j % CASE_B).astype(np.int32)
    return {"spec": spec, "buf_rows": buf_rows, "keys": keys, "gen_rows": gen_rows, "parent_ids": pids}


@functools.lru_cache(maxsize=None)
def case_reference(mode, num_edits, mask, p_edit):
    """edit_rows of the case's CASE_N slots (a row does not depend on the rows beside it, so the first n rows are the
    reference of a launch with n rows)."""
    c = case(mode)
    return edit_rows(c["buf_rows"], c["parent_ids"], c["keys"], c["gen_rows"], c["spec"], p_edit, num_edits, mask,
                     REWARD_DELTA)


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """Hand-built one-level buffers with 8 reset slots each (p_edit 1, 8 edits, all four ops).
    ``full``: a 2x2 grid in the mazes kwargs whose four cells are the start and the three objects, so no structural
    edit can apply.  ``no_objs``: a debug-kwargs level without objects (the objects and rewards ops never apply)."""
    import optret_ref as orf
    if name == "full":
        spec = olv.env_spec("mazes")
        p = orf.make_params(spec, grid_size=2, start_pos=3, obj_ids=[0, 1, 2], static_obj_poss=[0, 1, 2],
                            obj_rewards=[0.95, -0.95, 0.5], obj_p_terminate=[0.1, 0.2, 0.3],
                            obj_p_respawn=[0.5, 0.25, 0.125], max_steps=9)
    elif name == "no_objs":
        spec = olv.env_spec("debug")
        p = orf.make_params(spec, grid_size=3, start_pos=4, obj_ids=[], static_obj_poss=[], obj_rewards=[0.5, -0.5],
                            obj_p_terminate=[0.1, 0.2], obj_p_respawn=[0.5, 0.25], max_steps=7, walls=[2])
    else:
        raise KeyError(name)
    buf_rows = olv.pack_levels(p, np.array([17], np.int32), spec, buffer_id=np.array([0]))
    n = 8
    keys = jr.split(jr.PRNGKey(411 if name == "full" else 412), n)
    gen_rows = np.repeat(buf_rows, n, axis=0)
    gen_rows[:, olv.L_BUFID] = 50 + np.arange(n)
    gen_rows[:, olv.L_MAX_STEPS] = 1000 + np.arange(n)          # rows that differ from any child
    c = {"spec": spec, "buf_rows": buf_rows, "keys": keys, "gen_rows": gen_rows,
         "parent_ids": np.zeros(n, np.int32)}
    c["ref"] = edit_rows(buf_rows, c["parent_ids"], keys, gen_rows, spec, 1.0, 8, 15, REWARD_DELTA)
    return c
