"""numpy restatement of the level reachability statistics (toued_level_stats) and of the level editor's solvability
filter (LevelEditor(require_solvable=True)) -- the reference of tests/test_level_stats_cpu.py and
tests/test_gpu_level_stats.py.

Written from the definition (include/toued.h), one level at a time on the params dicts that
``level_edit_ref.unpack`` gives: R is the closure of {start} under ``oracle.gridworld.next_pos`` over the four moving
actions, found by a deque BFS over the level's transition table (next_pos of every cell below g^2, one call per
action); dist(c) is the BFS depth.  The start is in R whatever its wall bit says; a start >= g^2 stays alone.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import level_edit_ref as ler
import optret_ref as orf
from oracle import gridworld as ogw
from oracle import jaxrand as jr
from oracle import levels as olv

F32 = np.float32
WORDS = 16
CELLS, N_WALLS, N_REACH, ECC, N_OBJ_REACH, N_POS_REACH, NEAREST_POS, SOLVABLE, OBJ_DIST = range(9)
MAX_OBJS = 8


def _one(params, i, spec):
    """(stats int32 [16], dist int32 [G2]) of level i of a params dict."""
    G2 = spec.max_grid_size ** 2
    g = int(np.clip(params["grid_size"][i], 1, spec.max_grid_size))
    nobj = int(np.clip(params["n_objs"][i], 0, spec.max_n_objs))
    start = int(np.clip(params["start_pos"][i], 0, G2 - 1))
    g2 = g * g
    walls = np.asarray(params["walls"][i], bool)
    # the transition table of the cells below g^2: next_pos with the level's params, a batch of g^2 positions
    cells = np.arange(g2, dtype=np.int32)
    pb = {"grid_size": np.full(g2, g, np.int32), "walls": np.repeat(walls[None], g2, axis=0)}
    nxt = np.stack([ogw.next_pos(cells, np.full(g2, a, np.int32), pb) for a in range(4)], axis=1)
    dist = np.full(G2, -1, np.int32)
    reach = {start: 0}
    if start < g2:
        q = collections.deque([start])
        while q:
            p = q.popleft()
            for a in range(4):
                c = int(nxt[p, a])
                if c not in reach:
                    reach[c] = reach[p] + 1
                    q.append(c)
        for c, d in reach.items():
            dist[c] = d
    st = np.full(WORDS, -1, np.int32)
    st[CELLS] = g2
    st[N_WALLS] = int(walls[:g2].sum())
    st[N_REACH] = len(reach)
    st[ECC] = max(reach.values())
    st[N_OBJ_REACH] = st[N_POS_REACH] = 0
    if bool(params["random_respawn"][i]):
        return st, dist             # object cells are drawn per episode: NEAREST_POS, SOLVABLE and OBJ_DIST stay -1
    ids = np.asarray(params["obj_ids"][i], np.int64)
    rid = np.where(ids < 0, ids + spec.max_n_obj_types, ids)
    for o in range(nobj):
        c = int(params["static_obj_poss"][i][o])
        if not (0 <= c < g2 and c in reach):
            continue
        d = reach[c]
        st[OBJ_DIST + o] = d
        st[N_OBJ_REACH] += 1
        if F32(params["obj_rewards"][i][rid[o]]) > 0:
            st[N_POS_REACH] += 1
            st[NEAREST_POS] = d if st[NEAREST_POS] < 0 else min(st[NEAREST_POS], d)
    near = int(st[NEAREST_POS])
    st[SOLVABLE] = int(near >= 0 and max(near, 1) <= int(params["max_steps_in_episode"][i]))
    return st, dist


def level_stats(params, spec):
    """(stats int32 [n, 16], dist int32 [n, G2]) of a batched params dict."""
    n = len(params["start_pos"])
    out = [_one(params, i, spec) for i in range(n)]
    return (np.stack([o[0] for o in out]).astype(np.int32).reshape(n, WORDS),
            np.stack([o[1] for o in out]).astype(np.int32).reshape(n, spec.max_grid_size ** 2))


def level_stats_rows(rows, spec):
    """The same on packed rows int32 [n, 80]."""
    return level_stats(ler.unpack(rows, spec)[0], spec)


def edit_rows_filtered(buf_rows, parent_ids, keys, gen_rows, spec, p_edit, num_edits, mask, reward_delta):
    """LevelEditor(require_solvable=True) on packed rows: level_edit_ref.edit_rows, then every edited row whose child
    has SOLVABLE == 0 goes back to the generator's row (all 80 words).  Returns (rows, edited, rejected)."""
    rows, edited, _ = ler.edit_rows(buf_rows, parent_ids, keys, gen_rows, spec, p_edit, num_edits, mask, reward_delta)
    st, _ = level_stats_rows(rows, spec)
    rejected = edited & (st[:, SOLVABLE] == 0)
    rows = np.where(rejected[:, None], np.asarray(gen_rows, np.int32), rows)
    return rows, edited & ~rejected, rejected


# ---------------------------------------------------------------------------
# Shared cases
GEN_CASES = {"debug": 512, "all": 1024, "mazes": 256}        # generator levels of PRNGKey(GEN_SEED) per mode
GEN_SEED = 7
CHILD_CONFIG = (8, 1, 1.0)                                    # (num_edits, ops mask, p_edit): 8 wall-only edits


@functools.lru_cache(maxsize=None)
def gen_case(mode):
    """{"spec", "rows" int32 [n, 80], "stats", "dist"} of GEN_CASES[mode] generator levels."""
    spec = olv.env_spec(mode)
    n = GEN_CASES[mode]
    keys = jr.split(jr.PRNGKey(GEN_SEED), n)
    p, lt = olv.reset_env_params(keys, mode)
    rows = olv.pack_levels(p, lt, spec, buffer_id=np.arange(n))
    st, dist = level_stats_rows(rows, spec)
    return {"spec": spec, "rows": rows, "stats": st, "dist": dist}


@functools.lru_cache(maxsize=None)
def child_case(mode):
    """The ACCEL children of level_edit_ref.case(mode) at CHILD_CONFIG (``edited`` marks them among the case's rows)
    and their parents' stats."""
    c = ler.case(mode)
    rows, edited, _ = ler.case_reference(mode, *CHILD_CONFIG)
    st, dist = level_stats_rows(rows, c["spec"])
    pst, _ = level_stats_rows(c["buf_rows"], c["spec"])
    return {"spec": c["spec"], "rows": rows, "edited": edited, "stats": st, "dist": dist, "parent_stats": pst}


def _serpentine_walls():
    """13x13: the odd rows are walls but for one cell, at column 12 in rows 1, 5, 9 and at column 0 in rows 3, 7, 11."""
    w = []
    for r in range(1, 13, 2):
        gap = 12 if r % 4 == 1 else 0
        w += [13 * r + c for c in range(13) if c != gap]
    return w


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> (spec, params): the hand-built levels.  Their expected stats are written out in
    tests/test_level_stats_cpu.py (HAND_EXPECTED), not computed."""
    s13, s4 = olv.env_spec("mazes"), olv.env_spec("debug")
    mk = orf.make_params
    pt3, pr3 = [0.1, 0.2, 0.3], [0.5, 0.25, 0.125]
    pt2, pr2 = [0.1, 0.2], [0.5, 0.25]
    out = {}
    out["open13"] = (s13, mk(s13, 13, 0, [0, 1], [168, 12], [0.5, -0.5, 0.0], pt3, pr3, 50))
    out["enclosed"] = (s13, mk(s13, 13, 84, [0], [0], [1.0, 0.0, 0.0], pt3, pr3, 50, walls=[71, 97, 83, 85]))
    # cell 0 and cells 5, 6, 7 are walls: row 0's cells 1..3 touch the rest only where cell 3 wraps to cell 4
    out["wrap4_top"] = (s4, mk(s4, 4, 1, [0, 1], [8, 3], [1.0, 0.0], pt2, pr2, 10, walls=[0, 5, 6, 7]))
    out["wrap4_bottom"] = (s4, mk(s4, 4, 4, [0, 1], [8, 3], [1.0, 0.0], pt2, pr2, 1, walls=[0, 5, 6, 7]))
    sw = _serpentine_walls()
    out["serpentine_95"] = (s13, mk(s13, 13, 0, [0, 1], [168, 156], [0.9, -0.5, 0.0], pt3, pr3, 95, walls=sw))
    out["serpentine_96"] = (s13, mk(s13, 13, 0, [0, 1], [168, 156], [0.9, -0.5, 0.0], pt3, pr3, 96, walls=sw))
    # a 5x5 level in the 13x13 record: every wall bit from cell 25 up is set, and the centre cell 12
    out["beyond_g2"] = (s13, mk(s13, 5, 0, [0, 0, 0], [24, 30, 12], [0.5, 0.0, 0.0], pt3, pr3, 20,
                                walls=[12] + list(range(25, 169))))
    out["no_objs"] = (s4, mk(s4, 3, 4, [], [], [0.5, -0.5], pt2, pr2, 7, walls=[2]))
    p = mk(s13, 13, 0, [0, 1], [168, 12], [0.5, -0.5, 0.0], pt3, pr3, 50)
    p["random_respawn"] = np.array([True])
    out["randresp"] = (s13, p)
    # the start's own wall bit is set: the agent leaves it and cannot come back; object 1 lies on the start
    out["start_on_wall"] = (s4, mk(s4, 4, 5, [0, 1], [6, 5], [1.0, 0.5], pt2, pr2, 1, walls=[5]))
    out["start_on_wall_h0"] = (s4, mk(s4, 4, 5, [0, 1], [6, 5], [1.0, 0.5], pt2, pr2, 0, walls=[5]))
    return out


def hand_rows(name):
    spec, p = hand_cases()[name]
    return spec, olv.pack_levels(p, np.array([17], np.int32), spec, buffer_id=np.array([3]))


def malformed_rows(spec, n=16, seed=5):
    """Rows of arbitrary words (every field out of range somewhere): the kernel must hold them to the record."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2 ** 31, 2 ** 31, size=(n, olv.LEVEL_WORDS), dtype=np.int64).astype(np.int32)
    rows[: n // 2, olv.L_GRID] = rng.integers(-2, spec.max_grid_size + 3, n // 2)
    rows[: n // 2, olv.L_START] = rng.integers(-3, spec.max_grid_size ** 2 + 3, n // 2)
    rows[: n // 2, olv.L_NOBJS] = rng.integers(-1, 10, n // 2)
    rows[: n // 2, olv.L_RANDRESP] = 0
    rows[: n // 2, olv.L_STATIC:olv.L_STATIC + 8] = rng.integers(-2, spec.max_grid_size ** 2 + 2, (n // 2, 8))
    # the per-object rewards are the type table's, as in every packed row (the reference resolves them itself)
    ids = rng.integers(-1, spec.max_n_obj_types, (n, 8))
    rows[:, olv.L_OBJ_IDS:olv.L_OBJ_IDS + 8] = ids
    rid = np.where(ids < 0, ids + spec.max_n_obj_types, ids)
    rows[:, olv.L_REW:olv.L_REW + 8] = np.take_along_axis(rows[:, olv.L_TREW:olv.L_TREW + 5], rid, axis=1)
    return rows
