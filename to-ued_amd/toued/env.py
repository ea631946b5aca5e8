"""GridWorld on MI355X: level generation and the gymnax env API over the C ABI.

Mirrors environments/gridworld/gridworld.py (GridWorld: reset/step),
environments/environments.py:22-63 (get_env / reset_env_params / get_env_spec /
get_agent_hypers) and configs.py's mode tables — batched ("vmapped") over
levels/workers, with all state resident on the GPU.

Levels are packed int32[n, 80] tensors (include/toued.h); env state is
int32[12, n] SoA; observations are compact (tab_idx, time) int32 pairs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _lib
from . import modes as M

STATE_FIELDS = 12
LEVEL_WORDS = 80
# packed-level word offsets (csrc/common.h)
L_MAX_STEPS, L_GRID, L_START, L_NOBJS, L_RANDRESP, L_LIFETIME, L_BUFID = 0, 1, 2, 3, 4, 5, 6
L_OBJ_IDS, L_STATIC, L_REW, L_PTERM, L_PRESP, L_WALLS = 8, 16, 24, 32, 40, 48
L_TREW, L_TPTERM, L_TPRESP, L_AUTOC = 64, 69, 74, 79


def unpack_levels(levels, spec: "EnvSpec"):
    """Packed rows [B, 80] -> the reference's Level pytree fields (util/data.py:46-51; EnvParams
    gridworld.py:21-35) as numpy arrays: ({EnvParams field: array}, lifetime, buffer_id)."""
    import numpy as np
    lv = np.ascontiguousarray(levels.detach().cpu().numpy() if torch.is_tensor(levels) else levels, np.int32)
    n, t, g2 = spec.max_n_objs, spec.max_n_obj_types, spec.g2
    bits = lv[:, L_WALLS:L_WALLS + 8].view(np.uint32)
    cells = np.arange(g2)
    walls = ((bits[:, cells // 32] >> (cells % 32).astype(np.uint32)) & 1).astype(bool)
    f = lambda off: lv[:, off:off + t].view(np.float32).copy()
    params = {
        "max_steps_in_episode": lv[:, L_MAX_STEPS].copy(), "random_respawn": lv[:, L_RANDRESP].astype(bool),
        "auto_collect": lv[:, L_AUTOC].astype(bool), "grid_size": lv[:, L_GRID].copy(), "walls": walls,
        "start_pos": lv[:, L_START].copy(), "n_objs": lv[:, L_NOBJS].copy(),
        "obj_ids": lv[:, L_OBJ_IDS:L_OBJ_IDS + n].copy(), "static_obj_poss": lv[:, L_STATIC:L_STATIC + n].copy(),
        "obj_rewards": f(L_TREW), "obj_p_terminate": f(L_TPTERM), "obj_p_respawn": f(L_TPRESP),
    }
    return params, lv[:, L_LIFETIME].copy(), lv[:, L_BUFID].copy()


def pack_levels(params: dict, lifetime, buffer_id, spec: "EnvSpec"):
    """Inverse of unpack_levels: the packed rows (with the per-object tables resolved through obj_ids, a -1 id
    taking the last type as jnp.take does, gridworld.py:87,115,122) as an int32 numpy array [B, 80]."""
    import numpy as np
    B = np.asarray(params["start_pos"]).shape[0]
    n, t = spec.max_n_objs, spec.max_n_obj_types
    out = np.zeros((B, LEVEL_WORDS), np.int32)
    out[:, L_MAX_STEPS] = params["max_steps_in_episode"]
    out[:, L_GRID] = params["grid_size"]
    out[:, L_START] = params["start_pos"]
    out[:, L_NOBJS] = params["n_objs"]
    out[:, L_RANDRESP] = np.asarray(params["random_respawn"]).astype(np.int32)
    out[:, L_LIFETIME] = lifetime
    out[:, L_BUFID] = buffer_id
    ids = np.asarray(params["obj_ids"], np.int32)
    out[:, L_OBJ_IDS:L_OBJ_IDS + n] = ids
    out[:, L_STATIC:L_STATIC + n] = params["static_obj_poss"]
    rid = np.where(ids < 0, ids + t, ids)
    for off, toff, name in ((L_REW, L_TREW, "obj_rewards"), (L_PTERM, L_TPTERM, "obj_p_terminate"),
                            (L_PRESP, L_TPRESP, "obj_p_respawn")):
        tab = np.asarray(params[name], np.float32)
        out[:, off:off + n] = np.take_along_axis(tab, rid, axis=1).view(np.int32)
        out[:, toff:toff + t] = tab.view(np.int32)
    walls = np.asarray(params["walls"], bool)
    for c in range(walls.shape[1]):
        out[:, L_WALLS + c // 32] |= (walls[:, c].astype(np.int64) << (c % 32)).astype(np.uint32).view(np.int32)
    out[:, L_AUTOC] = np.asarray(params.get("auto_collect", True)).astype(np.int32)
    return out


@dataclass(frozen=True)
class EnvSpec:
    """Static env kwargs (configs.py:430-544)."""
    max_grid_size: int
    max_n_objs: int
    max_n_obj_types: int
    tabular: bool

    @property
    def g2(self) -> int:
        return self.max_grid_size ** 2

    @property
    def obs_dim(self) -> int:
        # gridworld.py:230-235
        if self.tabular:
            return self.g2 * (2 ** self.max_n_objs) + 1
        return self.g2 * (self.max_n_obj_types + 1) + 1

    @property
    def num_actions(self) -> int:
        return 5  # gridworld.py:218-222


def get_env_spec(env_mode: str):
    """environments.py:40-55: (env spec, max_rollout_len, max_lifetime)."""
    if env_mode not in M.ENV_MODE_KWARGS:
        raise ValueError(f"Environment mode {env_mode} has no get env spec method.")
    k = M.ENV_MODE_KWARGS[env_mode]
    spec = EnvSpec(k["max_grid_size"], k["max_n_objs"], k["max_n_obj_types"], k["tabular"])
    return spec, M.ENV_MODE_EPISODE_LEN[env_mode], M.ENV_MODE_LIFETIME_MAX[env_mode]


def get_agent_hypers(env_mode: str) -> dict:
    """environments.py:58-63 / configs.py:652-707."""
    if env_mode not in M.MODE_AGENT_HYPERS:
        raise ValueError(f"Environment mode {env_mode} has no get agent hyperparameters method.")
    return dict(M.MODE_AGENT_HYPERS[env_mode])


def _dev(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


class LevelGenerator:
    """Device ``reset_env_params`` (environments.py:22-37) for one env mode."""

    def __init__(self, env_mode: str, device=None):
        if env_mode not in M.ENV_MODE_PARAMS:
            raise ValueError(f"Environment mode {env_mode} not registered.")
        self.env_mode = env_mode
        self.spec, _, _ = get_env_spec(env_mode)
        prog = M.mode_program(env_mode)
        nbytes = int(_lib.lib().toued_mode_program_bytes())
        if prog.nbytes != nbytes:
            raise _lib.ToUEDError(f"ModeProgram size mismatch: host {prog.nbytes} vs device {nbytes}")
        self.program = torch.from_numpy(prog).to(_dev(device))

    def __call__(self, keys: torch.Tensor, buffer_ids: torch.Tensor | None = None, with_sub_mode=False):
        """keys int32[n,2] (threefry) -> levels int32[n, LEVEL_WORDS = 80] (lifetime and buffer_id packed in)."""
        n = keys.shape[0]
        levels = torch.empty((n, LEVEL_WORDS), dtype=torch.int32, device=keys.device)
        sub = torch.empty((n,), dtype=torch.int32, device=keys.device) if with_sub_mode else None
        if buffer_ids is not None:
            buffer_ids = buffer_ids.to(torch.int32).contiguous()
        _lib.call("toued_level_gen", _lib.ptr(self.program), _lib.ptr(keys.contiguous()), _lib.ptr(buffer_ids),
                  _lib.ptr(levels), _lib.ptr(sub), n, _lib.stream_ptr())
        return (levels, sub) if with_sub_mode else levels

    def regenerate(self, keys: torch.Tensor, levels: torch.Tensor, mask: torch.Tensor):
        """``levels[i] = self(keys)[i]`` in place for the i with ``mask[i]`` (u8) set (buffer_id 0)."""
        _lib.call("toued_level_gen_masked", _lib.ptr(self.program), _lib.ptr(keys.contiguous()), None,
                  _lib.ptr(levels), keys.shape[0], _lib.ptr(mask), _lib.stream_ptr())
        return levels


EDIT_OPS = ("walls", "objects", "start", "rewards")     # bit i of toued_level_edit's ops_mask


def parse_edit_ops(ops) -> int:
    """A comma list (or sequence) of EDIT_OPS names -> toued_level_edit's ops_mask; ValueError for an unknown name
    or an empty list."""
    names = [o.strip() for o in ops.split(",")] if isinstance(ops, str) else list(ops)
    names = [o for o in names if o]
    if not names:
        raise ValueError(f"edit_ops is empty: give a comma list of {EDIT_OPS}")
    mask = 0
    for o in names:
        if o not in EDIT_OPS:
            raise ValueError(f"edit_ops: unknown op {o!r} (known: {EDIT_OPS})")
        mask |= 1 << EDIT_OPS.index(o)
    return mask


LSTAT_WORDS = 16      # include/toued.h TOUED_LSTAT_*
LSTAT_CELLS, LSTAT_N_WALLS, LSTAT_N_REACH, LSTAT_ECC, LSTAT_N_OBJ_REACH, LSTAT_N_POS_REACH = 0, 1, 2, 3, 4, 5
LSTAT_NEAREST_POS, LSTAT_SOLVABLE, LSTAT_OBJ_DIST = 6, 7, 8


class LevelStats(NamedTuple):
    """Reachability statistics of n levels (toued_level_stats), int32 [n] each (0-d for a single level):
    ``cells`` g^2, ``n_walls`` inside the grid, ``n_reach`` cells the agent can stand on, ``ecc`` the farthest of
    them in moves from the start, ``n_obj_reach`` / ``n_pos_reach`` the objects / positive-reward objects among them,
    ``nearest_pos`` the moves to the nearest positive reward (-1: none), ``solvable`` (1, 0, or -1 for a level with
    random respawn, whose object cells are drawn per episode), ``obj_dist`` [n, max_n_objs] the moves to each object
    (-1: unused or unreachable) and ``dist`` [n, G^2] the whole distance map (-1: wall, unreachable or outside the
    grid), or None."""
    cells: torch.Tensor
    n_walls: torch.Tensor
    n_reach: torch.Tensor
    ecc: torch.Tensor
    n_obj_reach: torch.Tensor
    n_pos_reach: torch.Tensor
    nearest_pos: torch.Tensor
    solvable: torch.Tensor
    obj_dist: torch.Tensor
    dist: torch.Tensor | None


def level_stats_raw(levels: torch.Tensor, spec: EnvSpec, dist: torch.Tensor | None = None) -> torch.Tensor:
    """toued_level_stats on ``levels`` int32 [n, 80] on the current stream: the stats words int32 [n, 16];
    ``dist`` (int32 [n, G^2], optional) receives the distance maps."""
    n = levels.shape[0]
    stats = torch.empty((n, LSTAT_WORDS), dtype=torch.int32, device=levels.device)
    _lib.call("toued_level_stats", _lib.ptr(levels), n, spec.max_grid_size, spec.max_n_objs, _lib.ptr(stats),
              _lib.ptr(dist), _lib.stream_ptr())
    return stats


def level_stats(levels: torch.Tensor, spec: EnvSpec, return_dist: bool = False) -> LevelStats:
    """Which cells of each level the agent can reach from its start, how far they are, and whether a positive reward
    lies within ``max_steps_in_episode`` moves (toued_level_stats; one launch on the current stream, no host
    synchronisation): ACCEL's complexity metrics and the share of solvable levels.  ``levels`` int32 [n, 80] or a
    single [80] row; every env mode, tabular or not.  Not in the reference."""
    single = levels.dim() == 1
    lv = (levels.view(1, -1) if single else levels).contiguous()
    if lv.dim() != 2 or lv.shape[1] != LEVEL_WORDS or lv.dtype != torch.int32:
        raise ValueError(f"level_stats: levels must be int32 [n, {LEVEL_WORDS}] or [{LEVEL_WORDS}] "
                         f"(got {lv.dtype} {tuple(levels.shape)})")
    dist = torch.empty((lv.shape[0], spec.g2), dtype=torch.int32, device=lv.device) if return_dist else None
    st = level_stats_raw(lv, spec, dist)
    cols = [st[:, i] for i in range(LSTAT_OBJ_DIST)] + [st[:, LSTAT_OBJ_DIST:LSTAT_OBJ_DIST + spec.max_n_objs], dist]
    if single:
        cols = [None if c is None else c[0] for c in cols]
    return LevelStats(*cols)


ELIGIBLE_MODES = ("all", "others", "lower")      # toued_level_nearest's eligible: 0, 1, 2
LEVEL_DIST_MAX = 302                             # 46 words that differ + 256 wall bits


class LevelNearest(NamedTuple):
    """For each of n query levels, over the corpus entries eligible for it (toued_level_nearest), int32 [n] each (0-d
    for a single query): ``dist`` the least level distance (2^31 - 1 when nothing is eligible), ``idx`` the lowest
    corpus index that attains it (-1), ``dist_sum`` the sum of the distances and ``count`` the number of entries."""
    dist: torch.Tensor
    idx: torch.Tensor
    dist_sum: torch.Tensor
    count: torch.Tensor


def level_nearest(queries: torch.Tensor, corpus: torch.Tensor, corpus_mask: torch.Tensor | None = None,
                  eligible: str = "all", include_lifetime: bool = True) -> LevelNearest:
    """The nearest of the ``corpus`` levels int32 [b, 80] (b <= 65536) to each of the ``queries`` int32 [n, 80] or
    [80] (toued_level_nearest; one call on the current stream, no host synchronisation).  The distance is between the
    levels' canonical records -- the 54 words the env and the agent's lifetime read: the six scalars, the five fields
    of the object slots below n_objs and the wall bits of the cells inside the grid; not the buffer id or the per-type
    tables -- the wall bits that differ plus the other words that differ (floats by bit pattern), an integer in
    [0, 302] that is 0 exactly for equal records.  ``include_lifetime=False`` leaves the lifetime out.
    ``corpus_mask`` (bool or uint8 [b]) keeps the entries where it is set; ``eligible``: "all", "others" (every entry
    but the one with the query's own index) or "lower" (only the entries with a lower index than the query's).
    Not in the reference."""
    if eligible not in ELIGIBLE_MODES:
        raise ValueError(f"level_nearest: eligible {eligible!r} not in {ELIGIBLE_MODES}")
    single = queries.dim() == 1
    q = (queries.view(1, -1) if single else queries).contiguous()
    c = corpus.contiguous()
    for name, x in (("queries", q), ("corpus", c)):
        if x.dim() != 2 or x.shape[1] != LEVEL_WORDS or x.dtype != torch.int32:
            raise ValueError(f"level_nearest: {name} must be int32 [n, {LEVEL_WORDS}]"
                             f"{' or [' + str(LEVEL_WORDS) + ']' if name == 'queries' else ''} "
                             f"(got {x.dtype} {tuple(x.shape)})")
    n, b = q.shape[0], c.shape[0]
    if c.device != q.device:
        raise ValueError(f"level_nearest: queries on {q.device}, corpus on {c.device}")
    if corpus_mask is not None:
        if corpus_mask.shape != (b,) or corpus_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"level_nearest: corpus_mask must be bool or uint8 [{b}] "
                             f"(got {corpus_mask.dtype} {tuple(corpus_mask.shape)})")
        corpus_mask = corpus_mask.to(torch.uint8).contiguous()
    out = torch.empty((4, n), dtype=torch.int32, device=q.device)
    _lib.call("toued_level_nearest", _lib.ptr(q), n, _lib.ptr(c), b, _lib.ptr(corpus_mask),
              ELIGIBLE_MODES.index(eligible), int(bool(include_lifetime)), _lib.ptr(out[0]), _lib.ptr(out[1]),
              _lib.ptr(out[2]), _lib.ptr(out[3]), _lib.stream_ptr())
    return LevelNearest(*((out[k, 0] if single else out[k]) for k in range(4)))


class LevelEditor:
    """Device ACCEL editor (toued_level_edit; not in the reference): with probability ``p_edit`` a reset slot's
    generated level is replaced by ``num_edits`` small edits (``ops``: wall toggles, object moves, start moves,
    per-type reward nudges of at most ``reward_delta``) of a parent level from the buffer.

    ``require_solvable``: a child without a positive reward reachable within its episode (toued_level_stats'
    SOLVABLE == 0) is refused: the slot keeps the generator's level, all 80 words, and its flag comes back 0.  The
    key schedule does not change, so each row is bit for bit the unfiltered child or the generator's row; a level
    with random respawn (SOLVABLE == -1) passes.  ``last_rejected`` then holds the u8 [n] flags of the refused
    rows of the last call (None without the filter).

    ``min_distance`` D > 0: a child whose level distance (``level_nearest``) to a buffer slot outside this round's
    reset set, or to a lower-indexed row of this round's batch as edited, is below D is refused in the same way
    (D = 1 refuses exact duplicates, which an edit that never applies produces).  The call then needs ``reset_ids``.
    The batch is compared as it stands before any refusal, so a child can be refused because of an earlier child that
    was itself refused: accepted, and deterministic.  The generator's own rows are never refused.
    ``last_too_close`` holds the u8 [n] flags of the rows that were edited, passed the solvable filter and were too
    close (None with D == 0); ``last_rejected`` keeps its meaning.  With D == 0 nothing is launched for it."""

    def __init__(self, spec: EnvSpec, ops="walls,objects,start", num_edits: int = 5, p_edit: float = 0.5,
                 reward_delta: float = 0.1, require_solvable: bool = False, min_distance: int = 0):
        self.spec = spec
        self.ops_mask = parse_edit_ops(ops)
        if num_edits < 0:
            raise ValueError(f"num_edits {num_edits} is negative")
        if not 0.0 <= p_edit <= 1.0:
            raise ValueError(f"edit_prob {p_edit} outside [0, 1]")
        if int(min_distance) != min_distance or min_distance < 0:
            raise ValueError(f"edit_min_distance {min_distance} is not an integer >= 0")
        self.num_edits, self.p_edit, self.reward_delta = int(num_edits), float(p_edit), float(reward_delta)
        self.require_solvable = bool(require_solvable)
        self.min_distance = int(min_distance)
        self.last_rejected = None
        self.last_too_close = None

    def __call__(self, buffer_levels: torch.Tensor, parent_ids: torch.Tensor, keys: torch.Tensor,
                 levels: torch.Tensor, reset_ids: torch.Tensor | None = None) -> torch.Tensor:
        """Edits ``levels`` int32[n, 80] (the generator's levels of ``keys`` int32[n, 2]) in place: row j becomes the
        edited ``buffer_levels[parent_ids[j]]`` where the row's own coin says so and ``parent_ids[j] >= 0`` (and
        the child passes the filters).  ``reset_ids`` int [n]: the buffer slots this round refills, which the
        ``min_distance`` filter leaves out of its comparison.  Returns the u8 [n] flags of the rows that were
        replaced."""
        n = keys.shape[0]
        edited = torch.empty((n,), dtype=torch.uint8, device=keys.device)
        filtered = self.require_solvable or self.min_distance > 0
        if self.min_distance > 0 and reset_ids is None:
            raise ValueError("LevelEditor(min_distance > 0) needs reset_ids, the buffer slots of this round's rows")
        # the filters edit a copy, so that a refused row still holds the generator's level
        target = levels.clone() if filtered else levels
        _lib.call("toued_level_edit", _lib.ptr(buffer_levels), _lib.ptr(parent_ids), _lib.ptr(keys.contiguous()), n,
                  self.spec.max_n_objs, self.spec.max_n_obj_types, self.p_edit, self.num_edits, self.ops_mask,
                  self.reward_delta, _lib.ptr(target), _lib.ptr(edited), _lib.stream_ptr())
        if not filtered:
            return edited
        was_edited = edited != 0
        refused = None
        if self.require_solvable:
            # the unedited rows of the copy are the generator's own, so the one select below serves them too
            refused = level_stats_raw(target, self.spec)[:, LSTAT_SOLVABLE] == 0
            self.last_rejected = (refused & was_edited).to(torch.uint8)
        if self.min_distance > 0:
            outside = torch.ones((buffer_levels.shape[0],), dtype=torch.uint8, device=keys.device)
            outside.index_fill_(0, reset_ids.long(), 0)
            near = torch.minimum(level_nearest(target, buffer_levels, outside).dist,
                                 level_nearest(target, target, eligible="lower").dist)
            close = (near < self.min_distance) & was_edited
            if refused is not None:
                close = close & ~refused
            self.last_too_close = close.to(torch.uint8)
            refused = close if refused is None else refused | close
        levels.copy_(torch.where(refused[:, None], levels, target))
        return edited * (~(refused & was_edited)).to(torch.uint8)


class GridWorld:
    """gymnax ``Environment`` API for GridWorld (gridworld.py:38-236), vectorised.

    ``reset(keys, levels, W)`` and ``step(keys, state, actions, levels, W)``
    apply to n = keys.shape[0] workers; worker i uses level ``i // W``.
    ``step`` includes gymnax's auto-reset (select(done, reset, stepped)).
    """

    def __init__(self, spec: EnvSpec):
        self.spec = spec
        self._c = _lib.env_spec_c(spec)

    @property
    def num_actions(self) -> int:
        return 5

    def reset(self, keys, levels, W: int = 1):
        n = keys.shape[0]
        dev = keys.device
        state = torch.zeros((STATE_FIELDS, n), dtype=torch.int32, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        tm = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("toued_gw_reset", self._c, _lib.ptr(levels), W, _lib.ptr(keys), _lib.ptr(state), _lib.ptr(idx),
                  _lib.ptr(tm), n, _lib.stream_ptr())
        return (idx, tm), state

    def step(self, keys, state, actions, levels, W: int = 1):
        n = keys.shape[0]
        dev = keys.device
        state = state.clone()
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        tm = torch.empty(n, dtype=torch.int32, device=dev)
        rew = torch.empty(n, dtype=torch.float32, device=dev)
        done = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.call("toued_gw_step", self._c, _lib.ptr(levels), W, _lib.ptr(keys), _lib.ptr(state),
                  _lib.ptr(actions.to(torch.int32).contiguous()), _lib.ptr(idx), _lib.ptr(tm), _lib.ptr(rew),
                  _lib.ptr(done), n, _lib.stream_ptr())
        return (idx, tm), state, rew, done.bool()

    def obs_dense(self, idx, tm):
        """Materialise the reference's dense observation (gridworld.py:184-199) — debugging only."""
        D = self.spec.obs_dim
        out = torch.zeros((idx.shape[0], D), dtype=torch.float32, device=idx.device)
        out[torch.arange(idx.shape[0], device=idx.device), idx.long()] = 1.0
        out[:, -1] = tm.float() * torch.tensor(0.001, dtype=torch.float32)
        return out
