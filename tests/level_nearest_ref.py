"""numpy restatement of the level distance (toued_level_nearest), of the level editor's minimum-distance filter
(LevelEditor(min_distance=D)) and of the buffer diversity metrics (--buffer_diversity) -- the reference of
tests/test_level_nearest_cpu.py and tests/test_gpu_level_nearest.py.

Written from the definition (include/toued.h), not from the kernel.  The canonical record of a packed
level int32 [80] is 54 words:
  * the scalars max_steps, grid_size, start_pos, n_objs, random_respawn, lifetime (lifetime 0 without the flag);
  * obj_ids, static cell, reward, p_terminate, p_respawn of the object slots i < 8, field-major, every field of slot i
    0 when i >= clamp(n_objs, 0, 8);
  * the 8 wall words with only the bits of the cells c < g^2, g = clamp(grid_size, 0, 16); cell c is bit c & 31 of
    word c >> 5.
d(a, b) = popcount(walls_a ^ walls_b) + the number of the 46 other words that differ (bit patterns).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import jaxrand as jr
from oracle import levels as olv

CANON_WORDS, PLAIN_WORDS, DIST_MAX = 54, 46, 302
INT_MAX = 2 ** 31 - 1
SCALARS = (olv.L_MAX_STEPS, olv.L_GRID, olv.L_START, olv.L_NOBJS, olv.L_RANDRESP, olv.L_LIFETIME)
SLOT_FIELDS = (olv.L_OBJ_IDS, olv.L_STATIC, olv.L_REW, olv.L_PTERM, olv.L_PRESP)
ELIGIBLE = ("all", "others", "lower")


def canonical(levels, include_lifetime=True):
    """Packed rows int32 [n, 80] (or one [80]) -> canonical records int32 [n, 54]: 46 plain words, then 8 wall words."""
    lv = np.atleast_2d(np.asarray(levels, np.int32))
    n = len(lv)
    out = np.zeros((n, CANON_WORDS), np.int32)
    for k, off in enumerate(SCALARS):
        out[:, k] = lv[:, off]
    if not include_lifetime:
        out[:, SCALARS.index(olv.L_LIFETIME)] = 0
    nobj = np.clip(lv[:, olv.L_NOBJS], 0, 8)
    used = np.arange(8)[None, :] < nobj[:, None]
    for f, off in enumerate(SLOT_FIELDS):
        out[:, 6 + 8 * f:14 + 8 * f] = np.where(used, lv[:, off:off + 8], 0)
    g = np.clip(lv[:, olv.L_GRID], 0, 16).astype(np.int64)
    cells = np.arange(256)
    bits = (lv[:, olv.L_WALLS:olv.L_WALLS + 8].view(np.uint32)[:, cells >> 5] >> (cells & 31).astype(np.uint32)) & 1
    bits = np.where(cells[None, :] < (g * g)[:, None], bits, 0).astype(np.uint64)
    words = np.zeros((n, 8), np.uint64)
    for c in range(256):
        words[:, c >> 5] |= bits[:, c] << np.uint64(c & 31)
    out[:, PLAIN_WORDS:] = words.astype(np.uint32).view(np.int32)
    return out


def _popcount32(x):
    x = x.astype(np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (4,)), axis=-1).sum(axis=(-1, -2)).astype(np.int64)


def distance_matrix(queries, corpus, include_lifetime=True):
    """d(query i, corpus j) as int64 [n, b]."""
    q, c = canonical(queries, include_lifetime), canonical(corpus, include_lifetime)
    d = np.zeros((len(q), len(c)), np.int64)
    for i in range(len(q)):
        d[i] = (q[i, :PLAIN_WORDS] != c[:, :PLAIN_WORDS]).sum(axis=1)
        d[i] += _popcount32(q[i, PLAIN_WORDS:] ^ c[:, PLAIN_WORDS:]) if len(c) else 0
    return d


def distance(a, b, include_lifetime=True):
    return int(distance_matrix(a, b, include_lifetime)[0, 0])


def nearest(queries, corpus, corpus_mask=None, eligible="all", include_lifetime=True):
    """(nn_dist, nn_idx, dist_sum, count), int32 [n] each, over the eligible corpus entries of each query."""
    d = distance_matrix(queries, corpus, include_lifetime)
    n, b = d.shape
    i, j = np.arange(n)[:, None], np.arange(b)[None, :]
    ok = np.ones((n, b), bool) if corpus_mask is None else np.repeat(np.asarray(corpus_mask)[None, :] != 0, n, axis=0)
    ok &= {"all": np.ones((n, b), bool), "others": j != i, "lower": j < i}[eligible]
    cnt = ok.sum(axis=1)
    dm = np.where(ok, d, INT_MAX)
    nn = dm.min(axis=1, initial=INT_MAX)
    idx = np.where(cnt > 0, dm.argmin(axis=1) if b else 0, -1)       # argmin: the first (lowest) index of the minimum
    return (nn.astype(np.int32), idx.astype(np.int32), np.where(ok, d, 0).sum(axis=1).astype(np.int32),
            cnt.astype(np.int32))


def diversity(levels):
    """{"unique_frac", "nn_dist", "pair_dist"} of a buffer's packed rows (B >= 2)."""
    B = len(levels)
    nn, idx, ds, _ = nearest(levels, levels, eligible="others")
    first = (nn > 0) | (idx > np.arange(B))
    return {"unique_frac": float(first.mean()), "nn_dist": float(nn.astype(np.float64).mean()),
            "pair_dist": float(ds.astype(np.float64).sum() / (B * (B - 1)))}


def filter_children(children, edited, gen_rows, buf_rows, reset_ids, min_distance):
    """LevelEditor(min_distance=D) after the edit: ``children`` the batch as edited, ``edited`` bool [n].  A row is
    too close when it was edited and its distance to a buffer row outside ``reset_ids``, or to a lower-indexed row of
    ``children``, is below D; it goes back to the generator's row.  Returns (rows, kept, too_close)."""
    outside = np.ones(len(buf_rows), bool)
    outside[np.asarray(reset_ids, np.int64)] = False
    near = np.minimum(nearest(children, buf_rows, outside)[0], nearest(children, children, eligible="lower")[0])
    close = np.asarray(edited, bool) & (near < min_distance)
    rows = np.where(close[:, None], np.asarray(gen_rows, np.int32), np.asarray(children, np.int32))
    return rows, np.asarray(edited, bool) & ~close, close


# ---------------------------------------------------------------------------
# Shared cases
MODES = ("debug", "all", "mazes")
SEED = {"debug": 511, "all": 512, "mazes": 513}
N_GEN = 140


@functools.lru_cache(maxsize=None)
def gen_rows(mode, n=N_GEN, seed=None):
    spec = olv.env_spec(mode)
    keys = jr.split(jr.PRNGKey(SEED[mode] if seed is None else seed), n)
    p, lt = olv.reset_env_params(keys, mode)
    return olv.pack_levels(p, lt, spec, buffer_id=np.arange(n))


def perturbed(rows, seed):
    """Copies of ``rows`` with changes that leave the canonical record alone (garbage in the object slots past n_objs,
    wall bits past g^2, the buffer id, word 7, the per-type tables) on every row, and on every third row one that
    does not: a wall bit inside the grid (row % 9 == 0), the lifetime (== 3) or the start (== 6)."""
    rng = np.random.default_rng(seed)
    out = np.array(rows, np.int32)
    n = len(out)
    junk = lambda shape: rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    nobj = np.clip(out[:, olv.L_NOBJS], 0, 8)
    unused = np.arange(8)[None, :] >= nobj[:, None]
    for off in SLOT_FIELDS:
        out[:, off:off + 8] = np.where(unused, junk((n, 8)), out[:, off:off + 8])
    g2 = np.clip(out[:, olv.L_GRID], 0, 16).astype(np.int64) ** 2
    for k in range(8):
        rem = np.clip(g2 - 32 * k, 0, 32)
        keep = np.where(rem >= 32, 0xFFFFFFFF, (np.int64(1) << rem) - 1).astype(np.uint32)
        w = out[:, olv.L_WALLS + k].view(np.uint32)
        out[:, olv.L_WALLS + k] = ((w & keep) | (junk(n).view(np.uint32) & ~keep)).view(np.int32)
    out[:, olv.L_BUFID] = junk(n)
    out[:, 7] = junk(n)
    out[:, olv.L_TREW:olv.LEVEL_WORDS] = junk((n, olv.LEVEL_WORDS - olv.L_TREW))
    r = np.arange(n)
    cell = (r * 5) % np.maximum(g2, 1)
    sel = (r % 9 == 0) & (g2 > 0)
    out[sel, olv.L_WALLS + (cell[sel] >> 5)] ^= (np.uint32(1) << (cell[sel] & 31).astype(np.uint32)).view(np.int32)
    out[r % 9 == 3, olv.L_LIFETIME] += 1
    out[r % 9 == 6, olv.L_START] += 1
    return out


@functools.lru_cache(maxsize=None)
def case(mode):
    """{"corpus" [130, 80], "queries" [65, 80]}: generator levels, and queries that are perturbed copies of corpus rows
    (7 * i % 130), so that most queries have a corpus entry at distance 0 or 1 and, the copies of one row repeating,
    ties at the minimum."""
    rows = gen_rows(mode)
    corpus = rows[:130].copy()
    corpus[64:70] = perturbed(corpus[:6], SEED[mode] + 1)        # near copies inside the corpus: ties at the minimum
    src = (7 * np.arange(65)) % 130
    return {"corpus": corpus, "queries": perturbed(corpus[src], SEED[mode] + 2)}


@functools.lru_cache(maxsize=None)
def big_case():
    """4000 ``all`` levels (each of 500 generator levels eight times over, perturbed) and 512 queries among them."""
    base = gen_rows("all", 500, seed=77)
    corpus = perturbed(np.tile(base, (8, 1)), 78)
    corpus[:, olv.L_BUFID] = np.arange(4000)
    queries = perturbed(corpus[(13 * np.arange(512)) % 4000], 79)
    return {"corpus": corpus, "queries": queries}


def grid16_rows():
    """Six hand-built 16x16 levels: cell 255 set or clear, 0 or 8 objects."""
    import optret_ref as orf
    from oracle import gridworld as ogw
    spec16 = ogw.EnvSpec(16, 8, 5, True)
    out = []
    for walls, nobj in (([255], 8), ([], 8), ([255, 0], 0), ([0], 0), ([255, 31, 32], 8), ([31, 32], 8)):
        p = orf.make_params(spec16, 16, 17, [i % 5 for i in range(nobj)],
                            [40 + 3 * i for i in range(nobj)], [0.5, -0.5, 0.25, 0.0, 1.0],
                            [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, 0.25, 0.125, 0.0, 1.0], 30, walls=walls)
        out.append(olv.pack_levels(p, np.array([9], np.int32), spec16, buffer_id=np.array([len(out)]))[0])
    return np.stack(out)


EDITOR_B, EDITOR_RESET = 32, (31, 3, 17, 8, 25, 0, 12, 29)
EDITOR_PARENTS = (5, 9, 5, -1, 20, 9, 14, 5)


@functools.lru_cache(maxsize=None)
def editor_case(mode="debug"):
    """A buffer of EDITOR_B generator levels and a reset round of 8 slots (EDITOR_RESET, the generator's rows of fresh
    keys) whose parents (EDITOR_PARENTS: outside the reset set, some shared, one -1) the level editor edits."""
    import level_edit_ref as ler
    spec = olv.env_spec(mode)
    buf_rows = gen_rows(mode, EDITOR_B, seed=SEED[mode] + 10)
    keys = jr.split(jr.PRNGKey(SEED[mode] + 11), len(EDITOR_RESET))
    p, lt = olv.reset_env_params(keys, mode)
    gen = olv.pack_levels(p, lt, spec, buffer_id=np.array(EDITOR_RESET))
    return {"spec": spec, "buf_rows": buf_rows, "keys": keys, "gen_rows": gen,
            "reset_ids": np.array(EDITOR_RESET, np.int32), "parent_ids": np.array(EDITOR_PARENTS, np.int32),
            "edit_rows": lambda num_edits, mask=7, p_edit=1.0: ler.edit_rows(
                buf_rows, np.array(EDITOR_PARENTS, np.int32), keys, gen, spec, p_edit, num_edits, mask,
                ler.REWARD_DELTA)[:2]}
