"""The ACCEL level editor without a GPU: the invariants of the numpy restatement (tests/level_edit_ref.py) that the
device kernel is compared against bit for bit (tests/test_gpu_level_edit.py), the coverage of that comparison's cases,
and the command-line surface (--level_editor and its companions, LevelSampler's argument checks).
"""
import collections

import numpy as np
import pytest

import level_edit_ref as ler
from oracle import levels as olv


def _children(mode, num_edits, mask):
    """(parents' params, children's params, edited, logs) of the mode's shared case at p_edit = 1."""
    c = ler.case(mode)
    rows, edited, logs = ler.case_reference(mode, num_edits, mask, 1.0)
    par, par_lt, _ = ler.unpack(c["buf_rows"][np.maximum(c["parent_ids"], 0)], c["spec"])
    ch, ch_lt, ch_id = ler.unpack(rows, c["spec"])
    return c, rows, par, par_lt, ch, ch_lt, ch_id, edited, logs


@pytest.mark.parametrize("mask", ler.CASE_MASKS)
@pytest.mark.parametrize("mode", ler.CASE_MODES)
def test_edited_levels_keep_the_generator_invariants(mode, mask):
    c, rows, par, par_lt, ch, ch_lt, ch_id, edited, logs = _children(mode, 8, mask)
    spec = c["spec"]
    assert np.array_equal(edited, c["parent_ids"] >= 0) and edited.sum() >= 50
    changed = 0
    for j in np.flatnonzero(edited):
        g2 = int(ch["grid_size"][j]) ** 2
        cells = [int(ch["start_pos"][j])] + ch["static_obj_poss"][j].tolist()
        assert len(cells) == spec.max_n_objs + 1 and len(set(cells)) == len(cells), (j, cells)
        assert all(0 <= x < g2 for x in cells), (j, cells, g2)
        assert not ch["walls"][j][cells].any(), (j, cells)
        for name in ler.INHERITED:
            assert np.array_equal(ch[name][j], par[name][j]), (j, name)
        assert ch_lt[j] == par_lt[j] and ch_id[j] == 100 + j
        assert rows[j, olv.L_AUTOC] == 1
        # per-object reward words = the per-type table through obj_ids (-1 taking the last type)
        ids = ch["obj_ids"][j]
        rid = np.where(ids < 0, ids + spec.max_n_obj_types, ids)
        want = ch["obj_rewards"][j][rid].view(np.int32)
        assert np.array_equal(rows[j, olv.L_REW:olv.L_REW + spec.max_n_objs], want), j
        r = ch["obj_rewards"][j]
        assert 0.0 <= r[0] <= 1.0 and np.all(r[1:] >= -1.0) and np.all(r[1:] <= 1.0), (j, r)
        if mask == 8:       # the rewards op alone moves nothing else
            for name in ("walls", "start_pos", "static_obj_poss"):
                assert np.array_equal(ch[name][j], par[name][j]), (j, name)
        else:
            assert np.array_equal(ch["obj_rewards"][j], par["obj_rewards"][j]) or mask == 15, j
        changed += any(not np.array_equal(ch[k][j], par[k][j]) for k in ch)
    assert changed >= 40, changed
    # the untouched rows (parent -1) are the generator's
    for j in np.flatnonzero(~edited):
        assert np.array_equal(rows[j], c["gen_rows"][j])


@pytest.mark.parametrize("mode", ler.CASE_MODES)
def test_identities(mode):
    c = ler.case(mode)
    # num_edits = 0: the child is its parent under the slot's id
    rows, edited, _ = ler.case_reference(mode, 0, 15, 1.0)
    for j in np.flatnonzero(edited):
        want = c["buf_rows"][c["parent_ids"][j]].copy()
        want[olv.L_BUFID] = 100 + j
        assert np.array_equal(rows[j], want), j
    # p_edit = 0: nothing is edited
    rows, edited, logs = ler.case_reference(mode, 8, 15, 0.0)
    assert not edited.any() and np.array_equal(rows, c["gen_rows"]) and all(l is None for l in logs)
    # p_edit = 0.5: a proper subset, and the edited rows are the p_edit = 1 rows
    half, e_half, _ = ler.case_reference(mode, 8, 15, 0.5)
    full, e_full, _ = ler.case_reference(mode, 8, 15, 1.0)
    assert 0 < e_half.sum() < e_full.sum() and not (e_half & ~e_full).any()
    assert np.array_equal(half[e_half], full[e_half]) and np.array_equal(half[~e_half], c["gen_rows"][~e_half])


def test_the_gpu_cases_cover_every_op_both_ways():
    """Over the kernel test's cases every op is applied at least once and rejected at least once, and the mazes
    case edits cells in the wall bitmap's sixth word."""
    seen = collections.Counter()
    high = collections.Counter()
    for mode in ler.CASE_MODES:
        for (e, m, p) in ler.CASE_CONFIGS:
            for log in ler.case_reference(mode, e, m, p)[2]:
                for op, applied, cell in log or ():
                    seen[(op, applied)] += 1
                    if mode == "mazes" and cell >= 160 and applied:
                        high[op] += 1
    for name in ("full", "no_objs"):
        for log in ler.hand_case(name)["ref"][2]:
            for op, applied, _ in log:
                seen[(op, applied)] += 1
    print(dict(seen), dict(high))
    for op in ler.OPS:
        assert seen[(op, True)] > 0 and seen[(op, False)] > 0, (op, seen)
    assert all(high[op] > 0 for op in ("walls", "objects", "start")), high


def test_hand_cases_do_what_they_are_built_for():
    full = ler.hand_case("full")
    rows, edited, logs = full["ref"]
    assert edited.all()
    ops = {(op, a) for log in logs for op, a, _ in log}
    assert not ops & {("walls", True), ("objects", True), ("start", True)} and ("rewards", True) in ops
    par = full["buf_rows"][0]
    struct = [olv.L_START] + list(range(olv.L_STATIC, olv.L_STATIC + 8)) + list(range(olv.L_WALLS, olv.L_WALLS + 8))
    assert np.array_equal(rows[:, struct], np.repeat(par[None, struct], len(rows), 0))
    rew = rows[:, olv.L_TREW:olv.L_TREW + 3].view(np.float32)
    assert (rew != par[olv.L_TREW:olv.L_TREW + 3].view(np.float32)).any()
    assert rew[:, 0].max() <= 1.0 and rew[:, 1].min() >= -1.0
    assert (rew[:, 0] == 1.0).any() or (rew[:, 1] == -1.0).any()          # a clamp was hit (0.95 + 8 * 0.1 steps)
    none = ler.hand_case("no_objs")
    rows, edited, logs = none["ref"]
    ops = {(op, a) for log in logs for op, a, _ in log}
    assert ("objects", True) not in ops and ("rewards", True) not in ops
    assert {("objects", False), ("rewards", False)} <= ops
    keep = list(range(olv.L_OBJ_IDS, olv.L_WALLS)) + list(range(olv.L_TREW, olv.LEVEL_WORDS))
    assert np.array_equal(rows[:, keep], np.repeat(none["buf_rows"][:, keep], len(rows), 0))


def test_parent_ids_restatement():
    score = np.array([0.5, 2.0, -1.0, 2.0, 0.0, -0.0, 3.0, 1.0], np.float32)
    fresh = np.array([0, 0, 0, 0, 0, 0, 1, 0], bool)
    got = ler.parent_ids(score, fresh, np.array([7, 2]))
    # eligible 0 1 3 4 5 by score: 1, 3 (tie, by index), 0, 4, 5 (+-0 tie, by index)
    assert got.tolist() == [1, 3]
    assert ler.parent_ids(score, fresh, np.array([0, 1, 2, 3, 4, 5, 7])).tolist() == [-1] * 7
    assert ler.parent_ids(score, fresh, np.array([1, 3, 0, 6, 7, 2, 2])).tolist() == [4, 5, 4, 5, 4, 5, 4]


# ---------------------------------------------------------------------------------------------- command line

_BASE = ["--env_mode", "debug", "--num_agents", "8", "--num_mini_batches", "1", "--buffer_size", "32"]


def test_cli_defaults():
    from toued.parse_args import parse_args
    a = parse_args([])
    assert (a.level_editor, a.edit_prob, a.num_edits, a.edit_ops, a.edit_reward_delta) == \
        ("none", 0.5, 5, "walls,objects,start", 0.1)
    a = parse_args(["--level_editor", "accel", "--edit_prob", "0.25", "--num_edits", "3", "--edit_ops",
                    "walls,rewards", "--edit_reward_delta", "0.2"])
    assert (a.level_editor, a.edit_prob, a.num_edits, a.edit_ops, a.edit_reward_delta) == \
        ("accel", 0.25, 3, "walls,rewards", 0.2)
    with pytest.raises(SystemExit):
        parse_args(["--level_editor", "paired"])


def test_sampler_builds_the_editor():
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    s = LevelSampler(parse_args(_BASE + ["--score_function", "optimal_regret"]), device="cpu")
    assert s.editor is None and s.last_edit is None
    s = LevelSampler(parse_args(_BASE + ["--score_function", "optimal_regret", "--level_editor", "accel",
                                         "--edit_ops", "rewards, walls", "--num_edits", "0", "--edit_prob", "1"]),
                     device="cpu")
    assert (s.editor.ops_mask, s.editor.num_edits, s.editor.p_edit) == (9, 0, 1.0)
    assert abs(s.editor.reward_delta - 0.1) < 1e-12 and s.last_edit is None


@pytest.mark.parametrize("flags,match", [
    (["--score_function", "random"], "reset round"),
    (["--score_function", "frozen"], "reset round"),
    (["--score_function", "alg_regret", "--edit_ops", "walls,doors"], "doors"),
    (["--score_function", "alg_regret", "--edit_ops", ""], "empty"),
    (["--score_function", "alg_regret", "--edit_ops", ","], "empty"),
    (["--score_function", "alg_regret", "--edit_prob", "1.5"], "edit_prob"),
    (["--score_function", "alg_regret", "--edit_prob", "-0.1"], "edit_prob"),
    (["--score_function", "alg_regret", "--edit_prob", "nan"], "edit_prob"),
    (["--score_function", "alg_regret", "--num_edits", "-1"], "num_edits"),
])
def test_sampler_rejects_invalid_editor_arguments(flags, match):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(_BASE + ["--level_editor", "accel"] + flags)
    with pytest.raises(ValueError, match=match):
        LevelSampler(args, device="cpu")
    # the same flags are inert without the editor
    off = parse_args(_BASE + flags)
    assert LevelSampler(off, device="cpu").editor is None
