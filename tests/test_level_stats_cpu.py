"""Level reachability statistics without a GPU: the numpy restatement (tests/level_stats_ref.py) that the device kernel
is compared against word for word (tests/test_gpu_level_stats.py) on hand-built levels whose stats are written out
here, the non-vacuity of that comparison's generator and ACCEL cases, the filtered editor's logic on the restatement,
and the command-line surface (--edit_require_solvable, --level_metrics).
"""
import numpy as np
import pytest

import level_edit_ref as ler
import level_stats_ref as lsr
from oracle import levels as olv

# [CELLS, N_WALLS, N_REACH, ECC, N_OBJ_REACH, N_POS_REACH, NEAREST_POS, SOLVABLE, OBJ_DIST[0..7]], worked out by hand
_M = [-1] * 6
HAND_EXPECTED = {
    # 13x13, no walls, start in a corner: the far corner (object 0, +0.5) is 12 + 12 moves away, object 1 (-0.5) 12
    "open13": [169, 0, 169, 24, 2, 1, 24, 1, 24, 12] + _M,
    # the start's four neighbours are walls
    "enclosed": [169, 4, 1, 0, 0, 0, -1, 0, -1, -1] + _M,
    # cells 1, 2, 3 of row 0; cell 4 = cell 3 + 1 is the next row's first and stays apart.  Object 1 (reward 0) at 3
    "wrap4_top": [16, 4, 3, 2, 1, 0, -1, 0, -1, 2] + _M,
    # cell 4 and rows 2, 3: nine cells, the farthest (15) five moves away; object 0 at cell 8, one move, max_steps 1
    "wrap4_bottom": [16, 4, 9, 5, 1, 1, 1, 1, 1, -1] + _M,
    # 7 open rows of 13 joined by 6 single cells: 97 cells, the last 96 moves from the first; max_steps 95 and 96
    "serpentine_95": [169, 72, 97, 96, 2, 1, 96, 0, 96, 84] + _M,
    "serpentine_96": [169, 72, 97, 96, 2, 1, 96, 1, 96, 84] + _M,
    # 5x5 inside a 13x13 record: the wall bits from cell 25 on do not count; the objects at cell 30 (outside the grid)
    # and at cell 12 (a wall) are not reachable
    "beyond_g2": [25, 1, 24, 8, 1, 1, 8, 1, 8, -1, -1] + _M[1:],
    "no_objs": [9, 1, 8, 2, 0, 0, -1, 0, -1, -1] + _M,
    "randresp": [169, 0, 169, 24, 0, 0, -1, -1, -1, -1] + _M,
    # the start (cell 5) is a wall: it is in R at distance 0 and every other cell is reachable; object 1 lies on it, so
    # NEAREST_POS is 0 and the level is solvable from max_steps 1 on (max(NEAREST_POS, 1)), not at max_steps 0
    "start_on_wall": [16, 1, 16, 4, 2, 2, 0, 1, 1, 0] + _M,
    "start_on_wall_h0": [16, 1, 16, 4, 2, 2, 0, 0, 1, 0] + _M,
}


def test_hand_cases_are_all_listed():
    assert sorted(HAND_EXPECTED) == sorted(lsr.hand_cases())
    assert all(len(v) == lsr.WORDS for v in HAND_EXPECTED.values())


@pytest.mark.parametrize("name", sorted(HAND_EXPECTED))
def test_reference_on_hand_built_levels(name):
    spec, params = lsr.hand_cases()[name]
    st, dist = lsr.level_stats(params, spec)
    assert st.shape == (1, lsr.WORDS) and st.dtype == np.int32 and dist.shape == (1, spec.max_grid_size ** 2)
    assert st[0].tolist() == HAND_EXPECTED[name]
    # the packed row gives the same
    st2, dist2 = lsr.level_stats_rows(lsr.hand_rows(name)[1], spec)
    assert np.array_equal(st, st2) and np.array_equal(dist, dist2)
    # the map agrees with the stats
    g2 = int(st[0, lsr.CELLS])
    assert (dist[0, g2:] == -1).all() and dist[0].max() == st[0, lsr.ECC]
    assert (dist[0] >= 0).sum() == st[0, lsr.N_REACH]


def test_reference_distance_maps_of_hand_built_levels():
    spec, params = lsr.hand_cases()["open13"]
    _, dist = lsr.level_stats(params, spec)
    c = np.arange(169)
    assert np.array_equal(dist[0], c // 13 + c % 13)
    spec, params = lsr.hand_cases()["serpentine_96"]
    _, dist = lsr.level_stats(params, spec)
    d = dist[0].reshape(13, 13)
    assert (d[1::2] >= 0).sum() == 6 and d[1, 12] == 13 and d[3, 0] == 27 and d[11, 0] == 83
    assert np.array_equal(d[0], np.arange(13)) and np.array_equal(d[2], 26 - np.arange(13)) and d[12, 12] == 96
    spec, params = lsr.hand_cases()["wrap4_top"]
    _, dist = lsr.level_stats(params, spec)
    assert dist[0].tolist() == [-1, 0, 1, 2] + [-1] * 12
    spec, params = lsr.hand_cases()["wrap4_bottom"]
    _, dist = lsr.level_stats(params, spec)
    assert dist[0].tolist() == [-1] * 4 + [0, -1, -1, -1, 1, 2, 3, 4, 2, 3, 4, 5]
    spec, params = lsr.hand_cases()["start_on_wall"]
    _, dist = lsr.level_stats(params, spec)
    assert dist[0].tolist() == [2, 1, 2, 3, 1, 0, 1, 2, 2, 1, 2, 3, 3, 2, 3, 4]


# counts of the restatement on the shared cases: (unsolvable, with NEAREST_POS > max_steps) of the generator levels of
# PRNGKey(7) -- debug 512: (46, 2), all 1024: (11, 0), mazes 256: (9, 9) -- and unsolvable among the 56 children of
# level_edit_ref.case(mode) at 8 wall-only edits: debug 9, all 4, mazes 17 (one of the mazes' 24 parents is unsolvable)
GEN_FLOORS = {"debug": 20, "all": 5, "mazes": 4}
CHILD_FLOORS = {"debug": 4, "all": 2, "mazes": 8}


@pytest.mark.parametrize("mode", sorted(lsr.GEN_CASES))
def test_generator_cases_are_not_vacuous(mode):
    c = lsr.gen_case(mode)
    st, rows = c["stats"], c["rows"]
    assert len(st) == lsr.GEN_CASES[mode]
    solv = st[:, lsr.SOLVABLE]
    assert set(np.unique(solv)) <= {0, 1}
    assert (solv == 0).sum() >= GEN_FLOORS[mode] and (solv == 1).sum() >= len(st) // 2
    beyond = st[:, lsr.NEAREST_POS] > rows[:, olv.L_MAX_STEPS]
    assert not (beyond & (solv == 1)).any()
    if mode == "mazes":
        assert beyond.sum() >= 4 and st[:, lsr.ECC].max() > 80
    # the object on the start never happens in a generated level: an unsolvable one has no reward within reach
    assert (st[:, lsr.NEAREST_POS] != 0).all()


@pytest.mark.parametrize("mode", sorted(lsr.GEN_CASES))
def test_children_cases_are_not_vacuous(mode):
    c = lsr.child_case(mode)
    assert c["edited"].sum() == 56
    solv = c["stats"][c["edited"], lsr.SOLVABLE]
    assert (solv == 0).sum() >= CHILD_FLOORS[mode] and (solv == 1).sum() >= 30
    # editing walls makes levels unsolvable that were not: more among the children than among their parents
    assert (solv == 0).mean() > (c["parent_stats"][:, lsr.SOLVABLE] == 0).mean()


@pytest.mark.parametrize("num_edits,mask,p_edit", [(8, 1, 1.0), (8, 15, 0.5)])
@pytest.mark.parametrize("mode", ler.CASE_MODES)
def test_filtered_editor_on_the_reference(mode, num_edits, mask, p_edit):
    c = ler.case(mode)
    spec = c["spec"]
    plain, edited, _ = ler.case_reference(mode, num_edits, mask, p_edit)
    rows, kept, rejected = lsr.edit_rows_filtered(c["buf_rows"], c["parent_ids"], c["keys"], c["gen_rows"], spec, p_edit,
                                                  num_edits, mask, ler.REWARD_DELTA)
    assert not (kept & rejected).any() and np.array_equal(kept | rejected, edited)
    # every row is the unfiltered child or the generator's row, all 80 words
    assert np.array_equal(rows[kept], plain[kept]) and np.array_equal(rows[~kept], c["gen_rows"][~kept])
    st_plain, _ = lsr.level_stats_rows(plain, spec)
    assert np.array_equal(rejected, edited & (st_plain[:, lsr.SOLVABLE] == 0))
    st, _ = lsr.level_stats_rows(rows, spec)
    assert (st[kept, lsr.SOLVABLE] == 1).all()
    assert kept.sum() >= 10
    if (num_edits, mask, p_edit) == lsr.CHILD_CONFIG:       # the wall-only children: the floors of the case
        assert rejected.sum() >= CHILD_FLOORS[mode]
    else:                                                   # the coin: some slots were never the editor's
        assert (~edited & (c["parent_ids"] >= 0)).sum() >= 10


def test_filter_passes_random_respawn_children():
    c = ler.case("debug")
    buf = c["buf_rows"].copy()
    buf[:, olv.L_RANDRESP] = 1
    rows, kept, rejected = lsr.edit_rows_filtered(buf, c["parent_ids"], c["keys"], c["gen_rows"], c["spec"], 1.0, 8, 1,
                                                  ler.REWARD_DELTA)
    assert not rejected.any() and kept.sum() == 56 and (rows[kept, olv.L_RANDRESP] == 1).all()


# ---------------------------------------------------------------------------------------------- command line

_BASE = ["--env_mode", "debug", "--num_agents", "8", "--num_mini_batches", "1", "--buffer_size", "32",
         "--score_function", "positive_value_loss"]


def test_cli_defaults():
    from toued.parse_args import build_parser, parse_args
    a = parse_args([])
    assert a.edit_require_solvable is False and a.level_metrics is False
    a = parse_args(["--level_editor", "accel", "--edit_require_solvable", "--level_metrics"])
    assert a.edit_require_solvable is True and a.level_metrics is True
    assert parse_args(["--level_metrics"]).level_metrics is True            # needs no editor
    p = build_parser()
    assert p.get_default("edit_require_solvable") is not None and p.get_default("level_metrics") is not None


def test_require_solvable_needs_the_editor():
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    with pytest.raises(ValueError, match="edit_require_solvable"):
        parse_args(_BASE + ["--edit_require_solvable"])
    args = parse_args(_BASE)
    args.edit_require_solvable = True                                       # past the parser: the sampler checks too
    with pytest.raises(ValueError, match="edit_require_solvable"):
        LevelSampler(args, device="cpu")
    s = LevelSampler(parse_args(_BASE + ["--level_editor", "accel", "--edit_require_solvable"]), device="cpu")
    assert s.editor.require_solvable is True and s.editor.last_rejected is None
    s = LevelSampler(parse_args(_BASE + ["--level_editor", "accel"]), device="cpu")
    assert s.editor.require_solvable is False


def test_level_editor_constructor_default():
    from toued.env import LevelEditor, LevelStats, get_env_spec
    spec, _, _ = get_env_spec("debug")
    assert LevelEditor(spec).require_solvable is False
    assert LevelEditor(spec, require_solvable=True).require_solvable is True
    assert LevelStats._fields == ("cells", "n_walls", "n_reach", "ecc", "n_obj_reach", "n_pos_reach", "nearest_pos",
                                  "solvable", "obj_dist", "dist")


def test_header_names_the_stats_words():
    import re
    from pathlib import Path
    from toued import env
    text = (Path(__file__).resolve().parents[1] / "include" / "toued.h").read_text()
    defs = dict(re.findall(r"#define TOUED_LSTAT_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "WORDS": 16, "CELLS": 0, "N_WALLS": 1, "N_REACH": 2, "ECC": 3, "N_OBJ_REACH": 4, "N_POS_REACH": 5,
        "NEAREST_POS": 6, "SOLVABLE": 7, "OBJ_DIST": 8}
    for k, v in defs.items():
        assert getattr(env, "LSTAT_" + k) == int(v) == getattr(lsr, k, int(v))
