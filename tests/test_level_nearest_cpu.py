"""CPU: the level distance's numpy reference (tests/level_nearest_ref.py) on hand-built levels, the shared cases'
coverage, the new command-line flags and the presence of the Python API.  No GPU."""
import inspect

import numpy as np
import pytest

import level_nearest_ref as lnr
import optret_ref as orf
from oracle import levels as olv

F32 = np.float32


def _hand(grid=4, start=5, ids=(0, 1), cells=(6, 9), rew=(1.0, -0.5), walls=(3,), max_steps=10, lifetime=17):
    spec = olv.env_spec("debug")
    p = orf.make_params(spec, grid, start, list(ids), list(cells), list(rew), [0.1, 0.2], [0.5, 0.25], max_steps,
                        walls=list(walls))
    return olv.pack_levels(p, np.array([lifetime], np.int32), spec, buffer_id=np.array([3]))[0]


def test_canonical_record_layout():
    a = _hand()
    c = lnr.canonical(a)
    assert c.shape == (1, 54) and c.dtype == np.int32
    assert c[0, :6].tolist() == [10, 4, 5, 2, 0, 17]
    assert c[0, 6:14].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]              # obj_ids: the -1 padding past n_objs reads 0
    assert c[0, 14:22].tolist() == [6, 9, 0, 0, 0, 0, 0, 0]
    assert c[0, 22:24].view(F32).tolist() == [1.0, -0.5]
    assert c[0, 46:].tolist() == [1 << 3, 0, 0, 0, 0, 0, 0, 0]
    assert lnr.canonical(a, include_lifetime=False)[0, 5] == 0


def test_distance_zero_iff_canonical_equal_symmetric_triangle():
    rows = np.concatenate([lnr.case(m)["corpus"][:40] for m in lnr.MODES] + [lnr.case("debug")["queries"][:30]])
    canon = lnr.canonical(rows)
    d = lnr.distance_matrix(rows, rows)
    assert np.array_equal(d, d.T)
    assert d.min() >= 0 and d.max() <= lnr.DIST_MAX
    same = (canon[:, None, :] == canon[None, :, :]).all(axis=2)
    assert np.array_equal(d == 0, same)
    assert same.sum() > len(rows)                                     # the case holds duplicates beside the diagonal
    rng = np.random.default_rng(0)
    t = rng.integers(0, len(rows), (2000, 3))
    assert (d[t[:, 0], t[:, 2]] <= d[t[:, 0], t[:, 1]] + d[t[:, 1], t[:, 2]]).all()


def test_changes_outside_the_record_leave_distance_zero():
    a = _hand()
    for name, off, n in (("slots past n_objs", None, 0), ("buffer id", olv.L_BUFID, 1), ("word 7", 7, 1),
                         ("type rewards", olv.L_TREW, 5), ("type p_terminate", olv.L_TPTERM, 5),
                         ("type p_respawn", olv.L_TPRESP, 5), ("auto_collect", olv.L_AUTOC, 1)):
        b = a.copy()
        if off is None:
            for f in lnr.SLOT_FIELDS:
                b[f + 2:f + 8] = np.arange(6) * 1234567 - 99
        else:
            b[off:off + n] ^= 0x5A5A5A5A
        assert not np.array_equal(a, b) and lnr.distance(a, b) == 0, name
    # wall bits of the cells >= g^2 = 16: the rest of word 0 and every other word
    b = a.copy()
    b[olv.L_WALLS] |= np.int32(-65536)
    b[olv.L_WALLS + 1:olv.L_WALLS + 8] = -1
    assert lnr.distance(a, b) == 0
    b[olv.L_WALLS] ^= 1 << 15                                          # cell 15 is inside
    assert lnr.distance(a, b) == 1
    # an object slot below n_objs counts
    b = a.copy()
    b[olv.L_STATIC + 1] += 1
    assert lnr.distance(a, b) == 1


def test_lifetime_and_signed_zero():
    a = _hand(lifetime=17)
    b = _hand(lifetime=18)
    assert lnr.distance(a, b) == 1 and lnr.distance(a, b, include_lifetime=False) == 0
    z = _hand(rew=(0.0, -0.5))
    nz = z.copy()
    nz[olv.L_REW] = np.array([-0.0], F32).view(np.int32)[0]
    assert z[olv.L_REW] == 0 and nz[olv.L_REW] != 0
    assert lnr.distance(z, nz) == 1


def test_distance_counts_wall_bits_and_words():
    a = _hand(walls=(3,))
    b = _hand(walls=(3, 7, 8), start=2, max_steps=11)
    assert lnr.distance(a, b) == 2 + 2
    # the largest distance: every plain word and all 256 cells differ
    x = np.zeros(80, np.int32)
    y = np.full(80, -1, np.int32)
    x[olv.L_GRID], x[olv.L_NOBJS], y[olv.L_GRID], y[olv.L_NOBJS] = 16, 8, 17, 9
    assert lnr.distance(x, y) == lnr.DIST_MAX


def test_nearest_eligibility_ties_and_empty():
    c = lnr.case("debug")
    corpus = c["corpus"]
    d = lnr.distance_matrix(corpus, corpus)
    nn, idx, ds, cnt = lnr.nearest(corpus, corpus)
    assert (nn == 0).all() and (cnt == len(corpus)).all() and np.array_equal(ds, d.sum(axis=1))
    assert (idx <= np.arange(len(corpus))).all() and (idx < np.arange(len(corpus))).any()      # ties: the lower index
    nn, idx, _, cnt = lnr.nearest(corpus, corpus, eligible="lower")
    assert nn[0] == lnr.INT_MAX and idx[0] == -1 and cnt[0] == 0 and np.array_equal(cnt, np.arange(len(corpus)))
    nn, idx, ds, cnt = lnr.nearest(corpus, corpus, eligible="others")
    assert (idx != np.arange(len(corpus))).all() and (cnt == len(corpus) - 1).all()
    nn, idx, ds, cnt = lnr.nearest(corpus[:5], corpus, np.zeros(len(corpus), np.uint8))
    assert (nn == lnr.INT_MAX).all() and (idx == -1).all() and (ds == 0).all() and (cnt == 0).all()
    nn, idx, ds, cnt = lnr.nearest(corpus[:5], corpus[:0])
    assert (nn == lnr.INT_MAX).all() and (idx == -1).all() and (ds == 0).all() and (cnt == 0).all()


@pytest.mark.parametrize("mode", lnr.MODES)
def test_cases_cover_what_they_are_meant_to(mode):
    c = lnr.case(mode)
    nn, idx, _, _ = lnr.nearest(c["queries"], c["corpus"])
    assert (nn == 0).sum() >= 20 and (nn == 1).sum() >= 10           # copies up to non-canonical words, and near ones
    raw = (c["queries"][:, None, :] == c["corpus"][None, :, :]).all(axis=2)
    assert not raw.any()                                               # no query equals a corpus row word for word
    d = lnr.distance_matrix(c["queries"], c["corpus"])
    assert ((d == nn[:, None]).sum(axis=1) >= 2).sum() >= 3           # ties at the minimum
    assert (lnr.nearest(c["queries"], c["corpus"], include_lifetime=False)[0] < nn).any()
    g16 = lnr.grid16_rows()
    assert (g16[:, olv.L_GRID] == 16).all() and set(g16[:, olv.L_NOBJS]) == {0, 8}
    assert lnr.distance(g16[0], g16[1]) == 1 and lnr.distance(g16[2], g16[3]) == 1     # cell 255 alone


def test_diversity_and_filter_reference():
    rows = lnr.gen_rows("debug")[:6].copy()
    rows[4] = rows[1]
    rows[4, olv.L_BUFID] = 99
    dv = lnr.diversity(rows)
    assert dv["unique_frac"] == 5 / 6 and 0 <= dv["nn_dist"] <= dv["pair_dist"] <= lnr.DIST_MAX
    # a child equal to a kept buffer row is refused at D = 1; one equal to a reset slot's old row is not
    buf = lnr.gen_rows("debug")[:8]
    gen = lnr.gen_rows("debug")[100:104]
    children = np.stack([buf[2], buf[5], gen[2], buf[5]])
    edited = np.array([True, True, False, True])
    out, kept, close = lnr.filter_children(children, edited, gen, buf, reset_ids=[5, 6, 7, 0], min_distance=1)
    assert close.tolist() == [True, False, False, True] and kept.tolist() == [False, True, False, False]
    assert np.array_equal(out, np.stack([gen[0], buf[5], gen[2], gen[3]]))
    _, _, close = lnr.filter_children(children, edited, gen, buf, [5, 6, 7, 0], lnr.DIST_MAX + 1)
    assert close.tolist() == [True, True, False, True]                # the generator's own row is never refused


def test_new_flags_parse():
    from toued.parse_args import parse_args
    a = parse_args([])
    assert a.edit_min_distance == 0 and a.buffer_diversity is False
    a = parse_args(["--score_function", "alg_regret", "--level_editor", "accel", "--edit_min_distance", "3",
                    "--buffer_diversity"])
    assert a.edit_min_distance == 3 and a.buffer_diversity is True
    with pytest.raises(ValueError, match="edit_min_distance"):
        parse_args(["--score_function", "alg_regret", "--edit_min_distance", "1"])
    with pytest.raises(ValueError, match="edit_min_distance"):
        parse_args(["--score_function", "alg_regret", "--level_editor", "accel", "--edit_min_distance", "-1"])
    with pytest.raises(ValueError, match="buffer_diversity"):
        parse_args(["--buffer_diversity"])                             # score_function random: no buffer
    assert parse_args(["--score_function", "frozen", "--buffer_diversity"]).buffer_diversity


def test_python_api_exists():
    from toued import _lib, env
    assert env.LevelNearest._fields == ("dist", "idx", "dist_sum", "count")
    sig = inspect.signature(env.level_nearest)
    assert list(sig.parameters) == ["queries", "corpus", "corpus_mask", "eligible", "include_lifetime"]
    assert sig.parameters["eligible"].default == "all" and sig.parameters["include_lifetime"].default is True
    assert inspect.signature(env.LevelEditor.__init__).parameters["min_distance"].default == 0
    ed = env.LevelEditor(env.get_env_spec("debug")[0], min_distance=2)
    assert ed.min_distance == 2 and ed.last_too_close is None
    with pytest.raises(ValueError):
        env.LevelEditor(env.get_env_spec("debug")[0], min_distance=-1)
    assert "toued_level_nearest" in _lib._SIGS and hasattr(_lib.lib(), "toued_level_nearest")
    from toued import level_stats
    assert callable(level_stats.diversity_metrics)
