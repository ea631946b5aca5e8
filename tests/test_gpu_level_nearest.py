"""GPU: the level distance kernel (toued_level_nearest), the level editor's minimum-distance filter
(--edit_min_distance) and the buffer diversity metrics (--buffer_diversity).

  * toued_level_nearest against the numpy reference (tests/level_nearest_ref.py), all four outputs exactly, on
    perturbed generator levels of debug, all and mazes: corpus sizes 0 .. 130 and 4000, query counts 0 .. 512, masks,
    the three eligibility modes, ties, the lifetime flag, 16x16 levels, a repeat call; the argument checks
  * toued.env.level_nearest: shapes, the single-row form, a side stream, no host synchronisation
  * LevelEditor(min_distance=D) against level_edit_ref's children filtered by the reference; LevelSampler.sample
  * ``python -m toued.train --edit_min_distance 1 --buffer_diversity`` and ``python -m toued.level_stats --diversity``
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import level_edit_ref as ler
import level_nearest_ref as lnr
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle import sampler as osp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "to-ued_amd")
NAMES = ("nn_dist", "nn_idx", "dist_sum", "count")


def dk(a):
    from toued.prng import from_uint32_numpy
    return from_uint32_numpy(a, "cuda")


def _nearest(queries, corpus, mask=None, eligible="all", include_lifetime=True):
    """toued_level_nearest through the C ABI on numpy rows -> the four outputs as numpy; the inputs come back as they
    went in."""
    from toued import _lib
    n, b = len(queries), len(corpus)
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int32)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(corpus, np.int32)).cuda()
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    out = torch.full((4, max(n, 1)), -77, dtype=torch.int32, device="cuda")
    _lib.call("toued_level_nearest", _lib.ptr(q), n, _lib.ptr(c), b, _lib.ptr(m), lnr.ELIGIBLE.index(eligible),
              int(include_lifetime), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(out[3]),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy(), queries) and np.array_equal(c.cpu().numpy(), corpus)
    return tuple(out[k, :n].cpu().numpy() for k in range(4))


def _check(queries, corpus, what, **kw):
    got = _nearest(queries, corpus, **kw)
    want = lnr.nearest(queries, corpus, kw.get("mask"), kw.get("eligible", "all"), kw.get("include_lifetime", True))
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, kw.get("eligible"), name, bad[:5], g[bad[:5]], w[bad[:5]])
    return got


@pytest.mark.parametrize("mode", lnr.MODES)
def test_matches_reference_over_corpus_and_query_sizes(mode):
    c = lnr.case(mode)
    for b in (0, 1, 63, 64, 65, 130):
        for n in (0, 1, 65):
            _check(c["queries"][:n], c["corpus"][:b], (mode, n, b))
    got = _check(c["queries"], c["corpus"], mode)
    assert (got[0] == 0).sum() >= 20 and (got[0] == 1).sum() >= 10
    again = _nearest(c["queries"], c["corpus"])                           # a repeat call: bit-identical
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
    _check(c["queries"], c["corpus"], (mode, "no lifetime"), include_lifetime=False)


@pytest.mark.parametrize("mode", lnr.MODES)
def test_masks_and_eligibility(mode):
    c = lnr.case(mode)
    corpus = c["corpus"]
    b = len(corpus)
    rng = np.random.default_rng(3)
    for mask in (np.zeros(b, np.uint8), np.ones(b, np.uint8), (rng.random(b) < 0.4).astype(np.uint8),
                 (rng.random(b) < 0.5).astype(np.uint8) * 200):
        got = _check(c["queries"], corpus, (mode, "mask", int(mask.sum())), mask=mask)
        if not mask.any():
            assert (got[0] == lnr.INT_MAX).all() and (got[1] == -1).all() and not got[2].any() and not got[3].any()
    for eligible in lnr.ELIGIBLE:                                         # queries identical to the corpus
        got = _check(corpus, corpus, (mode, "self"), eligible=eligible)
        _check(corpus, corpus, (mode, "self, masked"), eligible=eligible, mask=(rng.random(b) < 0.5).astype(np.uint8))
        _check(corpus, corpus, (mode, "self, no lifetime"), eligible=eligible, include_lifetime=False)
    assert got[0][0] == lnr.INT_MAX and got[1][0] == -1 and got[3][0] == 0    # "lower": nothing below row 0


def test_ties_return_the_lower_index():
    rows = lnr.gen_rows("all")
    corpus = rows[:70].copy()
    corpus[66] = corpus[2]                         # exact copies across two LDS tiles: distance 0 twice
    corpus[66, olv.L_BUFID] = 1234
    q = rows[100:103].copy()
    q[0] = corpus[2]
    q[1] = corpus[66]
    q[1, olv.L_START] += 1                         # distance 1 to both
    nn, idx, _, _ = _check(q, corpus, "ties")
    assert nn[:2].tolist() == [0, 1] and idx[:2].tolist() == [2, 2]
    nn, idx, _, _ = _check(q, corpus, "ties, first masked", mask=(np.arange(70) != 2).astype(np.uint8))
    assert nn[:2].tolist() == [0, 1] and idx[:2].tolist() == [66, 66]


def test_grid16_and_object_counts():
    g16 = lnr.grid16_rows()                        # cell 255 set or clear, n_objs 0 and 8
    corpus = np.concatenate([g16, lnr.perturbed(g16, 5)])
    nn, idx, _, _ = _check(g16, corpus, "grid16", eligible="others")
    assert nn[1] == 0 and idx[1] == 7              # row 1's perturbed copy keeps its record
    assert nn[0] == 1 and idx[0] == 1              # row 0: cell 255 apart from row 1, cell 0 from its own copy
    d = lnr.distance_matrix(g16, g16)
    assert d[0, 1] == 1 and d[2, 3] == 1
    _check(g16, g16, "grid16 self", eligible="lower")


def test_large_corpus():
    c = lnr.big_case()                             # 512 queries against 4000: the corpus split over gridDim.y
    got = _check(c["queries"], c["corpus"], "4000")
    assert (got[3] == 4000).all() and (got[0] <= 1).all()
    mask = (np.arange(4000) % 3 != 0).astype(np.uint8)
    _check(c["queries"], c["corpus"], "4000 masked", mask=mask, eligible="lower")


def test_workgroups_with_several_tiles():
    """16 workgroups of queries against 65 tiles of corpus: more than the 1024 workgroups the corpus split aims at, so
    a workgroup takes two tiles in turn.  With every entry eligible a query's outputs depend on its own row only: the
    reference is computed for the 64 distinct query rows and repeated."""
    c = lnr.big_case()
    corpus = np.concatenate([c["corpus"], c["corpus"][:160]])
    n = 3841
    src = np.arange(n) % 64
    mask = (np.arange(4160) % 5 != 1).astype(np.uint8)
    for m in (None, mask):
        want = lnr.nearest(c["queries"][:64], corpus, m)
        got = _nearest(c["queries"][src], corpus, m)
        for name, g, w in zip(NAMES, got, want):
            assert np.array_equal(g, w[src]), name


def test_argument_checks():
    from toued import _lib
    L = _lib.lib()
    c = lnr.case("debug")
    q = torch.from_numpy(c["queries"][:4].copy()).cuda()
    co = torch.from_numpy(c["corpus"][:9].copy()).cuda()
    out = torch.full((4, 4), -77, dtype=torch.int32, device="cuda")
    before = out.clone()

    def call(n=4, b=9, queries=q, corpus=co, eligible=0, outs=(0, 1, 2, 3)):
        o = [None if k is None else _lib.ptr(out[k]) for k in outs]
        return L.toued_level_nearest(_lib.ptr(queries), n, _lib.ptr(corpus), b, None, eligible, 1, *o,
                                     _lib.stream_ptr())
    for kw in (dict(n=-1), dict(b=-1), dict(b=65537), dict(eligible=3), dict(eligible=-1), dict(queries=None),
               dict(corpus=None), dict(outs=(None, 1, 2, 3)), dict(outs=(0, None, 2, 3)), dict(outs=(0, 1, None, 3)),
               dict(outs=(0, 1, 2, None))):
        assert call(**kw) == -1, kw
        assert b"toued_level_nearest" in L.toued_last_error(), kw
    assert call(n=0) == 0 and call(n=0, queries=None, corpus=None, outs=(None,) * 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    assert call(b=0, corpus=None) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[lnr.INT_MAX] * 4, [-1] * 4, [0] * 4, [0] * 4]
    assert call() == 0
    torch.cuda.synchronize()
    want = lnr.nearest(c["queries"][:4], c["corpus"][:9])
    assert all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in range(4))


def test_env_level_nearest_api():
    from toued.env import LevelNearest, level_nearest
    c = lnr.case("mazes")
    q, co = torch.from_numpy(c["queries"]).cuda(), torch.from_numpy(c["corpus"]).cuda()
    mask = torch.from_numpy(np.arange(len(c["corpus"])) % 2 == 0).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # a host synchronisation inside the call raises
    try:
        r = level_nearest(q, co)
        rm = level_nearest(q, co, mask, eligible="lower", include_lifetime=False)
        one = level_nearest(q[5], co)
        none = level_nearest(q[:0], co)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(r, LevelNearest)
    want = lnr.nearest(c["queries"], c["corpus"])
    wantm = lnr.nearest(c["queries"], c["corpus"], mask.cpu().numpy(), "lower", False)
    for k, f in enumerate(LevelNearest._fields):
        x = getattr(r, f)
        assert x.shape == (len(c["queries"]),) and x.dtype == torch.int32, f
        assert np.array_equal(x.cpu().numpy(), want[k]) and np.array_equal(getattr(rm, f).cpu().numpy(), wantm[k]), f
        assert getattr(one, f).shape == () and int(getattr(one, f)) == int(x[5]), f
        assert getattr(none, f).shape == (0,)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = level_nearest(q, co)
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(side, r))
    empty = level_nearest(q[:3], co[:0])
    assert empty.dist.tolist() == [lnr.INT_MAX] * 3 and empty.idx.tolist() == [-1] * 3
    assert empty.count.tolist() == [0] * 3 and empty.dist_sum.tolist() == [0] * 3
    for bad in (lambda: level_nearest(q[:, :64], co), lambda: level_nearest(q, co.long()),
                lambda: level_nearest(q, co, eligible="upper"), lambda: level_nearest(q, co, mask[:5]),
                lambda: level_nearest(q, co, mask.float())):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------- editor

def _edit(c, num_edits, ops=("walls", "objects", "start"), p_edit=1.0, **kw):
    from toued.env import LevelEditor, get_env_spec
    spec, _, _ = get_env_spec("debug")
    ed = LevelEditor(spec, list(ops), num_edits, p_edit, ler.REWARD_DELTA, **kw)
    buf = torch.from_numpy(c["buf_rows"]).cuda()
    rows = torch.from_numpy(c["gen_rows"].copy()).cuda()
    args = (buf, torch.from_numpy(c["parent_ids"]).cuda(), dk(c["keys"]), rows)
    rid = torch.from_numpy(c["reset_ids"]).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")            # no host synchronisation in the reset round
    try:
        flags = ed(*args, reset_ids=rid) if kw.get("min_distance") else ed(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.from_numpy(c["buf_rows"]))
    return ed, rows.cpu().numpy(), flags.cpu().numpy()


def test_editor_refuses_exact_copies():
    c = lnr.editor_case()
    ed, rows, flags = _edit(c, 0, min_distance=1)      # no edit: every child is its parent, a buffer level that stays
    assert np.array_equal(rows, c["gen_rows"])
    assert flags.dtype == np.uint8 and not flags.any()
    close = ed.last_too_close.cpu().numpy()
    assert close.dtype == np.uint8 and np.array_equal(close, (c["parent_ids"] >= 0).astype(np.uint8))
    assert ed.last_rejected is None
    # without the filter the same call keeps the copies
    ed0, rows0, flags0 = _edit(c, 0)
    assert np.array_equal(flags0, (c["parent_ids"] >= 0).astype(np.uint8)) and ed0.last_too_close is None
    assert lnr.nearest(rows0[flags0 != 0], c["buf_rows"])[0].max() == 0


def test_editor_distance_bound_refuses_every_child():
    c = lnr.editor_case()
    ed, rows, flags = _edit(c, 2, min_distance=303)
    assert np.array_equal(rows, c["gen_rows"]) and not flags.any()
    assert np.array_equal(ed.last_too_close.cpu().numpy(), (c["parent_ids"] >= 0).astype(np.uint8))


@pytest.mark.parametrize("D", [1, 2, 3])
def test_editor_with_real_edits_matches_reference(D):
    c = lnr.editor_case()
    children, edited = c["edit_rows"](2)
    want, kept, close = lnr.filter_children(children, edited, c["gen_rows"], c["buf_rows"], c["reset_ids"], D)
    # a wall, object or start edit changes one canonical coordinate, so two edits stay within distance 2 of the parent:
    # D = 3 refuses every child, and the case has children on both sides of D = 1 and D = 2
    assert close.any() and kept.any() == (D < 3)
    ed, rows, flags = _edit(c, 2, min_distance=D)
    assert np.array_equal(rows, want)
    assert np.array_equal(flags.astype(bool), kept)
    assert np.array_equal(ed.last_too_close.cpu().numpy().astype(bool), close)
    # with the solvable filter beside it: too_close marks only the rows that filter let through
    ed2, rows2, flags2 = _edit(c, 2, min_distance=D, require_solvable=True)
    rej = ed2.last_rejected.cpu().numpy().astype(bool)
    close2 = ed2.last_too_close.cpu().numpy().astype(bool)
    assert not (rej & close2).any() and np.array_equal(close2, close & ~rej)
    assert np.array_equal(flags2.astype(bool), edited & ~rej & ~close2)
    assert np.array_equal(rows2, np.where((rej | close2)[:, None], c["gen_rows"], children))


def test_editor_default_is_unchanged():
    c = lnr.editor_case()
    children, edited = c["edit_rows"](2)
    ed0, rows0, flags0 = _edit(c, 2, min_distance=0)
    ed1, rows1, flags1 = _edit(c, 2)
    assert np.array_equal(rows0, rows1) and np.array_equal(flags0, flags1) and np.array_equal(rows0, children)
    assert np.array_equal(flags0.astype(bool), edited) and ed0.last_too_close is None and ed0.last_rejected is None
    from toued.env import LevelEditor, get_env_spec
    ed = LevelEditor(get_env_spec("debug")[0], min_distance=1)
    with pytest.raises(ValueError, match="reset_ids"):
        ed(torch.from_numpy(c["buf_rows"]).cuda(), torch.from_numpy(c["parent_ids"]).cuda(), dk(c["keys"]),
           torch.from_numpy(c["gen_rows"].copy()).cuda())


# ---------------------------------------------------------------------------------------------- sampler

_FLAGS = ["--env_mode", "debug", "--score_function", "optimal_regret", "--buffer_size", "32", "--num_agents", "8",
          "--env_workers", "2", "--num_mini_batches", "1", "--level_editor", "accel", "--edit_prob", "1",
          "--num_edits", "1", "--edit_ops", "walls,objects,start"]
_N, _ROUNDS = 8, 4


def _sample_rounds(extra):
    from toued import prng
    from toued.env import L_LIFETIME
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    smp = LevelSampler(parse_args(_FLAGS + extra))
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, _N, False)
    rng = prng.PRNGKey(2, "cuda")
    rec = []
    for _ in range(_ROUNDS):
        agents.step = agents.levels[:, L_LIFETIME].clone()
        pre = {k: getattr(buf, k).cpu().numpy().copy() for k in ("levels", "score", "active", "new")}
        pre["rng"] = prng.to_uint32_numpy(rng)
        buf, agents = smp.sample(rng, buf, agents)
        torch.cuda.synchronize()
        pre["last_edit"] = {k: v.cpu().numpy() for k, v in smp.last_edit.items()}
        pre["after"] = buf.levels.cpu().numpy().copy()
        rec.append(pre)
        rng = prng.split(rng, 2)[1].contiguous()
    return rec


def test_sampler_with_the_filter():
    spec = olv.env_spec("debug")
    rec = _sample_rounds(["--edit_min_distance", "1"])
    n_close = n_kept = 0
    for r in rec:
        ids, _, _, _ = osp.reset_lowest_scoring(r["score"], r["active"], r["new"], _N)
        keys = jr.split(jr.split(r["rng"], 2)[1], _N)
        p_new, lt_new = olv.reset_env_params(keys, "debug")
        gen_rows = olv.pack_levels(p_new, lt_new, spec, buffer_id=ids)
        le = r["last_edit"]
        assert set(le) == {"parent", "edited", "too_close"} and le["too_close"].dtype == np.uint8
        children, edited, _ = ler.edit_rows(r["levels"], le["parent"], keys, gen_rows, spec, 1.0, 1, 7, 0.1)
        want, kept, close = lnr.filter_children(children, edited, gen_rows, r["levels"], ids, 1)
        assert np.array_equal(r["after"][ids], want)
        assert np.array_equal(le["edited"].astype(bool), kept) and np.array_equal(le["too_close"].astype(bool), close)
        # no kept child duplicates a level the buffer kept this round
        after = r["after"]
        assert (lnr.nearest(after[ids][kept], np.delete(after, ids, axis=0))[0] > 0).all()
        n_close += int(close.sum())
        n_kept += int(kept.sum())
    print(f"{n_kept} children kept, {n_close} too close over {_ROUNDS} rounds")
    assert n_kept >= 4 and n_close >= 1
    rec0 = _sample_rounds([])                                              # without the flag: no "too_close" entry
    assert set(rec0[-1]["last_edit"]) == {"parent", "edited"}


# ---------------------------------------------------------------------------------------------- end to end

_TRAIN = ["--env_mode", "debug", "--score_function", "positive_value_loss", "--level_editor", "accel",
          "--train_steps", "2", "--num_agents", "8", "--buffer_size", "32", "--env_workers", "32",
          "--num_mini_batches", "1"]


def _run(module, flags):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + flags, cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("level_nearest_ckpt"))
    return d, _run("toued.train", _TRAIN + ["--edit_min_distance", "1", "--buffer_diversity", "--checkpoint_dir", d])


def _checkpointed_rows(d):
    from toued.checkpoint import level_buffer_from_state_dict, restore_checkpoint
    from toued.env import get_env_spec
    spec, _, _ = get_env_spec("debug")
    state = restore_checkpoint(d, prefix="buffer_", step=None)
    return level_buffer_from_state_dict(state, spec, torch.device("cuda")).levels.cpu().numpy()


def test_train_cli_logs_buffer_diversity(trained):
    d, lines = trained
    assert [m["step"] for m in lines] == [0, 1]
    for m in lines:
        bf = m["buffer"]
        assert set(bf) == {"unique_frac", "nn_dist", "pair_dist", "edit_too_close"}
        assert all(math.isfinite(v) for v in bf.values()), bf
        assert 0.0 < bf["unique_frac"] <= 1.0 and 0.0 <= bf["nn_dist"] <= bf["pair_dist"] <= 302.0
        assert bf["edit_too_close"] == int(bf["edit_too_close"]) and 0 <= bf["edit_too_close"] <= 8
    want = lnr.diversity(_checkpointed_rows(d))
    assert {k: lines[-1]["buffer"][k] for k in want} == want


def test_train_cli_without_the_flags_has_no_buffer_key(trained):
    lines = _run("toued.train", _TRAIN)
    assert [m["step"] for m in lines] == [0, 1]
    assert all("buffer" not in m for m in lines)


def test_level_stats_cli_diversity(trained):
    d, _ = trained
    plain, = _run("toued.level_stats", ["--checkpoint_dir", d, "--env_mode", "debug"])
    out, = _run("toued.level_stats", ["--checkpoint_dir", d, "--env_mode", "debug", "--diversity"])
    assert not {"unique_frac", "nn_dist", "pair_dist"} & set(plain)
    want = lnr.diversity(_checkpointed_rows(d))
    assert {k: out[k] for k in want} == want
    assert {k: v for k, v in out.items() if k not in want} == plain
