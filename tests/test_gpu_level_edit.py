"""GPU: the ACCEL level editor (--level_editor accel).

  * toued_level_edit against the numpy restatement (tests/level_edit_ref.py), all 80 words of every row bit-exact, over
    the cases whose coverage tests/test_level_edit_cpu.py asserts
  * toued_plr_parent_ids against numpy
  * LevelSampler.sample with the editor: --edit_prob 0 is --level_editor none bit for bit; with --edit_prob 1 the reset
    slots hold the restatement's children of the recorded parents; run to run identical
  * edited levels as environment inputs: optimal_return against the float64 restatement (tests/optret_ref.py) with
    tests/test_gpu_optret.py's bound, policy_return below it
  * ``python -m toued.train --level_editor accel`` end to end
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
import optret_ref as orf
import polret_ref as prf
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle import sampler as osp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "to-ued_amd")


def dk(a):
    from toued.prng import from_uint32_numpy
    return from_uint32_numpy(a, "cuda")


def _edit(c, n, num_edits, mask, p_edit, with_flags=True):
    """toued_level_edit on the first n slots of a case -> (rows, edited or None) as numpy."""
    from toued import _lib
    spec = c["spec"]
    buf = torch.from_numpy(c["buf_rows"]).cuda()
    rows = torch.from_numpy(c["gen_rows"][:n].copy()).cuda()
    pids = torch.from_numpy(c["parent_ids"][:n].copy()).cuda()
    keys = dk(c["keys"][:n])
    flags = torch.full((n,), 7, dtype=torch.uint8, device="cuda") if with_flags else None
    _lib.call("toued_level_edit", _lib.ptr(buf), _lib.ptr(pids), _lib.ptr(keys), n, spec.max_n_objs,
              spec.max_n_obj_types, p_edit, num_edits, mask, ler.REWARD_DELTA, _lib.ptr(rows), _lib.ptr(flags),
              _lib.stream_ptr())
    assert torch.equal(buf.cpu(), torch.from_numpy(c["buf_rows"]))        # the buffer is read only
    return rows.cpu().numpy(), (flags.cpu().numpy() if with_flags else None)


def _assert_rows(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, bad[:4], [np.flatnonzero(got[b] != want[b]) for b in bad[:4]])


@pytest.mark.parametrize("num_edits,mask,p_edit", ler.CASE_CONFIGS)
@pytest.mark.parametrize("mode", ler.CASE_MODES)
def test_level_edit_matches_restatement(mode, num_edits, mask, p_edit):
    c = ler.case(mode)
    want, want_flags, _ = ler.case_reference(mode, num_edits, mask, p_edit)
    for n in (1, 63, 64, 65):
        got, flags = _edit(c, n, num_edits, mask, p_edit)
        _assert_rows(got, want[:n], (mode, n))
        assert np.array_equal(flags, want_flags[:n].astype(np.uint8)), (mode, n)
    # rows without a parent and rows whose coin says no come back untouched
    untouched = ~want_flags
    assert untouched[c["parent_ids"] < 0].all() and np.array_equal(got[untouched], c["gen_rows"][untouched])
    if p_edit == 1.0:
        assert want_flags.sum() == (c["parent_ids"] >= 0).sum() > 50
    # edited_out = NULL is accepted and changes nothing
    got_null, _ = _edit(c, 65, num_edits, mask, p_edit, with_flags=False)
    _assert_rows(got_null, want, (mode, "NULL flags"))


@pytest.mark.parametrize("name", ["full", "no_objs"])
def test_level_edit_hand_built_levels(name):
    c = ler.hand_case(name)
    want, want_flags, _ = c["ref"]
    got, flags = _edit(c, len(want), 8, 15, 1.0)
    _assert_rows(got, want, name)
    assert flags.all() and want_flags.all()


def test_level_edit_argument_checks():
    from toued import _lib
    L = _lib.lib()
    c = ler.case("debug")
    buf, rows = torch.from_numpy(c["buf_rows"]).cuda(), torch.from_numpy(c["gen_rows"][:4].copy()).cuda()
    pids, keys = torch.from_numpy(c["parent_ids"][:4].copy()).cuda(), dk(c["keys"][:4])
    before = rows.clone()

    def call(n=4, max_n=2, types=2, p=0.5, edits=1, mask=7):
        return L.toued_level_edit(_lib.ptr(buf), _lib.ptr(pids), _lib.ptr(keys), n, max_n, types, p, edits, mask, 0.1,
                                  _lib.ptr(rows), None, _lib.stream_ptr())
    for kw in (dict(n=-1), dict(edits=-1), dict(mask=0), dict(mask=16), dict(mask=-1), dict(p=-0.01), dict(p=1.01),
               dict(p=float("nan")), dict(max_n=-1), dict(max_n=9), dict(types=0), dict(types=6)):
        assert call(**kw) == -1, kw
        assert b"toued_level_edit" in L.toued_last_error(), kw
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows, before)
    assert call(p=0.0) == 0 and call(p=1.0, mask=15, max_n=0, types=1) == 0 and call(max_n=8, types=5) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- parents

def _parent_case(B, N, seed, frac_fresh):
    rs = np.random.RandomState(seed)
    score = (np.round(rs.randn(B) * 4) / 4).astype(np.float32)            # ties, negative scores
    score[rs.rand(B) < 0.1] = -0.0
    score[rs.rand(B) < 0.1] = 0.0
    fresh = rs.rand(B) < frac_fresh
    reset = rs.choice(B, N, replace=False).astype(np.int32)
    return score, fresh, reset


def _parents(score, fresh, reset):
    from toued import _lib
    s, f, r = (torch.from_numpy(x).cuda() for x in (score, fresh, reset))
    out = torch.full((len(reset),), -7, dtype=torch.int32, device="cuda")
    _lib.call("toued_plr_parent_ids", len(score), len(reset), _lib.ptr(s), _lib.ptr(f), _lib.ptr(r), _lib.ptr(out),
              _lib.stream_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("B,N,frac_fresh", [(1, 1, 0.0), (5, 2, 0.0), (5, 5, 0.0), (1024, 100, 0.3), (1025, 512, 0.3),
                                            (1025, 700, 0.9), (8192, 512, 0.3), (8192, 8000, 0.5), (4000, 512, 1.0)])
def test_parent_ids_match_numpy(B, N, frac_fresh):
    score, fresh, reset = _parent_case(B, N, 7 * B + N, frac_fresh)
    got = _parents(score, fresh, reset)
    want = ler.parent_ids(score, fresh, reset)
    assert np.array_equal(got, want)
    elig = ~fresh
    elig[reset] = False
    n_elig = int(elig.sum())
    if n_elig == 0:
        assert (got == -1).all()
    else:
        assert elig[got].all()                                            # never a reset slot, never a fresh one
        assert np.array_equal(got, got[np.arange(N) % n_elig])            # the wrap-around, where N > n_elig
        first = got[:min(N, n_elig)]
        assert len(set(first.tolist())) == len(first) and np.all(np.diff(score[first]) <= 0)      # best first


def test_parent_ids_cases_cover_wrap_and_empty():
    wraps = empties = 0
    for B, N, ff in [(1, 1, 0.0), (5, 5, 0.0), (1025, 700, 0.9), (8192, 8000, 0.5), (4000, 512, 1.0)]:
        score, fresh, reset = _parent_case(B, N, 7 * B + N, ff)
        elig = ~fresh
        elig[reset] = False
        wraps += 0 < elig.sum() < N
        empties += elig.sum() == 0
    assert wraps >= 2 and empties >= 3


def test_parent_ids_wrapper_and_argument_checks():
    from toued import _lib
    from toued.level_sampler import LevelBuffer
    from toued.plr import parent_ids
    score, fresh, reset = _parent_case(64, 8, 5, 0.4)
    buf = LevelBuffer(torch.zeros((64, 80), dtype=torch.int32, device="cuda"), torch.from_numpy(score).cuda(),
                      torch.zeros(64, dtype=torch.bool, device="cuda"), torch.from_numpy(fresh).cuda())
    got = parent_ids(buf, torch.from_numpy(reset).cuda())
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ler.parent_ids(score, fresh, reset))
    L = _lib.lib()
    for B, N in ((0, 0), (8193, 1), (4, 5), (4, -1)):
        assert L.toued_plr_parent_ids(B, N, None, None, None, None, None) == -1
        assert b"toued_plr_parent_ids" in L.toued_last_error()
    assert L.toued_plr_parent_ids(4, 0, None, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- sampler

_FLAGS = ["--env_mode", "debug", "--score_function", "optimal_regret", "--buffer_size", "32", "--num_agents", "8",
          "--env_workers", "2", "--num_mini_batches", "1"]
_N, _B = 8, 32


def _sample_rounds(extra, rounds=2):
    """``rounds`` rounds of LevelSampler.sample with every agent terminated, recording each round's inputs."""
    from toued import prng
    from toued.env import L_LIFETIME
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    smp = LevelSampler(parse_args(_FLAGS + extra))
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, _N, False)
    rng = prng.PRNGKey(2, "cuda")
    rec = []
    for _ in range(rounds):
        agents.step = agents.levels[:, L_LIFETIME].clone()
        pre = {k: getattr(buf, k).cpu().numpy().copy() for k in ("levels", "score", "active", "new")}
        pre["rng"] = prng.to_uint32_numpy(rng)
        buf, agents = smp.sample(rng, buf, agents)
        torch.cuda.synchronize()
        pre["last_edit"] = None if smp.last_edit is None else {k: v.cpu().numpy() for k, v in smp.last_edit.items()}
        pre["after"] = {k: getattr(buf, k).cpu().numpy().copy() for k in ("levels", "score", "active", "new")}
        rec.append(pre)
        rng = prng.split(rng, 2)[1].contiguous()
    return smp, buf, agents, rec


def _state(buf, agents):
    return [buf.levels, buf.score, buf.active, buf.new, agents.levels, agents.theta, agents.phi, agents.state,
            agents.step]


def test_sampler_edit_prob_zero_is_the_generator_path():
    _, b0, a0, _ = _sample_rounds([])
    smp, b1, a1, rec = _sample_rounds(["--level_editor", "accel", "--edit_prob", "0"])
    for x, y in zip(_state(b0, a0), _state(b1, a1)):
        assert torch.equal(x, y)
    assert smp.last_edit is not None and not rec[-1]["last_edit"]["edited"].any()
    assert (rec[-1]["last_edit"]["parent"] >= 0).all()                    # parents were there; the coin said no


def test_sampler_reset_slots_hold_the_children():
    from toued import prng
    from toued.plr import reset_lowest_scoring
    extra = ["--level_editor", "accel", "--edit_prob", "1", "--num_edits", "3", "--edit_ops",
             "walls,objects,start,rewards"]
    smp, buf, agents, rec = _sample_rounds(extra)
    spec = olv.env_spec("debug")

    def check(pre, after_levels, last_edit, reset_key, expect_children):
        ids, _, _, _ = osp.reset_lowest_scoring(pre["score"], pre["active"], pre["new"], _N)
        keys = jr.split(reset_key, _N)
        p_new, lt_new = olv.reset_env_params(keys, "debug")
        gen_rows = olv.pack_levels(p_new, lt_new, spec, buffer_id=ids)
        parents = last_edit["parent"]
        assert np.array_equal(parents, ler.parent_ids(pre["score"], pre["new"], ids))
        want, edited, _ = ler.edit_rows(pre["levels"], parents, keys, gen_rows, spec, 1.0, 3, 15, 0.1)
        assert np.array_equal(last_edit["edited"].astype(bool), edited)
        assert edited.all() == expect_children and edited.any() == expect_children
        _assert_rows(after_levels[ids], want, "reset slots")
        assert np.array_equal(after_levels[ids, olv.L_BUFID], ids)
        if expect_children:
            assert (want != gen_rows).any(axis=1).all()                   # the children are not the generated levels
        return ids

    # round 1: the whole buffer is new, nothing has a score, so there are no parents and the generator's levels stay
    r0, r1 = rec
    check(r0, r0["after"]["levels"], r0["last_edit"], jr.split(r0["rng"], 2)[1], False)
    assert (r0["last_edit"]["parent"] == -1).all()
    # round 2: the eight levels scored in round 1 are the parents
    ids = check(r1, r1["after"]["levels"], r1["last_edit"], jr.split(r1["rng"], 2)[1], True)
    assert r1["after"]["new"][ids].all()
    untouched = np.setdiff1d(np.arange(_B), ids)
    assert np.array_equal(r1["after"]["levels"][untouched], r1["levels"][untouched])
    # the reset itself, straight: the children land new, inactive and with score 0
    pre = {k: getattr(buf, k).cpu().numpy().copy() for k in ("levels", "score", "active", "new")}
    key = prng.PRNGKey(77, "cuda")
    got_ids = reset_lowest_scoring(smp, key, buf, _N).cpu().numpy()
    torch.cuda.synchronize()
    last = {k: v.cpu().numpy() for k, v in smp.last_edit.items()}
    ids = check(pre, buf.levels.cpu().numpy(), last, prng.to_uint32_numpy(key), True)
    assert np.array_equal(got_ids, ids)
    assert buf.new.cpu().numpy()[ids].all() and not buf.active.cpu().numpy()[ids].any()
    assert not buf.score.cpu().numpy()[ids].any()


def test_sampler_with_editor_is_deterministic():
    extra = ["--level_editor", "accel", "--edit_prob", "1", "--edit_ops", "walls,objects,start,rewards"]
    _, b0, a0, r0 = _sample_rounds(extra)
    _, b1, a1, r1 = _sample_rounds(extra)
    for x, y in zip(_state(b0, a0), _state(b1, a1)):
        assert torch.equal(x, y)
    assert r0[-1]["last_edit"]["edited"].all()
    assert np.array_equal(r0[-1]["last_edit"]["parent"], r1[-1]["last_edit"]["parent"])


# ---------------------------------------------------------------------------------------------- children in the env

def test_children_as_environment_inputs():
    """Edited ``all`` levels through the exact-return kernels: optimal_return within tests/test_gpu_optret.py's bound
    H * 2^-23 * max(1, max|v|) of the float64 restatement (H = min(max_steps, L) backups), and policy_return of random
    tables not above optimal_return by more than that bound."""
    from toued.rollout import RolloutWrapper
    mode, L = "all", 60
    c = ler.case(mode)
    spec = c["spec"]
    rows, edited, _ = ler.case_reference(mode, 8, 15, 1.0)
    sel = np.flatnonzero(edited & (rows != c["buf_rows"][np.maximum(c["parent_ids"], 0)]).any(axis=1))[:6]
    assert len(sel) == 6
    got_rows, _ = _edit(c, ler.CASE_N, 8, 15, 1.0)
    levels = torch.from_numpy(got_rows[sel]).cuda()
    params, _, _ = ler.unpack(rows[sel], spec)
    ro = RolloutWrapper(mode, 20)
    v_opt = ro.optimal_return(levels, L).cpu().numpy().astype(np.float64)
    theta = torch.from_numpy(prf.random_tables(5, len(sel), ro.obs_dim)).cuda()
    v_pol = ro.policy_return(levels, theta, L).cpu().numpy().astype(np.float64)
    for i in range(len(sel)):
        v = orf.optimal_return_all(spec, params, i, L)
        ref0 = v[0, orf.start_index(spec, params, i)]
        vmax = np.abs(v[np.isfinite(v)]).max(initial=0.0)
        bound = min(int(params["max_steps_in_episode"][i]), L) * 2.0 ** -23 * max(1.0, float(vmax))
        print(f"level {sel[i]}: v* gpu {v_opt[i]!r} f64 {ref0!r} v_pi {v_pol[i]!r} bound {bound:.3e}")
        assert np.isfinite(ref0) and abs(v_opt[i] - ref0) <= bound, (i, v_opt[i], ref0, bound)
        assert np.isfinite(v_pol[i]) and v_pol[i] - v_opt[i] <= bound, (i, v_pol[i], v_opt[i], bound)


# ---------------------------------------------------------------------------------------------- end to end

def _numbers(x):
    if isinstance(x, dict):
        for v in x.values():
            yield from _numbers(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _numbers(v)
    elif isinstance(x, (int, float)) and not isinstance(x, bool):
        yield float(x)


def test_train_cli_with_the_editor():
    """Three meta-steps of the training driver with the editor on, in a child process.  --env_workers is 32, the
    fewest the meta-gradient step takes (its GRU row blocks hold 32 workers; toued.meta raises below that, editor or
    not)."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "toued.train", "--env_mode", "debug", "--score_function", "optimal_regret",
           "--level_editor", "accel", "--num_agents", "8", "--buffer_size", "32", "--env_workers", "32",
           "--num_mini_batches", "1", "--train_steps", "3"]
    r = subprocess.run(cmd, cwd=PKG, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [m["step"] for m in lines] == [0, 1, 2]
    for m in lines:
        vals = list(_numbers(m))
        assert len(vals) > 2 and all(math.isfinite(v) for v in vals), m
