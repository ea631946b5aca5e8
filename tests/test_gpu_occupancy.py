"""GPU: toued_policy_occupancy / RolloutWrapper.policy_occupancy against the float64 restatement
tests/occupancy_ref.py, its duality with RolloutWrapper.policy_return, the env's own rollouts, and the policy scores
with --policy_score_eval exact.

The cases, levels and actor tables are test_gpu_polret.py's (the zero table on level 0, the +-1e4 table on level 1).
The float64 restatement is evaluated on every level of debug10, debug3, small and hand, on the first four levels of
`all` (one object, five objects, two more) and on the first level of `tabular`; every level of every case goes through
the checks that need no restatement (no NaN, conservation, and the duality with policy_return).

Comparison per level: |gpu - f64| <= 2^-23 * max(1, scale), the scale being the reference value itself for visits,
occ_all, collected and the summary columns 1-6 (all their terms are non-negative) and ret_abs for column 0.  The
kernel's sums are f64; its mass is fixed point with an error below H * (contributions per state) * 2^-62; an output's
single f32 rounding is 2^-24 relative; the factor 2 is the margin.  Measured largest error over all cases: 0.482 of
the bound.
"""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import occupancy_ref as ocr
import optret_ref as orf
import polret_ref as prf
from oracle import jaxrand as jr
from oracle import levels as olv
from test_gpu_optret import HAND_SPEC, _dev_levels, _spec
from test_gpu_polret import CASES, _bound, _case, _tables, mc_case
from test_gpu_polret import _reference as _polret_reference

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EPS = 2.0 ** -23
REF_LEVELS = {"all": (0, 1, 2, 3), "tabular": (0,)}      # the other cases: every level


class _AbiWrapper:
    """RolloutWrapper.policy_occupancy's call for a table size that no mode has, straight on the C ABI."""

    def __init__(self, spec):
        self.spec, self.obs_dim = spec, spec.obs_dim

    def policy_occupancy(self, levels, theta, L, return_all=False):
        from toued import _lib
        from toued.rollout import PolicyOccupancy
        n, S = levels.shape[0], self.obs_dim - 1
        summary = torch.zeros((n, 8), device="cuda")
        visits = torch.zeros((n, S), device="cuda")
        collected = torch.zeros((n, self.spec.max_n_objs), device="cuda")
        occ_all = torch.empty((n, L, S), device="cuda") if return_all else None
        _lib.call("toued_policy_occupancy", _lib.ptr(levels), _lib.ptr(theta), n, self.obs_dim,
                  self.spec.max_grid_size, self.spec.max_n_objs, 1, L, _lib.ptr(summary), _lib.ptr(visits),
                  _lib.ptr(collected), _lib.ptr(occ_all), _lib.stream_ptr())
        return PolicyOccupancy(*summary.unbind(dim=1), visits, collected, occ_all)

    def policy_return(self, levels, theta, L):
        from test_gpu_polret import _AbiWrapper as PolretAbi
        return PolretAbi(self.spec).policy_return(levels, theta, L)


def _wrapper(mode):
    from toued.rollout import RolloutWrapper
    return _AbiWrapper(HAND_SPEC) if mode is None else RolloutWrapper(mode, 20)


def _ref_levels(name):
    _, params, _, _ = _case(name)
    return REF_LEVELS.get(name, tuple(range(params["start_pos"].shape[0])))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """{level: occupancy_ref.Occupancy} of the case's compared levels: computed once, never modified."""
    mode, params, L, _ = _case(name)
    spec, th = _spec(mode), _tables(name)
    return {i: ocr.occupancy(spec, params, i, th[i], L) for i in _ref_levels(name)}


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """The case on the GPU, as float64 numpy: (summary [n, 8], visits [n, S], collected [n, n_max]) and the f32
    policy_return of the same inputs."""
    mode, params, L, _ = _case(name)
    levels = _dev_levels(params, _spec(mode))
    theta = torch.from_numpy(_tables(name).copy()).cuda()
    ro = _wrapper(mode)
    occ = ro.policy_occupancy(levels, theta, L)
    n = levels.shape[0]
    assert occ.occ_all is None and all(x.shape == (n,) and x.dtype == torch.float32 for x in occ[:8])
    assert occ.visits.shape == (n, ro.obs_dim - 1) and occ.collected.shape == (n, ro.spec.max_n_objs)
    summary = torch.stack(list(occ[:8]), dim=1).cpu().numpy().astype(np.float64)
    return (summary, occ.visits.cpu().numpy().astype(np.float64), occ.collected.cpu().numpy().astype(np.float64),
            ro.policy_return(levels, theta, L).cpu().numpy().astype(np.float64))


def _close(what, got, ref, scale=None):
    """max |got - ref| against 2^-23 * max(1, scale), elementwise; the scale is the reference value by default."""
    scale = np.abs(ref) if scale is None else scale
    err = np.abs(got - ref)
    bound = EPS * np.maximum(1.0, scale)
    worst = float((err / bound).max(initial=0.0))
    print(f"{what}: max |gpu - f64| / bound = {worst:.3f} (max err {float(err.max(initial=0.0)):.3e})")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("name", CASES)
def test_occupancy_matches_float64(name):
    mode, params, L, all_idx = _case(name)
    spec = _spec(mode)
    summary, visits, collected, _ = _gpu(name)
    assert not np.isnan(summary).any() and not np.isnan(visits).any() and not np.isnan(collected).any()
    ref = _reference(name)
    for i, r in ref.items():
        _close(f"level {i} ret", summary[i, 0], r.summary[0], r.summary[7])
        _close(f"level {i} summary 1-7", summary[i, 1:], r.summary[1:])
        _close(f"level {i} visits", visits[i], r.visits)
        _close(f"level {i} collected", collected[i], r.collected)
        assert not visits[i][orf.invalid_states(spec, params, i)].any(), i          # zeros exactly
        assert not collected[i][int(params["n_objs"][i]):].any(), i
    idx = [i for i in all_idx if i in ref]
    if idx:
        sel = torch.tensor(idx, device="cuda")
        levels = _dev_levels(params, spec)[sel].contiguous()
        theta = torch.from_numpy(_tables(name).copy()).cuda()[sel].contiguous()
        occ = _wrapper(mode).policy_occupancy(levels, theta, L, return_all=True)
        rows = occ.occ_all.cpu().numpy().astype(np.float64)
        assert rows.shape == (len(idx), L, spec.obs_dim - 1) and not np.isnan(rows).any()
        for j, i in enumerate(idx):
            _close(f"level {i} occ_all", rows[j], ref[i].rows)
            assert not rows[j][:, orf.invalid_states(spec, params, i)].any(), i      # zeros exactly
            assert not rows[j][min(int(params["max_steps_in_episode"][i]), L):].any(), i
            # the other outputs do not depend on whether the rows are asked for
            assert np.array_equal(occ.visits[j].cpu().numpy(), visits[i].astype(np.float32))
            assert np.array_equal(torch.stack(list(occ[:8]), dim=1)[j].cpu().numpy(), summary[i].astype(np.float32))


@pytest.mark.parametrize("name", CASES)
def test_duality_with_policy_return_and_conservation(name):
    """On every level of the case: summary.ret against RolloutWrapper.policy_return on the same inputs, within
    policy_return's own bound (test_gpu_polret._bound) plus 2^-23 * max(1, ret_abs); the episode ends by termination
    or is alive at the end, and the length is the sum of the visits (f32 outputs of f64 sums: 2^-23 relative each,
    the visits' sum over at most S terms)."""
    _, params, L, _ = _case(name)
    summary, visits, _, vpi = _gpu(name)
    _, _, vmax = _polret_reference(name)
    for i in range(summary.shape[0]):
        ret, length, early, alive, ent, lc, mm, ret_abs = summary[i]
        tol = _bound(params, i, L, vmax[i]) + EPS * max(1.0, ret_abs)
        print(f"level {i}: ret {ret!r} policy_return {vpi[i]!r} tolerance {tol:.3e}")
        assert abs(ret - vpi[i]) <= tol, (i, ret, vpi[i], tol)
        assert abs(early + alive - 1.0) <= 2 * EPS, (i, early, alive)
        assert abs(visits[i].sum() - length) <= 2 * EPS * max(1.0, length), (i, length)
        H = min(int(params["max_steps_in_episode"][i]), L)
        assert 1.0 - EPS <= length <= H * (1 + EPS) and 0.0 <= min(ent, lc, mm) and max(ent, lc, mm) <= 1.0 + EPS


def test_deterministic_single_level_form_and_batch_independence():
    from toued.rollout import RolloutWrapper
    mode, params, L, _ = _case("small")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("small").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))
    a, b = ro.policy_occupancy(levels, theta, L, return_all=True), ro.policy_occupancy(levels, theta, L,
                                                                                       return_all=True)
    assert same(a, b)
    s = ro.policy_occupancy(levels, theta, L)
    assert s.occ_all is None and same(s[:10], a[:10])
    one = ro.policy_occupancy(levels[3], theta[3], L, return_all=True)
    assert one.ret.dim() == 0 and one.visits.shape == (ro.obs_dim - 1,) and one.occ_all.shape == (L, ro.obs_dim - 1)
    assert one.collected.shape == (ro.spec.max_n_objs,) and same(one, [x[3] for x in a])
    # a level's result does not depend on the batch it is in, nor on its place there
    alone = ro.policy_occupancy(levels[5:6].contiguous(), theta[5:6].contiguous(), L, return_all=True)
    assert same(alone, [x[5:6] for x in a])
    back = ro.policy_occupancy(levels.flip(0).contiguous(), theta.flip(0).contiguous(), L, return_all=True)
    assert same([x.flip(0) for x in back], a)


def test_empty_batch_and_zero_length():
    from toued.rollout import RolloutWrapper
    mode, params, _, _ = _case("debug10")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("debug10").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    e = ro.policy_occupancy(levels[:0].contiguous(), theta[:0].contiguous(), 10, return_all=True)
    assert e.ret.shape == (0,) and e.visits.shape == (0, ro.obs_dim - 1) and e.occ_all.shape == (0, 10, ro.obs_dim - 1)
    z = ro.policy_occupancy(levels, theta, 0, return_all=True)
    assert z.occ_all.shape == (64, 0, ro.obs_dim - 1)
    assert all(x.shape[0] == 64 and not x.any() for x in z[:10])


def test_argument_errors():
    from toued import _lib
    levels = torch.zeros((1, 80), dtype=torch.int32, device="cuda")
    theta = torch.zeros((1, 4 * 4 * 4 + 1, 5), device="cuda")
    sm = torch.zeros((1, 8), device="cuda")
    fn = _lib.lib().toued_policy_occupancy
    err = lambda: _lib.lib().toued_last_error().decode()
    P, st = _lib.ptr, _lib.stream_ptr()
    assert fn(P(levels), P(theta), 1, 65, 4, 2, 0, 10, P(sm), None, None, None, st) == -1
    assert "unsupported" in err()
    assert fn(P(levels), P(theta), 1, 64, 4, 2, 1, 10, P(sm), None, None, None, st) == -1
    assert "D=64" in err()
    assert fn(P(levels), P(theta), -1, 65, 4, 2, 1, 10, P(sm), None, None, None, st) == -1
    assert fn(P(levels), P(theta), 1, 65, 4, 2, 1, -1, P(sm), None, None, None, st) == -1
    assert fn(P(levels), P(theta), 1, 17 * 17 * 4 + 1, 17, 2, 1, 10, P(sm), None, None, None, st) == -1
    assert fn(P(levels), P(theta), 1, (16 << 9) + 1, 4, 9, 1, 10, P(sm), None, None, None, st) == -1
    assert fn(P(levels), P(theta), 1, 65, 4, 2, 1, 10, None, None, None, None, st) == -1
    assert "summary" in err()
    assert fn(P(levels), P(theta), 1, (256 << 8) + 1, 16, 8, 1, 10, P(sm), None, None, None, st) == -1
    assert "LDS" in err()
    assert fn(P(levels), P(theta), 1, (14 * 14 << 5) + 1, 14, 5, 1, 10, P(sm), None, None, None, st) == -1
    assert "states per thread" in err()
    # every nullable output absent: the summary alone
    assert fn(P(levels), P(theta), 1, 65, 4, 2, 1, 10, P(sm), None, None, None, st) == 0
    torch.cuda.synchronize()


def test_every_tabular_mode_fits():
    """One level of every tabular mode of toued/modes.py goes through (the LDS budget check admits them all, and
    every count of work items per thread that a mode has is run), and its 5 steps match the reference."""
    from toued import modes
    from toued.rollout import RolloutWrapper
    for k, (mode, kw) in enumerate(modes.ENV_MODE_KWARGS.items()):
        if not kw["tabular"]:
            continue
        spec = olv.env_spec(mode)
        params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(7), 1), mode)
        theta = prf.random_tables(3000 + k, 1, spec.obs_dim)
        ro = RolloutWrapper(mode, 20)
        got = ro.policy_occupancy(_dev_levels(params, spec), torch.from_numpy(theta).cuda(), 5, return_all=True)
        ref = ocr.occupancy(spec, params, 0, theta[0], 5)
        f = lambda x: x[0].cpu().numpy().astype(np.float64)
        _close(f"{mode} occ_all", f(got.occ_all), ref.rows)
        _close(f"{mode} visits", f(got.visits), ref.visits)
        _close(f"{mode} collected", f(got.collected), ref.collected)
        summary = torch.stack(list(got[:8]), dim=1)
        _close(f"{mode} ret", f(summary)[0], ref.summary[0], ref.summary[7])
        _close(f"{mode} summary 1-7", f(summary)[1:], ref.summary[1:])


# ------------------------------------------------------------------------------------ against sampled rollouts
def test_episode_length_agrees_with_eval_rollouts():
    """test_gpu_polret.mc_case(): 4 `small` levels, 16 x 64 = 1024 eval workers each.  The sampled length of a
    worker's first episode (the steps up to and including the first done of a batch_rollout(eval=True) trajectory,
    the whole trajectory when there is none) against the exact ``length``, within polret_ref.mc_tolerance's form:
    5 standard errors of the sample plus 8 H / M (a length is at most H = eval_rollout_len)."""
    from toued import prng
    from toued.agents import eval_agent_reset
    from toued.rollout import RolloutWrapper
    from test_gpu_polret import MC_COPIES, MC_LEVELS, MC_WORKERS
    spec, params, theta, keys = mc_case()
    ro = RolloutWrapper("small", 20)
    T = ro.eval_rollout_len
    levels = _dev_levels(params, spec)
    th = torch.from_numpy(theta).cuda()
    exact = ro.policy_occupancy(levels, th, T).length.cpu().numpy().astype(np.float64)
    sel = torch.from_numpy(np.repeat(np.arange(MC_LEVELS), MC_COPIES)).cuda()
    lv, tt = levels[sel].contiguous(), th[sel].contiguous()
    state, rkeys = eval_agent_reset(ro, prng.from_uint32_numpy(keys, "cuda"), lv, MC_WORKERS)
    tr, _, _ = ro.batch_rollout(rkeys, tt, lv, state, eval=True)
    done = tr.done.cpu().numpy().astype(bool)                      # [N, T, W]
    first = np.where(done.any(axis=1), done.argmax(axis=1) + 1, T)   # [N, W]
    first = first.reshape(MC_LEVELS, MC_COPIES * MC_WORKERS).astype(np.float64)
    M = first.shape[1]
    for i in range(MC_LEVELS):
        mean = float(first[i].mean())
        tol = 5.0 * float(np.std(first[i], ddof=1)) / np.sqrt(M) + 8.0 * T / M
        print(f"level {i}: sampled {mean:.4f} exact {exact[i]:.4f} tolerance {tol:.4f}")
        assert abs(mean - exact[i]) <= tol, (i, mean, exact[i], tol)


# ------------------------------------------------------------------------------------- --policy_score_eval exact
NAMES = ("policy_entropy", "least_confidence", "min_margin")


def _sampler(score_function, extra=(), N=8, B=16):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "small", "--score_function", score_function, "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B), *extra])
    return LevelSampler(args)


def _agents(N, seed):
    from toued import prng
    from toued.agents import create_agents
    from toued.env import LevelGenerator
    dk = lambda a: prng.from_uint32_numpy(a, "cuda")
    levels = LevelGenerator("small")(dk(jr.split(jr.PRNGKey(seed), N)))
    theta, _ = create_agents(dk(jr.split(jr.PRNGKey(seed + 1), N)), olv.env_spec("small").obs_dim, 8)
    theta.mul_(10.0)
    return levels, theta


def test_exact_policy_scores_are_the_summary_columns():
    from toued import plr, prng
    N = 8
    smp = _sampler("policy_entropy", ["--policy_score_eval", "exact"], N)
    ro = smp.rollout_manager
    levels, theta = _agents(N, 501)
    got = plr.exact_policy_scores(smp, levels, theta)
    occ = ro.policy_occupancy(levels, theta, ro.eval_rollout_len)
    for g, want in zip(got, (occ.entropy, occ.least_confidence, occ.min_margin)):
        assert g.shape == (N,) and g.dtype == torch.float32 and torch.equal(g, want)
    # the score functions take them, whatever the keys
    for j, name in enumerate(NAMES):
        for seed in (503, 504):
            keys = prng.from_uint32_numpy(jr.split(jr.PRNGKey(seed), N), "cuda")
            assert torch.equal(plr.SCORE_CALLS[name](smp, keys, levels, theta), got[j])
    assert all(x.shape == (0,) for x in plr.exact_policy_scores(smp, levels[:0], theta[:0]))
    # next to the sampled scores of the same agents: the same quantity up to the truncated last episode and the
    # sampling noise of 64 workers x 100 steps (printed, not asserted: the exact score is not the sampled one's mean)
    smp2 = _sampler("policy_entropy", (), N)
    keys = prng.from_uint32_numpy(jr.split(jr.PRNGKey(503), N), "cuda")
    sampled = plr.policy_scores(smp2, keys, levels, theta)
    for name, e, s in zip(NAMES, got, sampled):
        print(name, "exact", e.cpu().numpy().round(4), "sampled", s.cpu().numpy().round(4))


@pytest.mark.parametrize("name", NAMES)
def test_level_sampler_exact_scores_the_buffer_without_an_eval_rollout(name, monkeypatch):
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    N, B = 8, 16
    smp = _sampler(name, ["--policy_score_eval", "exact"], N, B)
    ro = smp.rollout_manager
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    agents.step = agents.levels[:, L_LIFETIME].clone()           # every agent has reached its lifetime
    levels0, theta0 = agents.levels.clone(), agents.theta.clone()
    old_ids = agents.levels[:, L_BUFID].long().clone()
    field = {"policy_entropy": "entropy"}.get(name, name)
    want = getattr(ro.policy_occupancy(levels0, theta0, ro.eval_rollout_len), field)

    def no_eval(*a, **k):
        raise AssertionError("an eval rollout was started with --policy_score_eval exact")

    for fn in ("batch_rollout", "eval_returns", "eval_returns_from_draws", "eval_draws", "policy_scores"):
        monkeypatch.setattr(ro, fn, no_eval)
    buf, agents = smp.sample(prng.PRNGKey(2, "cuda"), buf, agents)
    assert torch.equal(smp.last_plr["score"], want)
    assert torch.equal(buf.score[old_ids], want)


def test_default_sampled_scores_are_unchanged():
    """Without the flag (and with it spelled ``sampled``) the policy scores are RolloutWrapper.policy_scores of the
    eval trajectory, bit for bit: the sampler built from arguments that lack the flag altogether gives the same."""
    from toued import plr, prng
    from toued.level_sampler import LevelSampler
    N = 8
    levels, theta = _agents(N, 511)
    keys = prng.from_uint32_numpy(jr.split(jr.PRNGKey(513), N), "cuda")
    plain = _sampler("min_margin", (), N)
    spelled = _sampler("min_margin", ["--policy_score_eval", "sampled"], N)
    del plain.args.policy_score_eval
    legacy = LevelSampler(plain.args)                              # an args namespace from before the flag
    assert legacy.policy_score_eval == "sampled"
    a = plr.policy_scores(plain, keys, levels, theta)
    ro = plain.rollout_manager
    chunks = list(plr._eval_trajectory_chunks(plain, keys, levels, theta, None))
    assert len(chunks) == 1
    direct = ro.policy_scores(chunks[0][2], theta)
    for x, y, z, w in zip(a, plr.policy_scores(spelled, keys, levels, theta),
                          plr.policy_scores(legacy, keys, levels, theta), direct):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)


def test_train_cli_exact_policy_entropy_with_occupancy_metrics():
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([str(ROOT / "to-ued_amd"), str(ROOT), env.get("PYTHONPATH", "")])
    cmd = [sys.executable, "-m", "toued.train", "--env_mode", "small", "--num_agents", "8", "--num_mini_batches", "1",
           "--score_function", "policy_entropy", "--policy_score_eval", "exact", "--occupancy_metrics",
           "--train_steps", "2", "--buffer_size", "16"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for m in lines:
        occ = m["occupancy"]
        assert set(occ) == {"episode_len", "p_early_term", "exact_return", "collect_pos", "collect_neg",
                            "cell_coverage"}
        assert all(np.isfinite(v) for v in occ.values()), occ
        assert 0.0 < occ["cell_coverage"] <= 1.0 and 1.0 <= occ["episode_len"] <= 100.0
        assert 0.0 <= occ["p_early_term"] <= 1.0 and occ["collect_pos"] >= 0.0 and occ["collect_neg"] >= 0.0
