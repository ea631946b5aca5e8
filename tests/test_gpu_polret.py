"""GPU: toued_policy_return / RolloutWrapper.policy_return against the float64 restatement tests/polret_ref.py, and
the regret scores with --regret_eval exact.

The cases are test_gpu_optret.py's (_case; its one `hand` level three times, for three tables).  Every level has its
own actor table: N(0, 2^2) entries with the time row scaled by 30, from a fixed seed; level 0 of a case has theta = 0
(the uniform policy) and level 1 has a tenth of its entries at +-1e4 (a policy that is one-hot to the last bit in most
states; no NaN may come of it).

Comparison per level, with H = min(max_steps_in_episode, max_rollout_len) backups: the finite masks equal; on the
finite entries |gpu - f64| <= H * 2^-23 * max(1, max|v64|), test_gpu_optret.py's bound (the policy is evaluated in f64
on both sides and a policy backup is a convex combination of the q, a max-norm non-expansion like the max); the -inf
entries and the zero rows exact.
"""
import functools

import numpy as np
import pytest
import torch

import optret_ref as orf
import polret_ref as prf
from oracle import jaxrand as jr
from oracle import levels as olv
from test_gpu_optret import HAND_SPEC, _dev_levels, _spec
from test_gpu_optret import _case as _opt_case
from test_gpu_optret import _reference as _opt_reference

pytestmark = pytest.mark.gpu

CASES = ["debug10", "debug3", "small", "all", "tabular", "hand"]


def _case(name):
    """test_gpu_optret.py's case; `hand`, a single level there, three times over, so that it is run under the zero
    table, the +-1e4 table and a random one (its two objects on one cell get unequal policy weights)."""
    mode, params, L, all_idx = _opt_case(name)
    if name == "hand":
        return mode, orf.concat_params([params] * 3), L, (0, 1, 2)
    return mode, params, L, all_idx


@functools.lru_cache(maxsize=None)
def _tables(name):
    """f32 [n, D, 5] of the case's levels (never modified)."""
    mode, params, _, _ = _case(name)
    n, D = params["start_pos"].shape[0], _spec(mode).obs_dim
    th = prf.random_tables(1000 + CASES.index(name), n, D)
    th[0] = 0.0
    if n > 1:
        rng = np.random.default_rng(2000 + CASES.index(name))
        big = rng.random(th[1].shape) < 0.1
        th[1][big] = np.where(rng.random(th[1].shape) < 0.5, -1e4, 1e4).astype(np.float32)[big]
    th.setflags(write=False)
    return th


class _AbiWrapper:
    """RolloutWrapper.policy_return's calls for a table size that no mode has, straight on the C ABI."""

    def __init__(self, spec):
        self.spec, self.obs_dim = spec, spec.obs_dim

    def policy_return(self, levels, theta, L, return_all=False):
        from toued import _lib
        n = levels.shape[0]
        v0 = torch.zeros(n, device="cuda")
        va = torch.empty((n, L, self.obs_dim - 1), device="cuda") if return_all else None
        _lib.call("toued_policy_return", _lib.ptr(levels), _lib.ptr(theta), n, self.obs_dim, self.spec.max_grid_size,
                  self.spec.max_n_objs, 1, L, _lib.ptr(v0), _lib.ptr(va), _lib.stream_ptr())
        return va if return_all else v0


def _wrapper(mode):
    from toued.rollout import RolloutWrapper
    return _AbiWrapper(HAND_SPEC) if mode is None else RolloutWrapper(mode, 20)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 v_all of the levels whose table is compared, v_0(start) and max|v| over the finite table entries of
    every level: computed once."""
    mode, params, L, all_idx = _case(name)
    spec, th = _spec(mode), _tables(name)
    n = params["start_pos"].shape[0]
    v_all, v0, vmax = {}, np.zeros(n), np.zeros(n)
    for i in range(n):
        v = prf.policy_return_all(spec, params, i, th[i], L)
        v0[i] = v[0, orf.start_index(spec, params, i)] if L > 0 else 0.0
        vmax[i] = np.abs(v[np.isfinite(v)]).max(initial=0.0)
        if i in all_idx:
            v_all[i] = v
    return v_all, v0, vmax


def _bound(params, i, L, vmax):
    H = min(int(params["max_steps_in_episode"][i]), L)
    return H * 2.0 ** -23 * max(1.0, float(vmax))


def _check_table(got, ref, params, i, L, vmax):
    got = got.astype(np.float64)
    fin = np.isfinite(ref)
    assert not np.isnan(got).any(), i
    assert np.array_equal(np.isfinite(got), fin), i
    assert np.array_equal(got[~fin], ref[~fin]), i                    # -inf exactly
    ms = int(params["max_steps_in_episode"][i])
    assert not got[ms:].any(), i                                      # zero rows exactly
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    bound = _bound(params, i, L, vmax)
    print(f"level {i}: max|gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (i, err, bound)


@pytest.mark.parametrize("name", CASES)
def test_policy_return_matches_float64(name):
    mode, params, L, all_idx = _case(name)
    spec = _spec(mode)
    ref_all, ref0, vmax = _reference(name)
    levels = _dev_levels(params, spec)
    theta = torch.from_numpy(_tables(name).copy()).cuda()
    ro = _wrapper(mode)
    v0 = ro.policy_return(levels, theta, L)
    assert v0.shape == (levels.shape[0],) and v0.dtype == torch.float32
    v0 = v0.cpu().numpy().astype(np.float64)
    for i in range(levels.shape[0]):
        bound = _bound(params, i, L, vmax[i])
        print(f"level {i}: v0 gpu {v0[i]!r} f64 {ref0[i]!r}, bound {bound:.3e}")
        assert np.isfinite(ref0[i]) and abs(v0[i] - ref0[i]) <= bound, (i, v0[i], ref0[i], bound)
    if all_idx:
        sel = torch.tensor(all_idx, device="cuda")
        va = ro.policy_return(levels[sel].contiguous(), theta[sel].contiguous(), L, return_all=True)
        assert va.shape == (len(all_idx), L, ro.obs_dim - 1)
        va = va.cpu().numpy()
        for j, i in enumerate(all_idx):
            _check_table(va[j], ref_all[i], params, i, L, vmax[i])
            # the return_all table's start entry is the scalar result, bit for bit
            assert np.float32(va[j][0, orf.start_index(spec, params, i)]) == np.float32(v0[i])


def test_deterministic_single_agent_form_and_batch_independence():
    from toued.rollout import RolloutWrapper
    mode, params, L, _ = _case("small")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("small").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    a, b = ro.policy_return(levels, theta, L, return_all=True), ro.policy_return(levels, theta, L, return_all=True)
    assert torch.equal(a, b)
    s0, s1 = ro.policy_return(levels, theta, L), ro.policy_return(levels, theta, L)
    assert torch.equal(s0, s1)
    one = ro.policy_return(levels[3], theta[3], L)
    assert one.dim() == 0 and one == s0[3]
    one_all = ro.policy_return(levels[3], theta[3], L, return_all=True)
    assert one_all.shape == (L, ro.obs_dim - 1) and torch.equal(one_all, a[3])
    # a level's result does not depend on the batch it is in, nor on its place there
    alone = ro.policy_return(levels[5:6].contiguous(), theta[5:6].contiguous(), L)
    assert torch.equal(alone, s0[5:6])
    back = ro.policy_return(levels.flip(0).contiguous(), theta.flip(0).contiguous(), L)
    assert torch.equal(back.flip(0), s0)


def test_empty_batch_and_zero_length():
    from toued.rollout import RolloutWrapper
    mode, params, _, _ = _case("debug10")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("debug10").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    assert ro.policy_return(levels[:0].contiguous(), theta[:0].contiguous(), 10).shape == (0,)
    assert ro.policy_return(levels[:0].contiguous(), theta[:0].contiguous(), 10,
                            return_all=True).shape == (0, 10, ro.obs_dim - 1)
    z = ro.policy_return(levels, theta, 0)
    assert z.shape == (64,) and not z.any()
    assert ro.policy_return(levels, theta, 0, return_all=True).shape == (64, 0, ro.obs_dim - 1)


def test_argument_errors():
    from toued import _lib
    levels = torch.zeros((1, 80), dtype=torch.int32, device="cuda")
    theta = torch.zeros((1, 4 * 4 * 4 + 1, 5), device="cuda")
    v0 = torch.zeros(1, device="cuda")
    fn = _lib.lib().toued_policy_return
    err = lambda: _lib.lib().toued_last_error().decode()
    assert fn(_lib.ptr(levels), _lib.ptr(theta), 1, 65, 4, 2, 0, 10, _lib.ptr(v0), None, _lib.stream_ptr()) == -1
    assert "unsupported" in err()
    assert fn(_lib.ptr(levels), _lib.ptr(theta), 1, 64, 4, 2, 1, 10, _lib.ptr(v0), None, _lib.stream_ptr()) == -1
    assert "D=64" in err()
    assert fn(_lib.ptr(levels), _lib.ptr(theta), -1, 65, 4, 2, 1, 10, _lib.ptr(v0), None, _lib.stream_ptr()) == -1
    assert fn(_lib.ptr(levels), _lib.ptr(theta), 1, 65, 4, 2, 1, -1, _lib.ptr(v0), None, _lib.stream_ptr()) == -1
    assert fn(_lib.ptr(levels), _lib.ptr(theta), 1, 17 * 17 * 4 + 1, 17, 2, 1, 10, _lib.ptr(v0), None,
              _lib.stream_ptr()) == -1
    assert fn(_lib.ptr(levels), _lib.ptr(theta), 1, (16 << 9) + 1, 4, 9, 1, 10, _lib.ptr(v0), None,
              _lib.stream_ptr()) == -1
    with pytest.raises(_lib.ToUEDError, match="LDS"):      # 16x16 cells x 2^8 existence masks: over the LDS budget
        _lib.call("toued_policy_return", _lib.ptr(levels), _lib.ptr(theta), 1, (256 << 8) + 1, 16, 8, 1, 10,
                  _lib.ptr(v0), None, _lib.stream_ptr())


def test_every_tabular_mode_fits():
    """One level of every tabular mode of toued/modes.py goes through (the LDS budget check admits them all, and
    every count of work items per thread that a mode has is run), and its 5-step table matches the reference."""
    from toued import modes
    from toued.rollout import RolloutWrapper
    for k, (mode, kw) in enumerate(modes.ENV_MODE_KWARGS.items()):
        if not kw["tabular"]:
            continue
        spec = olv.env_spec(mode)
        params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(7), 1), mode)
        theta = prf.random_tables(3000 + k, 1, spec.obs_dim)
        ro = RolloutWrapper(mode, 20)
        got = ro.policy_return(_dev_levels(params, spec), torch.from_numpy(theta).cuda(), 5, return_all=True)
        ref = prf.policy_return_all(spec, params, 0, theta[0], 5)
        _check_table(got[0].cpu().numpy(), ref, params, 0, 5, np.abs(ref[np.isfinite(ref)]).max(initial=0.0))


def test_table_larger_than_any_mode():
    """S = 14^2 * 2^5 = 6272 states through the C ABI: more than six work items per thread, which no mode has; the
    kernel's instantiation whose further items read their table rows inside the time loop."""
    from oracle.gridworld import EnvSpec
    spec = EnvSpec(14, 5, 2, True)
    p = orf.make_params(spec, grid_size=14, start_pos=0, obj_ids=[0, 1, 0, 1, 0], static_obj_poss=[15, 30, 45, 16, 1],
                        obj_rewards=[1.0, -0.5], obj_p_terminate=[0.05, 0.3], obj_p_respawn=[0.2, 0.5],
                        max_steps=9, walls=[2, 17])
    L = 12
    theta = prf.random_tables(3100, 1, spec.obs_dim)
    got = _AbiWrapper(spec).policy_return(_dev_levels(p, spec), torch.from_numpy(theta).cuda(), L, return_all=True)
    ref = prf.policy_return_all(spec, p, 0, theta[0], L)
    assert np.isfinite(ref[0]).sum() == (14 * 14 - 2) * 32
    _check_table(got[0].cpu().numpy(), ref, p, 0, L, np.abs(ref[np.isfinite(ref)]).max(initial=0.0))


def test_policy_return_is_at_most_the_optimum():
    from toued.rollout import RolloutWrapper
    mode, params, L, _ = _case("small")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("small").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    vpi = ro.policy_return(levels, theta, L).cpu().numpy().astype(np.float64)
    vst = ro.optimal_return(levels, L).cpu().numpy().astype(np.float64)
    _, _, vmax_pi = _reference("small")
    _, _, vmax_opt = _opt_reference("small")
    for i in range(levels.shape[0]):
        slack = _bound(params, i, L, vmax_pi[i]) + _bound(params, i, L, vmax_opt[i])     # both kernels' bounds
        assert vpi[i] <= vst[i] + slack, (i, vpi[i], vst[i], slack)


# ------------------------------------------------------------------------------------ against sampled rollouts
MC_SEED, MC_LEVELS, MC_COPIES, MC_WORKERS = 311, 4, 16, 64


def mc_case():
    """4 `small` levels with random tables, each as 16 agent copies with distinct eval keys: (spec, params of the 4
    levels, theta f32 [4, D, 5], eval_agent keys u32 [64, 2] with agent 16 * i + j on level i)."""
    spec = olv.env_spec("small")
    params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(MC_SEED), MC_LEVELS), "small")
    theta = prf.random_tables(MC_SEED, MC_LEVELS, spec.obs_dim)
    keys = jr.split(jr.PRNGKey(MC_SEED + 1), MC_LEVELS * MC_COPIES)
    return spec, params, theta, keys


def test_policy_return_agrees_with_eval_rollouts():
    """The mean of eval_agent's per-worker returns (its reset and rollout, toued.agents.eval_agent_reset and
    RolloutWrapper.eval_returns, whose row means are eval_agent's result) over 16 x 64 = 1024 workers per level,
    within polret_ref.mc_tolerance of the exact return."""
    from toued import prng
    from toued.agents import eval_agent, eval_agent_reset
    from toued.rollout import RolloutWrapper
    spec, params, theta, keys = mc_case()
    ro = RolloutWrapper("small", 20)
    assert ro.eval_rollout_len == 100
    rep = np.repeat(np.arange(MC_LEVELS), MC_COPIES)
    levels = _dev_levels(params, spec)
    th = torch.from_numpy(theta).cuda()
    exact = ro.policy_return(levels, th, ro.eval_rollout_len).cpu().numpy().astype(np.float64)
    sel = torch.from_numpy(rep).cuda()
    lv, tt = levels[sel].contiguous(), th[sel].contiguous()
    dkeys = prng.from_uint32_numpy(keys, "cuda")
    state, rkeys = eval_agent_reset(ro, dkeys, lv, MC_WORKERS)
    cum = ro.eval_returns(rkeys, tt, lv, state)
    assert torch.equal(cum.mean(dim=1), eval_agent(ro, dkeys, lv, tt, MC_WORKERS))
    cum = cum.cpu().numpy().reshape(MC_LEVELS, MC_COPIES * MC_WORKERS)
    for i in range(MC_LEVELS):
        mean = float(cum[i].astype(np.float64).mean())
        tol = prf.mc_tolerance(cum[i], params["obj_rewards"][i])
        print(f"level {i}: sampled {mean:+.5f} exact {exact[i]:+.5f} tolerance {tol:.5f}")
        assert abs(mean - exact[i]) <= tol, (i, mean, exact[i], tol)


# ------------------------------------------------------------------------------------------- --regret_eval exact
def _sampler(mode, score_function, N=8, B=16):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", mode, "--score_function", score_function, "--regret_eval", "exact",
                       "--num_agents", str(N), "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size",
                       str(B)])
    return LevelSampler(args)


def _agents(mode, N, seed):
    from toued import prng
    from toued.agents import create_agents
    from toued.env import LevelGenerator
    dk = lambda a: prng.from_uint32_numpy(a, "cuda")
    levels = LevelGenerator(mode)(dk(jr.split(jr.PRNGKey(seed), N)))
    theta, _ = create_agents(dk(jr.split(jr.PRNGKey(seed + 1), N)), olv.env_spec(mode).obs_dim, 8)
    theta.mul_(10.0)
    return levels, theta


def test_exact_optimal_regret_is_optimum_minus_policy_return():
    from toued import prng
    from toued.plr import optimal_regret
    N = 8
    smp = _sampler("small", "optimal_regret", N)
    ro = smp.rollout_manager
    levels, theta = _agents("small", N, 401)
    dk = lambda a: prng.from_uint32_numpy(a, "cuda")
    got = optimal_regret(smp, dk(jr.split(jr.PRNGKey(403), N)), levels, theta)
    assert got.shape == (N,) and got.dtype == torch.float32
    L = ro.eval_rollout_len
    vst, vpi = ro.optimal_return(levels, L), ro.policy_return(levels, theta, L)
    assert torch.equal(got, vst - vpi)
    # no keys are used
    assert torch.equal(got, optimal_regret(smp, dk(jr.split(jr.PRNGKey(404), N)), levels, theta))
    # a true regret: not below zero by more than the sum of the two kernels' bounds, H * 2^-23 * max(1, max|v64|) of
    # the level's optimal and policy tables (the level generator is bit-exact with the oracle's on the same keys)
    spec = olv.env_spec("small")
    params, lifetime = olv.reset_env_params(jr.split(jr.PRNGKey(401), N), "small")
    assert np.array_equal(levels.cpu().numpy(), olv.pack_levels(params, lifetime, spec))
    th = theta.cpu().numpy()
    diff = vst.cpu().numpy().astype(np.float64) - vpi.cpu().numpy().astype(np.float64)
    fmax = lambda v: np.abs(v[np.isfinite(v)]).max(initial=0.0)
    for i in range(N):
        slack = (_bound(params, i, L, fmax(orf.optimal_return_all(spec, params, i, L)))
                 + _bound(params, i, L, fmax(prf.policy_return_all(spec, params, i, th[i], L))))
        print(f"level {i}: regret {diff[i]:.6e}, -(sum of the bounds) {-slack:.3e}")
        assert diff[i] >= -slack, (i, diff[i], slack)
    assert (got > 0).any()


def test_level_sampler_exact_optimal_regret_scores_the_buffer():
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    N, B = 8, 16
    smp = _sampler("small", "optimal_regret", N, B)
    ro = smp.rollout_manager
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    agents.step = agents.levels[:, L_LIFETIME].clone()           # every agent has reached its lifetime
    levels0, theta0 = agents.levels.clone(), agents.theta.clone()
    old_ids = agents.levels[:, L_BUFID].long().clone()
    assert old_ids.unique().numel() == N
    L = ro.eval_rollout_len
    want = ro.optimal_return(levels0, L) - ro.policy_return(levels0, theta0, L)
    buf, agents = smp.sample(prng.PRNGKey(2, "cuda"), buf, agents)
    assert torch.equal(smp.last_plr["score"], want)
    assert torch.equal(buf.score[old_ids], want)


def test_exact_alg_regret_is_the_difference_of_policy_returns(monkeypatch):
    """alg_regret with --regret_eval exact: one policy_return call on (levels, levels) and (lpg_theta, antagonists'
    tables), no eval rollout; the antagonists' tables are the sampled path's, bit for bit."""
    from toued import prng
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    from toued.plr import algorithmic_regret
    N = 8
    smp = _sampler("debug", "alg_regret", N)
    ro = smp.rollout_manager
    levels, theta = _agents("debug", N, 411)
    keys = prng.from_uint32_numpy(jr.split(jr.PRNGKey(413), N), "cuda")
    calls = []
    inner = ro.policy_return

    def spy(lv, th, L, return_all=False):
        out = inner(lv, th, L, return_all)
        calls.append((lv.clone(), th.clone(), L, out.clone()))
        return out

    def no_eval(*a, **k):
        raise AssertionError("an eval rollout was started with --regret_eval exact")

    monkeypatch.setattr(ro, "policy_return", spy)
    for name in ("eval_returns", "eval_returns_from_draws", "eval_draws"):
        monkeypatch.setattr(ro, name, no_eval)
    got = algorithmic_regret(smp, keys, levels, theta)
    assert len(calls) == 1
    lv, th, L, out = calls[0]
    assert L == ro.eval_rollout_len and out.shape == (2 * N,)
    assert torch.equal(lv, torch.cat([levels, levels])) and torch.equal(th[:N], theta)
    assert torch.equal(got, out[N:] - out[:N])
    # the sampled path on the same keys: the tables its eval rollout receives are the exact path's
    args = parse_args(["--env_mode", "debug", "--score_function", "alg_regret", "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", "16"])
    smp2 = LevelSampler(args)
    assert smp2.regret_eval == "sampled"
    ro2 = smp2.rollout_manager
    seen = []
    for name in ("eval_returns", "eval_returns_from_draws"):
        fn = getattr(ro2, name)
        monkeypatch.setattr(ro2, name, lambda a, t, *r, _fn=fn: (seen.append(t.clone()), _fn(a, t, *r))[1])
    algorithmic_regret(smp2, keys, levels, theta)
    assert len(seen) == 1 and torch.equal(seen[0], th)
