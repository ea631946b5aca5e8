"""GPU: toued_policy_return_moments / RolloutWrapper.policy_return_moments against the float64 restatement
tests/polvar_ref.py, and the return_variance PLR score.

The cases, levels and actor tables are test_gpu_polret.py's.  Comparison per level, with
H = min(max_steps_in_episode, max_rollout_len) backups:

  * the mean within test_gpu_polret.py's bound, H * 2^-23 * max(1, max|v64|), and bit-identical to
    toued_policy_return's;
  * the variance within H * 2^-23 * max(1, max|u64|).  Derived, not measured: the kernel's v tables are f64, as is
    every step's arithmetic; the u update is a non-expansion in u_{t+1} (its weights pi * c * P sum to at most 1), so
    the steps' errors add up and are not multiplied; and a step's only error is the f32 store of u_t, at most 2^-24
    relative to the table's magnitude;
  * the finite masks equal, the -inf entries and the zero rows exact.
"""
import functools

import numpy as np
import pytest
import torch

import optret_ref as orf
import polret_ref as prf
import polvar_ref as pvf
from oracle import jaxrand as jr
from oracle import levels as olv
from test_gpu_optret import HAND_SPEC, _spec
from test_gpu_polret import CASES, MC_COPIES, MC_LEVELS, MC_WORKERS, _case, _dev_levels, _tables, mc_case
from test_gpu_polret import _bound as _mean_bound

pytestmark = pytest.mark.gpu


def _abi(spec, levels, theta, L, want_v=False, want_u=False, tabular=1):
    """toued_policy_return_moments on the C ABI: (v0, var0, v_all or None, var_all or None)."""
    from toued import _lib
    n, S = levels.shape[0], spec.obs_dim - 1
    v0, u0 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    va = torch.empty((n, L, S), device="cuda") if want_v else None
    ua = torch.empty((n, L, S), device="cuda") if want_u else None
    _lib.call("toued_policy_return_moments", _lib.ptr(levels), _lib.ptr(theta), n, spec.obs_dim, spec.max_grid_size,
              spec.max_n_objs, tabular, L, _lib.ptr(v0), _lib.ptr(u0), _lib.ptr(va), _lib.ptr(ua), _lib.stream_ptr())
    return v0, u0, va, ua


class _AbiWrapper:
    """RolloutWrapper's two calls for a table size that no mode has, straight on the C ABI."""

    def __init__(self, spec):
        self.spec, self.obs_dim = spec, spec.obs_dim

    def policy_return_moments(self, levels, theta, L, return_all=False):
        v0, u0, va, ua = _abi(self.spec, levels, theta, L, return_all, return_all)
        return (va, ua) if return_all else (v0, u0)

    def policy_return(self, levels, theta, L, return_all=False):
        from test_gpu_polret import _AbiWrapper as PolretAbi
        return PolretAbi(self.spec).policy_return(levels, theta, L, return_all)


def _wrapper(mode):
    from toued.rollout import RolloutWrapper
    return _AbiWrapper(HAND_SPEC) if mode is None else RolloutWrapper(mode, 20)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 (v_all, u_all) of the levels whose tables are compared, (v_0, u_0)(start) and max|v|, max|u| over the
    finite table entries of every level: computed once."""
    mode, params, L, all_idx = _case(name)
    spec, th = _spec(mode), _tables(name)
    n = params["start_pos"].shape[0]
    tabs, v0, u0, vmax, umax = {}, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        v, u = pvf.moments_all(spec, params, i, th[i], L)
        si = orf.start_index(spec, params, i)
        v0[i], u0[i] = (v[0, si], u[0, si]) if L > 0 else (0.0, 0.0)
        vmax[i] = np.abs(v[np.isfinite(v)]).max(initial=0.0)
        umax[i] = np.abs(u[np.isfinite(u)]).max(initial=0.0)
        if i in all_idx:
            tabs[i] = (v, u)
    return tabs, v0, u0, vmax, umax


def _bound(params, i, L, umax):
    H = min(int(params["max_steps_in_episode"][i]), L)
    return H * 2.0 ** -23 * max(1.0, float(umax))


def _check_table(got, ref, params, i, bound, what):
    got = got.astype(np.float64)
    fin = np.isfinite(ref)
    assert not np.isnan(got).any(), (what, i)
    assert np.array_equal(np.isfinite(got), fin), (what, i)
    assert np.array_equal(got[~fin], ref[~fin]), (what, i)            # -inf exactly
    ms = int(params["max_steps_in_episode"][i])
    assert not got[ms:].any(), (what, i)                              # zero rows exactly
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    print(f"level {i}: {what} max|gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, i, err, bound)
    return err / bound


@pytest.mark.parametrize("name", CASES)
def test_moments_match_float64(name):
    mode, params, L, all_idx = _case(name)
    spec = _spec(mode)
    tabs, ref_v0, ref_u0, vmax, umax = _reference(name)
    levels = _dev_levels(params, spec)
    theta = torch.from_numpy(_tables(name).copy()).cuda()
    ro = _wrapper(mode)
    v0, u0 = ro.policy_return_moments(levels, theta, L)
    n = levels.shape[0]
    assert v0.shape == (n,) and u0.shape == (n,) and v0.dtype == torch.float32 and u0.dtype == torch.float32
    v0, u0 = v0.cpu().numpy().astype(np.float64), u0.cpu().numpy().astype(np.float64)
    worst_v = worst_u = 0.0
    for i in range(n):
        bv, bu = _mean_bound(params, i, L, vmax[i]), _bound(params, i, L, umax[i])
        print(f"level {i}: v0 gpu {v0[i]!r} f64 {ref_v0[i]!r} bound {bv:.3e}; "
              f"var0 gpu {u0[i]!r} f64 {ref_u0[i]!r} bound {bu:.3e}")
        assert np.isfinite(ref_v0[i]) and abs(v0[i] - ref_v0[i]) <= bv, (i, v0[i], ref_v0[i], bv)
        assert np.isfinite(ref_u0[i]) and abs(u0[i] - ref_u0[i]) <= bu, (i, u0[i], ref_u0[i], bu)
        assert u0[i] >= -bu, (i, u0[i], bu)                 # a variance: not below zero by more than the bound
        worst_v, worst_u = max(worst_v, abs(v0[i] - ref_v0[i]) / bv), max(worst_u, abs(u0[i] - ref_u0[i]) / bu)
    if all_idx:
        sel = torch.tensor(all_idx, device="cuda")
        va, ua = ro.policy_return_moments(levels[sel].contiguous(), theta[sel].contiguous(), L, return_all=True)
        assert va.shape == (len(all_idx), L, ro.obs_dim - 1) and ua.shape == va.shape
        va, ua = va.cpu().numpy(), ua.cpu().numpy()
        for j, i in enumerate(all_idx):
            worst_v = max(worst_v, _check_table(va[j], tabs[i][0], params, i, _mean_bound(params, i, L, vmax[i]),
                                                "mean"))
            worst_u = max(worst_u, _check_table(ua[j], tabs[i][1], params, i, _bound(params, i, L, umax[i]),
                                                "variance"))
            # the return_all tables' start entries are the scalar results, bit for bit
            si = orf.start_index(spec, params, i)
            assert np.float32(va[j][0, si]) == np.float32(v0[i]) and np.float32(ua[j][0, si]) == np.float32(u0[i])
    print(f"{name}: largest error / bound: mean {worst_v:.3f}, variance {worst_u:.3f}; max|u64| {umax.max():.4f}")


@pytest.mark.parametrize("name", CASES)
def test_mean_is_policy_return_bit_for_bit(name):
    mode, params, L, _ = _case(name)
    levels = _dev_levels(params, _spec(mode))
    theta = torch.from_numpy(_tables(name).copy()).cuda()
    ro = _wrapper(mode)
    assert torch.equal(ro.policy_return_moments(levels, theta, L)[0], ro.policy_return(levels, theta, L))
    lv, th = levels[:2].contiguous(), theta[:2].contiguous()
    assert torch.equal(ro.policy_return_moments(lv, th, L, return_all=True)[0],
                       ro.policy_return(lv, th, L, return_all=True))


def test_deterministic_single_agent_form_and_batch_independence():
    from toued.rollout import RolloutWrapper
    mode, params, L, _ = _case("small")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("small").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    a, b = ro.policy_return_moments(levels, theta, L, return_all=True), \
        ro.policy_return_moments(levels, theta, L, return_all=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s0, s1 = ro.policy_return_moments(levels, theta, L), ro.policy_return_moments(levels, theta, L)
    assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1])
    m, v = ro.policy_return_moments(levels[3], theta[3], L)
    assert m.dim() == 0 and v.dim() == 0 and m == s0[0][3] and v == s0[1][3]
    m_all, v_all = ro.policy_return_moments(levels[3], theta[3], L, return_all=True)
    assert m_all.shape == (L, ro.obs_dim - 1) and torch.equal(m_all, a[0][3]) and torch.equal(v_all, a[1][3])
    # a level's result does not depend on the batch it is in, nor on its place there
    alone = ro.policy_return_moments(levels[5:6].contiguous(), theta[5:6].contiguous(), L)
    assert torch.equal(alone[0], s0[0][5:6]) and torch.equal(alone[1], s0[1][5:6])
    back = ro.policy_return_moments(levels.flip(0).contiguous(), theta.flip(0).contiguous(), L)
    assert torch.equal(back[0].flip(0), s0[0]) and torch.equal(back[1].flip(0), s0[1])
    # the optional tables change no scalar, and each is the same with or without the other
    spec = olv.env_spec(mode)
    both = _abi(spec, levels, theta, L, True, True)
    assert torch.equal(both[2], a[0]) and torch.equal(both[3], a[1])
    for want_v, want_u in ((False, False), (True, False), (False, True), (True, True)):
        v0, u0, va, ua = _abi(spec, levels, theta, L, want_v, want_u)
        assert torch.equal(v0, s0[0]) and torch.equal(u0, s0[1])
        assert (va is None) == (not want_v) and (ua is None) == (not want_u)
        assert va is None or torch.equal(va, a[0])
        assert ua is None or torch.equal(ua, a[1])


def test_empty_batch_and_zero_length():
    from toued.rollout import RolloutWrapper
    mode, params, _, _ = _case("debug10")
    levels = _dev_levels(params, olv.env_spec(mode))
    theta = torch.from_numpy(_tables("debug10").copy()).cuda()
    ro = RolloutWrapper(mode, 20)
    for out in ro.policy_return_moments(levels[:0].contiguous(), theta[:0].contiguous(), 10):
        assert out.shape == (0,)
    for out in ro.policy_return_moments(levels[:0].contiguous(), theta[:0].contiguous(), 10, return_all=True):
        assert out.shape == (0, 10, ro.obs_dim - 1)
    for out in ro.policy_return_moments(levels, theta, 0):
        assert out.shape == (64,) and not out.any()
    for out in ro.policy_return_moments(levels, theta, 0, return_all=True):
        assert out.shape == (64, 0, ro.obs_dim - 1)


def test_argument_errors():
    from oracle.gridworld import EnvSpec
    from toued import _lib
    levels = torch.zeros((1, 80), dtype=torch.int32, device="cuda")
    theta = torch.zeros((1, 4 * 4 * 4 + 1, 5), device="cuda")
    v0, u0 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    fn = _lib.lib().toued_policy_return_moments
    err = lambda: _lib.lib().toued_last_error().decode()
    call = lambda n, D, G, nm, tab, L: fn(_lib.ptr(levels), _lib.ptr(theta), n, D, G, nm, tab, L, _lib.ptr(v0),
                                          _lib.ptr(u0), None, None, _lib.stream_ptr())
    assert call(1, 65, 4, 2, 0, 10) == -1
    assert "unsupported" in err()
    assert call(1, 64, 4, 2, 1, 10) == -1
    assert "D=64" in err()
    assert call(-1, 65, 4, 2, 1, 10) == -1
    assert call(1, 65, 4, 2, 1, -1) == -1
    assert call(1, 17 * 17 * 4 + 1, 17, 2, 1, 10) == -1
    assert call(1, (16 << 9) + 1, 4, 9, 1, 10) == -1
    assert call(1, 65, 4, 2, 1, 10) == 0
    # test_gpu_polret.py::test_table_larger_than_any_mode's 6272 states fit toued_policy_return's LDS, not this one's
    spec = EnvSpec(14, 5, 2, True)
    assert spec.obs_dim == 6272 + 1
    with pytest.raises(_lib.ToUEDError, match="LDS"):
        _lib.call("toued_policy_return_moments", _lib.ptr(levels), _lib.ptr(theta), 1, spec.obs_dim, 14, 5, 1, 10,
                  _lib.ptr(v0), _lib.ptr(u0), None, None, _lib.stream_ptr())
    with pytest.raises(_lib.ToUEDError, match="unsupported"):
        _abi(olv.env_spec("debug"), levels, theta, 10, tabular=0)


def test_every_tabular_mode_fits():
    """One level of every tabular mode of toued/modes.py goes through (the lower LDS limit admits them all, `tabular`
    tightly, and every count of work items per thread is run), and its 5-step tables match the reference."""
    from toued import modes
    from toued.rollout import RolloutWrapper
    items = set()
    for k, (mode, kw) in enumerate(modes.ENV_MODE_KWARGS.items()):
        if not kw["tabular"]:
            continue
        spec = olv.env_spec(mode)
        params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(7), 1), mode)
        theta = prf.random_tables(3000 + k, 1, spec.obs_dim)
        ro = RolloutWrapper(mode, 20)
        gv, gu = ro.policy_return_moments(_dev_levels(params, spec), torch.from_numpy(theta).cuda(), 5,
                                          return_all=True)
        rv, ru = pvf.moments_all(spec, params, 0, theta[0], 5)
        fmax = lambda x: np.abs(x[np.isfinite(x)]).max(initial=0.0)
        _check_table(gv[0].cpu().numpy(), rv, params, 0, _mean_bound(params, 0, 5, fmax(rv)), f"{mode} mean")
        _check_table(gu[0].cpu().numpy(), ru, params, 0, _bound(params, 0, 5, fmax(ru)), f"{mode} variance")
        S = spec.obs_dim - 1
        block = 64 if S <= 64 else (256 if S <= 256 else (512 if S <= 1024 else 1024))
        items.add(next(i for i in (1, 2, 4, 6) if -(-S // block) <= i))
    assert items == {1, 2, 4, 6}


def test_deterministic_level_and_policy_have_zero_variance():
    """The `hand` level with p_terminate 0 and p_respawn 0 / 1 under tables that are one-hot to the last bit (+1e4 on
    one action per state, -1e4 on the others): nothing is random, so the variance is zero up to the bound and no NaN
    comes of the huge logits."""
    p = orf.make_params(HAND_SPEC, grid_size=3, start_pos=0, obj_ids=[0, 1], static_obj_poss=[4, 4],
                        obj_rewards=[1.0, -0.25], obj_p_terminate=[0.0, 0.0], obj_p_respawn=[0.0, 1.0],
                        max_steps=12, walls=[2])
    n, L, D = 6, 12, HAND_SPEC.obs_dim
    rng = np.random.default_rng(4100)
    theta = np.full((n, D, 5), -1e4, np.float32)
    theta[:, -1] = 0.0
    np.put_along_axis(theta[:, :-1], rng.integers(0, 5, (n, D - 1, 1)), np.float32(1e4), axis=2)
    for e in range(4):                          # table 0: down from the start, right onto the objects' cell, stay
        theta[0, [0 + 9 * e, 3 + 9 * e, 4 + 9 * e]] = -1e4
        theta[0, 0 + 9 * e, 1] = theta[0, 3 + 9 * e, 3] = theta[0, 4 + 9 * e, 4] = 1e4
    params = orf.concat_params([p] * n)
    v0, u0, va, ua = _abi(HAND_SPEC, _dev_levels(params, HAND_SPEC), torch.from_numpy(theta).cuda(), L, True, True)
    assert not torch.isnan(va).any() and not torch.isnan(ua).any()
    v0, u0 = v0.cpu().numpy().astype(np.float64), u0.cpu().numpy().astype(np.float64)
    for i in range(n):
        rv, ru = pvf.moments_all(HAND_SPEC, params, i, theta[i], L)
        umax = np.abs(ru[np.isfinite(ru)]).max(initial=0.0)
        bound = _bound(params, i, L, umax)
        print(f"table {i}: v0 {v0[i]!r}, var0 {u0[i]!r}, f64 max|u| {umax:.3e}, bound {bound:.3e}")
        assert umax <= 1e-12
        assert -bound <= u0[i] <= bound, (i, u0[i], bound)
        fin = np.isfinite(ru)
        assert np.abs(ua[i].cpu().numpy().astype(np.float64)[fin]).max() <= bound
    assert v0[0] != 0.0                         # table 0 does collect


def test_variance_agrees_with_eval_rollouts():
    """The sample variance of eval_agent's per-worker returns over 16 x 64 = 1024 workers per level (test_gpu_polret's
    mc_case) within polvar_ref.variance_tolerance of the exact variance."""
    from toued import prng
    from toued.agents import eval_agent_reset
    from toued.rollout import RolloutWrapper
    spec, params, theta, keys = mc_case()
    ro = RolloutWrapper("small", 20)
    assert ro.eval_rollout_len == 100
    rep = np.repeat(np.arange(MC_LEVELS), MC_COPIES)
    levels = _dev_levels(params, spec)
    th = torch.from_numpy(theta).cuda()
    exact = ro.policy_return_moments(levels, th, ro.eval_rollout_len)[1].cpu().numpy().astype(np.float64)
    sel = torch.from_numpy(rep).cuda()
    lv, tt = levels[sel].contiguous(), th[sel].contiguous()
    state, rkeys = eval_agent_reset(ro, prng.from_uint32_numpy(keys, "cuda"), lv, MC_WORKERS)
    cum = ro.eval_returns(rkeys, tt, lv, state).cpu().numpy().reshape(MC_LEVELS, MC_COPIES * MC_WORKERS)
    for i in range(MC_LEVELS):
        s2, tol = pvf.variance_tolerance(cum[i], params["obj_rewards"][i])
        print(f"level {i}: sampled {s2:.6f} exact {exact[i]:.6f} difference {abs(s2 - exact[i]):.2e} "
              f"tolerance {tol:.2e}")
        assert abs(s2 - exact[i]) <= tol, (i, s2, exact[i], tol)


# ---------------------------------------------------------------------------------------------- return_variance
def _sampler(N=8, B=16, extra=()):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "small", "--score_function", "return_variance", "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B), *extra])
    return LevelSampler(args)


def test_return_variance_is_the_moments_variance_and_ignores_its_keys():
    from toued import prng
    from toued.plr import return_variance
    from test_gpu_polret import _agents
    N = 8
    smp = _sampler(N)
    ro = smp.rollout_manager
    levels, theta = _agents("small", N, 401)
    dk = lambda a: prng.from_uint32_numpy(a, "cuda")
    got = return_variance(smp, dk(jr.split(jr.PRNGKey(403), N)), levels, theta)
    assert got.shape == (N,) and got.dtype == torch.float32
    assert torch.equal(got, ro.policy_return_moments(levels, theta, ro.eval_rollout_len)[1])
    assert torch.equal(got, return_variance(smp, dk(jr.split(jr.PRNGKey(404), N)), levels, theta))
    assert (got > 0).any() and torch.isfinite(got).all()
    assert return_variance(smp, dk(jr.split(jr.PRNGKey(403), N))[:0], levels[:0], theta[:0]).shape == (0,)


@pytest.mark.parametrize("extra", [(), ("--use_es",)], ids=["adam", "use_es"])
def test_level_sampler_return_variance_scores_the_buffer(extra):
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    N, B = 8, 16
    smp = _sampler(N, B, extra)
    assert smp.args.use_es == bool(extra)
    ro = smp.rollout_manager
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    agents.step = agents.levels[:, L_LIFETIME].clone()           # every agent has reached its lifetime
    levels0, theta0 = agents.levels.clone(), agents.theta.clone()
    old_ids = agents.levels[:, L_BUFID].long().clone()
    assert old_ids.unique().numel() == N
    want = ro.policy_return_moments(levels0, theta0, ro.eval_rollout_len)[1]
    buf, agents = smp.sample(prng.PRNGKey(2, "cuda"), buf, agents)
    assert torch.equal(smp.last_plr["score"], want)
    assert torch.equal(buf.score[old_ids], want)
