"""GPU: toued_optimal_return / RolloutWrapper.optimal_return against the float64 restatement of
GridWorld.optimal_return (tests/optret_ref.py), and the optimal_regret PLR score built on it.

Comparison per level, with H = min(max_steps_in_episode, max_rollout_len) backups: the finite masks equal; on the
finite entries |gpu - f64| <= H * 2^-23 * max(1, max|v64|) (the Bellman backup is a max-norm non-expansion, so the
per-step roundings add up and are not multiplied; one step's rounding is taken as one f32 ulp of the table's
magnitude); the -inf entries and the zero rows exact.
"""
import functools

import numpy as np
import pytest
import torch

import optret_ref as orf
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle.gridworld import EnvSpec

pytestmark = pytest.mark.gpu


HAND_SPEC = EnvSpec(3, 2, 2, True)


def _spec(mode):
    return HAND_SPEC if mode is None else olv.env_spec(mode)


class _AbiWrapper:
    """RolloutWrapper.optimal_return's calls for a table size that no mode has, straight on the C ABI."""

    def __init__(self, spec):
        self.spec, self.obs_dim = spec, spec.obs_dim

    def optimal_return(self, levels, L, return_all=False):
        from toued import _lib
        n = levels.shape[0]
        v0 = torch.zeros(n, device="cuda")
        va = torch.empty((n, L, self.obs_dim - 1), device="cuda") if return_all else None
        _lib.call("toued_optimal_return", _lib.ptr(levels), n, self.spec.max_grid_size, self.spec.max_n_objs, 1, L,
                  _lib.ptr(v0), _lib.ptr(va), _lib.stream_ptr())
        return va if return_all else v0


def _wrapper(mode):
    from toued.rollout import RolloutWrapper
    return _AbiWrapper(HAND_SPEC) if mode is None else RolloutWrapper(mode, 20)


def _dev_levels(params, spec):
    lt = np.ones(params["start_pos"].shape[0], np.int32)
    return torch.from_numpy(olv.pack_levels(params, lt, spec)).cuda()


def _take(params, idx):
    return {k: v[np.asarray(idx)] for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(mode, params of the case's levels, max_rollout_len, indices of the levels whose v_all is compared)."""
    if name in ("debug10", "debug3"):
        params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(101), 64), "debug")
        L = 10 if name == "debug10" else 3
        if L == 3:
            assert (params["max_steps_in_episode"] > 3).any()      # truncated by the rollout length
        return "debug", params, L, tuple(range(64))
    if name == "small":
        params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(102), 32), "small")
        assert (params["max_steps_in_episode"] < 100).any()
        return "small", params, 100, tuple(range(32))
    if name == "all":
        pool, _ = olv.reset_env_params(jr.split(jr.PRNGKey(103), 64), "all")
        one = int(np.flatnonzero(pool["n_objs"] == 1)[0])
        five = int(np.flatnonzero(pool["n_objs"] == 5)[0])
        rest = [i for i in range(64) if i not in (one, five)][:14]
        return "all", _take(pool, [one, five] + rest), 750, (0, 1)
    if name == "tabular":
        pool, _ = olv.reset_env_params(jr.split(jr.PRNGKey(104), 48), "tabular")
        subs = olv.ENV_MODE_PARAMS["tabular"]["modes"]
        dense = int(np.flatnonzero(pool["sub_mode"] == subs.index("dense"))[0])
        longer = int(np.flatnonzero(pool["sub_mode"] == subs.index("longer"))[0])
        return "tabular", _take(pool, [dense, longer]), 2000, ()
    if name == "hand":
        # two objects on one cell (p_terminate 0.3 and 0.4 add up to 0.7 when both are collected), an object that
        # never respawns once collected (p_respawn exactly 0) and one that always does (exactly 1); S = 3^2 * 2^2, a
        # table no mode has, through the C ABI
        p = orf.make_params(HAND_SPEC, grid_size=3, start_pos=0, obj_ids=[0, 1], static_obj_poss=[4, 4],
                            obj_rewards=[1.0, -0.25], obj_p_terminate=[0.3, 0.4], obj_p_respawn=[0.0, 1.0],
                            max_steps=12, walls=[2])
        return None, p, 12, (0,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 v_all of the levels whose table is compared, v_0(start) and max|v| over the finite table entries of
    every level: computed once."""
    mode, params, L, all_idx = _case(name)
    spec = _spec(mode)
    n = params["start_pos"].shape[0]
    v_all, v0, vmax = {}, np.zeros(n), np.zeros(n)
    for i in range(n):
        v = orf.optimal_return_all(spec, params, i, L)
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
    assert np.array_equal(np.isfinite(got), fin), i
    assert np.array_equal(got[~fin], ref[~fin]), i                    # -inf exactly
    ms = int(params["max_steps_in_episode"][i])
    assert not got[ms:].any(), i                                      # zero rows exactly
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    bound = _bound(params, i, L, vmax)
    print(f"level {i}: max|gpu - f64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (i, err, bound)


@pytest.mark.parametrize("name", ["debug10", "debug3", "small", "all", "tabular", "hand"])
def test_optimal_return_matches_float64(name):
    mode, params, L, all_idx = _case(name)
    spec = _spec(mode)
    ref_all, ref0, vmax = _reference(name)
    levels = _dev_levels(params, spec)
    ro = _wrapper(mode)
    v0 = ro.optimal_return(levels, L)
    assert v0.shape == (levels.shape[0],) and v0.dtype == torch.float32
    v0 = v0.cpu().numpy().astype(np.float64)
    for i in range(levels.shape[0]):
        bound = _bound(params, i, L, vmax[i])
        print(f"level {i}: v0 gpu {v0[i]!r} f64 {ref0[i]!r}, bound {bound:.3e}")
        assert np.isfinite(ref0[i]) and abs(v0[i] - ref0[i]) <= bound, (i, v0[i], ref0[i], bound)
    if all_idx:
        sel = torch.tensor(all_idx, device="cuda")
        va = ro.optimal_return(levels[sel].contiguous(), L, return_all=True)
        assert va.shape == (len(all_idx), L, ro.obs_dim - 1)
        va = va.cpu().numpy()
        for j, i in enumerate(all_idx):
            _check_table(va[j], ref_all[i], params, i, L, vmax[i])
            # the return_all table's start entry is the scalar result, bit for bit
            assert np.float32(va[j][0, orf.start_index(spec, params, i)]) == np.float32(v0[i])


def test_all_case_covers_one_and_five_objects():
    _, params, _, _ = _case("all")
    assert params["n_objs"][0] == 1 and params["n_objs"][1] == 5


def test_deterministic_and_single_level_form():
    from toued.rollout import RolloutWrapper
    mode, params, L, _ = _case("small")
    levels = _dev_levels(params, olv.env_spec(mode))
    ro = RolloutWrapper(mode, 20)
    a, b = ro.optimal_return(levels, L, return_all=True), ro.optimal_return(levels, L, return_all=True)
    assert torch.equal(a, b)
    s0, s1 = ro.optimal_return(levels, L), ro.optimal_return(levels, L)
    assert torch.equal(s0, s1)
    one = ro.optimal_return(levels[3], L)
    assert one.dim() == 0 and one == s0[3]
    one_all = ro.optimal_return(levels[3], L, return_all=True)
    assert one_all.shape == (L, ro.obs_dim - 1) and torch.equal(one_all, a[3])


def test_empty_batch_and_zero_length():
    from toued.rollout import RolloutWrapper
    mode, params, _, _ = _case("debug10")
    levels = _dev_levels(params, olv.env_spec(mode))
    ro = RolloutWrapper(mode, 20)
    assert ro.optimal_return(levels[:0].contiguous(), 10).shape == (0,)
    assert ro.optimal_return(levels[:0].contiguous(), 10, return_all=True).shape == (0, 10, ro.obs_dim - 1)
    z = ro.optimal_return(levels, 0)
    assert z.shape == (64,) and not z.any()
    assert ro.optimal_return(levels, 0, return_all=True).shape == (64, 0, ro.obs_dim - 1)


def test_non_tabular_is_unsupported():
    from toued import _lib
    levels = torch.zeros((1, 80), dtype=torch.int32, device="cuda")
    v0 = torch.zeros(1, device="cuda")
    rc = _lib.lib().toued_optimal_return(_lib.ptr(levels), 1, 4, 2, 0, 10, _lib.ptr(v0), None, _lib.stream_ptr())
    assert rc == -1
    assert "unsupported" in _lib.lib().toued_last_error().decode()
    with pytest.raises(_lib.ToUEDError, match="LDS"):      # 16x16 cells x 2^8 existence masks: over the LDS budget
        _lib.call("toued_optimal_return", _lib.ptr(levels), 1, 16, 8, 1, 10, _lib.ptr(v0), None, _lib.stream_ptr())


def test_every_tabular_mode_fits():
    """One level of every tabular mode of toued/modes.py goes through (the LDS budget check admits them all)."""
    from toued import modes
    from toued.env import LevelGenerator
    from toued.prng import from_uint32_numpy
    from toued.rollout import RolloutWrapper
    for mode, kw in modes.ENV_MODE_KWARGS.items():
        if not kw["tabular"]:
            continue
        levels = LevelGenerator(mode)(from_uint32_numpy(jr.split(jr.PRNGKey(7), 1), "cuda"))
        v = RolloutWrapper(mode, 20).optimal_return(levels, 5)
        assert torch.isfinite(v).all(), mode


# ---------------------------------------------------------------------------------------------- optimal_regret
def _sampler(N=8, B=16):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "small", "--score_function", "optimal_regret", "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B)])
    return LevelSampler(args)


def test_optimal_regret_is_optimum_minus_lpg_eval():
    from toued import prng
    from toued.agents import create_agents, eval_agent
    from toued.env import LevelGenerator
    from toued.plr import optimal_regret
    N = 8
    smp = _sampler(N)
    ro = smp.rollout_manager
    dk = lambda a: prng.from_uint32_numpy(a, "cuda")
    levels = LevelGenerator("small")(dk(jr.split(jr.PRNGKey(201), N)))
    theta, _ = create_agents(dk(jr.split(jr.PRNGKey(202), N)), ro.obs_dim, 8)
    theta.mul_(10.0)
    keys = jr.split(jr.PRNGKey(203), N)
    got = optimal_regret(smp, dk(keys), levels, theta)
    assert got.shape == (N,) and got.dtype == torch.float32
    # lpg_rng of _compute_algorithmic_regret (level_sampler.py:293-329): rng, c = split(keys); rng, tr = split(rng);
    # lpg_rng, a2c_rng = split(rng)
    rng = jr.split(keys, 2)[:, 0]
    rng = jr.split(rng, 2)[:, 0]
    lpg_rng = np.ascontiguousarray(jr.split(rng, 2)[:, 0])
    want = ro.optimal_return(levels, ro.eval_rollout_len) - eval_agent(ro, dk(lpg_rng), levels, theta, 64)
    assert torch.equal(got, want)
    assert ro.eval_rollout_len == 100
    # a true regret: no policy beats the optimum by more than the evaluation's sampling noise allows on average
    assert torch.isfinite(got).all()


def test_level_sampler_optimal_regret_scores_the_buffer():
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    from toued.plr import optimal_regret
    N, B = 8, 16
    smp = _sampler(N, B)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    agents.step = agents.levels[:, L_LIFETIME].clone()           # every agent has reached its lifetime
    levels0, theta0 = agents.levels.clone(), agents.theta.clone()
    old_ids = agents.levels[:, L_BUFID].long().clone()
    assert old_ids.unique().numel() == N
    rng = prng.PRNGKey(2, "cuda")
    # plr_sample's keys: rng, sub = split(rng) (reset); rng, sub = split(rng); keys = split(sub, N)
    r = prng.split(rng, 2)[0].contiguous()
    sub = prng.split(r, 2)[1].contiguous()
    keys = prng.split(sub, N).contiguous()
    want = optimal_regret(smp, keys, levels0, theta0)
    buf, agents = smp.sample(rng, buf, agents)
    assert torch.equal(smp.last_plr["score"], want)
    assert torch.equal(buf.score[old_ids], want)
