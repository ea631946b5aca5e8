"""The exact return variance of tabular agents (RolloutWrapper.policy_return_moments) and the return_variance score,
CPU side: pins of the float64 restatement (tests/polvar_ref.py) that the GPU kernel is compared against — two closed
forms, an independent forward enumeration of the return's whole distribution, polret_ref's mean, the oracle's own
rollouts — and the host surface (header, ctypes signature, --score_function return_variance, argument checks).
No GPU calls."""
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

import optret_ref as orf
import polret_ref as prf
import polvar_ref as pvf
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle.modes import ENV_MODE_EPISODE_LEN
from test_polret_cpu import MC_CASES, _mc_case

ROOT = Path(__file__).resolve().parents[1]
RIGHT, STAY = 3, 4


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("r", [0.5, -0.3, 1.0, 0.75])
def test_one_step_bernoulli_closed_form(r):
    """2x2, start 0, one object of reward r on cell 1, p_terminate 0, one step, the uniform policy: one action in five
    reaches the object, so the return is r with probability 0.2 and 0 otherwise.  |r| <= 1, the environment's range
    of rewards: the absolute bound 1e-15 is then a few ulps of every intermediate."""
    spec = olv.env_spec("debug")
    p = orf.make_params(spec, grid_size=2, start_pos=0, obj_ids=[0], static_obj_poss=[1], obj_rewards=[r, 0.0],
                        obj_p_terminate=[0.0, 0.0], obj_p_respawn=[0.0, 0.0], max_steps=1)
    theta = np.zeros((spec.obs_dim, 5), np.float32)
    r32 = float(np.float32(r))
    for L in (1, 4):
        mean, var = pvf.moments(spec, p, 0, theta, L)
        assert abs(mean - 0.2 * r32) <= 1e-15
        assert abs(var - r32 * r32 * 0.2 * 0.8) <= 1e-15


@pytest.mark.parametrize("H,L", [(7, 7), (7, 10), (8, 8), (1, 5), (9, 4)])
def test_deterministic_policy_has_zero_variance(H, L):
    """test_polret_cpu.py::test_deterministic_policy_closed_form's level and one-hot policy (p_terminate 0,
    p_respawn 1): nothing is random, the variance is exactly 0 at every t, and the mean is that test's."""
    spec = olv.env_spec("debug")
    r = 0.5
    p = orf.make_params(spec, grid_size=2, start_pos=0, obj_ids=[0], static_obj_poss=[1], obj_rewards=[r, 0.0],
                        obj_p_terminate=[0.0, 0.0], obj_p_respawn=[1.0, 0.0], max_steps=H)
    G2, NE = spec.max_grid_size ** 2, 1 << spec.max_n_objs
    theta = np.zeros((G2 * NE + 1, 5), np.float32)
    for e in range(NE):
        theta[0 + G2 * e, RIGHT] = 1e4
        theta[1 + G2 * e, STAY] = 1e4
    k = min(H, L)
    assert pvf.moments(spec, p, 0, theta, L) == (r * ((k + 1) // 2), 0.0)
    v, u = pvf.moments_all(spec, p, 0, theta, L)
    si = orf.start_index(spec, p, 0)
    for t in range(L):
        assert v[t, si] == r * ((max(0, k - t) + 1) // 2), t
        assert u[t, si] == 0.0, t


def test_table_masks_and_zero_rows():
    spec = olv.env_spec("debug")
    params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(505), 4), "debug")
    theta = prf.random_tables(505, 4, spec.obs_dim)
    for i in range(4):
        L = int(params["max_steps_in_episode"][i]) + 3
        v, u = pvf.moments_all(spec, params, i, theta[i], L)
        inv = orf.invalid_states(spec, params, i)
        ms = int(params["max_steps_in_episode"][i])
        assert not v[ms:].any() and not u[ms:].any()
        assert (u[:ms, inv] == -np.inf).all() and np.isfinite(u[:ms, ~inv]).all()
        assert np.array_equal(np.isfinite(u), np.isfinite(v))
    assert pvf.moments(spec, params, 0, theta[0], 0) == (0.0, 0.0)


# ------------------------------------------------------------------------------- independent forward enumeration
def _enumerate(spec, params, i, theta, L):
    """(mean, variance) of the first-episode return from the exact joint distribution over (cell, existence mask,
    accumulated return) and the finished episodes' returns, propagated forward step by step with scalar dynamics
    written for this test: no value table, no backward recursion."""
    G2 = spec.max_grid_size ** 2
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    walls = np.asarray(params["walls"][i], bool)
    static = [int(x) for x in params["static_obj_poss"][i]]
    ids = [int(x) for x in params["obj_ids"][i]]
    rew = [float(params["obj_rewards"][i][ids[o]]) for o in range(nobj)]
    pterm = [float(params["obj_p_terminate"][i][ids[o]]) for o in range(nobj)]
    presp = [float(params["obj_p_respawn"][i][ids[o]]) for o in range(nobj)]
    H = min(int(params["max_steps_in_episode"][i]), L)

    def move(pos, a):
        row, col = divmod(pos, g)
        dr, dc = ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0))[a]
        r2, c2 = row + dr, col + dc
        if not (0 <= r2 < g and 0 <= c2 < g) or walls[r2 * g + c2]:
            return pos
        return r2 * g + c2

    live = {(int(params["start_pos"][i]), (1 << nobj) - 1, 0.0): 1.0}
    ended = defaultdict(float)
    for t in range(H):
        pi = prf.policy(theta, t)
        nxt = defaultdict(float)
        for (pos, e, G), p in live.items():
            for a in range(5):
                pa = p * pi[pos + G2 * e, a]
                if pa == 0.0:
                    continue
                p1 = move(pos, a)
                coll = [o for o in range(nobj) if (e >> o) & 1 and static[o] == p1]
                G1 = G + sum(rew[o] for o in coll)
                pt = sum(pterm[o] for o in coll)
                assert 0.0 <= pt <= 1.0
                ended[G1] += pa * pt
                keep = e
                for o in coll:
                    keep &= ~(1 << o)
                absent = [o for o in range(nobj) if not (e >> o) & 1]
                for R in range(1 << len(absent)):
                    pr, back = 1.0, 0
                    for j, o in enumerate(absent):
                        if (R >> j) & 1:
                            pr, back = pr * presp[o], back | (1 << o)
                        else:
                            pr *= 1.0 - presp[o]
                    if pr > 0.0:
                        nxt[(p1, keep | back, G1)] += pa * (1.0 - pt) * pr
        live = nxt
    for (_, _, G), p in live.items():
        ended[G] += p
    gs, ps = np.array(list(ended.keys())), np.array(list(ended.values()))
    assert abs(ps.sum() - 1.0) <= 1e-12
    mean = float((ps * gs).sum())
    return mean, float((ps * (gs - mean) ** 2).sum())


def _enum_cases():
    """(params, index, theta, L): ten generated `debug` levels with random tables, and a hand level whose only
    randomness is p_terminate (one-hot policy, p_respawn 1)."""
    spec = olv.env_spec("debug")
    params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(501), 10), "debug")
    theta = prf.random_tables(501, 10, spec.obs_dim)
    theta[0] = 0.0
    cases = [(params, i, theta[i], (6, 5, 4, 6, 3)[i % 5]) for i in range(10)]
    p = orf.make_params(spec, grid_size=2, start_pos=0, obj_ids=[0], static_obj_poss=[1], obj_rewards=[0.5, 0.0],
                        obj_p_terminate=[0.3, 0.0], obj_p_respawn=[1.0, 0.0], max_steps=6)
    G2, NE = spec.max_grid_size ** 2, 1 << spec.max_n_objs
    hot = np.zeros((G2 * NE + 1, 5), np.float32)
    for e in range(NE):
        hot[0 + G2 * e, RIGHT] = 1e4
        hot[1 + G2 * e, STAY] = 1e4
    return spec, cases + [(p, 0, hot, 6)]


def test_forward_enumeration_agrees():
    spec, cases = _enum_cases()
    assert len(cases) >= 9
    positive = 0
    for k, (params, i, theta, L) in enumerate(cases):
        mean, var = pvf.moments(spec, params, i, theta, L)
        emean, evar = _enumerate(spec, params, i, theta, L)
        print(f"case {k}: mean {mean:+.6f} / {emean:+.6f}, variance {var:.6e} / {evar:.6e}")
        assert abs(mean - emean) <= 1e-12 and abs(var - evar) <= 1e-12, (k, mean, emean, var, evar)
        positive += evar > 1e-6
    assert positive >= 5
    # the termination-only level: collections at steps 1, 3, 5, each ending the episode with probability 0.3
    params, i, theta, L = cases[-1]
    pt = float(np.float32(0.3))                         # the level holds its probabilities as f32
    ps, gs = np.array([pt, (1.0 - pt) * pt, (1.0 - pt) ** 2]), np.array([0.5, 1.0, 1.5])
    m = (ps * gs).sum()
    mean, var = pvf.moments(spec, params, i, theta, L)
    assert abs(mean - m) <= 1e-12 and abs(var - (ps * (gs - m) ** 2).sum()) <= 1e-12 and var > 0.1


# ------------------------------------------------------------------------------------- the mean; oracle rollouts
@pytest.mark.parametrize("mode", list(MC_CASES))
def test_mean_is_polret_ref_and_variance_is_not_negative(mode):
    spec, params, theta, exact, _ = _mc_case(mode)
    T = ENV_MODE_EPISODE_LEN[mode]
    umin = 0.0
    for i in range(exact.shape[0]):
        v, u = pvf.moments_all(spec, params, i, theta[i], T)
        si = orf.start_index(spec, params, i)
        assert abs(v[0, si] - exact[i]) <= 1e-12, i
        assert np.allclose(v, prf.policy_return_all(spec, params, i, theta[i], T), rtol=0.0, atol=1e-12,
                           equal_nan=True)
        umin = min(umin, float(u[np.isfinite(u)].min()))
    print(f"{mode}: smallest u over all table entries {umin:.3e}")
    assert umin >= -1e-12          # roundings of the last subtraction only (kept, not clamped)


@pytest.mark.parametrize("mode", list(MC_CASES))
def test_reference_agrees_with_the_oracle_rollouts(mode):
    """The sample variance of the oracle's 1024 first-episode returns per level against the exact variance, within
    polvar_ref.variance_tolerance: 5 standard errors of the sample variance plus 8 R^2 / M."""
    spec, params, theta, _, cum = _mc_case(mode)
    T = ENV_MODE_EPISODE_LEN[mode]
    for i in range(cum.shape[0]):
        _, u0 = pvf.moments(spec, params, i, theta[i], T)
        s2, tol = pvf.variance_tolerance(cum[i], params["obj_rewards"][i])
        print(f"{mode} level {i}: sampled {s2:.5f} exact {u0:.5f} tolerance {tol:.5f}")
        assert abs(s2 - u0) <= tol, (i, s2, u0, tol)


# ------------------------------------------------------------------------------------------------ host surface
def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_policy_return_moments\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_policy_return_moments not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 13
    assert len(_lib._SIGS["toued_policy_return_moments"]) == 13
    assert "toued_policy_return_moments" in _lib.exported_symbols()


def _args(mode, extra=()):
    from toued.parse_args import parse_args
    return parse_args(["--env_mode", mode, "--score_function", "return_variance", "--num_agents", "8",
                       "--num_mini_batches", "1", *extra])


def test_score_function_accepted_beside_the_pinned_list():
    from toued import level_sampler as ls
    from toued import plr
    assert ls.SCORE_FUNCTIONS == ["random", "frozen", "alg_regret", "positive_value_loss", "l1_value_loss",
                                  "optimal_regret"]
    assert ls.MOMENT_SCORE_FUNCTIONS == ("return_variance",)
    assert set(plr.MOMENT_FUNCTIONS) == set(ls.MOMENT_SCORE_FUNCTIONS)
    assert _args("small").score_function == "return_variance"
    smp = ls.LevelSampler(_args("small"), device="cpu")
    assert smp.score_function == "return_variance" and smp.regret_eval == "sampled"


@pytest.mark.parametrize("extra", [["--use_es"], ["--level_editor", "accel"], ["--score_transform", "proportional"],
                                   ["--score_transform", "rank_sampled"], ["--staleness_coeff", "0.3"],
                                   ["--use_es", "--level_editor", "accel", "--score_transform", "rank_sampled",
                                    "--staleness_coeff", "0.5"]])
def test_score_function_accepted_with(extra):
    from toued.level_sampler import LevelSampler
    assert LevelSampler(_args("small", extra), device="cpu").score_function == "return_variance"


def test_score_function_needs_a_tabular_mode():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="tabular"):
        LevelSampler(_args("rand_dense"), device="cpu")


def test_unknown_score_function_lists_both_tuples():
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "small", "--score_function", "return_skewness", "--num_agents", "8",
                       "--num_mini_batches", "1"])
    with pytest.raises(ValueError, match="not in known functions") as e:
        LevelSampler(args, device="cpu")
    assert "optimal_regret" in str(e.value) and "return_variance" in str(e.value)


def test_exact_regret_eval_is_not_for_this_score():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="regret_eval"):
        LevelSampler(_args("small", ["--regret_eval", "exact"]), device="cpu")


def test_non_tabular_wrapper_raises_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("rand_dense", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)       # host tensors: a device call would fail differently
    theta = torch.zeros((2, ro.obs_dim, 5))
    with pytest.raises(NotImplementedError):
        ro.policy_return_moments(levels, theta, 10)
    with pytest.raises(NotImplementedError):
        ro.policy_return_moments(levels[0], theta[0], 10, return_all=True)


def test_theta_shape_is_checked_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("debug", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return_moments(levels, torch.zeros((2, ro.obs_dim - 1, 5)), 10)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return_moments(levels, torch.zeros((3, ro.obs_dim, 5)), 10)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return_moments(levels, torch.zeros((2, ro.obs_dim, 5), dtype=torch.float64), 10)
    with pytest.raises(ValueError, match="theta"):                 # the table on another device than the levels
        ro.policy_return_moments(levels, torch.zeros((2, ro.obs_dim, 5), device="meta"), 10)
    with pytest.raises(ValueError, match="theta"):                 # the single-agent form goes through the same check
        ro.policy_return_moments(levels[0], torch.zeros((ro.obs_dim - 1, 5)), 10)
