"""The exact policy return of tabular agents (RolloutWrapper.policy_return), CPU side: pins of the float64 restatement
(tests/polret_ref.py) that the GPU kernel is compared against — a deterministic policy with a closed form, the uniform
policy against an independent Markov-chain computation, the oracle's own rollouts, the ordering below the optimum — and
the host surface (header, ctypes signature, --regret_eval, argument checks).  No GPU calls."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import optret_ref as orf
import polret_ref as prf
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle import rollout as orl
from oracle.modes import ENV_MODE_EPISODE_LEN

ROOT = Path(__file__).resolve().parents[1]
RIGHT, STAY = 3, 4


@pytest.mark.parametrize("H,L", [(7, 7), (7, 10), (8, 8), (1, 5), (9, 4)])
def test_deterministic_policy_closed_form(H, L):
    """The level of test_optret_cpu.py::test_respawning_object_closed_form (2x2, one object of reward 0.5 beside the
    start, p_terminate 0, p_respawn 1) under the policy "right on cell 0, stay on cell 1", a 1e4 logit in an otherwise
    zero table: exp(-1e4) is 0 in float64, so the policy is one-hot.  It steps onto the object (collected at step 1),
    stays while the object is absent (step 2, it respawns) and collects it again by staying (step 3), and so on:
    ceil(k / 2) collections in k = min(H, L) steps, the optimum."""
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
    assert prf.policy_return(spec, p, 0, theta, L) == r * ((k + 1) // 2)
    v = prf.policy_return_all(spec, p, 0, theta, L)
    si = orf.start_index(spec, p, 0)
    for t in range(L):
        assert v[t, si] == r * ((max(0, k - t) + 1) // 2), t


def test_uniform_policy_is_a_hitting_probability():
    """theta = 0 (uniform policy) on a 2x2 level whose one object (reward 1) ends the episode and never respawns:
    the return is the probability that the walk reaches the object's cell within max_steps = 6 steps, computed here
    from the 4x4 cell transition matrix with the object's cell made absorbing."""
    spec = olv.env_spec("debug")
    start, obj = 0, 3
    p = orf.make_params(spec, grid_size=2, start_pos=start, obj_ids=[0], static_obj_poss=[obj], obj_rewards=[1.0, 0.0],
                        obj_p_terminate=[1.0, 0.0], obj_p_respawn=[0.0, 0.0], max_steps=6)
    # moves on the 2x2 lattice (cell = 2 * row + column): up, down, left, right, stay
    P = np.zeros((4, 4))
    for c in range(4):
        row, col = divmod(c, 2)
        for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)):
            r2, c2 = min(max(row + dr, 0), 1), min(max(col + dc, 0), 1)
            P[c, 2 * r2 + c2] += 0.2
    P[obj] = 0.0
    P[obj, obj] = 1.0
    d = np.zeros(4)
    d[start] = 1.0
    for _ in range(6):
        d = d @ P
    theta = np.zeros((spec.obs_dim, 5), np.float32)
    for L in (6, 9):
        assert abs(prf.policy_return(spec, p, 0, theta, L) - d[obj]) <= 1e-12
    assert 0.3 < d[obj] < 0.9


# ------------------------------------------------------------------------------- against the oracle's rollouts
MC_WORKERS = 1024
MC_CASES = {"debug": (16, 301), "small": (8, 302)}      # mode -> (levels, seed of the level and rollout keys)


@functools.lru_cache(maxsize=None)
def _mc_case(mode):
    """(spec, params, theta, exact float64 [n], sampled first-episode returns f32 [n, MC_WORKERS])."""
    n, seed = MC_CASES[mode]
    spec = olv.env_spec(mode)
    params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(seed), n), mode)
    theta = prf.random_tables(seed, n, spec.obs_dim)
    T = ENV_MODE_EPISODE_LEN[mode]
    exact = np.array([prf.policy_return(spec, params, i, theta[i], T) for i in range(n)])
    state = orl.batch_reset(spec, jr.split(jr.PRNGKey(seed + 10), n), params, MC_WORKERS)
    _, _, cum = orl.batch_rollout(spec, jr.split(jr.PRNGKey(seed + 20), n), theta, params, state, T)
    return spec, params, theta, exact, cum


@pytest.mark.parametrize("mode", list(MC_CASES))
def test_reference_agrees_with_the_oracle_rollouts(mode):
    _, params, _, exact, cum = _mc_case(mode)
    for i in range(exact.shape[0]):
        mean = float(cum[i].astype(np.float64).mean())
        tol = prf.mc_tolerance(cum[i], params["obj_rewards"][i])
        print(f"{mode} level {i}: sampled {mean:+.5f} exact {exact[i]:+.5f} tolerance {tol:.5f}")
        assert abs(mean - exact[i]) <= tol, (i, mean, exact[i], tol)


@pytest.mark.parametrize("mode", list(MC_CASES))
def test_policy_return_is_at_most_the_optimum(mode):
    spec, params, _, exact, _ = _mc_case(mode)
    T = ENV_MODE_EPISODE_LEN[mode]
    for i in range(exact.shape[0]):
        assert exact[i] <= orf.optimal_return(spec, params, i, T), i


# ------------------------------------------------------------------------------------------------ host surface
def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_policy_return\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_policy_return not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 11
    assert len(_lib._SIGS["toued_policy_return"]) == 11
    assert "toued_policy_return" in _lib.exported_symbols()


def test_regret_eval_flag():
    from toued.parse_args import parse_args
    assert parse_args([]).regret_eval == "sampled"
    assert parse_args(["--regret_eval", "exact"]).regret_eval == "exact"


@pytest.mark.parametrize("flags", [["--env_mode", "rand_dense", "--score_function", "alg_regret"],
                                   ["--env_mode", "small", "--score_function", "random"],
                                   ["--env_mode", "small", "--score_function", "positive_value_loss"]])
def test_exact_regret_eval_needs_a_regret_score_and_a_tabular_mode(flags):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(flags + ["--regret_eval", "exact", "--num_agents", "8", "--num_mini_batches", "1"])
    with pytest.raises(ValueError, match="regret_eval"):
        LevelSampler(args, device="cpu")


def test_exact_regret_eval_accepted_on_tabular_regret_scores():
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    for fn in ("alg_regret", "optimal_regret"):
        args = parse_args(["--env_mode", "small", "--score_function", fn, "--regret_eval", "exact", "--num_agents",
                           "8", "--num_mini_batches", "1"])
        assert LevelSampler(args, device="cpu").regret_eval == "exact"


def test_non_tabular_wrapper_raises_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("rand_dense", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)       # host tensors: a device call would fail differently
    theta = torch.zeros((2, ro.obs_dim, 5))
    with pytest.raises(NotImplementedError):
        ro.policy_return(levels, theta, 10)
    with pytest.raises(NotImplementedError):
        ro.policy_return(levels[0], theta[0], 10, return_all=True)


def test_theta_shape_is_checked_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("debug", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return(levels, torch.zeros((2, ro.obs_dim - 1, 5)), 10)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return(levels, torch.zeros((3, ro.obs_dim, 5)), 10)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_return(levels, torch.zeros((2, ro.obs_dim, 5), dtype=torch.float64), 10)
    with pytest.raises(ValueError, match="theta"):                 # the table on another device than the levels
        ro.policy_return(levels, torch.zeros((2, ro.obs_dim, 5), device="meta"), 10)
