"""The exact optimal return of tabular GridWorld levels (gridworld.py:253-323), CPU side: closed-form pins of the
float64 restatement (tests/optret_ref.py) that the GPU kernel is compared against, and the host surface
(header, ctypes signature, score function, argument checks) — no GPU calls."""
import re
from pathlib import Path

import numpy as np
import pytest

import optret_ref as orf
from oracle import jaxrand as jr
from oracle import levels as olv

ROOT = Path(__file__).resolve().parents[1]


def test_sparse_level_optimum_is_one():
    """`sparse`: a +1 and a -1 object, both ending the episode (p_terminate = 1), never respawning, on an open 13x13
    grid with 50 steps.  The +1 object is at most 24 moves away and the single -1 cell can be walked around, so the
    optimum collects +1 once and the episode ends: V* = 1 exactly."""
    spec = olv.env_spec("sparse")
    params, _ = olv.reset_env_params(jr.split(jr.PRNGKey(3), 2), "sparse")
    for i in range(2):
        assert params["grid_size"][i] == 13 and not params["walls"][i].any()
        assert params["max_steps_in_episode"][i] == 50
        assert orf.optimal_return(spec, params, i, 50) == 1.0


@pytest.mark.parametrize("H,L", [(7, 7), (7, 10), (8, 8), (1, 5), (9, 4)])
def test_respawning_object_closed_form(H, L):
    """A 2x2 level with one object of reward r = 0.5, p_terminate = 0, p_respawn = 1, the start beside the object.

    Count of collections in k steps: the first step moves onto the object and collects it (reward at step 1).  A
    collected object is absent in the next state; an absent object respawns with probability 1 during the following
    step, whatever the agent does, and step_env tests collection against the existence BEFORE the step's respawn.  So
    after a collection at step j the object is absent at step j+1 (nothing to collect, it respawns) and present again
    at step j+2, where the agent collects it by stepping back on (or by staying: action 4 keeps the cell).  No policy
    collects on two consecutive steps, so the collections fall on steps 1, 3, 5, ...: ceil(k / 2) of them, and
    V* = r * ceil(k / 2) with k = min(max_steps, max_rollout_len) unmasked steps."""
    spec = olv.env_spec("debug")
    r = 0.5
    p = orf.make_params(spec, grid_size=2, start_pos=0, obj_ids=[0], static_obj_poss=[1], obj_rewards=[r, 0.0],
                        obj_p_terminate=[0.0, 0.0], obj_p_respawn=[1.0, 0.0], max_steps=H)
    k = min(H, L)
    assert orf.optimal_return(spec, p, 0, L) == r * ((k + 1) // 2)
    # v_t of the start state counts the steps left
    v = orf.optimal_return_all(spec, p, 0, L)
    si = orf.start_index(spec, p, 0)
    for t in range(L):
        left = max(0, k - t)
        assert v[t, si] == r * ((left + 1) // 2), t


def test_invalid_states_are_minus_inf_and_nothing_else():
    """n_objs below max_n_objs, a grid below max_grid_size and walls: for t < max_steps the -inf entries are exactly the
    states with an unused object present, a cell outside the grid or a wall; from max_steps on the rows are 0."""
    spec = olv.env_spec("small")
    keys = jr.split(jr.PRNGKey(5), 16)
    params, _ = olv.reset_env_params(keys, "small")
    pick = [i for i in range(16) if params["n_objs"][i] < spec.max_n_objs and params["grid_size"][i] < 6]
    assert pick
    i = pick[0]
    ms = int(params["max_steps_in_episode"][i])
    L = ms + 3
    v = orf.optimal_return_all(spec, params, i, L)
    inv = orf.invalid_states(spec, params, i)
    assert inv.any() and not inv.all()
    # the invalid set, spelled out again from the level
    G2 = spec.max_grid_size ** 2
    g, nobj = int(params["grid_size"][i]), int(params["n_objs"][i])
    for s in range(v.shape[1]):
        pos, e = s % G2, s // G2
        want = pos >= g * g or bool(params["walls"][i][pos]) or any((e >> o) & 1 for o in range(nobj, spec.max_n_objs))
        assert inv[s] == want
    for t in range(ms):
        assert np.array_equal(np.isneginf(v[t]), inv), t
        assert np.isfinite(v[t][~inv]).all()
    assert not v[ms:].any()


def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_optimal_return\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_optimal_return not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 9
    assert len(_lib._SIGS["toued_optimal_return"]) == 9
    assert "toued_optimal_return" in _lib.exported_symbols()


def test_score_function_registered_and_tabular_only():
    from toued.level_sampler import SCORE_FUNCTIONS, LevelSampler
    from toued.parse_args import parse_args
    assert SCORE_FUNCTIONS[-1] == "optimal_regret"
    assert SCORE_FUNCTIONS[:3] == ["random", "frozen", "alg_regret"]
    args = parse_args(["--env_mode", "rand_dense", "--score_function", "optimal_regret", "--num_agents", "8",
                       "--num_mini_batches", "1"])
    assert args.score_function == "optimal_regret"
    with pytest.raises(ValueError, match="optimal_regret"):
        LevelSampler(args, device="cpu")


def test_non_tabular_wrapper_raises_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("rand_dense", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)       # host tensors: a device call would fail differently
    with pytest.raises(NotImplementedError):
        ro.optimal_return(levels, 10)
    with pytest.raises(NotImplementedError):
        ro.optimal_return(levels[0], 10, return_all=True)
