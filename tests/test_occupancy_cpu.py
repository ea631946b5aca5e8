"""The exact state occupancy of tabular agents (RolloutWrapper.policy_occupancy), CPU side: the host surface (header,
ctypes signature, --policy_score_eval, --occupancy_metrics) and pins of the float64 restatement
(tests/occupancy_ref.py) that the GPU kernel is compared against -- above all the duality with tests/polret_ref.py: the
return summed forward over the occupancy equals the return of the backward recursion.  No GPU calls.

The levels and actor tables are test_gpu_polret.py's (its _case and _tables build them on the host); importing that
module needs torch, not a GPU."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import occupancy_ref as ocr
import polret_ref as prf
from test_gpu_optret import _spec
from test_gpu_polret import CASES, _case, _tables

ROOT = Path(__file__).resolve().parents[1]
REF_CASES = ["hand", "debug10", "small"]


# ------------------------------------------------------------------------------------------------ host surface
def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_policy_occupancy\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_policy_occupancy not declared in include/toued.h"
    params = [a.strip() for a in m.group(1).split(",")]
    assert len(params) == 13
    sig = _lib._SIGS["toued_policy_occupancy"]
    assert len(sig) == 13
    import ctypes
    for a, t in zip(params, sig):
        pointer = "*" in a or a.startswith("hipStream_t")
        assert t is (ctypes.c_void_p if pointer else ctypes.c_int), (a, t)
    assert "toued_policy_occupancy" in _lib.exported_symbols()


def test_flags_parse_with_their_defaults():
    from toued.parse_args import parse_args
    a = parse_args([])
    assert a.policy_score_eval == "sampled" and a.occupancy_metrics is False
    a = parse_args(["--policy_score_eval", "exact", "--occupancy_metrics"])
    assert a.policy_score_eval == "exact" and a.occupancy_metrics is True
    with pytest.raises(SystemExit):
        parse_args(["--policy_score_eval", "both"])


def _args(score, mode, extra=()):
    from toued.parse_args import parse_args
    return parse_args(["--env_mode", mode, "--score_function", score, "--num_agents", "8", "--num_mini_batches", "1",
                       *extra])


@pytest.mark.parametrize("score,mode", [("alg_regret", "small"), ("positive_value_loss", "small"),
                                        ("policy_entropy", "rand_dense")])
def test_exact_policy_score_eval_needs_a_policy_score_and_a_tabular_mode(score, mode):
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="policy_score_eval"):
        LevelSampler(_args(score, mode, ["--policy_score_eval", "exact"]), device="cpu")


@pytest.mark.parametrize("score", ["policy_entropy", "least_confidence", "min_margin"])
@pytest.mark.parametrize("extra", [[], ["--use_es"]])
def test_exact_policy_score_eval_accepted(score, extra):
    from toued.level_sampler import LevelSampler
    smp = LevelSampler(_args(score, "small", ["--policy_score_eval", "exact", *extra]), device="cpu")
    assert smp.policy_score_eval == "exact" and smp.regret_eval == "sampled"
    assert LevelSampler(_args(score, "small", extra), device="cpu").policy_score_eval == "sampled"


def test_occupancy_metrics_needs_a_tabular_mode():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="occupancy_metrics"):
        LevelSampler(_args("random", "rand_dense", ["--occupancy_metrics"]), device="cpu")
    LevelSampler(_args("random", "small", ["--occupancy_metrics"]), device="cpu")


def test_non_tabular_wrapper_and_theta_shape_raise_before_any_device_call():
    import torch
    from toued.rollout import RolloutWrapper
    ro = RolloutWrapper("rand_dense", 20)
    levels = torch.zeros((2, 80), dtype=torch.int32)       # host tensors: a device call would fail differently
    with pytest.raises(NotImplementedError):
        ro.policy_occupancy(levels, torch.zeros((2, ro.obs_dim, 5)), 10)
    ro = RolloutWrapper("debug", 20)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_occupancy(levels, torch.zeros((2, ro.obs_dim - 1, 5)), 10)
    with pytest.raises(ValueError, match="theta"):
        ro.policy_occupancy(levels, torch.zeros((2, ro.obs_dim, 5), dtype=torch.float64), 10)


def test_help_and_docstrings_say_what_the_exact_score_is():
    from toued import parse_args as pa
    from toued import plr
    text = pa.build_parser().format_help()
    assert "--policy_score_eval" in text and "--occupancy_metrics" in text
    assert "O(1/T)" in pa.__doc__ and "O(1/T)" in plr.exact_policy_scores.__doc__


# ------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def _occupancies(name):
    mode, params, L, _ = _case(name)
    spec, th = _spec(mode), _tables(name)
    return [ocr.occupancy(spec, params, i, th[i], L) for i in range(params["start_pos"].shape[0])]


@pytest.mark.parametrize("name", REF_CASES)
def test_return_over_the_occupancy_is_the_backward_return(name):
    mode, params, L, _ = _case(name)
    spec, th = _spec(mode), _tables(name)
    for i, occ in enumerate(_occupancies(name)):
        back = prf.policy_return(spec, params, i, th[i], L)
        ret, ret_abs = occ.summary[0], occ.summary[7]
        assert abs(ret - back) <= 1e-12 * max(1.0, ret_abs), (i, ret, back)


@pytest.mark.parametrize("name", REF_CASES)
def test_mass_is_conserved(name):
    _, params, L, _ = _case(name)
    for i, occ in enumerate(_occupancies(name)):
        ret, length, early, alive = occ.summary[:4]
        assert abs(length - occ.visits.sum()) <= 1e-12 * max(1.0, length), i
        assert abs(early + alive - 1.0) <= 1e-12, (i, early, alive)
        assert (occ.rows >= 0.0).all() and (occ.rows.sum(axis=1) <= 1.0 + 1e-12).all(), i
        H = min(int(params["max_steps_in_episode"][i]), L)
        assert occ.rows[0].sum() == 1.0 and not occ.rows[H:].any(), i
        assert 1.0 <= length <= H + 1e-9, (i, length)
        for k in (4, 5, 6):
            assert 0.0 <= occ.summary[k] <= 1.0 + 1e-12, (i, k, occ.summary[k])
        assert (occ.collected >= 0.0).all() and not occ.collected[int(params["n_objs"][i]):].any(), i


def test_zero_length_is_all_zero():
    mode, params, _, _ = _case("debug10")
    occ = ocr.occupancy(_spec(mode), params, 0, _tables("debug10")[0], 0)
    assert not occ.summary.any() and not occ.visits.any() and occ.rows.shape[0] == 0


def test_uniform_policy_terms():
    """Level 0 of a case has the zero table: every visited step has entropy log 5, 1 - max pi = 0.8 and margin 1."""
    occ = _occupancies("small")[0]
    assert occ.summary[4] == pytest.approx(1.0, abs=1e-14)
    assert occ.summary[5] == pytest.approx(0.8, abs=1e-14)
    assert occ.summary[6] == pytest.approx(1.0, abs=1e-14)


def test_deterministic_policy_closed_form():
    """test_polret_cpu.py's closed form, forward: a 2x2 level with one object of reward 0.5 beside the start that
    always respawns and never terminates, under the one-hot policy "right on cell 0, stay on cell 1": the agent sits
    on one state per step, the episode lasts H steps for certain and collects ceil(H / 2) times."""
    from oracle import levels as olv
    import optret_ref as orf
    spec = olv.env_spec("debug")
    H = 7
    p = orf.make_params(spec, grid_size=2, start_pos=0, obj_ids=[0], static_obj_poss=[1], obj_rewards=[0.5, 0.0],
                        obj_p_terminate=[0.0, 0.0], obj_p_respawn=[1.0, 0.0], max_steps=H)
    G2, NE = spec.max_grid_size ** 2, 1 << spec.max_n_objs
    theta = np.zeros((G2 * NE + 1, 5), np.float32)
    for e in range(NE):
        theta[0 + G2 * e, 3] = 1e4
        theta[1 + G2 * e, 4] = 1e4
    occ = ocr.occupancy(spec, p, 0, theta, 10)
    assert np.array_equal(occ.summary, [0.5 * 4, H, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5 * 4])
    assert np.array_equal(occ.collected, [4.0, 0.0])
    assert np.array_equal(np.sort(occ.rows[:H], axis=1)[:, -1], np.ones(H)) and occ.visits.sum() == H


def test_the_clamp_is_inactive_on_every_case():
    """keep = clip(1 - sum p_terminate, 0, 1) is the env's behaviour and polret_ref does not clip: the duality is
    tested where the two agree, on levels whose every collected set has sum p_terminate <= 1."""
    worst = 0.0
    for name in CASES:
        mode, params, _, _ = _case(name)
        for i in range(params["start_pos"].shape[0]):
            worst = max(worst, ocr.collected_sets_p_terminate(_spec(mode), params, i))
    print(f"largest sum of p_terminate over a collected set: {worst:.4f}")
    assert worst <= 1.0
