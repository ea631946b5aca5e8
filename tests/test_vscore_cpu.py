"""The value-loss PLR scores (positive value loss, L1 value loss), CPU side: closed-form pins of the numpy restatement
(tests/vscore_ref.py) that the GPU kernel is compared against, and the host surface (header, ctypes signature, score
function names, argument checks) — no GPU calls."""
import re
from pathlib import Path

import numpy as np
import pytest

import vscore_ref as vr

ROOT = Path(__file__).resolve().parents[1]
GAMMA, LAM = 0.99, 0.95


def _geometric(T):
    """adv_t of reward 1, value 0, no done (tests/test_gpu_gae.py): g = 1 + f32(gamma lambda) g from the end, f32."""
    c = np.float32(GAMMA * LAM)
    ref = np.zeros(T, np.float32)
    g = np.float32(0.0)
    for t in reversed(range(T)):
        g = np.float32(np.float32(1.0) + c * g)
        ref[t] = g
    return ref


def _traj(N, T, W, D, seed=0):
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32)
    time = rs.randint(0, 1000, size=(N, T + 1, W)).astype(np.int32)
    return idx, time


def test_zero_critic_unit_reward_is_the_geometric_sum():
    N, T, W, D = 2, 20, 3, 7
    idx, time = _traj(N, T, W, D)
    vcrit = np.zeros((N, D), np.float32)
    r = np.ones((N, T, W), np.float32)
    d = np.zeros((N, T, W), np.uint8)
    pvl, l1, adv = vr.value_loss_scores(vcrit, idx, time, r, d, GAMMA, LAM)
    ref = _geometric(T)
    np.testing.assert_array_equal(adv, np.broadcast_to(ref[None, :, None], (N, T, W)))
    want = ref.astype(np.float64).mean()
    np.testing.assert_allclose(pvl, want, rtol=1e-15)
    np.testing.assert_array_equal(pvl, l1)
    closed = np.array([(1 - float(np.float32(GAMMA * LAM)) ** (T - t)) / (1 - float(np.float32(GAMMA * LAM)))
                       for t in range(T)])
    np.testing.assert_allclose(adv[0, :, 0], closed, rtol=1e-5)


def test_negative_reward_has_zero_positive_value_loss():
    N, T, W, D = 2, 20, 3, 7
    idx, time = _traj(N, T, W, D, seed=1)
    vcrit = np.zeros((N, D), np.float32)
    r = -np.ones((N, T, W), np.float32)
    d = np.zeros((N, T, W), np.uint8)
    pvl, l1, adv = vr.value_loss_scores(vcrit, idx, time, r, d, GAMMA, LAM)
    assert (adv < 0).all()
    assert (pvl == 0.0).all()
    np.testing.assert_allclose(l1, _geometric(T).astype(np.float64).mean(), rtol=1e-15)


def test_all_done_advantage_is_reward_minus_value():
    N, T, W, D = 3, 9, 5, 11
    rs = np.random.RandomState(2)
    idx, time = _traj(N, T, W, D, seed=2)
    vcrit = rs.randn(N, D).astype(np.float32)
    r = rs.randn(N, T, W).astype(np.float32)
    d = np.ones((N, T, W), np.uint8)
    pvl, l1, adv = vr.value_loss_scores(vcrit, idx, time, r, d, GAMMA, LAM)
    v = vr.values(vcrit, idx, time)
    np.testing.assert_array_equal(adv, r - v[:, :T])          # one f32 subtraction
    a64 = adv.astype(np.float64).reshape(N, -1)
    np.testing.assert_allclose(pvl, np.maximum(a64, 0).sum(axis=1) / (T * W), rtol=1e-14)
    np.testing.assert_allclose(l1, np.abs(a64).sum(axis=1) / (T * W), rtol=1e-14)


def test_values_follow_the_critic_formula():
    """v = vcrit[idx] + ((float)time * 0.001f) * vcrit[D-1], one f32 rounding per operation."""
    f = np.float32
    vcrit = np.array([[0.5, -1.25, 3.0]], f)
    idx = np.array([[[0, 1]], [[1, 0]]], np.int32).reshape(1, 2, 2)
    time = np.array([[[7, 333]], [[999, 0]]], np.int32).reshape(1, 2, 2)
    v = vr.values(vcrit, idx, time)
    for t in range(2):
        for w in range(2):
            want = f(vcrit[0, idx[0, t, w]] + f(f(f(time[0, t, w]) * f(0.001)) * f(3.0)))
            assert v[0, t, w] == want


def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_value_loss_scores\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_value_loss_scores not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 15
    assert len(_lib._SIGS["toued_value_loss_scores"]) == 15
    assert "toued_value_loss_scores" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "toued_value_loss_scores")


@pytest.mark.parametrize("name", ["positive_value_loss", "l1_value_loss"])
def test_parse_args_accepts_the_score_function(name):
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "debug", "--score_function", name, "--num_agents", "8",
                       "--num_mini_batches", "1"])
    assert args.score_function == name


def test_score_function_order():
    from toued.level_sampler import SCORE_FUNCTIONS
    assert SCORE_FUNCTIONS == ["random", "frozen", "alg_regret", "positive_value_loss", "l1_value_loss",
                               "optimal_regret"]


@pytest.mark.parametrize("name", ["positive_value_loss", "l1_value_loss"])
def test_use_es_is_rejected_before_any_device_work(name):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "debug", "--score_function", name, "--num_agents", "8",
                       "--num_mini_batches", "1", "--use_es"])
    with pytest.raises(ValueError, match=name):
        LevelSampler(args, device="cpu")
