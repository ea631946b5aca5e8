"""The MaxMC PLR score, CPU side: closed-form pins of the numpy restatement (tests/maxmc_ref.py) that the GPU kernel
is compared against, and the host surface (header, ctypes signature, --score_function max_mc, LevelBuffer.max_return
and its checkpoint) — no GPU calls."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import maxmc_ref as mr

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
GAMMA = 0.99


def _one(reward, done, gamma=GAMMA, prior=None, vcrit=None):
    """One agent, one worker: (score, rmax, wmax[0]) of a reward / done list under a zero critic (or ``vcrit``)."""
    T = len(reward)
    r = np.asarray(reward, f32).reshape(1, T, 1)
    d = np.asarray(done, np.uint8).reshape(1, T, 1)
    vc = np.zeros((1, 3), f32) if vcrit is None else np.asarray(vcrit, f32).reshape(1, -1)
    idx = np.zeros((1, T + 1, 1), np.int32)
    tm = np.zeros((1, T + 1, 1), np.int32)
    pr = None if prior is None else np.asarray([prior], f32)
    score, rmax, wmax = mr.max_mc_scores(vc, idx, tm, r, d, gamma, pr)
    assert rmax.dtype == f32 and wmax.dtype == f32 and score.dtype == np.float64
    return score[0], rmax[0], wmax[0, 0]


def test_done_on_the_last_step_gives_the_negative_return_not_zero():
    """The trailing segment after a done on step T-1 is empty: it must not put a 0 into the maximum."""
    g = f32(GAMMA)
    want = f32(f32(f32(-1.0) + f32(g * f32(-2.0))) + f32(f32(g * g) * f32(-3.0)))
    score, rmax, wmax = _one([-1.0, -2.0, -3.0], [0, 0, 1])
    assert wmax == want and rmax == want and want < 0
    assert score == float(want)                    # zero critic: the score is R_max


def test_without_done_the_truncated_return_counts():
    g = f32(GAMMA)
    want = f32(f32(f32(0.5) + f32(g * f32(-2.0))) + f32(f32(g * g) * f32(4.0)))
    _, rmax, wmax = _one([0.5, -2.0, 4.0], [0, 0, 0])
    assert wmax == want and rmax == want and np.isfinite(want)


def test_open_last_episode_competes_with_the_finished_ones():
    # episodes: [-5] (done), then the open [3, 1]: the truncated return 3 + gamma wins
    _, rmax, _ = _one([-5.0, 3.0, 1.0], [1, 0, 0])
    assert rmax == f32(f32(3.0) + f32(f32(GAMMA) * f32(1.0)))
    # episodes: [2] (done), then the open [-1, -1]: the finished one wins
    _, rmax, _ = _one([2.0, -1.0, -1.0], [1, 0, 0])
    assert rmax == f32(2.0)


def test_done_on_every_step_gives_the_largest_reward():
    rs = np.random.RandomState(0)
    N, T, W = 3, 17, 5
    r = rs.randn(N, T, W).astype(f32)
    wmax = mr.worker_max(r, np.ones((N, T, W), np.uint8), GAMMA)
    np.testing.assert_array_equal(wmax, r.max(axis=1))


def test_gamma_one_gives_plain_sums():
    r = [0.25, 0.5, -1.0, 2.0, 4.0]
    _, rmax, _ = _one(r, [0, 0, 1, 0, 0], gamma=1.0)
    assert rmax == f32(6.0)                        # max(0.25 + 0.5 - 1, 2 + 4), exact in binary
    _, rmax, _ = _one(r, [0, 0, 0, 0, 1], gamma=1.0)
    assert rmax == f32(5.75)


@pytest.mark.parametrize("prior,want", [(-np.inf, 1.5), (-7.0, 1.5), (9.0, 9.0)])
def test_prior_below_or_above_the_rollout_maximum(prior, want):
    score, rmax, wmax = _one([1.5, -1.0], [1, 0], prior=prior)
    assert wmax == f32(1.5)                        # the rollout's own maximum does not see the prior
    assert rmax == f32(want) and score == want


def test_score_is_rmax_minus_the_mean_value_of_the_first_T_rows():
    rs = np.random.RandomState(3)
    N, T, W, D = 2, 9, 4, 6
    vcrit = rs.randn(N, D).astype(f32)
    idx = rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32)
    tm = rs.randint(0, 1000, size=(N, T + 1, W)).astype(np.int32)
    r = rs.randn(N, T, W).astype(f32)
    d = (rs.rand(N, T, W) < 0.3).astype(np.uint8)
    score, rmax, wmax = mr.max_mc_scores(vcrit, idx, tm, r, d, GAMMA)
    np.testing.assert_array_equal(rmax, wmax.max(axis=1))
    v = mr.values(vcrit, idx, tm)
    # the mean of R_max - V(s_t), term by term in float64: row T (the end observation) is not a term
    want = (rmax.astype(np.float64)[:, None, None] - v[:, :T].astype(np.float64)).mean(axis=(1, 2))
    np.testing.assert_allclose(score, want, rtol=1e-13, atol=1e-13)
    idx2 = idx.copy()
    idx2[:, T] = (idx[:, T] + 1) % (D - 1)
    np.testing.assert_array_equal(mr.max_mc_scores(vcrit, idx2, tm, r, d, GAMMA)[0], score)


def test_worker_chains_match_a_scalar_loop():
    """The vectorised restatement against the definition written as one python loop per worker."""
    rs = np.random.RandomState(4)
    N, T, W = 2, 40, 3
    r = rs.randn(N, T, W).astype(f32)
    d = (rs.rand(N, T, W) < 0.15).astype(np.uint8)
    d[0, T - 1, 0] = 1
    d[1, :, 1] = 0
    wmax = mr.worker_max(r, d, GAMMA)
    g = f32(GAMMA)
    for a in range(N):
        for w in range(W):
            cum, disc, best, is_open = f32(0), f32(1), f32(-np.inf), False
            for t in range(T):
                cum = f32(cum + f32(disc * r[a, t, w]))
                disc = f32(disc * g)
                is_open = True
                if d[a, t, w]:
                    best, cum, disc, is_open = max(best, cum), f32(0), f32(1), False
            if is_open:
                best = max(best, cum)
            assert wmax[a, w] == best, (a, w)


# ------------------------------------------------------------------------------------------------ host surface
def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_max_mc_scores\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_max_mc_scores not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 15
    assert len(_lib._SIGS["toued_max_mc_scores"]) == 15
    assert "toued_max_mc_scores" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "toued_max_mc_scores")


def _args(extra=(), mode="debug"):
    from toued.parse_args import parse_args
    return parse_args(["--env_mode", mode, "--score_function", "max_mc", "--num_agents", "8",
                       "--num_mini_batches", "1", *extra])


@pytest.mark.parametrize("mode", ["debug", "small", "mazes", "all_shortlife"])
def test_flag_parses_and_the_sampler_accepts_it(mode):
    from toued.level_sampler import LevelSampler
    assert _args(mode=mode).score_function == "max_mc"
    assert LevelSampler(_args(mode=mode), device="cpu").score_function == "max_mc"


def test_no_tabular_requirement():
    """A non-tabular mode gets past the score function's checks (optimal_regret and return_variance stop there with a
    ValueError) and ends where every score function does on such a mode, at the MLP agents the build does not have."""
    from toued.level_sampler import LevelSampler
    with pytest.raises(NotImplementedError, match="MLP agents"):
        LevelSampler(_args(mode="rand_dense"), device="cpu")


@pytest.mark.parametrize("extra", [["--level_editor", "accel"], ["--score_transform", "rank_sampled"],
                                   ["--staleness_coeff", "0.3", "--level_editor", "accel"]])
def test_accepted_with_the_editor_and_the_replay_flags(extra):
    from toued.level_sampler import LevelSampler
    assert LevelSampler(_args(extra), device="cpu").score_function == "max_mc"


def test_the_pinned_tuples_are_unchanged_and_the_third_mirrors_plr():
    from toued import level_sampler as ls
    from toued import plr
    assert ls.SCORE_FUNCTIONS == ["random", "frozen", "alg_regret", "positive_value_loss", "l1_value_loss",
                                  "optimal_regret"]
    assert ls.MOMENT_SCORE_FUNCTIONS == ("return_variance",)
    assert ls.VALUE_LOSS_FUNCTIONS == ("positive_value_loss", "l1_value_loss")
    assert ls.RETURN_SCORE_FUNCTIONS == ("max_mc",)
    assert set(plr.RETURN_FUNCTIONS) == set(ls.RETURN_SCORE_FUNCTIONS)
    assert plr.RETURN_FUNCTIONS["max_mc"] is plr.max_mc_scores


def test_unknown_score_function_lists_max_mc():
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", "small", "--score_function", "max_mcc", "--num_agents", "8",
                       "--num_mini_batches", "1"])
    with pytest.raises(ValueError, match="not in known functions") as e:
        LevelSampler(args, device="cpu")
    assert "'max_mc'" in str(e.value) and "return_variance" in str(e.value) and "optimal_regret" in str(e.value)


def test_use_es_is_rejected_before_any_device_work():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="max_mc"):
        LevelSampler(_args(["--use_es"]), device="cpu")


def test_exact_regret_eval_is_not_for_this_score():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="regret_eval"):
        LevelSampler(_args(["--regret_eval", "exact"], mode="small"), device="cpu")


def test_level_buffer_field_is_last_and_optional():
    import dataclasses
    from toued.level_sampler import LevelBuffer
    names = [f.name for f in dataclasses.fields(LevelBuffer)]
    assert names == ["levels", "score", "active", "new", "stamp", "clock", "max_return"]
    z = torch.zeros(4)
    stamp = torch.zeros(4, dtype=torch.int32)
    buf = LevelBuffer(z, z, z, z, stamp, 7)                # every earlier positional construction keeps working
    assert buf.stamp is stamp and buf.clock == 7 and buf.max_return is None
    assert LevelBuffer(z, z, z, z).max_return is None


def _packed_buffer(B, mode="all_shortlife"):
    from oracle import jaxrand as jr
    from oracle import levels as olv
    p, lt = olv.reset_env_params(jr.split(jr.PRNGKey(3), B), mode)
    return olv.pack_levels(p, lt, olv.env_spec(mode), np.arange(B, dtype=np.int32))


def test_checkpoint_round_trip_keeps_max_return(tmp_path):
    from toued.checkpoint import (level_buffer_from_state_dict, level_buffer_state_dict, restore_checkpoint,
                                  save_checkpoint)
    from toued.env import get_env_spec
    from toued.level_sampler import LevelBuffer
    B, mode = 12, "all_shortlife"
    spec, _, _ = get_env_spec(mode)
    rs = np.random.RandomState(1)
    packed = torch.from_numpy(_packed_buffer(B, mode))
    base = (packed, torch.from_numpy(rs.randn(B).astype(f32)), torch.from_numpy(rs.rand(B) < 0.3),
            torch.from_numpy(rs.rand(B) < 0.5))
    mret = rs.randn(B).astype(f32)
    mret[[0, 5, 11]] = -np.inf
    for stamp, clock in ((None, 0), (torch.arange(B, dtype=torch.int32), 9)):
        buf = LevelBuffer(*base, stamp, clock, torch.from_numpy(mret.copy()))
        d = level_buffer_state_dict(buf, spec)
        assert list(d)[:4] == ["level", "score", "active", "new"] and list(d)[-1] == "max_return"
        assert d["max_return"].dtype == f32
        sub = str(tmp_path / f"with_{clock}")
        save_checkpoint(sub, d, 3, prefix="buffer_")
        back = level_buffer_from_state_dict(restore_checkpoint(sub, prefix="buffer_"), spec, "cpu")
        assert back.max_return.dtype == torch.float32
        assert torch.equal(back.max_return, buf.max_return)            # -inf entries included
        assert torch.isinf(back.max_return[[0, 5, 11]]).all() and (back.max_return[[0, 5, 11]] < 0).all()
        assert torch.equal(back.levels, buf.levels) and torch.equal(back.score, buf.score)
        assert back.clock == clock and (back.stamp is None) == (stamp is None)
    # a buffer without the field writes no such leaf and restores to None
    plain = LevelBuffer(*base)
    d = level_buffer_state_dict(plain, spec)
    assert list(d) == ["level", "score", "active", "new"]
    save_checkpoint(str(tmp_path / "plain"), d, 3, prefix="buffer_")
    back = level_buffer_from_state_dict(restore_checkpoint(str(tmp_path / "plain"), prefix="buffer_"), spec, "cpu")
    assert back.max_return is None and back.stamp is None


def test_wrapper_rejects_mismatched_shapes_before_any_device_call():
    from toued.rollout import RolloutWrapper, Transition
    ro = RolloutWrapper("debug", 20)
    N, T, W, D = 2, 4, 3, ro.obs_dim
    tr = Transition(torch.zeros((N, T + 1, W), dtype=torch.int32), torch.zeros((N, T, W), dtype=torch.int32),
                    torch.zeros((N, T, W), dtype=torch.uint8), torch.zeros((N, T, W)),
                    torch.zeros((N, T, W), dtype=torch.uint8))
    with pytest.raises(ValueError, match="max_mc_scores"):
        ro.max_mc_scores(tr, torch.zeros((N, D)), GAMMA)
    good = Transition(tr.obs_idx, torch.zeros((N, T + 1, W), dtype=torch.int32), tr.action, tr.reward, tr.done)
    with pytest.raises(ValueError, match="rmax_in"):
        ro.max_mc_scores(good, torch.zeros((N, D)), GAMMA, rmax_in=torch.zeros(N + 1))
