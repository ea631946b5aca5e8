"""The policy PLR scores (policy entropy, least confidence, min margin), CPU side: the numpy restatement
(tests/polscore_ref.py) that the GPU kernel is compared against, pinned to the float64 form of the same definitions and
to their closed-form properties, and the host surface (header, ctypes signature, --score_function policy_entropy /
least_confidence / min_margin) — no GPU calls."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import polscore_ref as pr

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
NAMES = ("policy_entropy", "least_confidence", "min_margin")

# (N, T, W, D, first_scale): five agents, so every table scale of polscore_ref.SCALES, the tied rows and the clamped
# indices are in each case
F64_CASES = [(5, 20, 4, 19, 0), (5, 50, 64, 677, 1), (5, 8, 256, 65, 2)]
# 4 x the worst |float32 restatement - float64 form| measured on F64_CASES, per score (see the test's docstring)
F64_BOUND = (4 * 1.87e-8, 4 * 1.20e-8, 4 * 1.13e-8)


@pytest.mark.parametrize("case", F64_CASES)
def test_restatement_matches_the_float64_form(case):
    """The float32 restatement's scores against policy_scores_f64 on the same inputs.  Measured worst deviation over
    F64_CASES (numpy 2.2, glibc libm): entropy 1.87e-8, least confidence 1.20e-8, min margin 1.13e-8 -- the zero
    table's terms, f32(log 5) against log 5 and f32(1 - f32(0.2)) against 0.8, which every step repeats; the per-step
    terms of the other tables differ by up to 1.8e-5 (scale 300: logits near 1000 carry 6e-5 of rounding) and average
    out.  The bound is 4 x the measured figure, to cover other libm builds."""
    N, T, W, D, fs = case
    c = pr.make_case(N, T, W, D, fs)
    got = pr.policy_scores(c["theta"], c["idx"], c["time"])
    want = pr.policy_scores_f64(c["theta"], c["idx"], c["time"])
    for name, g, w, bound in zip(NAMES, got, want, F64_BOUND):
        assert g.dtype == np.float64 and g.shape == (N,)
        dev = np.abs(g - w).max()
        print(f"{name}: worst |f32 restatement - f64| {dev:.3e}, bound {bound:.3e}")
        assert dev <= bound, (name, dev, bound)


def _one(rows, idx=0, time=0):
    """One agent, one worker, one step on the table ``rows`` [D][5]: the float64 scores and the float32 restatement's."""
    theta = np.asarray(rows, f32).reshape(1, -1, 5)
    ix = np.full((1, 2, 1), idx, np.int32)
    tm = np.full((1, 2, 1), time, np.int32)
    return ([float(x[0]) for x in pr.policy_scores_f64(theta, ix, tm)],
            [float(x[0]) for x in pr.policy_scores(theta, ix, tm)])


def test_zero_table_is_the_uniform_policy():
    s64, s32 = _one(np.zeros((3, 5)), time=1234)
    assert s64[0] == pytest.approx(1.0, abs=1e-15) and s64[1] == pytest.approx(0.8, abs=1e-15) and s64[2] == 1.0
    assert s32[0] == pytest.approx(1.0, abs=1e-7) and s32[1] == pytest.approx(0.8, abs=1e-7) and s32[2] == 1.0


def test_one_logit_far_above_the_rest_is_the_deterministic_policy():
    rows = np.zeros((3, 5))
    rows[0, 3] = 200.0
    s64, s32 = _one(rows)
    # float64: least confidence and min margin are 0 exactly; the entropy is its analytic value 4 * 200 * exp(-200)
    # (1.1e-84 before the division by log 5), zero at any precision a score is kept in
    assert s64[1:] == [0.0, 0.0]
    assert s64[0] == pytest.approx(800.0 * math.exp(-200.0) / math.log(5), rel=1e-12) and s64[0] < 1e-80
    assert s32 == [0.0, 0.0, 0.0]                  # exp(-200) underflows to 0 in float32


def test_two_equal_top_logits_give_a_min_margin_term_of_one():
    rows = np.array([[0.5, 2.0, -1.0, 2.0, 0.25], [0.0] * 5, [0.0] * 5])
    for s in _one(rows):
        assert s[2] == 1.0
        assert 0.0 < s[1] < 0.8 and 0.0 < s[0] < 1.0
    # with a time row that moves both by the same amount
    rows[2] = [-0.3, 0.7, 0.1, 0.7, 0.2]
    for s in _one(rows, time=1999):
        assert s[2] == 1.0


def test_scores_lie_in_the_unit_interval():
    for case in F64_CASES:
        c = pr.make_case(*case)
        for s in pr.policy_scores_f64(c["theta"], c["idx"], c["time"]) + pr.policy_scores(c["theta"], c["idx"],
                                                                                          c["time"]):
            assert (s >= 0.0).all() and (s <= 1.0 + 1e-7).all()
        t = pr.terms_f64(c["theta"], c["idx"], c["time"])
        assert (t >= 0.0).all() and (t[:, 0] <= math.log(5) + 1e-12).all() and (t[:, 1:] <= 1.0).all()
        assert (t[:, 1] <= 0.8 + 1e-12).all()            # the largest of five probabilities is at least 1/5
        assert (t[:, 2] >= t[:, 1] - 1e-15).all()        # 1 - (p1 - p2) >= 1 - p1


def test_a_constant_added_to_a_table_row_changes_nothing():
    c = pr.make_case(5, 20, 4, 19, 0)
    theta = c["theta"].astype(np.float64)
    shifted = theta.copy()
    shifted[:, ::2] += 0.75                         # every second row, the time row (D - 1 = 18) included
    base = pr.terms_f64(theta, c["idx"], c["time"])
    # float64 tables: the shift is exact up to the rounding of l + 0.75, far below the tolerance
    l_abs = np.abs(theta).max() * 3.0 + 1.0
    moved = _terms_f64_of_f64_table(shifted, c["idx"], c["time"])
    np.testing.assert_allclose(moved, base, rtol=0, atol=64 * l_abs * 2.0 ** -52)


def _terms_f64_of_f64_table(theta, idx, time):
    """polscore_ref.terms_f64 on a float64 table (the restatement's own entry point rounds its table to float32)."""
    N, D = theta.shape[0], theta.shape[1]
    i = np.where((idx >= 0) & (idx < D - 1), idx, D - 1)
    row = theta[np.arange(N).reshape(N, 1, 1), i]
    l = row + (time.astype(np.float64)[..., None] * 0.001) * theta[:, D - 1][:, None, None, :]
    d = l - l.max(axis=-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=-1, keepdims=True)
    p = e / s
    ps = np.sort(p, axis=-1)
    return np.stack([-(p * (d - np.log(s))).sum(axis=-1), 1.0 - ps[..., 4], 1.0 - (ps[..., 4] - ps[..., 3])], axis=1)


def test_rows_past_T_and_indices_outside_the_table():
    c = pr.make_case(2, 6, 3, 9, 2)
    base = pr.policy_scores(c["theta"], c["idx"], c["time"])
    idx2 = c["idx"].copy()
    idx2[:, 6] = (idx2[:, 6] + 1) % 8               # the end observation is not a term
    for x, y in zip(pr.policy_scores(c["theta"], idx2, c["time"]), base):
        np.testing.assert_array_equal(x, y)
    assert c["idx"][0, 0, 0] == 9 + 3 and c["idx"][0, 0, 1] == -1      # make_case's clamped indices
    idx3 = c["idx"].copy()
    idx3[0, 0, :2] = 8                              # the same pairs on row D - 1 itself
    for x, y in zip(pr.policy_scores(c["theta"], idx3, c["time"]), base):
        np.testing.assert_array_equal(x, y)


def test_probabilities_are_the_oracle_rollouts():
    """p of the restatement against oracle/rollout.py's actor (logits_of, softmax), the distribution the numpy rollout
    draws its actions from: bit for bit."""
    from oracle import rollout as oro
    c = pr.make_case(3, 5, 4, 11, 2)
    idx, time = c["idx"][:, :5], c["time"][:, :5]
    p, _ = pr.probs_terms(c["theta"], idx, time)
    held = np.where((idx >= 0) & (idx < 10), idx, 10)
    np.testing.assert_array_equal(p, oro.softmax(oro.logits_of(c["theta"], held, time)))


# ------------------------------------------------------------------------------------------------ host surface
def test_entry_point_declared_and_bound():
    from toued import _lib
    text = (ROOT / "include" / "toued.h").read_text()
    m = re.search(r"\bint\s+toued_policy_scores\s*\(([^)]*)\)\s*;", text)
    assert m, "toued_policy_scores not declared in include/toued.h"
    assert len(m.group(1).split(",")) == 12
    assert len(_lib._SIGS["toued_policy_scores"]) == 12
    assert "toued_policy_scores" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "toued_policy_scores")


def _args(name, extra=(), mode="debug"):
    from toued.parse_args import parse_args
    return parse_args(["--env_mode", mode, "--score_function", name, "--num_agents", "8",
                       "--num_mini_batches", "1", *extra])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["debug", "small", "mazes", "all_shortlife"])
def test_flag_parses_and_the_sampler_accepts_it(name, mode):
    from toued.level_sampler import LevelSampler
    assert _args(name, mode=mode).score_function == name
    smp = LevelSampler(_args(name, mode=mode), device="cpu")
    assert smp.score_function == name and smp.regret_eval == "sampled"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("extra", [["--use_es"], ["--use_es", "--lifetime_conditioning"], ["--level_editor", "accel"],
                                   ["--score_transform", "rank_sampled"], ["--score_transform", "proportional"],
                                   ["--staleness_coeff", "0.3", "--level_editor", "accel"],
                                   ["--use_es", "--level_editor", "accel", "--score_transform", "rank_sampled",
                                    "--staleness_coeff", "0.5"]])
def test_accepted_with_es_the_editor_and_the_replay_flags(name, extra):
    from toued.level_sampler import LevelSampler
    assert LevelSampler(_args(name, extra), device="cpu").score_function == name


@pytest.mark.parametrize("name", NAMES)
def test_no_tabular_requirement(name):
    """A non-tabular mode gets past the score function's checks (optimal_regret and return_variance stop there with a
    ValueError) and ends where every score function does on such a mode, at the MLP agents the build does not have."""
    from toued.level_sampler import LevelSampler
    with pytest.raises(NotImplementedError, match="MLP agents"):
        LevelSampler(_args(name, mode="rand_dense"), device="cpu")


def test_the_pinned_tuples_are_unchanged_and_the_new_one_mirrors_plr():
    from toued import level_sampler as ls
    from toued import plr
    assert ls.SCORE_FUNCTIONS == ["random", "frozen", "alg_regret", "positive_value_loss", "l1_value_loss",
                                  "optimal_regret"]
    assert ls.MOMENT_SCORE_FUNCTIONS == ("return_variance",)
    assert ls.RETURN_SCORE_FUNCTIONS == ("max_mc",)
    assert ls.POLICY_SCORE_FUNCTIONS == NAMES
    assert tuple(plr.POLICY_FUNCTIONS) == ls.POLICY_SCORE_FUNCTIONS
    assert plr.POLICY_FUNCTIONS["policy_entropy"] is plr.policy_entropy
    assert plr.POLICY_FUNCTIONS["least_confidence"] is plr.least_confidence
    assert plr.POLICY_FUNCTIONS["min_margin"] is plr.min_margin
    assert not set(NAMES) & (set(plr.REGRET_FUNCTIONS) | set(plr.MOMENT_FUNCTIONS) | set(plr.VALUE_LOSS_FUNCTIONS)
                             | set(plr.RETURN_FUNCTIONS))


def test_unknown_score_function_lists_the_new_names():
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="not in known functions") as e:
        LevelSampler(_args("policy_entropyy", mode="small"), device="cpu")
    for name in NAMES + ("max_mc", "return_variance", "optimal_regret"):
        assert f"'{name}'" in str(e.value)


@pytest.mark.parametrize("name", NAMES)
def test_exact_regret_eval_is_not_for_these_scores(name):
    from toued.level_sampler import LevelSampler
    with pytest.raises(ValueError, match="regret_eval"):
        LevelSampler(_args(name, ["--regret_eval", "exact"], mode="small"), device="cpu")


@pytest.mark.parametrize("name", NAMES)
def test_no_new_buffer_field(name):
    import dataclasses
    from toued.level_sampler import LevelBuffer
    assert [f.name for f in dataclasses.fields(LevelBuffer)] == ["levels", "score", "active", "new", "stamp", "clock",
                                                                 "max_return"]


def test_help_and_docstring_name_the_scores():
    from toued import parse_args as pa
    text = pa.build_parser().format_help()
    for name in NAMES:
        assert name in text and name in pa.__doc__


def test_wrapper_rejects_mismatched_shapes_before_any_device_call():
    from toued.rollout import RolloutWrapper, Transition
    ro = RolloutWrapper("debug", 20)
    N, T, W, D = 2, 4, 3, ro.obs_dim
    tr = Transition(torch.zeros((N, T + 1, W), dtype=torch.int32), torch.zeros((N, T, W), dtype=torch.int32),
                    torch.zeros((N, T, W), dtype=torch.uint8), torch.zeros((N, T, W)),
                    torch.zeros((N, T, W), dtype=torch.uint8))
    with pytest.raises(ValueError, match="policy_scores"):
        ro.policy_scores(tr, torch.zeros((N, D, 5)))
    good = Transition(tr.obs_idx, torch.zeros((N, T + 1, W), dtype=torch.int32), tr.action, tr.reward, tr.done)
    for theta in (torch.zeros((N + 1, D, 5)), torch.zeros((N, D, 4)), torch.zeros((N, D, 5), dtype=torch.float64),
                  torch.zeros((N, D * 5))):
        with pytest.raises(ValueError, match="theta"):
            ro.policy_scores(good, theta)
