"""toued.evaluate without a GPU: parser defaults and refusals, the curve-point schedule, normalisation with a
degenerate level, the sampled bucket values and the JSON schema; toued.train's --eval_every flags."""
import json
import math

import numpy as np
import pytest

from toued import evaluate as ev
from toued.parse_args import parse_args


def test_parser_defaults():
    a = ev.parse_eval_args(["--checkpoint_dir", "ckpt"])
    assert (a.checkpoint_dir, a.step, a.es_member, a.eval_mode, a.eval_levels, a.eval_seed) == \
        ("ckpt", None, "mean", "mazes", 64, 0)
    assert (a.levels_from_buffer, a.curve_points, a.baseline, a.env_workers, a.train_rollout_len) == \
        (None, 11, "none", 64, 20)
    assert a.lifetime_conditioning is False and a.out is None
    b = ev.parse_eval_args(["--checkpoint_dir", "c", "--step", "7", "--es_member", "best", "--eval_mode", "debug",
                            "--eval_levels", "3", "--eval_seed", "5", "--curve_points", "2", "--baseline", "a2c",
                            "--env_workers", "32", "--train_rollout_len", "5", "--lifetime_conditioning", "--out",
                            "o.json", "--levels_from_buffer", "buf"])
    assert (b.step, b.es_member, b.eval_mode, b.eval_levels, b.eval_seed, b.curve_points, b.baseline) == \
        (7, "best", "debug", 3, 5, 2, "a2c")
    assert (b.env_workers, b.train_rollout_len, b.lifetime_conditioning, b.out, b.levels_from_buffer) == \
        (32, 5, True, "o.json", "buf")


@pytest.mark.parametrize("extra,word", [
    (["--eval_mode", "rand_all"], "tabular"), (["--eval_mode", "nope"], "not registered"),
    (["--es_member", "worst"], "es_member"), (["--baseline", "ppo"], "baseline"), (["--curve_points", "0"], "curve_points"),
    (["--eval_levels", "0"], "eval_levels"), (["--env_workers", "48"], "multiple of 32"),
    (["--train_rollout_len", "0"], "train_rollout_len"), (["--bogus", "1"], "Unknown args")])
def test_parser_refusals(extra, word):
    with pytest.raises(ValueError, match=word):
        ev.parse_eval_args(["--checkpoint_dir", "c", *extra])


def test_parser_needs_a_checkpoint_dir():
    with pytest.raises(SystemExit):
        ev.parse_eval_args([])


def test_train_flags():
    base = ["--num_agents", "4", "--num_mini_batches", "1"]
    a = parse_args(base)
    assert (a.eval_every, a.eval_mode, a.eval_levels, a.eval_seed, a.curve_points) == (0, "mazes", 64, 0, 11)
    # without --eval_every the other flags are inert: nothing about them is refused
    assert parse_args(base + ["--eval_mode", "rand_all"]).eval_every == 0
    assert parse_args(base + ["--eval_every", "3", "--eval_mode", "debug"]).eval_every == 3
    with pytest.raises(ValueError, match="negative"):
        parse_args(base + ["--eval_every", "-1"])
    with pytest.raises(ValueError, match="tabular"):
        parse_args(base + ["--eval_every", "1", "--eval_mode", "rand_all"])
    with pytest.raises(ValueError, match="tabular"):
        parse_args(base + ["--eval_every", "1", "--eval_mode", "nope"])
    with pytest.raises(ValueError, match="curve_points"):
        parse_args(base + ["--eval_every", "1", "--curve_points", "0"])


def test_curve_schedule():
    assert ev.curve_schedule(2500, 11) == list(range(0, 2501, 250))
    assert ev.curve_schedule(4, 3) == [0, 2, 4]
    assert ev.curve_schedule(10, 1) == [10]                 # P = 1: the final point alone
    assert ev.curve_schedule(10, 2) == [0, 10]              # P = 2: both ends
    assert ev.curve_schedule(3, 11) == [0, 1, 2, 3]         # P > U: every count once
    assert ev.curve_schedule(0, 5) == [0] and ev.curve_schedule(0, 1) == [0]      # U = 0
    assert ev.curve_schedule(5, 3) == [0, 3, 5]             # 2.5 rounds half up
    for U in range(0, 40):
        for P in range(1, 45):
            pts = ev.curve_schedule(U, P)
            assert pts == sorted(set(pts)) and pts[-1] == U and len(pts) <= P
            assert P == 1 or pts[0] == 0
            assert all(isinstance(p, int) and 0 <= p <= U for p in pts)
            if 2 <= P <= U + 1:
                assert len(pts) == P
                gaps = np.diff(pts)
                assert gaps.max() - gaps.min() <= 1
    with pytest.raises(ValueError):
        ev.curve_schedule(3, 0)
    with pytest.raises(ValueError):
        ev.curve_schedule(-1, 2)


def _result(P=3):
    n = 4
    v_opt = np.array([2.0, 1.0, 0.5, 3.0], np.float32)
    v_uni = np.array([1.0, 1.0, 0.5 - 5e-7, 1.0], np.float32)         # levels 1 and 2: nothing to gain
    exact = np.array([[1.0, 1.5, 2.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [1.0, 1.0, 2.0]], np.float64)[:, :P]
    stats = np.zeros((n, P, 6))
    stats[:, 1:, :] = [4.0, 6.0, 11.0, 40.0, 7.0, 100.0]            # 4 episodes: returns sum 6, squares 11
    stats[:, 0, 5] = 0.0                                            # the bucket of point 0 is empty
    stats[3, P - 1] = [1.0, 2.0, 4.0, 9.0, 2.5, 100.0]              # a single episode: no standard error
    return ev.summarise("mazes", [0, 1, 2][:P], 2, exact, v_opt, v_uni, stats, np.full(n, 2),
                        sub_mode=np.array([0, 0, 1, 1]), baseline_exact=np.array([1.5, 1.0, 0.5, 1.0]))


def test_normalisation_with_degenerate_levels():
    with np.errstate(all="raise"):                                  # no division by a vanishing gap anywhere
        r = _result()
    assert r.n_degenerate == 2 and r.degenerate.tolist() == [False, True, True, False]
    assert np.isnan(r.normalised[1]).all() and np.isnan(r.normalised[2]).all()
    np.testing.assert_allclose(r.normalised[0], [0.0, 0.5, 1.0])
    np.testing.assert_allclose(r.normalised[3], [0.0, 0.0, 0.5])
    a = r.aggregates
    np.testing.assert_allclose(a["curve_normalised"], [0.0, 0.25, 0.75])
    assert a["final_normalised"] == pytest.approx(0.75) and a["final_normalised_se"] == pytest.approx(0.25)
    assert a["auc"] == pytest.approx((0.5 + 0.5 / 3) / 2)
    assert a["final_exact_return"] == pytest.approx((2.0 + 1.0 + 0.5 + 2.0) / 4)       # every level counts here
    for k, v in a.items():
        if "normalised" in k or k.startswith("auc"):
            assert np.all(np.isfinite(v)), k                        # no inf or NaN in the normalised means
    assert r.baseline["final_normalised"] == pytest.approx(0.25) and r.baseline["final_exact_return"] == pytest.approx(1.0)
    # per sub-mode: the mode's own levels, its own degenerate count
    names = list(r.per_mode)
    assert len(names) == 2 and r.per_mode[names[0]]["n_degenerate"] == 1 and r.per_mode[names[1]]["n_levels"] == 2
    assert r.per_mode[names[0]]["final_normalised"] == pytest.approx(1.0)
    assert r.per_mode[names[1]]["final_normalised"] == pytest.approx(0.5)


def test_all_levels_degenerate_gives_nan_not_inf():
    r = ev.summarise("debug", [0, 4], 4, np.ones((2, 2)), np.ones(2), np.ones(2), np.zeros((2, 2, 6)), np.full(2, 4))
    assert r.n_degenerate == 2 and math.isnan(r.aggregates["final_normalised"]) and math.isnan(r.aggregates["auc"])
    assert r.log_dict() == {"final_normalised": None, "final_exact_return": 1.0, "auc": None, "n_degenerate": 2}


def test_sampled_bucket_values():
    r = _result()
    s = r.sampled
    assert np.isnan(s["episode_return"][:, 0]).all() and np.isnan(s["reward_per_step"][:, 0]).all()
    assert s["episode_return"][0, 1] == 1.5 and s["episode_len"][0, 1] == 10.0 and s["reward_per_step"][0, 1] == 0.07
    # variance (11 - 4 * 1.5^2) / 3 = 2/3, standard error sqrt(2/3 / 4)
    assert s["episode_return_se"][0, 1] == pytest.approx(math.sqrt(2.0 / 3.0 / 4.0))
    assert s["episode_return"][3, 2] == 2.0 and np.isnan(s["episode_return_se"][3, 2])


def test_json_schema():
    r = _result()
    line = json.loads(json.dumps(r.summary()))                     # plain JSON, no NaN tokens
    for k in ("env_mode", "n_levels", "updates", "points", "n_degenerate", "auc", "auc_se", "per_mode", "baseline"):
        assert k in line, k
    for name in ("exact_return", "normalised", "episode_return", "episode_len", "reward_per_step"):
        for k in ("final_" + name, "final_" + name + "_se", "curve_" + name, "curve_" + name + "_se"):
            assert k in line, k
        assert len(line["curve_" + name]) == len(line["points"]) == 3
    assert line["n_levels"] == 4 and line["points"] == [0, 1, 2] and line["curve_episode_return"][0] is None
    assert set(line["baseline"]) == {"name", "final_exact_return", "final_exact_return_se", "final_normalised",
                                     "final_normalised_se"}
    full = json.loads(json.dumps(r.to_json()))
    lv = full["levels"]
    for k in ("exact_return", "normalised", "episode_return", "episode_return_se", "episode_len", "reward_per_step",
              "episodes", "v_opt", "v_uniform", "degenerate", "lifetime", "sub_mode", "baseline_exact_return",
              "baseline_normalised"):
        assert k in lv and len(lv[k]) == 4, k
    assert lv["normalised"][1] == [None, None, None] and lv["degenerate"] == [False, True, True, False]
    assert set(r.log_dict()) == {"final_normalised", "final_exact_return", "auc", "n_degenerate"}
    assert "NaN" not in json.dumps(full) and "Infinity" not in json.dumps(full)


def test_eta_size_names_the_flag():
    """MetaTest refuses an eta of the other layout before it touches the device."""
    import torch
    from toued.lpg import LPGLayout
    args = ev.parse_eval_args(["--checkpoint_dir", "c", "--eval_mode", "debug", "--env_workers", "32"])
    with pytest.raises(ValueError, match="--lifetime_conditioning"):
        ev.MetaTest(args, torch.zeros(LPGLayout(7).size), device="cpu")
