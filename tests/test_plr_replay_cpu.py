"""PLR's rank-weighted, staleness-aware replay distribution without a GPU: the invariants of the numpy restatement
(tests/plr_replay_ref.py) that toued_plr_sample_prio is compared against bit for bit (tests/test_gpu_plr_replay.py),
and the host surface: --score_transform rank_sampled, --staleness_coeff, LevelSampler's argument checks, the
LevelBuffer's stamp / clock fields and their checkpoint keys.
"""
import numpy as np
import pytest
import torch

import plr_replay_ref as prr
from oracle import jaxrand as jr
from oracle import sampler as osp

F32 = np.float32
TINY = prr.TINY


def _buffer_state(B, seed, n_active, frac_new):
    """tests/test_gpu_plr.py's buffers: quarter-rounded scores (ties), some -0.0."""
    rs = np.random.RandomState(seed)
    score = (np.round(rs.randn(B).astype(F32) * 4) / 4).astype(F32)
    score[rs.rand(B) < 0.05] = -0.0
    active = np.zeros(B, bool)
    active[rs.choice(B, n_active, replace=False)] = True
    new = (rs.rand(B) < frac_new) & ~active
    stamp = rs.randint(0, 50, B).astype(np.int32)
    return score, active, new, stamp


# (B, N, T, rho): the shapes the restatement was prototyped at
CASES = [(64, 8, 0.02, 0.0), (64, 8, 0.1, 0.3), (4000, 512, 0.1, 0.1), (4000, 512, 0.1, 0.0), (33, 7, 1.0, 1.0),
         (8192, 512, 0.1, 0.0)]


# the softmax of score / 0.02 overflows float32: that temperature is a rank_sampled case only
@pytest.mark.parametrize("B,N,T,rho,transform", [c + (t,) for c in CASES for t in prr.TRANSFORMS
                                                 if c[2] >= 0.1 or t == "rank_sampled"])
def test_p_sums_to_one_and_ids_are_valid(B, N, T, rho, transform):
    score, active, new, stamp = _buffer_state(B, B + N, N // 2, 0.3)
    valid = ~(new | active)
    assert valid.sum() >= N
    p = prr.replay_p(score, active, new, N, transform, T, rho, stamp, 60)
    assert p.dtype == F32 and np.all(p[~valid] == 0)
    assert abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6
    ids = prr.replay_ids(jr.PRNGKey(B), p, N, transform)
    if transform != "proportional" or rho > 0:      # the reference's softmax has no floor
        assert valid[ids].all() and len(set(ids.tolist())) == N


def test_rank_sampled_is_monotone_in_rank_and_ignores_score_scale():
    score, active, new, _ = _buffer_state(300, 3, 32, 0.4)
    valid = ~(new | active)
    for T in (1.0, 0.3, 0.02):
        p = prr.replay_p(score, active, new, 16, "rank_sampled", T)
        r = prr.ranks(score, valid)
        order = np.argsort(r[valid], kind="stable")
        assert np.all(np.diff(p[valid][order]) <= 0)
        assert np.all(p[valid] >= TINY)
        # a function of the ranks alone: any increasing map of the scores leaves it unchanged
        assert np.array_equal(p, prr.replay_p((score * F32(1024.0)).astype(F32), active, new, 16, "rank_sampled", T))
    # ties go to the lower index, -0.0 == +0.0
    s = np.array([0.0, 1.0, -0.0, 1.0, -2.0], F32)
    none = np.zeros(5, bool)
    assert prr.ranks(s, ~none).tolist() == [3, 1, 4, 2, 5]
    assert prr.ranks(s, np.array([True, False, True, True, True])).tolist() == [2, 5, 3, 1, 4]


def test_staleness_part():
    score, active, new, stamp = _buffer_state(64, 5, 6, 0.3)
    valid = ~(new | active)
    now = 70
    # rho = 1: p is the staleness distribution
    for transform in prr.TRANSFORMS:
        p = prr.replay_p(score, active, new, 8, transform, 0.5, 1.0, stamp, now)
        a = np.where(valid, now - stamp.astype(np.int64), 0)
        assert np.array_equal(p, np.where(valid, (a.astype(F32) / F32(a.sum())).astype(F32), 0).astype(F32))
    # A == 0: uniform over the valid slots
    pc = prr.staleness_part(valid, np.full(64, now, np.int32), now)
    assert np.array_equal(pc, np.where(valid, F32(1.0) / F32(valid.sum()), 0).astype(F32))
    # now < stamp clamps to 0 (and does not lower the sum)
    st = np.where(np.arange(64) == np.flatnonzero(valid)[0], now + 1000, stamp).astype(np.int32)
    pc = prr.staleness_part(valid, st, now)
    assert pc[np.flatnonzero(valid)[0]] == 0 and np.all(pc >= 0)
    assert abs(float(pc.astype(np.float64).sum()) - 1.0) < 1e-6
    # and the mixture floors that slot: it stays drawable under rho = 1
    p = prr.replay_p(score, active, new, 8, "rank", 1.0, 1.0, st, now)
    assert p[np.flatnonzero(valid)[0]] == TINY
    # the sum is exact in 64 bits: ages near 2^31 over many slots
    big = np.full(64, -2 ** 31, np.int32)
    pc = prr.staleness_part(np.ones(64, bool), big, 2 ** 31 - 1)
    assert np.array_equal(pc, np.full(64, F32(1.0) / F32(64.0), F32))


def test_floor_applies_only_where_stated():
    score, active, new, stamp = _buffer_state(64, 64 * 7 + 8, 6, 0.25)
    valid = ~(new | active)
    # rank_sampled at a low temperature: most rank weights underflow; the floor keeps every valid slot drawable
    raw = prr.replay_p(score, active, new, 8, "rank_sampled", 0.02, floor=False)
    p = prr.replay_p(score, active, new, 8, "rank_sampled", 0.02)
    assert (raw[valid] < TINY).sum() > valid.sum() // 2
    assert np.all(p[valid] >= TINY) and np.all(p[~valid] == 0)
    assert np.array_equal(p, np.where(valid, np.maximum(raw, TINY), 0).astype(F32))
    # proportional / rank with rho == 0 is the reference's distribution: an underflowed weight stays 0
    low = score.copy()
    low[np.flatnonzero(valid)[:40]] = F32(-200.0)
    for transform in ("rank", "proportional"):
        p0 = prr.replay_p(low, active, new, 8, transform, 1.0)
        assert (p0[valid] == 0).sum() == 40
        # ... and with rho > 0 it is floored
        p1 = prr.replay_p(low, active, new, 8, transform, 1.0, 0.3, np.full(64, 9, np.int32), 9)
        assert np.all(p1[valid] >= TINY) and np.all(p1[~valid] == 0)
    # fewer valid slots than N: the reference's fallback, p = 1 everywhere, whatever the transform and rho
    for transform in prr.TRANSFORMS:
        assert np.array_equal(prr.replay_p(score, active, new, 60, transform, 0.1, 0.5, stamp, 60), np.ones(64, F32))


@pytest.mark.parametrize("B,N,n_active,frac_new", [(33, 7, 3, 0.3), (300, 64, 32, 0.5), (100, 16, 0, 0.0),
                                                    (1000, 1000, 500, 0.3)])
def test_rho0_equals_oracle_sampler(monkeypatch, B, N, n_active, frac_new):
    """With rho = 0 the two reference transforms are oracle/sampler.py's: the same p (read where replay_ids hands it
    to the Gumbel top-k) and the same ids."""
    score, active, new, _ = _buffer_state(B, B * 7 + N, n_active, frac_new)
    key = jr.PRNGKey(B + N)
    seen = []
    real = jr.choice_p_noreplace
    monkeypatch.setattr(osp.jr, "choice_p_noreplace", lambda k, p, n: (seen.append(p.copy()), real(k, p, n))[1])
    for T in (1.0, 0.1):
        ref_ids = osp.replay_ids(key, score, active, new, N, "proportional", T)
        p = prr.replay_p(score, active, new, N, "proportional", T)
        assert np.array_equal(p.view(np.uint32), seen[-1].view(np.uint32))
        assert np.array_equal(prr.replay_ids(key, p, N, "proportional"), ref_ids)
        p = prr.replay_p(score, active, new, N, "rank", T)
        assert np.array_equal(p.view(np.uint32), seen[-1].view(np.uint32))
        assert np.array_equal(prr.replay_ids(key, p, N, "rank"), osp.replay_ids(key, score, active, new, N, "rank", T))


# ---------------------------------------------------------------------------------------------- host surface
_BASE = ["--env_mode", "tabular", "--num_agents", "8", "--num_mini_batches", "1", "--buffer_size", "64"]


def test_flags_parse():
    from toued.level_sampler import SCORE_TRANSFORMS, LevelSampler
    from toued.parse_args import parse_args
    a = parse_args(_BASE)
    assert a.staleness_coeff == 0.0 and a.score_transform == "rank"
    assert "rank_sampled" in SCORE_TRANSFORMS
    a = parse_args(_BASE + ["--score_function", "optimal_regret", "--score_transform", "rank_sampled",
                            "--staleness_coeff", "0.3"])
    s = LevelSampler(a, device="cpu")
    assert s.score_transform == "rank_sampled" and s.staleness_coeff == 0.3
    assert LevelSampler(parse_args(_BASE), device="cpu").staleness_coeff == 0.0
    with pytest.raises(ValueError, match="transform"):
        LevelSampler(parse_args(_BASE + ["--score_transform", "rank_weighted"]), device="cpu")


@pytest.mark.parametrize("flags", [["--score_function", "alg_regret", "--staleness_coeff", "-0.1"],
                                   ["--score_function", "alg_regret", "--staleness_coeff", "1.5"],
                                   ["--score_function", "random", "--staleness_coeff", "0.3"],
                                   ["--score_function", "frozen", "--staleness_coeff", "0.3"]])
def test_sampler_rejects_invalid_staleness(flags):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    with pytest.raises(ValueError, match="staleness_coeff"):
        LevelSampler(parse_args(_BASE + flags), device="cpu")


def _cpu_buffer(B, with_stamp):
    from oracle import levels as olv
    from toued.level_sampler import LevelBuffer
    p, lt = olv.reset_env_params(jr.split(jr.PRNGKey(3), B), "tabular")
    packed = olv.pack_levels(p, lt, olv.env_spec("tabular"), np.arange(B, dtype=np.int32))
    rs = np.random.RandomState(1)
    buf = LevelBuffer(torch.from_numpy(packed), torch.from_numpy(rs.randn(B).astype(F32)),
                      torch.from_numpy(rs.rand(B) < 0.3), torch.from_numpy(rs.rand(B) < 0.5))
    assert buf.stamp is None and buf.clock == 0 and len(buf) == B      # the four-argument constructor
    if with_stamp:
        buf.stamp = torch.from_numpy(rs.randint(0, 17, B).astype(np.int32))
        buf.clock = 17
    return buf


def test_checkpoint_keys_and_roundtrip(tmp_path):
    from toued.checkpoint import (level_buffer_from_state_dict, level_buffer_state_dict, restore_checkpoint,
                                  save_checkpoint)
    from toued.env import get_env_spec
    spec, _, _ = get_env_spec("tabular")
    plain, stamped = _cpu_buffer(40, False), _cpu_buffer(40, True)
    d0, d1 = level_buffer_state_dict(plain, spec), level_buffer_state_dict(stamped, spec)
    assert list(d0) == ["level", "score", "active", "new"]
    assert list(d1) == ["level", "score", "active", "new", "stamp", "clock"]
    assert d1["stamp"].dtype == np.int32 and d1["stamp"].shape == (40,)
    assert d1["clock"].dtype == np.int32 and d1["clock"].shape == ()
    for name, buf, d in (("plain", plain, d0), ("stamped", stamped, d1)):
        save_checkpoint(str(tmp_path / name), d, 5, prefix="buffer_")
        back = level_buffer_from_state_dict(restore_checkpoint(str(tmp_path / name), prefix="buffer_"), spec, "cpu")
        for f in ("levels", "score", "active", "new"):
            assert torch.equal(getattr(back, f), getattr(buf, f)), (name, f)
        assert back.clock == buf.clock
        if buf.stamp is None:
            assert back.stamp is None
        else:
            assert back.stamp.dtype == torch.int32 and torch.equal(back.stamp, buf.stamp)
