"""GPU: toued_max_mc_scores / RolloutWrapper.max_mc_scores / toued.plr.max_mc_scores against the numpy restatement
(tests/maxmc_ref.py), and the max_mc PLR score with its per-slot memory LevelBuffer.max_return built on them.

The per-worker maxima and the level maximum are compared bit for bit.  The score is
f32((double)rmax - S / (W T)) with S the float64 sum of the W T float32 values:
    |gpu - f32(ref)| <= 2^-23 |ref| + W T 2^-52 mean|V|
The first term is the one final rounding to float32.  The second bounds the float64 sum's dependence on the order of
its W T terms: each of at most W T - 1 additions rounds a partial sum of magnitude at most sum|V| by 2^-53 relative,
so two orders differ by at most 2 (W T) 2^-53 sum|V| in S, that is W T 2^-52 mean|V| after the division by W T.
"""
import functools

import numpy as np
import pytest
import torch

import maxmc_ref as mr
from oracle import jaxrand as jr

pytestmark = pytest.mark.gpu

GAMMA = 0.99
NEG_INF = float("-inf")

# (N, T, W, D, p_done).  The kernel walks time in chunks of 2048 // min(W, 256) steps: T = 1000 at W = 64 is 31 chunks
# of 32 steps and one of 8; T = 33 at W = 96 is a chunk of 21 and one of 12; W = 200 leaves a worker tile that is no
# multiple of 64; W = 300 is a tile of 256 workers and one of 44; D = 5409 is the largest critic row of any mode.
# The seams of the loader shared with k_value_loss_scores (SEAMS is the same list in test_gpu_vscore.py): T one chunk
# exactly (W = 256: 8 steps) and one step more, where the double buffer flips with a one-row chunk; a second tile of a
# single worker; W = 1 with a chunk boundary at the last step
SEAMS = [(2, 8, 256, 7, 0.3), (2, 9, 256, 7, 0.3), (1, 9, 257, 7, 0.3), (1, 2049, 1, 7, 0.2)]
CASES = [(3, 1, 64, 10, 0.5), (5, 20, 1, 65, 0.2), (2, 33, 96, 65, 0.0), (2, 20, 64, 2, 1.0),
         (2, 1000, 64, 3201, 0.05), (1, 300, 200, 5409, 0.1), (1, 40, 300, 65, 0.1), (0, 20, 64, 65, 0.1)] + SEAMS


@functools.lru_cache(maxsize=None)
def _case(N, T, W, D, p_done):
    rs = np.random.RandomState(N * 1000 + T + W + D)
    tr = {"vcrit": rs.randn(N, D).astype(np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": rs.randn(N, T, W).astype(np.float32),
          "done": (rs.rand(N, T, W) < p_done).astype(np.uint8)}
    for v in tr.values():
        v.setflags(write=False)
    return tr


def _ref(tr, prior=None):
    """(score f64 [N], rmax f32 [N], wmax f32 [N, W], mean|V| f64 [N]) of a trajectory dict."""
    N, T, W = tr["reward"].shape
    if N == 0:
        return np.zeros(0), np.zeros(0, np.float32), np.zeros((0, W), np.float32), np.zeros(0)
    score, rmax, wmax = mr.max_mc_scores(tr["vcrit"], tr["idx"], tr["time"], tr["reward"], tr["done"], GAMMA, prior)
    v = mr.values(tr["vcrit"], tr["idx"], tr["time"])[:, :T].astype(np.float64)
    return score, rmax, wmax, np.abs(v).reshape(N, -1).mean(axis=1)


@functools.lru_cache(maxsize=None)
def _reference(N, T, W, D, p_done):
    """The case's reference without a prior, computed once."""
    return _ref(_case(N, T, W, D, p_done))


def _abi(tr, prior=None, wmax=True, gamma=GAMMA):
    """toued_max_mc_scores on host arrays; prior None and wmax False are passed as NULL.  Returns numpy
    (score, rmax, wmax)."""
    from toued import _lib
    N, T, W = tr["reward"].shape
    D = tr["vcrit"].shape[1]
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in tr.items()}
    d_prior = None if prior is None else torch.from_numpy(np.asarray(prior, np.float32).copy()).cuda()
    o_score = torch.full((N,), float("nan"), device="cuda")
    o_rmax = torch.full((N,), float("nan"), device="cuda")
    o_wmax = torch.full((N, W), float("nan"), device="cuda") if wmax else None
    _lib.call("toued_max_mc_scores", N, W, T, D, _lib.ptr(dev["vcrit"]), _lib.ptr(dev["idx"]), _lib.ptr(dev["time"]),
              _lib.ptr(dev["reward"]), _lib.ptr(dev["done"]), gamma, _lib.ptr(d_prior), _lib.ptr(o_score),
              _lib.ptr(o_rmax), _lib.ptr(o_wmax), _lib.stream_ptr())
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in (o_score, o_rmax, o_wmax))


def _check_scores(got, ref, mean_abs_v, W, T):
    got = got.astype(np.float64)
    assert got.shape == ref.shape
    for a in range(ref.shape[0]):
        want = float(np.float32(ref[a]))
        err = abs(got[a] - want)
        round_term, order_term = 2.0 ** -23 * abs(ref[a]), W * T * 2.0 ** -52 * mean_abs_v[a]
        print(f"score[{a}]: gpu {got[a]!r} f32(ref) {want!r} |diff| {err:.3e} bound {round_term:.3e} + "
              f"{order_term:.3e}")
        assert err <= round_term + order_term, (a, got[a], want, round_term, order_term)


@pytest.mark.parametrize("N,T,W,D,p_done", CASES)
def test_kernel_matches_restatement(N, T, W, D, p_done):
    tr = _case(N, T, W, D, p_done)
    ref_score, ref_rmax, ref_wmax, mav = _reference(N, T, W, D, p_done)
    score, rmax, wmax = _abi(tr, prior=np.full(N, -np.inf, np.float32))
    assert score.shape == (N,) and rmax.shape == (N,) and wmax.shape == (N, W)
    np.testing.assert_array_equal(wmax, ref_wmax)
    np.testing.assert_array_equal(rmax, ref_rmax)
    _check_scores(score, ref_score, mav, W, T)
    if N == 0:
        return
    assert np.isfinite(wmax).all()                     # an unfinished last episode counts: never -inf
    # NULL wmax and NULL rmax_in change no other output bit; a second run gives the same bits
    s2, r2, w2 = _abi(tr, prior=np.full(N, -np.inf, np.float32), wmax=False)
    assert w2 is None and np.array_equal(s2, score) and np.array_equal(r2, rmax)
    for s3, r3, w3 in (_abi(tr), _abi(tr)):
        assert np.array_equal(s3, score) and np.array_equal(r3, rmax) and np.array_equal(w3, wmax)
    # a zero critic: the mean value is 0 and the score is R_max exactly
    zero = dict(tr, vcrit=np.zeros_like(tr["vcrit"]))
    s4, r4, w4 = _abi(zero)
    assert np.array_equal(s4, r4) and np.array_equal(r4, rmax) and np.array_equal(w4, wmax)
    # a prior per agent, alternately above and below everything the rollout reaches
    prior = np.where(np.arange(N) % 2 == 0, 1e3, -1e3).astype(np.float32)
    p_score, p_rmax, _, _ = _ref(tr, prior)
    s5, r5, w5 = _abi(tr, prior=prior)
    np.testing.assert_array_equal(r5, p_rmax)
    np.testing.assert_array_equal(w5, wmax)
    assert (r5[0::2] == np.float32(1e3)).all() and np.array_equal(r5[1::2], rmax[1::2])
    _check_scores(s5, p_score, mav, W, T)


def test_negative_rewards_and_done_at_the_chunk_edges():
    """W = 64: chunks of 32 steps, T = 70 is rows [0, 32), [32, 64), [64, 70).  Rewards all negative; done on the last
    row of a chunk (t = 31), on the first row of one (t = 32) and on the last step (t = 69), alone and together: an
    empty trailing segment must not put a 0 into the maximum."""
    N, T, W, D = 2, 70, 64, 9
    rs = np.random.RandomState(21)
    done = np.zeros((N, T, W), np.uint8)
    w = np.arange(W)
    done[0, 69, w % 4 == 0] = 1
    done[0, 31, w % 4 == 1] = 1
    done[0, 32, w % 4 == 2] = 1
    for t in (31, 32, 69):
        done[0, t, w % 4 == 3] = 1
        done[1, t, :] = 1
    tr = {"vcrit": rs.randn(N, D).astype(np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": (-0.1 - rs.rand(N, T, W)).astype(np.float32), "done": done}
    ref_score, ref_rmax, ref_wmax, mav = _ref(tr)
    assert (ref_wmax < 0).all()
    score, rmax, wmax = _abi(tr)
    np.testing.assert_array_equal(wmax, ref_wmax)
    np.testing.assert_array_equal(rmax, ref_rmax)
    assert (wmax < 0).all() and (rmax < 0).all()
    _check_scores(score, ref_score, mav, W, T)
    # agent 1, every worker: episodes [0, 31], [32, 32], [33, 69]: the one-step episode's (negative) reward is the best
    np.testing.assert_array_equal(wmax[1], tr["reward"][1, 32])


def test_prior_forms():
    """rmax_in of -inf, of a value above every return, and NULL."""
    case = (3, 1, 64, 10, 0.5)
    tr = _case(*case)
    N, T, W = tr["reward"].shape
    ref_score, ref_rmax, ref_wmax, mav = _reference(*case)
    null = _abi(tr)
    minus = _abi(tr, prior=np.full(N, -np.inf, np.float32))
    for x, y in zip(null, minus):
        assert np.array_equal(x, y)
    np.testing.assert_array_equal(null[1], ref_rmax)
    above = np.float32(ref_wmax.max() + 5.0)
    s, r, w = _abi(tr, prior=np.full(N, above, np.float32))
    assert (r == above).all()
    np.testing.assert_array_equal(w, ref_wmax)
    # the score moves by the same amount as R_max, up to the final rounding
    p_score, p_rmax, _, _ = _ref(tr, np.full(N, above, np.float32))
    assert (p_rmax == above).all()
    _check_scores(s, p_score, mav, W, T)


def test_independent_of_the_batch():
    """Agent 1 of a 3-agent call against a call on its rows alone."""
    rs = np.random.RandomState(11)
    N, T, W, D = 3, 45, 96, 33
    tr = {"vcrit": rs.randn(N, D).astype(np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": rs.randn(N, T, W).astype(np.float32), "done": (rs.rand(N, T, W) < 0.1).astype(np.uint8)}
    prior = np.array([0.5, 0.25, -3.0], np.float32)
    s, r, w = _abi(tr, prior=prior)
    s1, r1, w1 = _abi({k: v[1:2] for k, v in tr.items()}, prior=prior[1:2])
    assert s1[0] == s[1] and r1[0] == r[1] and np.array_equal(w1[0], w[1])


def test_wrapper_matches_abi():
    from toued.rollout import RolloutWrapper, Transition
    case = (2, 33, 96, 65, 0.0)
    tr = _case(*case)
    N, T, W = tr["reward"].shape
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in tr.items()}
    trans = Transition(dev["idx"], dev["time"], torch.zeros((N, T, W), dtype=torch.uint8, device="cuda"),
                       dev["reward"], dev["done"])
    ro = RolloutWrapper("debug", 20)
    prior = np.array([-np.inf, 50.0], np.float32)
    a_s, a_r, a_w = _abi(tr, prior=prior)
    s, r, w = ro.max_mc_scores(trans, dev["vcrit"], GAMMA, torch.from_numpy(prior).cuda(), return_worker_max=True)
    assert s.dtype == torch.float32 and r.dtype == torch.float32 and w.shape == (N, W)
    assert np.array_equal(s.cpu().numpy(), a_s) and np.array_equal(r.cpu().numpy(), a_r)
    assert np.array_equal(w.cpu().numpy(), a_w)
    two = ro.max_mc_scores(trans, dev["vcrit"].view(N, -1, 1), GAMMA, torch.from_numpy(prior).cuda())   # critic table
    assert len(two) == 2 and torch.equal(two[0], s) and torch.equal(two[1], r)
    n_s, n_r, _ = _abi(tr)
    none = ro.max_mc_scores(trans, dev["vcrit"], GAMMA)                    # no prior: NULL
    assert np.array_equal(none[0].cpu().numpy(), n_s) and np.array_equal(none[1].cpu().numpy(), n_r)


def test_argument_checks():
    from toued import _lib
    L = _lib.lib()
    N, T, W, D = 2, 4, 8, 5
    vc = torch.zeros((N, D), device="cuda")
    ix = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    tm = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    rw = torch.zeros((N, T, W), device="cuda")
    dn = torch.zeros((N, T, W), dtype=torch.uint8, device="cuda")
    sc, rm = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    P = _lib.ptr
    st = _lib.stream_ptr()
    good = dict(N=N, W=W, T=T, D=D, vc=P(vc), ix=P(ix), tm=P(tm), rw=P(rw), dn=P(dn), sc=P(sc), rm=P(rm))

    def call(**kw):
        a = dict(good, **kw)
        return L.toued_max_mc_scores(a["N"], a["W"], a["T"], a["D"], a["vc"], a["ix"], a["tm"], a["rw"], a["dn"],
                                     GAMMA, None, a["sc"], a["rm"], None, st)

    assert call() == 0
    assert call(N=0) == 0
    assert call(N=0, vc=None, ix=None, tm=None, rw=None, dn=None, sc=None, rm=None) == 0      # empty tensors
    bad = [dict(T=0), dict(W=0), dict(D=1), dict(D=8193), dict(N=-1), dict(vc=None), dict(ix=None), dict(tm=None),
           dict(rw=None), dict(dn=None), dict(sc=None), dict(rm=None), dict(W=65536, T=32768)]
    for kw in bad:
        # a fresh error text per case: another entry point's failure in between
        assert L.toued_gae(1, 0, 1, None, None, None, 0.5, 0.5, None, None, st) == -1
        assert "toued_gae" in L.toued_last_error().decode()
        assert call(**kw) == -1, kw
        msg = L.toued_last_error().decode()
        assert msg and "toued_max_mc_scores" in msg, (kw, msg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ toued.plr.max_mc_scores
def _sampler(mode, score_function, N=8, B=16, extra=()):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", mode, "--score_function", score_function, "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B), *extra])
    return LevelSampler(args)


def test_max_mc_scores_match_restatement_on_the_eval_trajectory():
    from toued import prng
    from toued.agents import create_agents, create_value_critics, eval_agent_reset
    from toued.env import LevelGenerator
    from toued.plr import max_mc_scores
    mode, N, W = "debug", 8, 64
    smp = _sampler(mode, "max_mc", N)
    ro = smp.rollout_manager
    dk = lambda a: prng.from_uint32_numpy(np.ascontiguousarray(a), "cuda")
    levels = LevelGenerator(mode)(dk(jr.split(jr.PRNGKey(401), N)))
    theta, _ = create_agents(dk(jr.split(jr.PRNGKey(402), N)), ro.obs_dim, 8)
    theta.mul_(10.0)
    vcrit = create_value_critics(dk(jr.split(jr.PRNGKey(403), N)), ro.obs_dim).mul_(10.0)
    keys = jr.split(jr.PRNGKey(404), N)
    prior_np = np.array([-np.inf, 100.0, -100.0, -np.inf, 0.0, -np.inf, 100.0, -np.inf], np.float32)
    prior = torch.from_numpy(prior_np).cuda()
    score, rmax = max_mc_scores(smp, dk(keys), levels, theta, vcrit, prior)
    assert score.shape == (N,) and rmax.shape == (N,) and score.dtype == torch.float32 and rmax.dtype == torch.float32
    # lpg_rng of _compute_algorithmic_regret (level_sampler.py:293-329): rng, c = split(keys); rng, tr = split(rng);
    # lpg_rng, a2c_rng = split(rng); then eval_agent's reset and rollout key
    rng = jr.split(keys, 2)[:, 0]
    rng = jr.split(rng, 2)[:, 0]
    lpg_rng = jr.split(rng, 2)[:, 0]
    state, ro_keys = eval_agent_reset(ro, dk(lpg_rng), levels, W)
    tr, _, _ = ro.batch_rollout(ro_keys, theta, levels, state, eval=True)
    T = ro.eval_rollout_len
    assert tr.reward.shape == (N, T, W)
    host = {"vcrit": vcrit.cpu().numpy().reshape(N, -1), "idx": tr.obs_idx.cpu().numpy(),
            "time": tr.obs_time.cpu().numpy(), "reward": tr.reward.cpu().numpy(), "done": tr.done.cpu().numpy()}
    assert smp.args.gamma == GAMMA
    ref_score, ref_rmax, _, mav = _ref(host, prior_np)
    np.testing.assert_array_equal(rmax.cpu().numpy(), ref_rmax)
    assert (ref_rmax[[1, 6]] == 100.0).all() and (ref_rmax[2] > -100.0)
    _check_scores(score.cpu().numpy(), ref_score, mav, W, T)
    # a chunk size that leaves a shorter last chunk, and one agent per chunk: the same bits
    for chunk in (3, 1):
        s_c, r_c = max_mc_scores(smp, dk(keys), levels, theta, vcrit, prior, chunk_agents=chunk)
        assert torch.equal(s_c, score) and torch.equal(r_c, rmax), chunk
    e_s, e_r = max_mc_scores(smp, dk(keys)[:0], levels[:0], theta[:0], vcrit[:0], prior[:0])
    assert e_s.shape == (0,) and e_r.shape == (0,)


@pytest.mark.parametrize("extra", [(), ("--level_editor", "accel", "--staleness_coeff", "0.3")])
def test_level_sampler_keeps_the_slots_best_returns(extra, monkeypatch):
    """Three sample rounds: max_return is -inf on the slots reset in the round, max(prior, rollout max) on the
    terminated agents' slots and untouched elsewhere; last_plr["score"] holds the kernel's scores."""
    from toued import plr, prng
    from toued.env import L_BUFID, L_LIFETIME
    N, B = 8, 16
    smp = _sampler("small", "max_mc", N, B, extra)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    assert buf.max_return is not None and buf.max_return.dtype == torch.float32 and buf.max_return.shape == (B,)
    assert (buf.max_return == NEG_INF).all()
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, True)
    assert agents.vcrit is not None
    resets = []
    real_reset = plr.reset_lowest_scoring

    def recording_reset(*a, **kw):
        ids = real_reset(*a, **kw)
        resets.append(ids)
        return ids

    monkeypatch.setattr(plr, "reset_lowest_scoring", recording_reset)
    terms = [[1, 0, 1, 1, 0, 0, 1, 0], [0, 1, 1, 0, 1, 0, 1, 1], [1, 1, 0, 1, 0, 1, 0, 1]]
    seen_finite_prior = False
    for rnd, t in enumerate(terms):
        term = torch.tensor(t, dtype=torch.bool, device="cuda")
        agents.vcrit.mul_(10.0)
        agents.step = torch.where(term, agents.levels[:, L_LIFETIME], torch.zeros_like(agents.step))
        assert (agents.levels[:, L_LIFETIME] > 0).all()
        old_ids = agents.levels[:, L_BUFID].long().clone()
        sel = term.nonzero().flatten()
        if rnd == 0:       # a remembered return far above, and one far below, what the rollout reaches
            buf.max_return[old_ids[sel[0]]] = 1e3
            buf.max_return[old_ids[sel[1]]] = -1e3
        before = buf.max_return.clone()
        levels0, theta0, vcrit0 = agents.levels.clone(), agents.theta.clone(), agents.vcrit.clone()
        rng = prng.PRNGKey(2 + rnd, "cuda")
        # plr_sample's keys: rng, sub = split(rng) (reset); rng, sub = split(rng); keys = split(sub, N)
        r = prng.split(rng, 2)[0].contiguous()
        sub = prng.split(r, 2)[1].contiguous()
        keys = prng.split(sub, N).contiguous()
        k_sel, l_sel = keys[sel].contiguous(), levels0[sel].contiguous()
        t_sel, v_sel = theta0[sel].contiguous(), vcrit0[sel].contiguous()
        prior = before[old_ids[sel]].contiguous()
        want_score, want_rmax = plr.max_mc_scores(smp, k_sel, l_sel, t_sel, v_sel, prior)
        _, rollout_max = plr.max_mc_scores(smp, k_sel, l_sel, t_sel, v_sel, torch.full_like(prior, NEG_INF))
        assert torch.isfinite(rollout_max).all()
        assert torch.equal(want_rmax, torch.maximum(prior, rollout_max))
        seen_finite_prior |= bool(torch.isfinite(prior).any())
        buf, agents = smp.sample(rng, buf, agents)
        torch.cuda.synchronize()
        assert len(resets) == rnd + 1
        reset_ids = resets[-1].long()
        assert torch.equal(smp.last_plr["score"][sel], want_score)
        assert not smp.last_plr["score"][~term].any()
        assert torch.equal(buf.score[old_ids[sel]], want_score)
        # expected max_return, slot by slot on the host (two agents on one slot: the larger return stays)
        expect = before.cpu().numpy().copy()
        for slot, rm in zip(old_ids[sel].tolist(), rollout_max.cpu().numpy()):
            expect[slot] = max(expect[slot], rm)
        assert not set(reset_ids.tolist()) & set(old_ids[sel].tolist())      # a scored slot is active, never reset
        expect[reset_ids.cpu().numpy()] = -np.inf
        np.testing.assert_array_equal(buf.max_return.cpu().numpy(), expect)
        assert (buf.max_return[reset_ids] == NEG_INF).all()
        if rnd == 0:
            assert buf.max_return[old_ids[sel[0]]] == 1e3
            assert buf.max_return[old_ids[sel[1]]] == rollout_max[1] and rollout_max[1] > -1e3
        touched = torch.zeros(B, dtype=torch.bool, device="cuda")
        touched[reset_ids] = True
        touched[old_ids[sel]] = True
        assert torch.equal(buf.max_return[~touched], before[~touched])
    assert seen_finite_prior


@pytest.mark.parametrize("name", ["alg_regret", "positive_value_loss", "frozen"])
def test_other_score_functions_have_no_max_return(name):
    from toued import prng
    smp = _sampler("small", name, 8, 16)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    assert buf.max_return is None


def test_level_sampler_without_value_critics_raises():
    from toued import prng
    smp = _sampler("small", "max_mc", 8, 16)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, 8, False)
    assert agents.vcrit is None
    with pytest.raises(ValueError, match="max_mc"):
        smp.sample(prng.PRNGKey(2, "cuda"), buf, agents)


def test_trainer_runs_with_max_mc_and_accel():
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = parse_args(["--env_mode", "debug", "--num_agents", "8", "--num_mini_batches", "1", "--seed", "5",
                       "--score_function", "max_mc", "--level_editor", "accel", "--buffer_size", "32"])
    tr = Trainer(args)
    assert tr.buffer.max_return is not None
    scored = 0
    for _ in range(3):
        tr.agents.levels[:4, L_LIFETIME] = 1            # four agents reach their lifetime in every step
        m = tr.meta_step()
        torch.cuda.synchronize()
        scored += int(tr.sampler.last_plr["score"].count_nonzero().item())

        def finite(x):
            if isinstance(x, dict):
                return all(finite(v) for v in x.values())
            return bool(torch.isfinite(torch.as_tensor(x, dtype=torch.float32)).all())
        assert finite(m)
    tr.finish()
    assert scored > 0
    assert torch.isfinite(tr.buffer.score).all()
    known = torch.isfinite(tr.buffer.max_return)
    assert known.any() and (tr.buffer.max_return[~known] == NEG_INF).all()
