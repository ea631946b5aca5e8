"""GPU: toued_policy_scores / RolloutWrapper.policy_scores / toued.plr.policy_scores against the numpy restatement
(tests/polscore_ref.py), and the policy_entropy / least_confidence / min_margin PLR scores built on them.

The per-step terms (the kernel's ``steps`` output) are compared bit for bit.  A score is the float64 mean of the W T
float32 terms, rounded to float32 once; the kernel's float64 sum runs in another order than numpy's, which moves the
sum by a few 2^-53 relative and so the single final rounding by at most one float32 ulp:
    |gpu - f32(ref)| <= ulp_f32(ref)
"""
import functools
import math

import numpy as np
import pytest
import torch

import polscore_ref as pr
from oracle import jaxrand as jr

pytestmark = pytest.mark.gpu

NAMES = ("policy_entropy", "least_confidence", "min_margin")
D_MAX = 7065            # the largest table toued_policy_scores stages in LDS (csrc/polscore.hip kPsMaxD)

# (N, T, W, D, first_scale): agent a's table has scale polscore_ref.SCALES[(a + first_scale) % 5].  The kernel walks
# the T W pairs of an agent flat, in chunks of 2048, 512 threads x 4: T W = 1 is the smallest legal case; 255, 256 and
# 257 straddle a multiple of the wave and half a workgroup; 8 x 256 is exactly one chunk and 2049 one pair into the
# second; D = 5409 is the largest table of any mode, above the default 64 KB of dynamic LDS
CASES = [(1, 1, 1, 2, 2), (3, 1, 255, 7, 0), (3, 1, 256, 7, 2), (2, 1, 257, 7, 3), (2, 8, 256, 65, 1),
         (2, 2049, 1, 65, 2), (2, 50, 64, 677, 3), (1, 33, 64, 5409, 2), (5, 20, 4, 19, 0)]


@functools.lru_cache(maxsize=None)
def _case(*case):
    return pr.make_case(*case)


@functools.lru_cache(maxsize=None)
def _reference(*case):
    """(scores float64 [3][N], terms float32 [N, 3, T, W]) of the case, computed once."""
    c, T = _case(*case), case[1]
    _, terms = pr.probs_terms(c["theta"], c["idx"][:, :T], c["time"][:, :T])
    terms.setflags(write=False)
    return pr.policy_scores(c["theta"], c["idx"], c["time"]), terms


def _abi(c, outs=(True, True, True), steps=True):
    """toued_policy_scores on host arrays; an output whose flag is False is passed as NULL.  Returns numpy
    (entropy, least_conf, min_margin, steps), None for the NULL ones."""
    from toued import _lib
    N, R, W = c["idx"].shape
    T, D = R - 1, c["theta"].shape[1]
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in c.items()}
    o = [torch.full((N,), float("nan"), device="cuda") if f else None for f in outs]
    o.append(torch.full((N, 3, T, W), float("nan"), device="cuda") if steps else None)
    _lib.call("toued_policy_scores", N, W, T, D, _lib.ptr(dev["theta"]), _lib.ptr(dev["idx"]), _lib.ptr(dev["time"]),
              *map(_lib.ptr, o), _lib.stream_ptr())
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in o)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _check_scores(got, ref):
    """Each float32 score within one float32 ulp of the float32-rounded float64 mean."""
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == np.float32 and g.shape == r.shape
        for a in range(r.shape[0]):
            want = np.float32(r[a])
            ulp = float(np.spacing(np.abs(want)))
            err = abs(float(g[a]) - float(want))
            print(f"{name}[{a}]: gpu {float(g[a])!r} f32(ref) {float(want)!r} |diff| {err:.3e} ulp {ulp:.3e}")
            assert err <= ulp, (name, a, float(g[a]), float(want))


@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_restatement(case):
    N, T, W, D, _ = case
    c = _case(*case)
    ref, ref_terms = _reference(*case)
    ent, lc, mm, steps = _abi(c)
    assert steps.shape == (N, 3, T, W)
    np.testing.assert_array_equal(_bits(steps), _bits(ref_terms))
    _check_scores((ent, lc, mm), ref)


def test_the_cases_hold_what_they_are_for():
    """The inputs' own properties: every scale, exact ties, the deterministic policy, clamped indices."""
    c = _case(5, 20, 4, 19, 0)
    _, terms = _reference(5, 20, 4, 19, 0)
    assert (terms[0, 2] == 1.0).all() and (terms[0, 1] == np.float32(1.0) - np.float32(0.2)).all()     # theta = 0
    assert (terms[4, 2] == 1.0).any() and (terms[4, 2] < 1.0).any()       # scale 300: tied rows and untied ones
    assert (terms[4, 0] == 0.0).any()                                     # a deterministic step
    assert list(c["idx"][0, 0, :4]) == [19 + 3, -1, 18, 18]
    assert c["time"].max() > 1900 and np.abs(c["theta"][2, 18]).min() > 0


@pytest.mark.parametrize("case", [(5, 20, 4, 19, 0), (2, 2049, 1, 65, 2)])
def test_nullable_outputs_and_repeat_runs(case):
    """Each output alone and each pair give the bits of all three together, with and without ``steps``; a second run
    gives the same bits."""
    c = _case(*case)
    full = _abi(c)
    again = _abi(c)
    for x, y in zip(full, again):
        assert np.array_equal(_bits(x), _bits(y))
    for mask in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        for steps in (False, True):
            got = _abi(c, outs=tuple(bool(m) for m in mask), steps=steps)
            for k in range(3):
                assert (got[k] is None) == (not mask[k])
                if mask[k]:
                    assert np.array_equal(_bits(got[k]), _bits(full[k])), (mask, steps, k)
            assert (got[3] is None) == (not steps)
            if steps:
                assert np.array_equal(_bits(got[3]), _bits(full[3]))


def test_independent_of_the_batch():
    """Every agent of a 5-agent call against a call on its rows alone."""
    c = _case(5, 20, 4, 19, 0)
    full = _abi(c)
    for a in range(5):
        one = _abi({k: v[a:a + 1] for k, v in c.items()})
        for x, y in zip(one, full):
            assert np.array_equal(_bits(x[0]), _bits(y[a])), a


def test_argument_checks():
    from toued import _lib
    L = _lib.lib()
    N, T, W, D = 2, 4, 8, 5
    th = torch.zeros((N, D, 5), device="cuda")
    ix = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    tm = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    e, l, m = (torch.zeros(N, device="cuda") for _ in range(3))
    P = _lib.ptr
    st = _lib.stream_ptr()
    good = dict(N=N, W=W, T=T, D=D, th=P(th), ix=P(ix), tm=P(tm), e=P(e), l=P(l), m=P(m))

    def call(**kw):
        a = dict(good, **kw)
        return L.toued_policy_scores(a["N"], a["W"], a["T"], a["D"], a["th"], a["ix"], a["tm"], a["e"], a["l"], a["m"],
                                     None, st)

    assert call() == 0
    assert call(N=0) == 0
    assert call(N=0, th=None, ix=None, tm=None, e=None, l=None, m=None) == 0      # empty tensors
    bad = [dict(T=0), dict(W=0), dict(D=1), dict(D=D_MAX + 1), dict(N=-1), dict(th=None), dict(ix=None), dict(tm=None),
           dict(e=None, l=None, m=None), dict(W=65536, T=32768)]
    for kw in bad:
        # a fresh error text per case: another entry point's failure in between
        assert L.toued_gae(1, 0, 1, None, None, None, 0.5, 0.5, None, None, st) == -1
        assert "toued_gae" in L.toued_last_error().decode()
        assert call(**kw) == -1, kw
        msg = L.toued_last_error().decode()
        assert msg and "toued_policy_scores" in msg, (kw, msg)
    torch.cuda.synchronize()


def test_the_largest_table_the_kernel_accepts():
    """D at the limit: the whole 150 KB of dynamic LDS, against the restatement."""
    case = (1, 3, 40, D_MAX, 2)
    c = _case(*case)
    ref, ref_terms = _reference(*case)
    ent, lc, mm, steps = _abi(c)
    np.testing.assert_array_equal(_bits(steps), _bits(ref_terms))
    _check_scores((ent, lc, mm), ref)


# ------------------------------------------------------------------------------------ RolloutWrapper.policy_scores
def _sampler(mode, score_function, N=8, B=16, extra=()):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", mode, "--score_function", score_function, "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B), *extra])
    return LevelSampler(args)


def _dk(a):
    from toued import prng
    return prng.from_uint32_numpy(np.ascontiguousarray(a), "cuda")


@functools.lru_cache(maxsize=None)
def _eval_trajectory(mode="debug", N=8, W=64):
    """A sampler, levels, actor tables and keys, and the eval trajectory toued.plr's scores roll from those keys
    (regenerated here with the same splits), with its restatement: shared by the tests below, never modified."""
    from toued.agents import create_agents, eval_agent_reset
    from toued.env import LevelGenerator
    smp = _sampler(mode, "policy_entropy", N)
    ro = smp.rollout_manager
    levels = LevelGenerator(mode)(_dk(jr.split(jr.PRNGKey(501), N)))
    theta, _ = create_agents(_dk(jr.split(jr.PRNGKey(502), N)), ro.obs_dim, 8)
    theta.mul_(10.0)
    keys = jr.split(jr.PRNGKey(504), N)
    # lpg_rng of _compute_algorithmic_regret (level_sampler.py:293-329): rng, c = split(keys); rng, tr = split(rng);
    # lpg_rng, a2c_rng = split(rng); then eval_agent's reset and rollout key
    rng = jr.split(keys, 2)[:, 0]
    rng = jr.split(rng, 2)[:, 0]
    lpg_rng = jr.split(rng, 2)[:, 0]
    state, ro_keys = eval_agent_reset(ro, _dk(lpg_rng), levels, W)
    tr, _, _ = ro.batch_rollout(ro_keys, theta, levels, state, eval=True)
    T = ro.eval_rollout_len
    assert tr.reward.shape == (N, T, W)
    host = {"theta": theta.cpu().numpy(), "idx": tr.obs_idx.cpu().numpy(), "time": tr.obs_time.cpu().numpy()}
    ref = pr.policy_scores(host["theta"], host["idx"], host["time"])
    return smp, levels, theta, keys, tr, host, ref


def test_wrapper_matches_abi_on_a_rolled_trajectory():
    smp, levels, theta, keys, tr, host, ref = _eval_trajectory()
    ro = smp.rollout_manager
    N, T, W = tr.reward.shape
    a_ent, a_lc, a_mm, a_steps = _abi(host)
    three = ro.policy_scores(tr, theta)
    assert len(three) == 3
    for got, want in zip(three, (a_ent, a_lc, a_mm)):
        assert got.dtype == torch.float32 and got.shape == (N,)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    four = ro.policy_scores(tr, theta, return_steps=True)
    assert len(four) == 4 and four[3].shape == (N, 3, T, W) and four[3].dtype == torch.float32
    assert np.array_equal(_bits(four[3].cpu().numpy()), _bits(a_steps))
    for x, y in zip(four[:3], three):
        assert torch.equal(x, y)
    _check_scores(tuple(x.cpu().numpy() for x in three), ref)
    # a real policy: neither uniform nor deterministic on average
    assert 0.01 < float(three[0].mean()) < 0.99


def test_entropy_against_the_entropy_metric_kernel():
    """The unnormalised entropy mean against toued_entropy's actor-entropy metric (k_entropy_metric: the sum over the
    same rows t < T of -sum_j (p_j + 1e-8) log(p_j + 1e-8), in float32 with the fast exponential and logarithm).  The
    tolerance is what that kernel's own test allows it against the oracle, tests/test_gpu_meta.py
    _assert_run_matches_oracle: rtol 2e-5, atol 1e-7 on "policy_entropy".  Indices inside the table only: that kernel
    does not hold an index to the row."""
    from toued import _lib
    N, T, W, D = 3, 20, 64, 65
    rs = np.random.RandomState(5)
    c = {"theta": rs.randn(N, D, 5).astype(np.float32),
         "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
         "time": rs.randint(0, 2001, size=(N, T + 1, W)).astype(np.int32)}
    _, _, _, steps = _abi(c)
    mean_h = steps[:, 0].astype(np.float64).reshape(N, -1).mean(axis=1)
    ent = _abi(c, steps=False)[0]
    np.testing.assert_allclose(ent.astype(np.float64) * math.log(5), mean_h, rtol=2.0 ** -23, atol=0)
    dev = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    phi = torch.zeros((N, D, 8), device="cuda")
    met = torch.zeros((N, 8), device="cuda")
    _lib.call("toued_entropy", N, W, T, D, _lib.ptr(dev["theta"]), _lib.ptr(phi), _lib.ptr(dev["idx"]),
              _lib.ptr(dev["time"]), _lib.ptr(met), 0.0, 0.0, None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    metric = met[:, 3].cpu().numpy().astype(np.float64) / (T * W)
    print("mean entropy", mean_h, "toued_entropy / (T W)", metric, "rel diff", np.abs(metric - mean_h) / mean_h)
    np.testing.assert_allclose(metric, mean_h, rtol=2e-5, atol=1e-7)


# ------------------------------------------------------------------------------------ toued.plr.policy_scores
def test_policy_scores_match_restatement_on_the_eval_trajectory():
    from toued import plr
    smp, levels, theta, keys, tr, host, ref = _eval_trajectory()
    N = levels.shape[0]
    got = plr.policy_scores(smp, _dk(keys), levels, theta)
    assert len(got) == 3 and all(g.shape == (N,) and g.dtype == torch.float32 for g in got)
    _check_scores(tuple(g.cpu().numpy() for g in got), ref)
    # the same trajectory as the wrapper test's: the same bits as one direct call on it
    for g, w in zip(got, smp.rollout_manager.policy_scores(tr, theta)):
        assert torch.equal(g, w)
    # a chunk size that leaves a shorter last chunk, and one agent per chunk: the same bits
    for chunk in (3, 1):
        for g, w in zip(plr.policy_scores(smp, _dk(keys), levels, theta, chunk_agents=chunk), got):
            assert torch.equal(g, w), chunk
    for k, name in enumerate(NAMES):
        assert torch.equal(plr.POLICY_FUNCTIONS[name](smp, _dk(keys), levels, theta), got[k])
    empty = plr.policy_scores(smp, _dk(keys)[:0], levels[:0], theta[:0])
    assert all(e.shape == (0,) for e in empty)


@pytest.mark.parametrize("name,extra", [("policy_entropy", ()), ("least_confidence", ("--use_es",)),
                                        ("min_margin", ("--level_editor", "accel", "--staleness_coeff", "0.3"))])
def test_plr_round_writes_the_terminated_agents_scores_only(name, extra, monkeypatch):
    from toued import plr, prng
    from toued.env import L_BUFID, L_LIFETIME
    N, B = 8, 16
    smp = _sampler("small", name, N, B, extra)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    assert buf.max_return is None
    assert (buf.stamp is not None) == ("--staleness_coeff" in extra)
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    assert agents.vcrit is None                      # no critic anywhere in the round
    agents.theta.mul_(10.0)
    resets = []
    real_reset = plr.reset_lowest_scoring

    def recording_reset(*a, **kw):
        ids = real_reset(*a, **kw)
        resets.append(ids)
        return ids

    monkeypatch.setattr(plr, "reset_lowest_scoring", recording_reset)
    k = NAMES.index(name)
    for rnd, t in enumerate([[1, 0, 1, 1, 0, 0, 1, 0], [0, 1, 1, 0, 1, 0, 1, 1]]):
        term = torch.tensor(t, dtype=torch.bool, device="cuda")
        agents.step = torch.where(term, agents.levels[:, L_LIFETIME], torch.zeros_like(agents.step))
        old_ids = agents.levels[:, L_BUFID].long().clone()
        sel = term.nonzero().flatten()
        before = buf.score.clone()
        levels0, theta0 = agents.levels.clone(), agents.theta.clone()
        rng = prng.PRNGKey(2 + rnd, "cuda")
        # plr_sample's keys: rng, sub = split(rng) (reset); rng, sub = split(rng); keys = split(sub, N)
        r = prng.split(rng, 2)[0].contiguous()
        sub = prng.split(r, 2)[1].contiguous()
        keys = prng.split(sub, N).contiguous()
        want = plr.policy_scores(smp, keys[sel].contiguous(), levels0[sel].contiguous(), theta0[sel].contiguous())[k]
        assert (want > 0).all() and (want <= 1).all()
        buf, agents = smp.sample(rng, buf, agents)
        torch.cuda.synchronize()
        reset_ids = resets[-1].long()
        assert torch.equal(smp.last_plr["score"][sel], want)
        assert not smp.last_plr["score"][~term].any()
        assert torch.equal(buf.score[old_ids[sel]], want)
        touched = torch.zeros(B, dtype=torch.bool, device="cuda")
        touched[reset_ids] = True
        touched[old_ids[sel]] = True
        assert torch.equal(buf.score[~touched], before[~touched])
        assert not buf.score[reset_ids].any()
        assert buf.max_return is None and (buf.stamp is not None) == ("--staleness_coeff" in extra)
        agents.theta.mul_(10.0)                      # the terminated agents' fresh tables: a policy worth scoring


# ------------------------------------------------------------------------------------ Trainer
def _finite(x):
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if x is None or isinstance(x, str):
        return True
    return bool(torch.isfinite(torch.as_tensor(x, dtype=torch.float32)).all())


def test_trainer_runs_with_min_margin_accel_and_rank_sampled():
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = parse_args(["--env_mode", "debug", "--num_agents", "8", "--num_mini_batches", "1", "--seed", "5",
                       "--score_function", "min_margin", "--level_editor", "accel", "--score_transform",
                       "rank_sampled", "--buffer_size", "32"])
    tr = Trainer(args)
    assert tr.buffer.max_return is None and tr.buffer.stamp is None
    scored = 0
    for _ in range(2):
        tr.agents.levels[:4, L_LIFETIME] = 1            # four agents reach their lifetime in every step
        m = tr.meta_step()
        torch.cuda.synchronize()
        scored += int(tr.sampler.last_plr["score"].count_nonzero().item())
        assert _finite(m)
    tr.finish()
    assert scored > 0
    assert torch.isfinite(tr.buffer.score).all() and (tr.buffer.score >= 0).all() and (tr.buffer.score <= 1).all()
    assert tr.buffer.score.count_nonzero() > 0


def test_trainer_runs_with_es_and_policy_entropy():
    """TA-LPG (--use_es --lifetime_conditioning) with a buffer-driven score: OpenES trains no value critic, so every
    critic-based score is refused there; the policy scores need none."""
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = parse_args(["--env_mode", "all_vrandlife", "--num_agents", "2", "--num_mini_batches", "1", "--seed", "3",
                       "--score_function", "policy_entropy", "--use_es", "--lifetime_conditioning",
                       "--lpg_learning_rate", "0.01", "--buffer_size", "16"])
    tr = Trainer(args)
    tr.step_fn.K = 2           # two agent updates per candidate instead of the mode's max_lifetime (test_gpu_es_curve)
    assert tr.agents.vcrit is None and tr.buffer.max_return is None
    scored = 0
    for _ in range(2):
        tr.agents.levels[:1, L_LIFETIME] = 1            # agent 0 reaches its lifetime in every step
        m = tr.meta_step()
        torch.cuda.synchronize()
        scored += int(tr.sampler.last_plr["score"].count_nonzero().item())
        assert _finite(m)
    tr.finish()
    assert scored > 0
    assert torch.isfinite(tr.buffer.score).all() and (tr.buffer.score >= 0).all() and (tr.buffer.score <= 1).all()
