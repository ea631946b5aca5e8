"""GPU: toued_value_loss_scores / RolloutWrapper.value_loss_scores / toued.plr.value_loss_scores against the numpy
restatement (tests/vscore_ref.py), and the positive_value_loss / l1_value_loss PLR scores built on them.

The advantages are compared bit for bit.  A score is the float64 sum of float32 terms divided by the count and
rounded to float32 once: |gpu - f32(ref)| <= 2^-23 |ref| is that one rounding (the float64 sums' own error, about
n 2^-53 relative, is far below it and can only move the result across one float32 rounding boundary).
"""
import functools

import numpy as np
import pytest
import torch

import vscore_ref as vr
from oracle import jaxrand as jr

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95
GL = float(np.float32(GAMMA * LAM))

# (N, T, W, D, p_done).  The kernel walks time in chunks of 2048 // min(W, 256) steps: T = 1000 at W = 64 is 31 chunks
# of 32 steps and one of 8; T = 33 at W = 96 is a chunk of 21 and one of 12; W = 200 leaves a worker tile that is no
# multiple of 64; W = 300 is a tile of 256 workers and one of 44; D = 5409 is the largest critic row of any mode
# (tabular).  The seams of the loader shared with k_max_mc_scores (SEAMS is the same list in test_gpu_maxmc.py): T one
# chunk exactly (W = 256: 8 steps) and one step more, where the row handed on and the double buffer flip with a one-row
# chunk; a second tile of a single worker; W = 1 with a chunk boundary at the last step
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


@functools.lru_cache(maxsize=None)
def _reference(N, T, W, D, p_done):
    """(pvl f64 [N], l1 f64 [N], adv f32 [N, T, W]) of the case, computed once."""
    tr = _case(N, T, W, D, p_done)
    if N == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, T, W), np.float32)
    return vr.value_loss_scores(tr["vcrit"], tr["idx"], tr["time"], tr["reward"], tr["done"], GAMMA, LAM)


def _abi(tr, pvl=True, l1=True, adv=True):
    """toued_value_loss_scores on host arrays; a False output is passed as NULL.  Returns numpy (pvl, l1, adv)."""
    from toued import _lib
    N, T, W = tr["reward"].shape
    D = tr["vcrit"].shape[1]
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in tr.items()}
    o_pvl = torch.full((N,), float("nan"), device="cuda") if pvl else None
    o_l1 = torch.full((N,), float("nan"), device="cuda") if l1 else None
    o_adv = torch.full((N, T, W), float("nan"), device="cuda") if adv else None
    _lib.call("toued_value_loss_scores", N, W, T, D, _lib.ptr(dev["vcrit"]), _lib.ptr(dev["idx"]),
              _lib.ptr(dev["time"]), _lib.ptr(dev["reward"]), _lib.ptr(dev["done"]), GAMMA, GL, _lib.ptr(o_pvl),
              _lib.ptr(o_l1), _lib.ptr(o_adv), _lib.stream_ptr())
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in (o_pvl, o_l1, o_adv))


def _check_scores(name, got, ref):
    got = got.astype(np.float64)
    for a in range(ref.shape[0]):
        want = float(np.float32(ref[a]))
        err, bound = abs(got[a] - want), 2.0 ** -23 * abs(ref[a])
        print(f"{name}[{a}]: gpu {got[a]!r} f32(ref) {want!r} |diff| {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, a, got[a], want, bound)


@pytest.mark.parametrize("N,T,W,D,p_done", CASES)
def test_kernel_matches_restatement(N, T, W, D, p_done):
    tr = _case(N, T, W, D, p_done)
    ref_pvl, ref_l1, ref_adv = _reference(N, T, W, D, p_done)
    pvl, l1, adv = _abi(tr)
    assert pvl.shape == (N,) and l1.shape == (N,) and adv.shape == (N, T, W)
    np.testing.assert_array_equal(adv, ref_adv)
    _check_scores("pvl", pvl, ref_pvl)
    _check_scores("l1", l1, ref_l1)
    if N:
        assert (l1 >= pvl).all() and (pvl >= 0).all()
        # outputs left out (NULL) change nothing in the others
        p2, l2, a2 = _abi(tr, adv=False)
        assert a2 is None and np.array_equal(p2, pvl) and np.array_equal(l2, l1)
        p3, l3, a3 = _abi(tr, l1=False)
        assert l3 is None and np.array_equal(p3, pvl) and np.array_equal(a3, adv)
        p4, l4, a4 = _abi(tr, pvl=False, adv=False)
        assert p4 is None and a4 is None and np.array_equal(l4, l1)


def test_wrapper_matches_abi_and_gae():
    """RolloutWrapper.value_loss_scores is the ABI call, and its advantages are toued.metrics.gae's on the gathered
    values."""
    from toued.metrics import gae
    from toued.rollout import RolloutWrapper, Transition
    case = (2, 33, 96, 65, 0.0)
    tr = _case(*case)
    N, T, W = tr["reward"].shape
    dev = {k: torch.from_numpy(np.array(v)).cuda() for k, v in tr.items()}
    trans = Transition(dev["idx"], dev["time"], torch.zeros((N, T, W), dtype=torch.uint8, device="cuda"),
                       dev["reward"], dev["done"])
    ro = RolloutWrapper("debug", 20)
    pvl, l1, adv = ro.value_loss_scores(trans, dev["vcrit"], GAMMA, LAM, return_adv=True)
    a_pvl, a_l1, a_adv = _abi(tr)
    assert np.array_equal(pvl.cpu().numpy(), a_pvl) and np.array_equal(l1.cpu().numpy(), a_l1)
    assert np.array_equal(adv.cpu().numpy(), a_adv)
    two = ro.value_loss_scores(trans, dev["vcrit"].view(N, -1, 1), GAMMA, LAM)       # the critic table's shape
    assert len(two) == 2 and torch.equal(two[0], pvl) and torch.equal(two[1], l1)
    v = torch.from_numpy(vr.values(tr["vcrit"], tr["idx"], tr["time"])).cuda()
    g_adv, _ = gae(v, dev["reward"], dev["done"], GAMMA, LAM)
    assert torch.equal(adv, g_adv)


def test_all_negative_advantages_give_zero_pvl():
    N, T, W, D = 2, 70, 64, 9
    rs = np.random.RandomState(5)
    tr = {"vcrit": np.zeros((N, D), np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": -np.ones((N, T, W), np.float32), "done": np.zeros((N, T, W), np.uint8)}
    pvl, l1, adv = _abi(tr)
    assert (adv < 0).all()
    assert (pvl == 0.0).all()
    ref_pvl, ref_l1, ref_adv = vr.value_loss_scores(tr["vcrit"], tr["idx"], tr["time"], tr["reward"], tr["done"],
                                                    GAMMA, LAM)
    np.testing.assert_array_equal(adv, ref_adv)
    _check_scores("l1", l1, ref_l1)


def test_more_than_256_workers_go_in_tiles():
    """W = 300: a tile of 256 workers and one of 44, each with its own walk over time (8 and 46 steps per chunk)."""
    rs = np.random.RandomState(7)
    N, T, W, D = 2, 50, 300, 9
    tr = {"vcrit": rs.randn(N, D).astype(np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": rs.randn(N, T, W).astype(np.float32), "done": (rs.rand(N, T, W) < 0.1).astype(np.uint8)}
    pvl, l1, adv = _abi(tr)
    ref_pvl, ref_l1, ref_adv = vr.value_loss_scores(tr["vcrit"], tr["idx"], tr["time"], tr["reward"], tr["done"],
                                                    GAMMA, LAM)
    np.testing.assert_array_equal(adv, ref_adv)
    _check_scores("pvl", pvl, ref_pvl)
    _check_scores("l1", l1, ref_l1)


def test_deterministic_and_independent_of_the_batch():
    case = (3, 1, 64, 10, 0.5)
    big = (2, 1000, 64, 3201, 0.05)
    for c in (case, big):
        a, b = _abi(_case(*c)), _abi(_case(*c))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # agent 1 of a 3-agent call against a call on its rows alone
    rs = np.random.RandomState(11)
    N, T, W, D = 3, 45, 96, 33
    tr = {"vcrit": rs.randn(N, D).astype(np.float32),
          "idx": rs.randint(0, D - 1, size=(N, T + 1, W)).astype(np.int32),
          "time": rs.randint(0, 2000, size=(N, T + 1, W)).astype(np.int32),
          "reward": rs.randn(N, T, W).astype(np.float32), "done": (rs.rand(N, T, W) < 0.1).astype(np.uint8)}
    pvl, l1, adv = _abi(tr)
    p1, l1_1, a1 = _abi({k: v[1:2] for k, v in tr.items()})
    assert p1[0] == pvl[1] and l1_1[0] == l1[1] and np.array_equal(a1[0], adv[1])


def test_argument_checks():
    from toued import _lib
    L = _lib.lib()
    N, T, W, D = 2, 4, 8, 5
    vc = torch.zeros((N, D), device="cuda")
    ix = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    tm = torch.zeros((N, T + 1, W), dtype=torch.int32, device="cuda")
    rw = torch.zeros((N, T, W), device="cuda")
    dn = torch.zeros((N, T, W), dtype=torch.uint8, device="cuda")
    pv, l1 = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    P = _lib.ptr
    st = _lib.stream_ptr()
    good = dict(N=N, W=W, T=T, D=D, vc=P(vc), ix=P(ix), tm=P(tm), rw=P(rw), dn=P(dn), pv=P(pv), l1=P(l1))

    def call(**kw):
        a = dict(good, **kw)
        return L.toued_value_loss_scores(a["N"], a["W"], a["T"], a["D"], a["vc"], a["ix"], a["tm"], a["rw"], a["dn"],
                                         GAMMA, GL, a["pv"], a["l1"], None, st)

    assert call() == 0
    assert call(N=0) == 0
    assert call(N=0, vc=None, ix=None, tm=None, rw=None, dn=None, pv=None, l1=None) == 0      # empty tensors
    bad = [dict(T=0), dict(W=0), dict(D=1), dict(N=-1), dict(vc=None), dict(ix=None), dict(tm=None), dict(rw=None),
           dict(dn=None), dict(pv=None, l1=None), dict(W=65536, T=32768)]
    for kw in bad:
        # a fresh error text per case: another entry point's failure in between
        assert L.toued_gae(1, 0, 1, None, None, None, 0.5, 0.5, None, None, st) == -1
        assert "toued_gae" in L.toued_last_error().decode()
        assert call(**kw) == -1, kw
        msg = L.toued_last_error().decode()
        assert msg and "toued_value_loss_scores" in msg, (kw, msg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- toued.plr.value_loss_scores
def _sampler(mode, score_function, N=4, B=16):
    from toued.level_sampler import LevelSampler
    from toued.parse_args import parse_args
    args = parse_args(["--env_mode", mode, "--score_function", score_function, "--num_agents", str(N),
                       "--num_mini_batches", "1", "--env_workers", "64", "--buffer_size", str(B)])
    return LevelSampler(args)


@pytest.mark.parametrize("mode", ["debug", "small"])
def test_value_loss_scores_match_restatement_on_the_eval_trajectory(mode):
    from toued import prng
    from toued.agents import create_agents, create_value_critics, eval_agent_reset
    from toued.env import LevelGenerator
    from toued.plr import value_loss_scores
    N, W = 4, 64
    smp = _sampler(mode, "positive_value_loss", N)
    ro = smp.rollout_manager
    dk = lambda a: prng.from_uint32_numpy(np.ascontiguousarray(a), "cuda")
    levels = LevelGenerator(mode)(dk(jr.split(jr.PRNGKey(301), N)))
    theta, _ = create_agents(dk(jr.split(jr.PRNGKey(302), N)), ro.obs_dim, 8)
    theta.mul_(10.0)
    vcrit = create_value_critics(dk(jr.split(jr.PRNGKey(303), N)), ro.obs_dim).mul_(10.0)
    keys = jr.split(jr.PRNGKey(304), N)
    pvl, l1 = value_loss_scores(smp, dk(keys), levels, theta, vcrit)
    assert pvl.shape == (N,) and l1.shape == (N,) and pvl.dtype == torch.float32 and l1.dtype == torch.float32
    # lpg_rng of _compute_algorithmic_regret (level_sampler.py:293-329): rng, c = split(keys); rng, tr = split(rng);
    # lpg_rng, a2c_rng = split(rng); then eval_agent's reset and rollout key
    rng = jr.split(keys, 2)[:, 0]
    rng = jr.split(rng, 2)[:, 0]
    lpg_rng = jr.split(rng, 2)[:, 0]
    state, ro_keys = eval_agent_reset(ro, dk(lpg_rng), levels, W)
    tr, _, _ = ro.batch_rollout(ro_keys, theta, levels, state, eval=True)
    T = ro.eval_rollout_len
    assert tr.reward.shape == (N, T, W)
    ref_pvl, ref_l1, _ = vr.value_loss_scores(vcrit.cpu().numpy(), tr.obs_idx.cpu().numpy(),
                                              tr.obs_time.cpu().numpy(), tr.reward.cpu().numpy(),
                                              tr.done.cpu().numpy(), smp.args.gamma, smp.args.gae_lambda)
    _check_scores("pvl", pvl.cpu().numpy(), ref_pvl)
    _check_scores("l1", l1.cpu().numpy(), ref_l1)
    assert (ref_l1 > 0).all()
    # one agent per chunk, and a chunk size that leaves a shorter last chunk: the same bits
    for chunk in (1, 3):
        p_c, l_c = value_loss_scores(smp, dk(keys), levels, theta, vcrit, chunk_agents=chunk)
        assert torch.equal(p_c, pvl) and torch.equal(l_c, l1), chunk
    e_p, e_l = value_loss_scores(smp, dk(keys)[:0], levels[:0], theta[:0], vcrit[:0])
    assert e_p.shape == (0,) and e_l.shape == (0,)


@pytest.mark.parametrize("which,name", [(0, "positive_value_loss"), (1, "l1_value_loss")])
def test_level_sampler_value_loss_scores_the_buffer(which, name):
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    from toued.plr import value_loss_scores
    N, B = 8, 16
    smp = _sampler("small", name, N, B)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, True)
    assert agents.vcrit is not None
    agents.vcrit.mul_(10.0)
    term = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.bool, device="cuda")
    agents.step = torch.where(term, agents.levels[:, L_LIFETIME], torch.zeros_like(agents.step))
    assert (agents.levels[:, L_LIFETIME] > 0).all()
    levels0, theta0, vcrit0 = agents.levels.clone(), agents.theta.clone(), agents.vcrit.clone()
    old_ids = agents.levels[:, L_BUFID].long().clone()
    assert old_ids.unique().numel() == N
    assert not buf.score.any()
    rng = prng.PRNGKey(2, "cuda")
    # plr_sample's keys: rng, sub = split(rng) (reset); rng, sub = split(rng); keys = split(sub, N)
    r = prng.split(rng, 2)[0].contiguous()
    sub = prng.split(r, 2)[1].contiguous()
    keys = prng.split(sub, N).contiguous()
    sel = term.nonzero().flatten()
    want = value_loss_scores(smp, keys[sel].contiguous(), levels0[sel].contiguous(), theta0[sel].contiguous(),
                             vcrit0[sel].contiguous())[which]
    assert (want > 0).all()
    buf, agents = smp.sample(rng, buf, agents)
    assert torch.equal(smp.last_plr["score"][sel], want)
    assert not smp.last_plr["score"][~term].any()
    assert torch.equal(buf.score[old_ids[sel]], want)
    others = torch.ones(B, dtype=torch.bool, device="cuda")
    others[old_ids[sel]] = False
    assert not buf.score[others].any()                  # every other slot keeps its score (0)


def test_level_sampler_without_value_critics_raises():
    from toued import prng
    smp = _sampler("small", "positive_value_loss", 8, 16)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, 8, False)
    assert agents.vcrit is None
    with pytest.raises(ValueError, match="positive_value_loss"):
        smp.sample(prng.PRNGKey(2, "cuda"), buf, agents)


def test_trainer_runs_with_positive_value_loss():
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = parse_args(["--env_mode", "debug", "--num_agents", "8", "--num_mini_batches", "1", "--seed", "5",
                       "--score_function", "positive_value_loss", "--buffer_size", "32"])
    tr = Trainer(args)
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
    assert torch.isfinite(tr.buffer.score).all() and (tr.buffer.score >= 0).all()
