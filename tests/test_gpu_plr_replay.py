"""GPU parity of PLR's rank-weighted, staleness-aware replay sampling (toued_plr_sample_prio; not in the reference).

  * transforms 0 / 1 with staleness_coeff = 0 and no stamps reproduce toued_plr_sample on every output
  * p_out, rep, rnd, use and chosen bit-exact against the numpy restatement (tests/plr_replay_ref.py) over the three
    transforms x rho x temperature at the power-of-two padding edges, at C3's shape, at the LDS maximum B = 8192 and in
    the too-few-valid-slots fallback
  * the floor: at a temperature where most rank weights underflow every replay id is still a valid slot
  * the staleness edges: no age at all, a stamp from the future, equal ages, one very stale slot
  * every argument check of the entry
  * LevelSampler.sample end to end with --score_transform rank_sampled --staleness_coeff 0.3: buffer (stamps and
    clock included), agents and replay distribution against the restatement driven by the device's scores

Single-workgroup launches on buffers of at most 8192 slots.
"""
import numpy as np
import pytest
import torch

import plr_replay_ref as prr
from oracle import jaxrand as jr
from oracle import sampler as osp

pytestmark = pytest.mark.gpu

F32 = np.float32
CODES = {"rank": 0, "proportional": 1, "rank_sampled": 2}
OUTS = ("chosen", "rep", "rnd", "use")


def dk(a):
    from toued.prng import from_uint32_numpy
    return from_uint32_numpy(a, "cuda")


def _buffer_state(B, seed, n_active, frac_new):
    """tests/test_gpu_plr.py's buffers: quarter-rounded scores (ties) with some -0.0; plus stamps in [0, 50)."""
    rs = np.random.RandomState(seed)
    score = rs.randn(B).astype(F32)
    score = (np.round(score * 4) / 4).astype(F32)
    score[rs.rand(B) < 0.05] = -0.0
    active = np.zeros(B, bool)
    active[rs.choice(B, n_active, replace=False)] = True
    new = (rs.rand(B) < frac_new) & ~active
    if frac_new == 0.0:
        new[:] = False
    stamp = rs.randint(0, 50, B).astype(np.int32)
    return score, active, new, stamp


def _keys(seed):
    """(kbuf for the device, keys3 for the restatement): replay_rng, random_rng, select_rng."""
    k = jr.split(jr.PRNGKey(seed), 3)
    k3 = np.stack([k[1], k[2], k[0]])
    return k3, (k3[0], k3[1], k3[2])


def _prio(score, active, new, stamp, now, kbuf, transform, T, rho, N, p_replay=0.5):
    from toued import _lib
    B = score.shape[0]
    s, a, n = (torch.from_numpy(x).cuda() for x in (score, active, new))
    st = None if stamp is None else torch.from_numpy(stamp).cuda()
    out = [torch.full((N,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    p = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
    _lib.call("toued_plr_sample_prio", B, N, _lib.ptr(s), _lib.ptr(a), _lib.ptr(n), _lib.ptr(st), int(now),
              _lib.ptr(dk(kbuf)), CODES[transform], float(T), float(rho), float(p_replay),
              *[_lib.ptr(o) for o in out], _lib.ptr(p), _lib.stream_ptr())
    got = {k: o.cpu().numpy() for k, o in zip(OUTS, out)}
    got["p"] = p.cpu().numpy()
    return got


def _assert_equals_ref(got, ref, tag):
    assert np.array_equal(got["p"].view(np.uint32), ref["p"].view(np.uint32)), (tag, "p")
    for k in ("rep", "rnd", "use", "chosen"):
        assert np.array_equal(got[k], ref[k]), (tag, k)


# ------------------------------------------------------------------------------------------------ 1. the old entry
@pytest.mark.parametrize("transform", ["rank", "proportional"])
@pytest.mark.parametrize("B,N,n_active,frac_new", [(33, 7, 3, 0.3), (300, 64, 32, 0.5), (100, 16, 0, 0.0)])
def test_reproduces_plr_sample(transform, B, N, n_active, frac_new):
    from toued import _lib
    score, active, new, _ = _buffer_state(B, B * 7 + N, n_active, frac_new)
    kbuf, _ = _keys(B + N)
    s, a, n = (torch.from_numpy(x).cuda() for x in (score, active, new))
    old = [torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(4)]
    _lib.call("toued_plr_sample", B, N, _lib.ptr(s), _lib.ptr(a), _lib.ptr(n), _lib.ptr(dk(kbuf)),
              int(transform == "proportional"), 1.0, 0.5, *[_lib.ptr(o) for o in old], _lib.stream_ptr())
    got = _prio(score, active, new, None, 0, kbuf, transform, 1.0, 0.0, N)
    for k, o in zip(OUTS, old):
        assert np.array_equal(got[k], o.cpu().numpy()), k


# ------------------------------------------------------------------------------- 2. bit-exact vs the restatement
@pytest.mark.parametrize("B,N,n_active,frac_new", [(33, 7, 3, 0.3), (64, 8, 6, 0.25), (300, 64, 32, 0.5)])
def test_bitexact_small(B, N, n_active, frac_new):
    """All three transforms x rho in {0, 0.3, 1} x T in {1, 0.1} on one buffer per shape (B = 33 and 64: one slot
    past and exactly at a power of two of the sort's padding)."""
    score, active, new, stamp = _buffer_state(B, B * 7 + N, n_active, frac_new)
    assert (~(new | active)).sum() >= N
    kbuf, k3 = _keys(B + N)
    now = 57
    for transform in prr.TRANSFORMS:
        for rho in (0.0, 0.3, 1.0):
            for T in (1.0, 0.1):
                ref = prr.sample(k3, score, active, new, N, transform, T, rho, stamp, now)
                got = _prio(score, active, new, stamp, now, kbuf, transform, T, rho, N)
                _assert_equals_ref(got, ref, (transform, rho, T))
                valid = ~(new | active)
                if transform == "rank_sampled" or rho > 0:
                    assert valid[got["rep"]].all() and len(set(got["rep"].tolist())) == N


@pytest.mark.parametrize("B,N,n_active,transform,T,rho", [
    (4000, 512, 512, "rank_sampled", 0.1, 0.1),     # C3's shape
    (8192, 512, 512, "rank_sampled", 0.1, 0.3),     # the LDS maximum
    (1000, 1000, 500, "rank_sampled", 0.1, 0.3),    # fewer valid slots than N: p = 1, use = 0
])
def test_bitexact_large(B, N, n_active, transform, T, rho):
    score, active, new, stamp = _buffer_state(B, B * 7 + N, n_active, 0.3)
    kbuf, k3 = _keys(B + N)
    ref = prr.sample(k3, score, active, new, N, transform, T, rho, stamp, 64)
    got = _prio(score, active, new, stamp, 64, kbuf, transform, T, rho, N)
    _assert_equals_ref(got, ref, (B, N))
    if N == B:
        assert np.all(got["p"] == 1.0) and np.all(got["use"] == 0)
    else:
        assert abs(float(got["p"].astype(np.float64).sum()) - 1.0) < 1e-6
        assert got["use"].sum() > 0


# ------------------------------------------------------------------------------------------------- 3. underflow
@pytest.mark.parametrize("N", [8, 16])
def test_underflow_floor_keeps_replay_ids_valid(N):
    """rank^(-1/T) at T = 0.02 is rank^-50: ranks 1-5 keep a normal float32 weight, ranks 6-8 a subnormal one and
    every later rank's weight is 0.  Without the floor a valid slot with p = 0 shares the invalid slots' +inf Gumbel
    key and the top-k fills up by index, active slots included; with it every id is a valid slot.

    N = 8: the floor changes p (only 5 valid slots stay above it), but 8 = N weights are still positive, so even the
    unfloored restatement draws 8 valid ids at this N -- whatever the buffer, the weights being a function of the rank
    alone.  N = 16 is the smallest agent count of this suite's shapes past those 8 ranks: there the unfloored
    restatement does return invalid ids, which shows that the input exercises the floor."""
    B, T = 64, 0.02
    score, active, new, _ = _buffer_state(B, B * 7 + 8, 6, 0.25)
    valid = ~(new | active)
    kbuf, k3 = _keys(B + N)
    no_floor = prr.sample(k3, score, active, new, N, "rank_sampled", T, floor=False)
    assert (no_floor["p"][valid] >= prr.TINY).sum() < N
    assert (no_floor["p"][valid] > 0).sum() == 8
    assert valid[no_floor["rep"]].all() == (N == 8)
    ref = prr.sample(k3, score, active, new, N, "rank_sampled", T)
    got = _prio(score, active, new, None, 0, kbuf, "rank_sampled", T, 0.0, N)
    assert valid[got["rep"]].all() and len(set(got["rep"].tolist())) == N
    _assert_equals_ref(got, ref, "underflow")


# ------------------------------------------------------------------------------------------- 4. staleness edges
def test_staleness_edges():
    B, N, now = 64, 8, 40
    score, active, new, stamp = _buffer_state(B, B * 7 + N, 6, 0.25)
    valid = ~(new | active)
    v = np.flatnonzero(valid)
    kbuf, k3 = _keys(B + N)
    future = stamp.copy()
    future[v[3]] = now + 5
    # one slot not scored for a long time, the others scored last round; it has the lowest score of all
    stale = np.full(B, now - 1, np.int32)
    stale[v[-1]] = now - 30000
    low = score.copy()
    low[v[-1]] = F32(-9.0)
    cases = [("no age: uniform staleness part", score, np.full(B, now, np.int32)),
             ("a stamp past now clamps to age 0", score, future),
             ("equal ages", score, np.full(B, 7, np.int32)),
             ("one very stale slot", low, stale)]
    for tag, sc, st in cases:
        for transform in prr.TRANSFORMS:
            for rho in (0.3, 1.0):
                ref = prr.sample(k3, sc, active, new, N, transform, 1.0, rho, st, now)
                got = _prio(sc, active, new, st, now, kbuf, transform, 1.0, rho, N)
                _assert_equals_ref(got, ref, (tag, transform, rho))
                assert valid[got["rep"]].all(), (tag, transform, rho)
    got = _prio(score, active, new, np.full(B, now, np.int32), now, kbuf, "rank", 1.0, 1.0, N)
    assert np.array_equal(got["p"], np.where(valid, F32(1.0) / F32(valid.sum()), 0).astype(F32))
    got = _prio(score, active, new, future, now, kbuf, "rank", 1.0, 1.0, N)
    assert got["p"][v[3]] == prr.TINY                    # age 0 under rho = 1: floored, not 0
    got = _prio(low, active, new, stale, now, kbuf, "rank", 1.0, 1.0, N)
    assert got["rep"][0] == v[-1]                        # top-N of the staleness part alone: the stale slot first
    got = _prio(low, active, new, stale, now, kbuf, "rank", 1.0, 0.0, N)
    assert v[-1] not in got["rep"]                       # and by score alone it is never replayed


# ------------------------------------------------------------------------------------------- 5. argument checks
_OK = dict(B=64, N=8, stamp=None, transform=2, T=1.0, rho=0.0)


@pytest.mark.parametrize("change,word", [
    (dict(B=0), "<= N <= B"), (dict(B=8193), "<= N <= B"), (dict(N=-1), "<= N <= B"), (dict(N=65), "<= N <= B"),
    (dict(T=0.0), "temperature"), (dict(T=-1.0), "temperature"), (dict(T=float("nan")), "temperature"),
    (dict(transform=-1), "transform"), (dict(transform=3), "transform"),
    (dict(rho=-0.1), "staleness_coeff"), (dict(rho=1.5), "staleness_coeff"), (dict(rho=float("nan")), "staleness_coeff"),
    (dict(rho=0.3), "stamps"),
])
def test_argument_checks(change, word):
    """Every violated requirement returns -1 with a message naming the entry, before anything is launched (all
    pointers are null)."""
    from toued import _lib
    L = _lib.lib()
    a = dict(_OK, **change)
    rc = L.toued_plr_sample_prio(a["B"], a["N"], None, None, None, a["stamp"], 1, None, a["transform"], a["T"], a["rho"],
                                 0.5, None, None, None, None, None, None)
    msg = L.toued_last_error().decode()
    assert rc == -1, (change, rc)
    assert "toued_plr_sample_prio" in msg and word in msg, msg


def test_zero_agents_launch_nothing():
    from toued import _lib
    assert _lib.lib().toued_plr_sample_prio(64, 0, None, None, None, None, 1, None, 2, 1.0, 0.0, 0.5, None, None, None,
                                            None, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_level_sampler_rank_sampled_staleness_end_to_end():
    """Three sample() rounds of a tabular optimal_regret sampler with --score_transform rank_sampled
    --staleness_coeff 0.3, each replayed in numpy from the device's own scores (shaped like
    test_gpu_plr.py::test_level_sampler_alg_regret_end_to_end).  --num_mini_batches 1 only makes 8 agents a legal
    batch."""
    from toued import prng
    from toued.env import L_BUFID, L_LIFETIME
    from toued.level_sampler import LevelBuffer, LevelSampler
    from toued.parse_args import parse_args
    from toued.plr import replay_distribution
    N, B, rho = 8, 64, 0.3
    base = ["--env_mode", "tabular", "--score_function", "optimal_regret", "--buffer_size", str(B), "--num_agents",
            str(N), "--num_mini_batches", "1"]
    args = parse_args(base + ["--score_transform", "rank_sampled", "--staleness_coeff", str(rho)])
    smp = LevelSampler(args)
    buf = smp.initialize_buffer(prng.PRNGKey(0, "cuda"))
    assert buf.stamp is not None and buf.stamp.dtype == torch.int32 and not buf.stamp.any() and buf.clock == 0
    buf, agents = smp.initial_sample(prng.PRNGKey(1, "cuda"), buf, N, False)
    agents.step = agents.levels[:, L_LIFETIME].clone()      # a first round with every agent terminated
    rng = prng.PRNGKey(2, "cuda")
    replayed = 0
    for it in range(3):
        pre = {k: getattr(buf, k).cpu().numpy().copy() for k in ("score", "active", "new", "stamp")}
        now = buf.clock + 1
        term = (agents.step >= agents.levels[:, L_LIFETIME]).cpu().numpy()
        old_ids = agents.levels[:, L_BUFID].cpu().numpy()
        rng_np = prng.to_uint32_numpy(rng)
        buf, agents = smp.sample(rng, buf, agents)
        rng = prng.split(rng, 2)[1].contiguous()
        r, _ = jr.split(rng_np, 2)
        ids, score, active, new = osp.reset_lowest_scoring(pre["score"], pre["active"], pre["new"], N)
        stamp = pre["stamp"].copy()
        stamp[ids] = now
        r, _ = jr.split(r, 2)
        sc = smp.last_plr["score"].cpu().numpy()
        score[old_ids[term]] = sc[term]
        active[old_ids[term]] = False
        new[old_ids[term]] = False
        stamp[old_ids[term]] = now
        k3 = jr.split(r, 3)
        ref = prr.sample((k3[1], k3[2], k3[0]), score, active, new, N, "rank_sampled", 1.0, rho, stamp, now)
        replayed += int((ref["use"].astype(bool) & term).sum())
        assert np.array_equal(smp.last_plr["p"].cpu().numpy().view(np.uint32), ref["p"].view(np.uint32)), it
        # the public helper on the buffer as the kernel saw it (before this round's agents are marked active)
        t = lambda x: torch.from_numpy(x).cuda()
        seen = LevelBuffer(buf.levels, t(score), t(active), t(new), t(stamp), now - 1)
        assert torch.equal(replay_distribution(seen, N, "rank_sampled", 1.0, rho), smp.last_plr["p"]), it
        new_ids = np.where(term, ref["chosen"], old_ids)
        active[new_ids] = True
        assert np.array_equal(buf.score.cpu().numpy(), score), it
        assert np.array_equal(buf.active.cpu().numpy(), active), it
        assert np.array_equal(buf.new.cpu().numpy(), new), it
        assert np.array_equal(buf.stamp.cpu().numpy(), stamp), it
        assert buf.clock == now == it + 1
        assert np.array_equal(agents.levels[:, L_BUFID].cpu().numpy(), new_ids), it
        assert np.array_equal(agents.levels.cpu().numpy(), buf.levels.cpu().numpy()[new_ids]), it
        agents.step = torch.where(torch.arange(N, device="cuda") % 2 == it % 2, agents.levels[:, L_LIFETIME],
                                  torch.zeros_like(agents.step))
    assert replayed > 0          # the rounds did draw replay levels from the new distribution
    # the default flags keep the buffer without stamps and the reference's sampler call
    plain = LevelSampler(parse_args(base))
    pbuf = plain.initialize_buffer(prng.PRNGKey(0, "cuda"))
    assert pbuf.stamp is None and pbuf.clock == 0
