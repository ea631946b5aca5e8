"""toued_episode_stats (csrc/epstats.hip) on the MI355X against its numpy restatement tests/episode_stats_ref.py.

The carry (run_ret, run_len) is bit-exact; the integer columns (episodes, len_sum, steps) are exact; the f64 sums are
within W * T * 2^-52 * sum|terms| of math.fsum: a column is the sum of at most W * T exact f64 terms, so the kernel
makes at most W * T f64 additions, each with a relative error of at most 2^-53 of a partial sum that is itself at most
sum|terms| (1 + small), which gives less than half the bound; the reference is correctly rounded.  Every case prints
the largest measured fraction of that bound (``pytest -s``; DESIGN.md section 6 records it).
"""
import numpy as np
import pytest
import torch

import episode_stats_ref as er

pytestmark = pytest.mark.gpu

WS = (1, 63, 64, 65, 257)          # below, at and above a wave; one past it; more than one 256-worker tile
TS = (1, 2, 20, 33)                # one step, a pair, the train rollout, more than a 64-worker chunk of 32 steps
SHAPES = [(N, W, T) for N in (1, 3) for W in WS for T in TS] + [(3, 64, 750)]
INT_COLS, SUM_COLS = [0, 3, 5], [1, 2, 4]


def _inputs(seed, N, T, W, pattern):
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((N, T, W)) * rng.choice([0.0, 0.01, 1.0, 30.0], (N, T, W))).astype(np.float32)
    done = er.done_pattern(pattern, N, T, W, rng)
    cr = rng.standard_normal((N, W)).astype(np.float32)
    cl = rng.integers(0, 50, (N, W)).astype(np.int32)
    return rew, done, cr, cl


def _run(rew, done, cr, cl, stats=None):
    """The raw entry point on copies of the inputs: (stats f64 [N, 6], run_ret, run_len) as numpy."""
    from toued import _lib
    N, T, W = rew.shape
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    trew, tdone, rr, rl = d(rew), d(done), d(cr), d(cl)
    st = torch.zeros((N, 6), dtype=torch.float64, device="cuda") if stats is None else d(stats)
    _lib.call("toued_episode_stats", N, W, T, _lib.ptr(trew), _lib.ptr(tdone), _lib.ptr(rr), _lib.ptr(rl),
              _lib.ptr(st), _lib.stream_ptr())
    torch.cuda.synchronize()
    return st.cpu().numpy(), rr.cpu().numpy(), rl.cpu().numpy()


def _check(got, want, mag, W, T):
    """The exact columns and the derived bound; returns the largest fraction of the bound used."""
    st, rr, rl = got
    ws, wr, wl = want
    assert np.array_equal(rr.view(np.uint32), wr.view(np.uint32)), "run_ret is not bit-exact"
    assert np.array_equal(rl, wl), "run_len"
    assert np.array_equal(st[:, INT_COLS], ws[:, INT_COLS]), "episodes / len_sum / steps"
    bound = W * T * 2.0 ** -52 * mag[:, SUM_COLS]
    err = np.abs(st[:, SUM_COLS] - ws[:, SUM_COLS])
    assert np.all(err <= bound), (err, bound)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


@pytest.mark.parametrize("N,W,T", SHAPES, ids=[f"N{n}-W{w}-T{t}" for n, w, t in SHAPES])
def test_matches_restatement(N, W, T):
    """Random rewards, every done pattern, non-zero incoming carries."""
    worst = 0.0
    for i, pattern in enumerate(er.PATTERNS):
        rew, done, cr, cl = _inputs(100 * i + W + T, N, T, W, pattern)
        ws, wr, wl, mag = er.episode_stats(rew, done, cr, cl)
        worst = max(worst, _check(_run(rew, done, cr, cl), (ws, wr, wl), mag, W, T))
    print(f"episode_stats N={N} W={W} T={T}: largest fraction of the f64 bound {worst:.3e}")


def test_zero_carry_through_the_wrapper():
    """RolloutWrapper.episode_stats: carry=None starts a lifetime, the carry returned feeds the next call, ``out``
    accumulates; two calls on T1 and T2 steps leave the carry of one call on T1 + T2 steps bit for bit."""
    from toued.rollout import EpisodeStats, RolloutWrapper, Transition
    N, W, T1, T2 = 3, 65, 20, 13
    rew, done, _, _ = _inputs(7, N, T1 + T2, W, "random")
    ro = RolloutWrapper("debug", T1, env_workers=W)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def tr(lo, hi):
        return Transition(None, None, None, d(rew[:, lo:hi]), d(done[:, lo:hi]))

    whole, carry_w = ro.episode_stats(tr(0, T1 + T2))
    assert isinstance(whole, EpisodeStats) and whole._fields == er.COLUMNS
    s1, carry = ro.episode_stats(tr(0, T1))
    s2, carry2 = ro.episode_stats(tr(T1, T1 + T2), carry=carry, out=s1)
    assert carry2[0] is carry[0] and s2.table.data_ptr() == s1.table.data_ptr()
    assert torch.equal(carry2[0].view(torch.int32), carry_w[0].view(torch.int32)) and torch.equal(carry2[1], carry_w[1])
    ws, wr, wl, mag = er.episode_stats(rew, done)
    _check((whole.table.cpu().numpy(), carry_w[0].cpu().numpy(), carry_w[1].cpu().numpy()), (ws, wr, wl), mag, W,
           T1 + T2)
    _check((s2.table.cpu().numpy(), carry2[0].cpu().numpy(), carry2[1].cpu().numpy()), (ws, wr, wl), mag, W, T1 + T2)
    with pytest.raises(ValueError, match="carry"):
        ro.episode_stats(tr(0, T1), carry=(carry[0][:, :3], carry[1][:, :3]))
    with pytest.raises(ValueError, match="out"):
        ro.episode_stats(tr(0, T1), out=torch.zeros((N, 5), dtype=torch.float64, device="cuda"))


def test_episode_spanning_three_calls():
    rew = np.full((1, 12, 1), 0.1, np.float32)
    done = np.zeros((1, 12, 1), np.uint8)
    done[0, 9, 0] = 1
    cr, cl = np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32)
    wr = wl = None
    for lo, hi in ((0, 4), (4, 8), (8, 12)):
        ws, wr, wl, mag = er.episode_stats(rew[:, lo:hi], done[:, lo:hi], wr, wl)
        st, cr, cl = _run(rew[:, lo:hi], done[:, lo:hi], cr, cl)
        _check((st, cr, cl), (ws, wr, wl), mag, 1, 4)
    assert st[0, 0] == 1 and st[0, 3] == 10 and cl[0, 0] == 2


def test_stats_are_added_to_and_runs_repeat():
    """``stats`` is added to, not overwritten: stats0 + (the zero-start result), one f64 addition per entry; and a
    second run gives the same bits."""
    N, W, T = 3, 257, 33
    rew, done, cr, cl = _inputs(11, N, T, W, "random")
    a = _run(rew, done, cr, cl)
    b = _run(rew, done, cr, cl)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    stats0 = np.random.default_rng(3).standard_normal((N, 6)) * 1e3
    c = _run(rew, done, cr, cl, stats0)
    assert np.array_equal(c[0], stats0 + a[0]) and not np.array_equal(c[0], a[0])
    assert c[1].tobytes() == a[1].tobytes() and c[2].tobytes() == a[2].tobytes()


@pytest.mark.parametrize("W", [64, 257])
def test_row_depends_on_its_agent_only(W):
    N, T = 3, 20
    rew, done, cr, cl = _inputs(13, N, T, W, "random")
    base = _run(rew, done, cr, cl)
    rew2, done2, cr2, cl2 = _inputs(14, N, T, W, "random")
    for a in range(N):
        r, d, c, l = rew2.copy(), done2.copy(), cr2.copy(), cl2.copy()
        r[a], d[a], c[a], l[a] = rew[a], done[a], cr[a], cl[a]
        got = _run(r, d, c, l)
        for x, y in zip(got, base):
            assert x[a].tobytes() == y[a].tobytes()
        alone = _run(rew[a:a + 1], done[a:a + 1], cr[a:a + 1], cl[a:a + 1])
        for x, y in zip(alone, base):
            assert x[0].tobytes() == y[a].tobytes()


def test_no_agents_and_bad_shapes():
    """N == 0 returns 0 before any pointer is looked at; bad shapes return -1 with a message."""
    from toued import _lib
    L = _lib.lib()
    st = _lib.stream_ptr()
    assert L.toued_episode_stats(0, 64, 20, None, None, None, None, None, st) == 0
    for (N, W, T), word in (((-1, 64, 20), "N=-1"), ((1, 0, 20), "W=0"), ((1, 64, 0), "T=0"),
                            ((1, 65536, 32768), "2^31")):
        assert L.toued_episode_stats(N, W, T, None, None, None, None, None, st) == -1
        msg = L.toued_last_error().decode()
        assert "toued_episode_stats" in msg and word in msg, msg
    assert L.toued_episode_stats(1, 64, 20, None, None, None, None, None, st) == -1
    assert "null" in L.toued_last_error().decode()
    with pytest.raises(_lib.ToUEDError, match="toued_episode_stats"):
        _lib.call("toued_episode_stats", 1, 0, 1, None, None, None, None, None, st)
