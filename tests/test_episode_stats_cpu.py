"""tests/episode_stats_ref.py, the numpy restatement of toued_episode_stats, against a plain per-episode enumeration,
for the split invariance and on the edge done patterns (no GPU)."""
import math

import numpy as np
import pytest

import episode_stats_ref as er


def _inputs(seed, N, T, W, pattern="random"):
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((N, T, W)) * rng.choice([0.0, 0.01, 1.0, 30.0], (N, T, W))).astype(np.float32)
    return rew, er.done_pattern(pattern, N, T, W, rng), rng


def _carry(rng, N, W):
    return rng.standard_normal((N, W)).astype(np.float32), rng.integers(0, 50, (N, W)).astype(np.int32)


@pytest.mark.parametrize("pattern", er.PATTERNS)
@pytest.mark.parametrize("with_carry", [False, True])
def test_matches_plain_enumeration(pattern, with_carry):
    N, T, W = 3, 17, 5
    rew, done, rng = _inputs(1, N, T, W, pattern)
    cr, cl = _carry(rng, N, W) if with_carry else (None, None)
    stats, ret, ln, mag = er.episode_stats(rew, done, cr, cl)
    eps, ret_e, len_e = er.enumerate_episodes(rew, done, cr, cl)
    assert np.array_equal(ret.view(np.uint32), ret_e.view(np.uint32)) and np.array_equal(ln, len_e)
    for a in range(N):
        rets = [r for r, _ in eps[a]]
        # fsum is order-independent: the vectorised walk records in time order, the enumeration worker by worker
        want = (len(eps[a]), math.fsum(rets), math.fsum(r * r for r in rets), sum(n for _, n in eps[a]),
                math.fsum(float(x) for x in rew[a].ravel()), W * T)
        assert tuple(stats[a]) == tuple(float(x) for x in want)
    assert np.all(mag >= np.abs(stats))
    if pattern == "never":
        assert not stats[:, :4].any() and np.all(ln == (0 if cl is None else cl) + T)
    if pattern == "always":
        assert np.all(stats[:, 0] == W * T) and not ln.any() and not ret.any()
        first = 0 if cl is None else cl.sum(axis=1)
        assert np.all(stats[:, 3] == W * T + first)
    if pattern == "first":
        assert np.all(stats[:, 0] == W) and np.all(ln == T - 1)
    if pattern == "last":
        assert np.all(stats[:, 0] == W) and not ln.any() and not ret.any()


@pytest.mark.parametrize("T1,T2", [(1, 1), (1, 19), (20, 13), (7, 26)])
def test_split_invariance(T1, T2):
    """One call on T1 + T2 steps: the carry of a call on T1 steps followed by one on T2 steps bit for bit, the
    integer columns exactly, the f64 sums as the exact sums they are."""
    N, W = 2, 9
    rew, done, rng = _inputs(2, N, T1 + T2, W)
    cr, cl = _carry(rng, N, W)
    s, ret, ln, mag = er.episode_stats(rew, done, cr, cl)
    s1, r1, l1, _ = er.episode_stats(rew[:, :T1], done[:, :T1], cr, cl)
    s2, r2, l2, _ = er.episode_stats(rew[:, T1:], done[:, T1:], r1, l1)
    assert np.array_equal(ret.view(np.uint32), r2.view(np.uint32)) and np.array_equal(ln, l2)
    assert np.array_equal(s[:, [0, 3, 5]], (s1 + s2)[:, [0, 3, 5]])
    # three correctly rounded sums (two fsums and their f64 addition) against one: two roundings of the scale apart
    assert np.all(np.abs(s1 + s2 - s) <= 2.0 * 2.0 ** -52 * mag)


def test_episode_spanning_three_calls():
    """A single episode that starts in the first call, runs through the second and ends in the third is recorded
    once, in the third, with its whole return and length."""
    rew = np.full((1, 12, 1), 0.1, np.float32)
    done = np.zeros((1, 12, 1), np.uint8)
    done[0, 9, 0] = 1
    cr = cl = None
    rows = []
    for lo, hi in ((0, 4), (4, 8), (8, 12)):
        s, cr, cl, _ = er.episode_stats(rew[:, lo:hi], done[:, lo:hi], cr, cl)
        rows.append(s[0])
    assert rows[0][0] == 0 and rows[1][0] == 0 and rows[2][0] == 1
    acc = np.float32(0.0)
    for _ in range(10):
        acc = np.float32(acc + np.float32(0.1))
    assert rows[2][1] == float(acc) and rows[2][2] == float(acc) * float(acc) and rows[2][3] == 10
    assert cl[0, 0] == 2 and cr[0, 0] == np.float32(np.float32(0.1) + np.float32(0.1))
    assert [r[5] for r in rows] == [4, 4, 4]


def test_f32_running_sum_is_the_contract():
    """The return is the f32 sum in time order, not the f64 sum rounded: 2^24 + 1 + 1 stays 2^24 in f32."""
    rew = np.array([2.0 ** 24, 1.0, 1.0], np.float32).reshape(1, 3, 1)
    done = np.array([0, 0, 1], np.uint8).reshape(1, 3, 1)
    s, _, _, _ = er.episode_stats(rew, done)
    assert s[0, 1] == 2.0 ** 24 and s[0, 4] == 2.0 ** 24 + 2
