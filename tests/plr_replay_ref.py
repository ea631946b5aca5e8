"""numpy restatement of toued_plr_sample_prio's replay distribution (include/toued.h) -- test oracle.

Prioritized Level Replay's replay distribution (Jiang et al. 2021, section 3): a score part P_S (the reference's
softmax for ``rank`` / ``proportional``, rank^(-1/T) over the descending-score ranks for ``rank_sampled``) mixed with a
staleness part P_C by rho, then floored on the valid slots where the weights can underflow.  Every value is float32
and every operation one correctly rounded step, in the kernel's order; the float sum is oracle.sampler.seq_sum and the
Gumbel top-k is jaxrand.choice_p_noreplace on the second key of split(replay_key), as oracle.sampler.replay_ids draws.
"""
from __future__ import annotations

import numpy as np

from oracle import jaxrand as jr
from oracle import pmath
from oracle import sampler as osp

F32 = np.float32
TINY = F32(1.17549435e-38)
TRANSFORMS = ("rank", "proportional", "rank_sampled")


def ranks(score, valid):
    """rank_i = 1 + the position of slot i in the stable argsort of where(valid, -score, +inf) (-0 == +0, NaN last,
    ties to the lower index: numpy's float order is jax's)."""
    key = np.where(valid, -score.astype(F32), F32(np.inf)).astype(F32)
    order = np.argsort(key, kind="stable")
    r = np.empty(score.shape[0], np.int64)
    r[order] = np.arange(1, score.shape[0] + 1)
    return r


def staleness_part(valid, stamp, now):
    """pc [B] f32: a = valid ? max(now - stamp, 0) : 0 in integers, a / sum(a), or uniform over the valid slots when
    the sum is 0."""
    a = np.where(valid, np.maximum(np.int64(now) - stamp.astype(np.int64), 0), 0).astype(np.int64)
    A = int(a.sum())
    if A > 0:
        return (a.astype(F32) / F32(A)).astype(F32)
    n_valid = int(valid.sum())
    with np.errstate(divide="ignore"):
        return np.where(valid, F32(1.0) / F32(n_valid), F32(0.0)).astype(F32)


def replay_p(score, active, new, N, transform="rank", temperature=1.0, staleness_coeff=0.0, stamp=None, now=0,
             floor=True):
    """The replay distribution p [B] f32.  ``floor=False`` leaves the floor out (to show what it is for)."""
    assert transform in TRANSFORMS, transform
    score = np.asarray(score, F32)
    valid = ~(np.asarray(new, bool) | np.asarray(active, bool))
    B = score.shape[0]
    if int(valid.sum()) < N:
        return np.ones(B, F32)
    T = F32(temperature)
    rho = F32(staleness_coeff)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        if transform == "rank_sampled":
            w = pmath.exp(((-pmath.log(ranks(score, valid).astype(F32))) / T).astype(F32))
        else:
            w = pmath.exp((score / T).astype(F32))
        w = np.where(valid, w, F32(0.0)).astype(F32)
        p = (w / osp.seq_sum(w)).astype(F32)
        if rho > 0:
            pc = staleness_part(valid, np.asarray(stamp), now)
            p = (((F32(1.0) - rho) * p).astype(F32) + (rho * pc).astype(F32)).astype(F32)
        if floor and (transform == "rank_sampled" or rho > 0):
            p = np.where(valid, np.where(p < TINY, TINY, p), F32(0.0)).astype(F32)
    return p


def replay_ids(key, p, N, transform):
    """The N replay ids drawn from p: flip(argsort(p))[:N] for ``rank``, else the Gumbel top-k."""
    if transform == "rank":
        return osp.argsort_stable(p)[::-1][:N].astype(np.int32)
    with np.errstate(divide="ignore"):
        return jr.choice_p_noreplace(jr.split(key, 2)[1], p, N)


def sample(keys3, score, active, new, N, transform="rank", temperature=1.0, staleness_coeff=0.0, stamp=None, now=0,
           p_replay=0.5, floor=True):
    """One toued_plr_sample_prio call: keys3 = (replay_rng, random_rng, select_rng).  Returns a dict of ``p`` [B] and
    ``chosen``, ``rep``, ``rnd``, ``use`` [N]."""
    p = replay_p(score, active, new, N, transform, temperature, staleness_coeff, stamp, now, floor)
    rep = replay_ids(keys3[0], p, N, transform)
    with np.errstate(divide="ignore", invalid="ignore"):
        rnd = osp.random_ids(keys3[1], active, new, N)
    chosen, use = osp.select(keys3[2], rep, rnd, active, new, N, p_replay)
    return {"p": p, "chosen": chosen, "rep": rep, "rnd": rnd, "use": use.astype(np.int32)}
