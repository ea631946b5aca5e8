"""numpy restatement of the value-loss PLR scores (toued_value_loss_scores), the target the GPU tests compare with.

Values in float32 by the critic's formula, one rounding per operation (what k_eval_loss computes):
    v = vcrit[a][idx] + ((float)time * 0.001f) * vcrit[a][D-1]
advantages by oracle.meta.gae_f32 (util/metrics.py:17-38 in float32, the reference's operation order: the bit-exact
target of toued_gae), and the two scores as the float64 means of max(adv, 0) and |adv| over those float32 terms.
Layouts are the trajectory's: idx / time [N, T+1, W], reward / done [N, T, W], vcrit [N, D].
"""
import numpy as np

from oracle import meta as ometa


def values(vcrit, idx, time):
    """float32 [N, T+1, W]."""
    f = np.float32
    vcrit = np.asarray(vcrit, f)
    n = vcrit.shape[0]
    gathered = vcrit[np.arange(n)[:, None, None], np.asarray(idx)]
    c = (np.asarray(time).astype(f) * f(0.001)).astype(f)
    return (gathered + (c * vcrit[:, -1][:, None, None]).astype(f)).astype(f)


def advantages(vcrit, idx, time, reward, done, gamma, gae_lambda):
    """float32 [N, T, W]: gae_f32 on the float32 values, in its per-worker layout [.., T]."""
    v = values(vcrit, idx, time)
    adv, _ = ometa.gae_f32(v.transpose(0, 2, 1), np.asarray(reward, np.float32).transpose(0, 2, 1),
                           np.asarray(done).transpose(0, 2, 1), gamma, gae_lambda)
    return np.ascontiguousarray(adv.transpose(0, 2, 1))


def scores_of(adv):
    """(positive value loss, L1 value loss) float64 [N] of float32 advantages [N, T, W]."""
    a = np.asarray(adv, np.float32).astype(np.float64)
    a = a.reshape(a.shape[0], -1)
    if a.shape[1] == 0:
        raise ValueError("scores_of: no (worker, step) pairs")
    return np.maximum(a, 0.0).mean(axis=1), np.abs(a).mean(axis=1)


def value_loss_scores(vcrit, idx, time, reward, done, gamma, gae_lambda):
    """(pvl float64 [N], l1 float64 [N], adv float32 [N, T, W])."""
    adv = advantages(vcrit, idx, time, reward, done, gamma, gae_lambda)
    pvl, l1 = scores_of(adv)
    return pvl, l1, adv
