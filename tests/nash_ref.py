"""float64 numpy restatement of the reference's game solver, the reference of tests/test_nash_cpu.py and
tests/test_gpu_nash.py (never modified by a test):

  projection_simplex     util/projection.py:9-37, line by line in its sorted-cumsum form
  get_nash               environments/nash_sampler.py:39-58 (simultaneous projected-gradient steps, mean of the
                         num_iters + 1 iterates)
  value_exploitability   x^T M y and max_{j < ny} (x^T M)_j - min_{i < nx} (M y)_i of a strategy pair
  initial_strategies     compute_nash's random start (:196-198) on oracle/jaxrand.py
  training_level_ids     get_training_levels' draw (:210-211) on oracle/jaxrand.py
"""
import numpy as np

from oracle import jaxrand as jr


def projection_simplex(x, max_nz):
    """util/projection.py:9-37 in float64.  The reference's argsort(descending=True) is stable among ties; the result
    does not depend on the tie order (tied entries get the same value)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    ar = np.arange(n)
    idx = np.argsort(-np.where(ar < max_nz, x, -np.inf), kind="stable")
    max_nz_values = x[idx]
    cumsum = np.cumsum(max_nz_values)
    cumsum = np.where(ar < max_nz, cumsum, 0.0)
    ind = ar + 1
    with np.errstate(invalid="ignore"):
        cond = np.nan_to_num(1.0 / ind + (max_nz_values - cumsum / ind)) > 0
    cond = np.where(ar < max_nz, cond, False)
    k = int(np.count_nonzero(cond))
    to_relu = 1.0 / k + (max_nz_values - cumsum[k - 1] / k)
    to_relu = np.where(ar < max_nz, to_relu, 0.0)
    proj = np.maximum(to_relu, 0.0)
    out = np.zeros(n, np.float64)
    out[idx] = proj              # sum(proj[:, None] * one_hot(idx, n), axis=0)
    return out


def get_nash(M, x0, y0, x_nz, y_nz, num_iters=10000, lr=0.01):
    """nash_sampler.py:39-58 in float64: x_grad = M y, y_grad = -(x^T M), both from the old pair."""
    M = np.asarray(M, np.float64)
    x, y = np.asarray(x0, np.float64).copy(), np.asarray(y0, np.float64).copy()
    xs, ys = x.copy(), y.copy()
    for _ in range(num_iters):
        gx = M @ y
        gy = -(x @ M)
        x, y = projection_simplex(x - lr * gx, x_nz), projection_simplex(y - lr * gy, y_nz)
        xs += x
        ys += y
    return xs / (num_iters + 1), ys / (num_iters + 1)


def value_exploitability(M, x, y, x_nz, y_nz):
    """The inactive block of M (rows >= x_nz, columns >= y_nz) does not enter."""
    A = np.asarray(M, np.float64)[:x_nz, :y_nz]
    x, y = np.asarray(x, np.float64)[:x_nz], np.asarray(y, np.float64)[:y_nz]
    return float(x @ A @ y), float((x @ A).max() - (A @ y).min())


def initial_strategies(key, B, nz):
    """where(arange(B) < nz, uniform(key, (2, B)), 0), each row projected with nz (the f32 draws, f64 projection)."""
    u = jr.uniform(np.asarray(key, np.uint32), (2, B))
    u = np.where(np.arange(B)[None, :] < nz, u, np.float32(0.0))
    return u, projection_simplex(u[0], nz), projection_simplex(u[1], nz)


def training_level_ids(key, x, n):
    """jax.random.choice(key, arange(B), (n,), True, x) for an f32 x."""
    return jr.choice_p_replace(np.asarray(key, np.uint32), np.asarray(x, np.float32), (n,))


MATCHING_PENNIES = np.array([[1, -1], [-1, 1]], np.float64)
ROCK_PAPER_SCISSORS = np.array([[0, -1, 1], [1, 0, -1], [-1, 1, 0]], np.float64)
PURE_SADDLE = np.array([[3, 1, 4], [0, -1, 2], [5, 2, 6]], np.float64)


def one_hot(B, i=0):
    v = np.zeros(B, np.float64)
    v[i] = 1.0
    return v
