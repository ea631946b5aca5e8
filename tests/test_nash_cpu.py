"""The double-oracle Nash solver, CPU side: pins of the float64 restatement (tests/nash_ref.py) that the GPU kernels
are compared against -- the projection's KKT conditions, three games with known equilibria -- and the host surface
(header, ctypes table, command line).  No GPU calls."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import nash_ref as nr

ROOT = Path(__file__).resolve().parents[1]


def _rows(seed, n):
    """(x, nz): random rows of length 1..40 at scales 1e-3, 1, 1e3, every third one rounded to quarters (ties), with
    large numbers at index >= nz."""
    rng = np.random.default_rng(seed)
    for t in range(n):
        B = int(rng.integers(1, 41))
        nz = int(rng.integers(1, B + 1))
        x = rng.standard_normal(B) * (1e-3, 1.0, 1e3)[t % 3]
        if t % 3 == 1:
            x = np.round(x * 4) / 4
        x[nz:] = 1e30
        yield x, nz


def test_projection_satisfies_kkt():
    """out is the Euclidean projection of x[:nz] onto the simplex iff it is feasible (>= 0, sum 1, zero from nz on) and
    x_i - out_i is one constant tau on the support and <= tau off it.  float64: 1e-12 relative to the row's scale."""
    ties = 0
    for x, nz in _rows(11, 300):
        out = nr.projection_simplex(x, nz)
        tol = 1e-12 * max(1.0, np.abs(x[:nz]).max())
        assert (out >= 0).all() and not out[nz:].any()
        assert abs(out.sum() - 1.0) <= tol
        a, o = x[:nz], out[:nz]
        sup = o > 0
        tau = (a - o)[sup]
        assert np.ptp(tau) <= tol
        assert ((a - o)[~sup] <= tau.max() + tol).all() if (~sup).any() else True
        ties += int(np.unique(a[sup]).size < sup.sum())
    assert ties > 0          # tied entries inside a support did occur


def test_projection_special_rows():
    on = np.array([0.25, 0.0, 0.5, 0.25, 7.0])
    assert np.allclose(nr.projection_simplex(on, 4), [0.25, 0.0, 0.5, 0.25, 0.0], atol=1e-15)
    assert np.allclose(nr.projection_simplex(np.full(8, -3.0), 5), [0.2] * 5 + [0.0] * 3, atol=1e-15)
    assert np.array_equal(nr.projection_simplex(np.array([100.0, 1.0, 2.0]), 3), [1.0, 0.0, 0.0])
    assert np.array_equal(nr.projection_simplex(np.array([-5.0, 9.0]), 1), [1.0, 0.0])


def test_restatement_solves_the_known_games():
    """10 000 iterations from the one-hot starts (train_do.py:17-18), lr 0.01: matching pennies and
    rock-paper-scissors reach their uniform equilibria within 0.01, the pure-saddle game its saddle (row 1, column 2,
    value 2)."""
    x, y = nr.get_nash(nr.MATCHING_PENNIES, nr.one_hot(2), nr.one_hot(2), 2, 2)
    assert np.abs(x - 0.5).max() < 0.01 and np.abs(y - 0.5).max() < 0.01
    x, y = nr.get_nash(nr.ROCK_PAPER_SCISSORS, nr.one_hot(3), nr.one_hot(3), 3, 3)
    assert np.abs(x - 1 / 3).max() < 0.01 and np.abs(y - 1 / 3).max() < 0.01
    x, y = nr.get_nash(nr.PURE_SADDLE, nr.one_hot(3), nr.one_hot(3), 3, 3)
    value, expl = nr.value_exploitability(nr.PURE_SADDLE, x, y, 3, 3)
    assert x[1] > 0.99 and y[2] > 0.99 and abs(value - 2.0) < 0.05 and expl >= 0


def test_restatement_start_and_inactive_block():
    """iters == 0 returns the start; the inactive block of the payoff meets zeros of x and y."""
    rng = np.random.default_rng(5)
    M = rng.standard_normal((6, 6))
    x0, y0 = nr.projection_simplex(rng.random(6), 4), nr.projection_simplex(rng.random(6), 2)
    x, y = nr.get_nash(M, x0, y0, 4, 2, 0)
    assert np.array_equal(x, x0) and np.array_equal(y, y0)
    M2 = M.copy()
    M2[4:, :] = 1e6
    M2[:, 2:] = -1e6
    a, b = nr.get_nash(M, x0, y0, 4, 2, 50), nr.get_nash(M2, x0, y0, 4, 2, 50)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not a[0][4:].any() and not a[1][2:].any()


def test_restatement_draws():
    key = np.array([0, 7], np.uint32)
    u, x0, y0 = nr.initial_strategies(key, 9, 4)
    assert u.shape == (2, 9) and u.dtype == np.float32 and not u[:, 4:].any() and (u[:, :4] > 0).all()
    for s in (x0, y0):
        assert abs(s.sum() - 1.0) < 1e-12 and not s[4:].any()
    assert not nr.training_level_ids(key, nr.one_hot(9).astype(np.float32), 32).any()
    ids = nr.training_level_ids(key, x0.astype(np.float32), 64)
    assert ids.dtype == np.int32 and ids.shape == (64,) and (ids < 4).all() and len(set(ids.tolist())) > 1


def test_header_declares_the_entries():
    text = (ROOT / "include" / "toued.h").read_text()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int toued_project_simplex(const float* x, const int* nz, int R, int B, float* out, hipStream_t stream);"
            in flat)
    assert "int toued_nash_fits(int B);" in flat
    assert ("int toued_nash_solve(const float* payoff, const int* nx, const int* ny, const float* x0, const float* y0, "
            "int G, int B, int iters, float lr, float* x_avg, float* y_avg, float* stats, hipStream_t stream);"
            in flat)
    from toued import _lib
    for name in ("toued_project_simplex", "toued_nash_fits", "toued_nash_solve"):
        assert name in _lib.exported_symbols()


def test_public_names():
    import toued
    from toued import nash
    for name in ("project_simplex", "solve_nash", "initial_strategies", "training_level_ids", "cross_regret",
                 "NashSolution"):
        assert getattr(toued, name) is getattr(nash, name)
    assert nash.NashSolution._fields == ("x", "y", "value", "exploitability")


def test_cross_regret_refuses_non_tabular_modes():
    from types import SimpleNamespace
    from toued.nash import cross_regret
    ro = SimpleNamespace(spec=SimpleNamespace(tabular=False))
    with pytest.raises(NotImplementedError, match="not implemented for non-tabular environments"):
        cross_regret(ro, None, None, 10)


def test_command_line_help_runs_without_a_gpu():
    pkg = str(ROOT / "to-ued_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "toued.nash", "--help"], capture_output=True, text=True, cwd=pkg,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--payoff" in r.stdout and "--iters" in r.stdout
