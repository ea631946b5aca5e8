"""GPU: toued_project_simplex / toued_nash_solve and toued.nash against the float64 restatement tests/nash_ref.py.

Projection: |out - ref| <= 2^-21 * max(1, max|x[:nz]|) (four f32 ulps of the input's scale), exactly 0 from nz on,
nothing below 0.

Solver: |xbar - ref|, |ybar - ref| <= 1e-6 pointwise.  That is a comparison of two trajectories, so it is made where
the float64 restatement is itself determined to 1e-6: the iteration is a discrete dynamical system whose sensitivity
to a rounding error grows with the step lr * |M| and the number of steps.  Re-running the float64 restatement with
its sums in another order (an error of 1e-16 per step) moved the averages by < 1e-14 at lr = 0.01 and 1000
iterations for every size here (and by 2.4e-17 at B = 128), but by 4.5e-9 at B = 64, 4e-4 at B = 127 and 5e-3 at
B = 128 with lr = 0.1 and 1000 iterations on N(0, 1) payoffs, and by 1.5e-3 at B = 128 with payoffs of scale 10 at
lr = 0.01: there an f32 iterate, 1e9 times coarser, is not comparable pointwise with any reference.  So lr = 0.1
runs 1000 iterations for B <= 8 only (up to 10 iterations for every B), and the scale-10 game runs at lr = 0.01 for
at most 10 iterations past B = 8.  Every B, every iteration count and both step sizes of the grid are run.

A game that starts from initial_strategies (both rows projected with the train count nx, as the reference does) can
carry mass of y0 at columns >= ny; the kernel reads the payoff's inactive block as zeros, the reference's own fill
for inactive levels, so these games hold zeros there.  The games from one-hot starts hold N(0, 1) numbers there.
"""
import functools

import numpy as np
import pytest
import torch

import nash_ref as nr
from oracle import jaxrand as jr

pytestmark = pytest.mark.gpu

F32_TOL = 2.0 ** -21
SOLVE_TOL = 1e-6


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()      # a copy: the cases stay read-only


def _abi():
    from toued import _lib
    return _lib, _lib.lib(), (lambda: _lib.lib().toued_last_error().decode())


# ------------------------------------------------------------------------------------------------ projection
PROJ_B = [1, 2, 3, 63, 64, 65, 128, 129, 4000, 8192]
KINDS = ["normal", "small", "large", "simplex", "equal", "quarters", "negative", "dominant"]


def _nz_list(B):
    return [max(1, min(B, n)) for n in (1, 2, B - 1, B, B)]


def _row(kind, B, nz, rng):
    if kind == "normal":
        x = rng.standard_normal(B)
    elif kind == "small":
        x = rng.standard_normal(B) * 1e-3
    elif kind == "large":
        x = rng.standard_normal(B) * 1e3
    elif kind == "simplex":            # already on the simplex of its first nz entries, a third of them zeros
        x = rng.random(B) * (rng.random(B) > 1 / 3)
        x[0] += 0.5
        x[:nz] /= x[:nz].sum()
    elif kind == "equal":
        x = np.full(B, rng.standard_normal())
    elif kind == "quarters":
        x = np.round(rng.standard_normal(B) * 4) / 4
    elif kind == "negative":
        x = -1.0 - np.abs(rng.standard_normal(B)) * 5
    elif kind == "dominant":
        x = rng.standard_normal(B) * 0.1
        x[int(rng.integers(0, nz))] = 50.0
    x = x.astype(np.float32)
    x[nz:] = np.float32(3e38) * np.where(rng.random(B - nz) < 0.5, -1, 1)   # large finite numbers, never read
    return x


@functools.lru_cache(maxsize=None)
def _proj_case(B):
    """Rows of every kind with nz = 1, 2, B - 1, B, B mixed per row, and their float64 projections: computed once."""
    rng = np.random.default_rng(9000 + B)
    rows, nzs = [], []
    for kind in KINDS:
        for nz in _nz_list(B):
            rows.append(_row(kind, B, nz, rng))
            nzs.append(nz)
    x, nz = np.stack(rows), np.array(nzs, np.int32)
    ref = np.stack([nr.projection_simplex(r, n) for r, n in zip(x, nz)])
    for a in (x, nz, ref):
        a.setflags(write=False)
    return x, nz, ref


def _check_projection(out, x, nz, ref):
    assert out.dtype == np.float32 and out.shape == x.shape
    worst = 0.0
    for r in range(x.shape[0]):
        n = int(nz[r])
        assert not out[r, n:].any(), r                       # exactly 0.0
        assert (out[r] >= 0).all(), r
        tol = F32_TOL * max(1.0, float(np.abs(x[r, :n]).max()))
        err = float(np.abs(out[r].astype(np.float64) - ref[r]).max())
        worst = max(worst, err / tol)
        assert err <= tol, (r, n, err, tol)
    return worst


@pytest.mark.parametrize("B", PROJ_B)
def test_projection_matches_float64(B):
    from toued.nash import project_simplex
    x, nz, ref = _proj_case(B)
    worst = 0.0
    for k in range(len(KINDS)):                              # R = 5: one kind, the five counts
        sl = slice(5 * k, 5 * k + 5)
        out = project_simplex(_dev(x[sl]), _dev(nz[sl], np.int32)).cpu().numpy()
        worst = max(worst, _check_projection(out, x[sl], nz[sl], ref[sl]))
    for r in (3, 13, 38):                                    # R = 1, and the one-row form with an int count
        out = project_simplex(_dev(x[r:r + 1]), _dev(nz[r:r + 1], np.int32)).cpu().numpy()
        _check_projection(out, x[r:r + 1], nz[r:r + 1], ref[r:r + 1])
        one = project_simplex(_dev(x[r]), int(nz[r]))
        assert one.shape == (B,) and np.array_equal(one.cpu().numpy(), out[0])
    print(f"B={B}: worst |out - f64| = {worst:.3f} of the tolerance")


def test_projection_of_a_point_on_the_simplex_is_the_point():
    from toued.nash import project_simplex
    for B in (3, 129, 4000):
        x, nz, _ = _proj_case(B)
        k = KINDS.index("simplex")
        sl = slice(5 * k, 5 * k + 5)
        out = project_simplex(_dev(x[sl]), _dev(nz[sl], np.int32)).cpu().numpy()
        for r in range(5):
            n = int(nz[sl][r])
            assert np.abs(out[r, :n] - x[sl][r, :n]).max() <= F32_TOL


def test_projection_is_deterministic_in_place_and_clamps_counts():
    from toued import _lib
    from toued.nash import project_simplex
    x, nz, ref = _proj_case(4000)
    dx, dn = _dev(x), _dev(nz, np.int32)
    a, b = project_simplex(dx, dn), project_simplex(dx, dn)
    assert torch.equal(a, b)
    buf = dx.clone()
    _lib.call("toued_project_simplex", _lib.ptr(buf), _lib.ptr(dn), x.shape[0], 4000, _lib.ptr(buf), _lib.stream_ptr())
    assert torch.equal(buf, a)
    # counts outside [1, B] are clamped on the device
    y = np.random.default_rng(3).standard_normal((2, 65)).astype(np.float32)
    got = project_simplex(_dev(y), _dev(np.array([0, 1000], np.int32), np.int32))
    want = project_simplex(_dev(y), _dev(np.array([1, 65], np.int32), np.int32))
    assert torch.equal(got, want)
    assert project_simplex(torch.zeros((0, 7), device="cuda"), 3).shape == (0, 7)


# ---------------------------------------------------------------------------------------------------- solver
SOLVE_B = [1, 2, 3, 8, 64, 65, 127, 128]
G = 3


def _counts(B):
    """(nx, ny) of the three games: nx != ny where B allows, 1 and B among them."""
    if B == 1:
        return [(1, 1)] * 3
    if B == 2:
        return [(2, 1), (1, 2), (2, 2)]
    return [(B, 1), (B // 2, B), (B - 1, B // 3 + 1)]


@functools.lru_cache(maxsize=None)
def _games(B, scale):
    """G games of N(0, scale^2) payoffs (f32), their counts and starts: game 0 from the one-hot start with N(0, 1)
    numbers in its inactive block, games 1 and 2 from initial_strategies(key, B, nx) with zeros there."""
    rng = np.random.default_rng(7000 + 10 * B + int(scale))
    M = (rng.standard_normal((G, B, B)) * scale).astype(np.float32)
    cnt = _counts(B)
    x0, y0 = np.zeros((G, B)), np.zeros((G, B))
    x0[0, 0] = y0[0, 0] = 1.0
    for g in (1, 2):
        nx, ny = cnt[g]
        M[g, nx:, :] = 0.0
        M[g, :, ny:] = 0.0
        _, x0[g], y0[g] = nr.initial_strategies(np.array([B, g], np.uint32), B, nx)
    x0, y0 = x0.astype(np.float32), y0.astype(np.float32)
    for a in (M, x0, y0):
        a.setflags(write=False)
    return M, cnt, x0, y0


@functools.lru_cache(maxsize=None)
def _solve_ref(B, scale, iters, lr):
    M, cnt, x0, y0 = _games(B, scale)
    lr = float(np.float32(lr))           # the step size the ABI carries (float lr), the same number on both sides
    return [nr.get_nash(M[g], x0[g], y0[g], cnt[g][0], cnt[g][1], iters, lr) for g in range(G)]


def _grid(B):
    """(scale, iters, lr): see the module docstring for the cases that are well-posed."""
    out = [(1, it, lr) for it in (0, 1, 2, 10) for lr in (0.01, 0.1)] + [(1, 1000, 0.01)]
    if B <= 8:
        out += [(1, 1000, 0.1), (10, 1000, 0.01)]
    else:
        out += [(10, 10, 0.01)]
    return out


def _solve(M, cnt, x0, y0, iters, lr):
    from toued.nash import solve_nash
    nx = _dev(np.array([c[0] for c in cnt], np.int32), np.int32)
    ny = _dev(np.array([c[1] for c in cnt], np.int32), np.int32)
    return solve_nash(_dev(M), nx, ny, _dev(x0), _dev(y0), iters, lr)


def _check_stats(s, M, cnt):
    """value and exploitability against the restatement's, from the kernel's own averages."""
    x, y = s.x.cpu().numpy(), s.y.cpu().numpy()
    val, expl = s.value.cpu().numpy(), s.exploitability.cpu().numpy()
    for g, (nx, ny) in enumerate(cnt):
        v, e = nr.value_exploitability(M[g], x[g], y[g], nx, ny)
        tol = 1e-5 * max(1.0, float(np.abs(M[g][:nx, :ny]).max()))
        assert abs(val[g] - v) <= tol and abs(expl[g] - e) <= tol, (g, val[g], v, expl[g], e, tol)


@pytest.mark.parametrize("B", SOLVE_B)
def test_solver_matches_float64_pointwise(B):
    worst = 0.0
    for scale, iters, lr in _grid(B):
        M, cnt, x0, y0 = _games(B, scale)
        ref = _solve_ref(B, scale, iters, lr)
        s = _solve(M, cnt, x0, y0, iters, lr)
        assert s.x.shape == (G, B) and s.value.shape == (G,) and s.x.dtype == torch.float32
        x, y = s.x.cpu().numpy(), s.y.cpu().numpy()
        if iters == 0:
            assert np.array_equal(x, x0) and np.array_equal(y, y0)          # bit for bit
        for g in range(G):
            err = max(np.abs(x[g] - ref[g][0]).max(), np.abs(y[g] - ref[g][1]).max())
            print(f"B={B} scale={scale} iters={iters} lr={lr} game {g} {cnt[g]}: max|gpu - f64| = {err:.3e}")
            worst = max(worst, err)
            assert err <= SOLVE_TOL, (scale, iters, lr, g, err)
        _check_stats(s, M, cnt)
    print(f"B={B}: worst deviation {worst:.3e}")


def test_full_length_solve():
    """B = 128, every slot active, 10 000 iterations at lr 0.01 from the one-hot starts."""
    rng = np.random.default_rng(128)
    M = rng.standard_normal((2, 128, 128)).astype(np.float32)
    cnt = [(128, 128)] * 2
    x0 = np.zeros((2, 128), np.float32)
    x0[:, 0] = 1.0
    s = _solve(M, cnt, x0, x0, 10000, 0.01)
    x, y, expl = s.x.cpu().numpy(), s.y.cpu().numpy(), s.exploitability.cpu().numpy()
    for g in range(2):
        rx, ry = nr.get_nash(M[g], x0[g], x0[g], 128, 128, 10000, float(np.float32(0.01)))
        err = max(np.abs(x[g] - rx).max(), np.abs(y[g] - ry).max())
        ref_expl = nr.value_exploitability(M[g], rx, ry, 128, 128)[1]
        print(f"game {g}: max|gpu - f64| = {err:.3e}, exploitability gpu {expl[g]:.4e} f64 {ref_expl:.4e}")
        assert err <= SOLVE_TOL, (g, err)
        assert expl[g] <= ref_expl + 1e-5, (g, expl[g], ref_expl)
    _check_stats(s, M, cnt)


def test_known_games():
    from toued.nash import solve_nash
    s = solve_nash(_dev(nr.MATCHING_PENNIES), 2, 2)
    assert s.x.shape == (2,) and s.value.dim() == 0
    assert (s.x - 0.5).abs().max() < 0.01 and (s.y - 0.5).abs().max() < 0.01
    s = solve_nash(_dev(nr.ROCK_PAPER_SCISSORS), 3, 3)
    assert (s.x - 1 / 3).abs().max() < 0.01 and (s.y - 1 / 3).abs().max() < 0.01
    s = solve_nash(_dev(nr.PURE_SADDLE), 3, 3)
    assert s.x[1] > 0.99 and s.y[2] > 0.99 and abs(float(s.value) - 2.0) < 0.05
    assert float(s.exploitability) >= -1e-6


def test_inactive_block_does_not_enter():
    rng = np.random.default_rng(41)
    B, cnt = 65, [(40, 65), (65, 17), (33, 21)]
    M = rng.standard_normal((G, B, B)).astype(np.float32)
    x0 = np.zeros((G, B), np.float32)
    x0[:, 0] = 1.0
    Z, H = M.copy(), M.copy()
    for g, (nx, ny) in enumerate(cnt):
        Z[g, nx:, :] = 0.0
        Z[g, :, ny:] = 0.0
        sign = np.where(rng.random((B, B)) < 0.5, -1e6, 1e6).astype(np.float32)
        H[g, nx:, :] = sign[nx:, :]
        H[g, :, ny:] = sign[:, ny:]
    a, b = _solve(Z, cnt, x0, x0, 200, 0.01), _solve(H, cnt, x0, x0, 200, 0.01)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for g, (nx, ny) in enumerate(cnt):
        assert not a.x[g, nx:].any() and not a.y[g, ny:].any()


def test_deterministic_and_independent_of_the_batch():
    rng = np.random.default_rng(43)
    B, n = 32, 64
    M = rng.standard_normal((n, B, B)).astype(np.float32)
    cnt = [(1 + (7 * g) % B, 1 + (11 * g) % B) for g in range(n)]
    x0 = np.zeros((n, B), np.float32)
    x0[:, 0] = 1.0
    a, b = _solve(M, cnt, x0, x0, 300, 0.01), _solve(M, cnt, x0, x0, 300, 0.01)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    one = _solve(M[5:6], cnt[5:6], x0[5:6], x0[5:6], 300, 0.01)
    assert torch.equal(one.x[0], a.x[5]) and torch.equal(one.exploitability[0], a.exploitability[5])
    M3, cnt3, s0, t0 = _games(128, 1)
    a, b = _solve(M3, cnt3, s0, t0, 100, 0.01), _solve(M3, cnt3, s0, t0, 100, 0.01)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_argument_checks():
    _lib, L, err = _abi()
    st = _lib.stream_ptr()
    f = torch.zeros(16, device="cuda")
    i = torch.ones(4, dtype=torch.int32, device="cuda")
    pf, pi = _lib.ptr(f), _lib.ptr(i)
    # toued_project_simplex
    P = L.toued_project_simplex
    assert P(pf, pi, 1, 4, pf, st) == 0
    assert P(pf, pi, -1, 4, pf, st) == -1 and "R=-1" in err()
    assert P(pf, pi, 1, 0, pf, st) == -1 and "B=0" in err()
    assert P(pf, pi, 1, 8193, pf, st) == -1 and "B=8193" in err()
    for args in ((None, pi, 1, 4, pf), (pf, None, 1, 4, pf), (pf, pi, 1, 4, None)):
        assert P(*args, st) == -1 and "null" in err()
    assert P(None, None, 0, 4, None, st) == 0
    # toued_nash_fits
    assert [L.toued_nash_fits(b) for b in (-1, 0, 1, 128, 129)] == [0, 0, 1, 1, 0]
    # toued_nash_solve
    S = L.toued_nash_solve
    o1, o2, o3 = (torch.zeros(4, device="cuda") for _ in range(3))
    ok = [pf, pi, pi, pf, pf, 1, 2, 3, 0.01, _lib.ptr(o1), _lib.ptr(o2), _lib.ptr(o3)]
    assert S(*ok, st) == 0

    def bad(k, v):
        a = list(ok)
        a[k] = v
        return S(*a, st)

    assert bad(6, 0) == -1 and "B=0" in err()
    assert bad(6, 129) == -1 and "B=129" in err()
    assert bad(5, -1) == -1 and "G=-1" in err()
    assert bad(7, -1) == -1 and "iters=-1" in err()
    assert bad(7, 1000001) == -1 and "iters=1000001" in err()
    for lr in (float("nan"), float("inf"), float("-inf")):
        assert bad(8, lr) == -1 and "lr" in err()
    for k in (0, 1, 2, 3, 4, 9, 10, 11):
        assert bad(k, None) == -1 and "null" in err(), k
    assert S(None, None, None, None, None, 0, 2, 3, 0.01, None, None, None, st) == 0
    with pytest.raises(_lib.ToUEDError, match="B=129"):
        from toued.nash import solve_nash
        solve_nash(torch.zeros((129, 129), device="cuda"), 1, 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- Python layer
def test_initial_strategies_and_training_level_ids():
    from toued import prng
    from toued.nash import initial_strategies, solve_nash, training_level_ids
    B, nz = 50, 37
    key = np.array([3, 2024], np.uint32)
    x0, y0 = initial_strategies(prng.from_uint32_numpy(key, "cuda"), B, nz)
    u, rx, ry = nr.initial_strategies(key, B, nz)
    for got, ref, row in ((x0, rx, u[0]), (y0, ry, u[1])):
        got = got.cpu().numpy()
        assert got.shape == (B,) and not got[nz:].any()
        # the draws are jax's, bit for bit: the support is the reference's and the projection is within its tolerance
        assert np.abs(got - ref).max() <= F32_TOL
        assert np.array_equal(got > 0, ref.astype(np.float32) > 0)
    t0 = initial_strategies(prng.from_uint32_numpy(key, "cuda"), B, torch.tensor(nz, device="cuda"))
    assert torch.equal(t0[0], x0) and torch.equal(t0[1], y0)
    # the draw: same key, same ids
    k2 = np.array([5, 77], np.uint32)
    dk2 = prng.from_uint32_numpy(k2, "cuda")
    ids = training_level_ids(dk2, x0, 200)
    assert ids.dtype == torch.int32 and ids.shape == (200,)
    assert np.array_equal(ids.cpu().numpy(), nr.training_level_ids(k2, x0.cpu().numpy(), 200))
    # train_do.py:17-18's initial nash: every id is 0
    hot = torch.zeros(B, device="cuda")
    hot[0] = 1.0
    assert not training_level_ids(dk2, hot, 64).any()
    # a solved x: every id lies in its support
    M = torch.from_numpy(np.random.default_rng(8).standard_normal((B, B)).astype(np.float32)).cuda()
    s = solve_nash(M, nz, B, x0, y0, iters=2000)
    ids = training_level_ids(dk2, s.x, 512).long()
    assert np.array_equal(ids.cpu().numpy(), nr.training_level_ids(k2, s.x.cpu().numpy(), 512))
    assert (s.x[ids] > 0).all() and (ids < nz).all()


def test_solve_nash_shapes_and_defaults():
    from toued.nash import solve_nash
    M = torch.from_numpy(np.random.default_rng(9).standard_normal((4, 8, 8)).astype(np.float32)).cuda()
    many = solve_nash(M, 8, 5, iters=100)
    assert many.x.shape == (4, 8) and many.y.shape == (4, 8) and many.value.shape == (4,)
    assert many.exploitability.shape == (4,)
    one = solve_nash(M[2], 8, 5, iters=100)
    assert one.x.shape == (8,) and one.value.dim() == 0
    for a, b in zip(one, many):
        assert torch.equal(a, b[2])
    hot = torch.zeros((4, 8), device="cuda")
    hot[:, 0] = 1.0
    for a, b in zip(many, solve_nash(M, torch.full((4,), 8), torch.full((4,), 5), hot, hot.clone(), iters=100)):
        assert torch.equal(a, b)
    none = solve_nash(M[:0], 8, 5)
    assert none.x.shape == (0, 8) and none.value.shape == (0,)
    with pytest.raises(ValueError):
        solve_nash(M[0, :, :5].contiguous(), 5, 5)
    with pytest.raises(ValueError):
        solve_nash(M, 8, 8, x0=hot[0])


def test_command_line_solves_a_saved_matrix(tmp_path, capsys):
    from toued import nash
    np.save(tmp_path / "M.npy", nr.PURE_SADDLE)
    assert nash.main(["--payoff", str(tmp_path / "M.npy"), "--out", str(tmp_path / "sol.npz")]) == 0
    assert "value" in capsys.readouterr().out
    sol = np.load(tmp_path / "sol.npz")
    assert sol["x"][1] > 0.99 and sol["y"][2] > 0.99 and abs(float(sol["value"]) - 2.0) < 0.05


# ---------------------------------------------------------------------------------------------- cross_regret
def test_cross_regret_of_tabular_agents():
    """Three agents x four levels of `debug`, the smallest tabular mode, against tests/optret_ref.py and
    tests/polret_ref.py: each entry within the sum of the two kernels' bounds, H * 2^-23 * max(1, max|v64|) each
    (test_gpu_optret.py, test_gpu_polret.py)."""
    import optret_ref as orf
    import polret_ref as prf
    from oracle import levels as olv
    from toued import prng
    from toued.level_sampler import LevelSampler
    from toued.nash import cross_regret, solve_nash
    from toued.parse_args import parse_args
    from toued.plr import optimal_regret
    mode, n_agents, n_levels = "debug", 3, 4
    spec = olv.env_spec(mode)
    keys = jr.split(jr.PRNGKey(501), n_levels)
    params, lifetime = olv.reset_env_params(keys, mode)
    levels = torch.from_numpy(olv.pack_levels(params, lifetime, spec)).cuda()
    theta_np = prf.random_tables(502, n_agents, spec.obs_dim)
    theta = torch.from_numpy(theta_np).cuda()
    args = parse_args(["--env_mode", mode, "--score_function", "optimal_regret", "--regret_eval", "exact",
                       "--num_agents", str(n_agents), "--num_mini_batches", "1", "--env_workers", "64",
                       "--buffer_size", "16"])
    smp = LevelSampler(args)
    ro = smp.rollout_manager
    L = ro.eval_rollout_len
    got = cross_regret(ro, levels, theta, L)
    assert got.shape == (n_agents, n_levels) and got.dtype == torch.float32
    g64 = got.cpu().numpy().astype(np.float64)
    fmax = lambda v: np.abs(v[np.isfinite(v)]).max(initial=0.0)
    for j in range(n_levels):
        H = min(int(params["max_steps_in_episode"][j]), L)
        vs = orf.optimal_return_all(spec, params, j, L)
        si = orf.start_index(spec, params, j)
        for i in range(n_agents):
            vp = prf.policy_return_all(spec, params, j, theta_np[i], L)
            ref = vs[0, si] - vp[0, si]
            # the two tables' bounds, and the rounding of the f32 subtraction
            bound = H * 2.0 ** -23 * (max(1.0, fmax(vs)) + max(1.0, fmax(vp))) + 2.0 ** -24 * abs(ref)
            print(f"agent {i} level {j}: gpu {g64[i, j]:.6f} f64 {ref:.6f} bound {bound:.2e}")
            assert abs(g64[i, j] - ref) <= bound, (i, j, g64[i, j], ref, bound)
            assert g64[i, j] >= -bound
    # the diagonal is optimal_regret's exact score of agent i on its own level
    own = optimal_regret(smp, prng.from_uint32_numpy(jr.split(jr.PRNGKey(503), n_agents), "cuda"),
                         levels[:n_agents].contiguous(), theta)
    assert torch.equal(torch.diagonal(got[:, :n_agents]), own)
    # a payoff for the solver: agents (rows) minimise their regret, levels (columns) maximise it
    B = 4
    M = torch.zeros((B, B), device="cuda")
    M[:n_agents] = got
    s = solve_nash(M, n_agents, n_levels, iters=2000)
    e = float(s.exploitability)
    assert np.isfinite(e) and e >= -1e-6
    assert abs(float(s.x.sum()) - 1.0) < 1e-5 and abs(float(s.y.sum()) - 1.0) < 1e-5 and not s.x[n_agents:].any()
