"""The clipped-SGD branches of the inner LPG update and their VJP, with the clip live.

Every inner update ends in clip_by_global_norm(max_grad_norm) + SGD (models/optim.py:5-11) and the meta-gradient
differentiates through it.  Per table the device code has three branches, each with its VJP coefficients
(agent.hip clip_coef):

    not applied (step + 1 > lifetime)   copy                         aa = ba = 0
    applied, |G| <  max_norm            p - lr g                     aa = 1, ba = 0
    applied, |G| >= max_norm            p - lr (g / |G|) max_norm    aa = max_norm / |G|,
                                                                     ba = lr max_norm <G, adj> / |G|^3

At the reference's max_grad_norm = 0.5 the gradient norms of the suite's inputs are 7-300x below the threshold, so
the third row (and with it <G_k, adjoint>, the ba * g terms of the HVP and apply_seg<2>) never runs there.  Here
max_grad_norm is lowered into the norms:

  * test_clipped_meta_step_matches_oracle: a whole meta-step against the float64 autograd oracle on the same
    trajectories (the contract of tests/test_gpu_meta.py, unchanged: parameters and metrics 2e-5, meta-gradient
    relative L2 < 1e-5, cosine > 1 - 1e-9), on every launch path, after a first meta-step of the same object has
    left its gradient rows, adjoint tables and cotangents behind.  Which (update, agent, table) entries clipped and
    which updates were applied is asserted from gstat against the oracle's float64 norms, every norm at least 2 %
    away from max_grad_norm (so float32 cannot decide the branch differently).
  * test_clip_dot_matches_float64 / test_agent_apply_matches_float32_numpy: the dense pair toued_clip_dot and
    toued_agent_apply on synthetic tables, every agent role in one launch, odd table offsets, 16-byte aligned and
    one-float-offset tensors (the scalar vec4 == 0 path).
"""
import numpy as np
import pytest
import torch

from oracle import meta as ometa

from test_gpu_meta import _assert_run_matches_oracle, _clone_agents, _oracle_of_run, _run_checked_step, _setup

pytestmark = pytest.mark.gpu

N, W, T, K = 3, 64, 20, 3

# max_norm: lowered into the gradient norms of these inputs.  clipped: the (actor, critic) number of applied
# (update, agent) entries whose table clipped, of K * N = 9; not_applied: updates discarded by the lifetime test.
# life: (lifetimes, start steps) -- agent 0 applies update 0 only, agent 2 applies update 0 only.
_CASES = {
    "dense-critic-only": dict(mode="dense", lc=False, max_norm=0.01, clipped=(0, 9), not_applied=0),
    "dense-both": dict(mode="dense", lc=False, max_norm=0.002, clipped=(9, 9), not_applied=0),
    "vrandlife-mixed": dict(mode="all_vrandlife", lc=True, max_norm=0.012, clipped=(3, 9), not_applied=0, mixed=True),
    "mazes": dict(mode="mazes", lc=False, max_norm=0.003, clipped=(8, 9), not_applied=0),
    "dense-lifetime": dict(mode="dense", lc=False, max_norm=0.002, clipped=(5, 5), not_applied=4,
                           life=([5, 2500, 1], [4, 0, 0])),
}
_PATHS = {
    "default": {},
    "dense-path": {"TOUED_META_FUSED_STEP": "0"},
    "separate-launches": {"TOUED_REVERSE_PAIR": "0", "TOUED_STEP_ENTROPY": "0"},
}
_RUNS = {}      # (case, path) -> host arrays of the checked step
_ORACLE = {}    # case -> (g_ref, aux, norms): the trajectories are bit-identical across paths (asserted)


def _gpu_run(case, path, monkeypatch):
    """The checked meta-step of `case` on launch path `path` (rng [0, 77], pristine agents), after one meta-step of
    the same MetaGradStep object on cloned agents with rng [0, 76]: the checked step finds G_th / G_ph, the adjoint
    tables and d_pi_hat / d_y_hat holding the first step's contents, gradient rows it does not touch included."""
    if (case, path) in _RUNS:
        return _RUNS[(case, path)]
    from toued.env import L_LIFETIME
    from toued.meta import AdamState
    c = _CASES[case]
    for name in ("TOUED_META_FUSED_STEP", "TOUED_REVERSE_PAIR", "TOUED_STEP_ENTROPY"):
        monkeypatch.delenv(name, raising=False)
    for name, value in _PATHS[path].items():
        monkeypatch.setenv(name, value)
    agents, step, eta, adam, hyp, D = _setup(c["mode"], N, W, T, K, c["lc"], max_grad_norm=c["max_norm"])
    assert step.fused_step == (path != "dense-path")
    assert step.step_entropy == step.reverse_pair == (path != "separate-launches")
    assert hyp.max_grad_norm == c["max_norm"]
    if "life" in c:
        life, start = c["life"]
        agents.levels[:, L_LIFETIME] = torch.tensor(life, dtype=torch.int32, device="cuda")
        agents.step.copy_(torch.tensor(start, dtype=torch.int32, device="cuda"))
    step(torch.tensor([0, 76], dtype=torch.int32, device="cuda"), eta.clone(), AdamState(eta.numel(), "cuda"),
         _clone_agents(agents))
    torch.cuda.synchronize()
    run = _run_checked_step(agents, step, eta, adam, (0, 77))
    run["d_pi_hat"], run["d_y_hat"] = step.d_pi_hat.cpu().numpy(), step.d_y_hat.cpu().numpy()
    _RUNS[(case, path)] = run
    return run


def _assert_coverage(c, run, norms64):
    """The branches this case exists for were taken: read from gstat [K][N][4] = (|G_theta|, |G_phi|, applied, -),
    against the oracle's float64 norms on the same trajectories and the reference's lifetime rule."""
    m = c["max_norm"]
    gstat = run["gstat"]
    lifetime = run["levels"][:, 5].astype(np.int64)
    s = run["step0"].astype(np.int64).copy()
    applied_ref = np.zeros((K, N), bool)
    for k in range(K):              # lpg_agent.py:71-82: the update is kept when step + 1 <= lifetime
        applied_ref[k] = s + 1 <= lifetime
        s += applied_ref[k]
    g32 = gstat[..., :2].astype(np.float64)
    for k in range(K):
        print(f"update {k}: |G|/max_norm device {np.array2string(g32[k] / m, precision=3)} "
              f"oracle {np.array2string(norms64[k] / m, precision=3)} applied {gstat[k, :, 2]}")
    assert np.array_equal(gstat[..., 2] > 0.5, applied_ref), gstat[..., 2]
    assert np.array_equal(run["step"], s)
    gap = min(np.abs(g32 / m - 1.0).min(), np.abs(norms64 / m - 1.0).min())
    print(f"smallest | |G| / max_norm - 1 | = {gap:.3f}")
    assert gap >= 0.02, gap
    clipped = g32 >= m
    assert np.array_equal(clipped, norms64 >= m)
    live = clipped & applied_ref[..., None]
    census = (int(live[..., 0].sum()), int(live[..., 1].sum()))
    print(f"applied updates with the actor / critic table clipped: {census} of {int(applied_ref.sum())}; "
          f"not applied: {int((~applied_ref).sum())}")
    assert census == c["clipped"] and int((~applied_ref).sum()) == c["not_applied"]
    if c.get("mixed"):   # one launch with clipped and unclipped actor tables side by side
        assert any(0 < live[k, :, 0].sum() < N for k in range(K)), live[..., 0]


@pytest.mark.parametrize("path", list(_PATHS))
@pytest.mark.parametrize("case", list(_CASES))
def test_clipped_meta_step_matches_oracle(case, path, monkeypatch):
    c = _CASES[case]
    run = _gpu_run(case, path, monkeypatch)
    base = _gpu_run(case, "default", monkeypatch)
    # every path walks the same theta_k / phi_k bit for bit, so the trajectories and the oracle result are shared
    for name in ("theta_h", "phi_h", "theta", "phi", "step", "gstat"):
        assert np.array_equal(run[name], base[name]), name
    for name in run["traj"]:
        assert np.array_equal(run["traj"][name], base["traj"][name]), name
    assert np.array_equal(run["metrics"]["lpg_loss"], base["metrics"]["lpg_loss"])
    for name, v in run["metrics"]["lpg_agent"].items():
        assert np.array_equal(v, base["metrics"]["lpg_agent"][name]), name
    if case not in _ORACLE:
        ohyp = ometa.Hypers(max_grad_norm=c["max_norm"], lifetime_conditioning=c["lc"])
        _ORACLE[case] = _oracle_of_run(c["mode"], base, K, T, ohyp)
    g_ref, aux, norms64 = _ORACLE[case]
    _assert_coverage(c, run, norms64)
    _assert_run_matches_oracle(run, g_ref, aux)
    rel = np.linalg.norm(run["grad"] - base["grad"]) / np.linalg.norm(base["grad"])
    print(f"meta-gradient {path} vs default rel L2 {rel:.2e}")
    if path == "separate-launches":     # the one-launch update and reverse step change no bit
        assert np.array_equal(run["grad"], base["grad"])
        assert np.array_equal(run["d_pi_hat"], base["d_pi_hat"]) and np.array_equal(run["d_y_hat"], base["d_y_hat"])
    else:                               # the triangle inequality of the two oracle bounds
        assert rel < 2e-5, rel


# ------------------------------------------------------------------ the dense pair on synthetic tables
_LR_A, _LR_C, _MAX_NORM = 40.0, 4.0, 0.5
# agent a's role: (applied, actor clipped, critic clipped)
_ROLES = ((False, True, True), (True, False, False), (True, True, False), (True, False, True), (True, True, True))


def _dev(arr, aligned, fill=None):
    """arr on the device, 16-byte aligned or offset by one element from a 16-byte boundary, with one guard element
    on each side.  Returns (buffer, view, offset); fill: the view holds `fill` instead of arr (an output)."""
    arr = np.ascontiguousarray(arr)
    off = 4 if aligned else 1
    t = torch.from_numpy(arr.reshape(-1))
    buf = torch.full((arr.size + 8,), float("nan") if t.dtype.is_floating_point else -77, dtype=t.dtype, device="cuda")
    view = buf[off:off + arr.size]
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == (0 if aligned else 4) and view.is_contiguous()
    return buf, view, off


def _guards_intact(buf, off, n):
    g = torch.cat([buf[:off], buf[off + n:]])
    return bool(torch.isnan(g).all()) if buf.dtype.is_floating_point else bool((g == -77).all())


def _tables(D, seed):
    """Gradient tables with a random subset of zero rows (as the sorted path leaves the rows it does not touch),
    scaled so that each agent's norms put it in its role; gstat from the float64 norms rounded to float32."""
    rs = np.random.RandomState(seed)
    Na = len(_ROLES)
    G = [rs.randn(Na, D, 5).astype(np.float32), rs.randn(Na, D, 8).astype(np.float32)]
    adj = [rs.randn(Na, D, 5).astype(np.float32), rs.randn(Na, D, 8).astype(np.float32)]
    if D > 1:
        for t in range(2):
            G[t][rs.rand(Na, D) < 0.4] = 0.0
            adj[t][rs.rand(Na, D) < 0.1] = 0.0
    gstat = np.zeros((Na, 4), np.float32)
    for a, (applied, clip_a, clip_c) in enumerate(_ROLES):
        for t, clip in enumerate((clip_a, clip_c)):
            target = (2.9 + 0.3 * a if clip else 0.37 + 0.05 * a) * _MAX_NORM
            n = np.sqrt(np.sum(G[t][a].astype(np.float64) ** 2))
            G[t][a] = (G[t][a] * np.float32(target / n)).astype(np.float32)
            gstat[a, t] = np.float32(np.sqrt(np.sum(G[t][a].astype(np.float64) ** 2)))
            assert (gstat[a, t] >= _MAX_NORM) == clip and abs(gstat[a, t] / _MAX_NORM - 1.0) > 0.02
        gstat[a, 2] = 1.0 if applied else 0.0
    return G, adj, gstat


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("D", [1, 1937])
def test_clip_dot_matches_float64(D, aligned):
    """toued_clip_dot's coef[N][4] = (aa, ba, ac, bc) against the float64 formulas of the module docstring: aa / ac
    at rtol 1e-6; ba / bc within 1e-5 * sum|G_i adj_i| * lr max_norm / |G|^3 of the float64 dot (float32 partial
    sums over at most 15.5 k terms; one dropped row of a 1937-row table is >= ~5e-4 of that sum).  N = 5 with
    5 * 1937 odd: agent a's actor table starts at offset a * 9685, so the scalar heads cycle through 0, 3, 2, 1
    elements; D = 1 leaves the float4 body empty for a >= 1."""
    from toued import _lib as L
    Na = len(_ROLES)
    G, adj, gstat = _tables(D, 100 + D)
    dev = [_dev(x, aligned) for x in (G[0], G[1], adj[0], adj[1], gstat)]
    cbuf, coef, coff = _dev(np.zeros((Na, 4), np.float32), aligned, fill=float("nan"))
    L.call("toued_clip_dot", Na, D, L.ptr(dev[0][1]), L.ptr(dev[1][1]), L.ptr(dev[2][1]), L.ptr(dev[3][1]),
           L.ptr(dev[4][1]), _LR_A, _LR_C, _MAX_NORM, L.ptr(coef), L.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(cbuf, coff, Na * 4)
    got = coef.cpu().numpy().reshape(Na, 4).astype(np.float64)
    assert np.isfinite(got).all()
    worst = 0.0
    for a, (applied, clip_a, clip_c) in enumerate(_ROLES):
        for t, (clip, lr) in enumerate(((clip_a, _LR_A), (clip_c, _LR_C))):
            alpha, beta = got[a, 2 * t], got[a, 2 * t + 1]
            gn = float(gstat[a, t])
            if not applied:
                assert alpha == 0.0 and beta == 0.0, (a, t)
            elif not clip:
                assert alpha == 1.0 and beta == 0.0, (a, t)
            else:
                prod = G[t][a].astype(np.float64) * adj[t][a].astype(np.float64)
                scale = lr * _MAX_NORM / gn ** 3
                assert abs(alpha - _MAX_NORM / gn) <= 1e-6 * _MAX_NORM / gn, (a, t)
                err = abs(beta - prod.sum() * scale) / (np.abs(prod).sum() * scale)
                worst = max(worst, err)
                assert err <= 1e-5, (a, t, err)
    print(f"D={D} aligned={aligned}: worst beta error {worst:.2e} of sum|G adj| lr max_norm / |G|^3")


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("D", [1, 1937])
def test_agent_apply_matches_float32_numpy(D, aligned):
    """toued_agent_apply against numpy doing the same float32 operations, p + (-(lr * ((g / |G|) * max_norm))), at
    rtol 1e-6 plus 1e-7 |p|; not-applied agents bit-equal to the input; step advanced exactly where the update was
    applied; every element written (the outputs start as NaN) and nothing outside the outputs."""
    from toued import _lib as L
    f = np.float32
    Na = len(_ROLES)
    G, _, gstat = _tables(D, 200 + D)
    rs = np.random.RandomState(300 + D)
    P = [(rs.randn(Na, D, 5) * 3).astype(f), (rs.randn(Na, D, 8) * 3).astype(f)]
    step0 = rs.randint(0, 1000, Na).astype(np.int32)
    dev = [_dev(x, aligned) for x in (P[0], P[1], G[0], G[1], gstat)]
    sbuf, step, soff = _dev(step0, aligned)
    outs = [_dev(P[t], aligned, fill=float("nan")) for t in range(2)]
    L.call("toued_agent_apply", Na, D, L.ptr(dev[0][1]), L.ptr(dev[1][1]), L.ptr(dev[2][1]), L.ptr(dev[3][1]),
           _LR_A, _LR_C, _MAX_NORM, L.ptr(step), L.ptr(outs[0][1]), L.ptr(outs[1][1]), L.ptr(dev[4][1]),
           L.stream_ptr())
    torch.cuda.synchronize()
    applied = np.array([r[0] for r in _ROLES])
    assert np.array_equal(step.cpu().numpy(), step0 + applied) and _guards_intact(sbuf, soff, Na)
    for t, lr in enumerate((_LR_A, _LR_C)):
        buf, view, off = outs[t]
        assert _guards_intact(buf, off, P[t].size), t
        got = view.cpu().numpy().reshape(P[t].shape)
        assert np.isfinite(got).all(), t
        for a, role in enumerate(_ROLES):
            p, g, gn = P[t][a], G[t][a], f(gstat[a, t])
            if not role[0]:
                assert np.array_equal(got[a], p), (t, a)
                continue
            assert (gn >= _MAX_NORM) == role[1 + t]
            gc = (g / gn) * f(_MAX_NORM) if role[1 + t] else g
            ref = p + (-(f(lr) * gc))
            assert ref.dtype == f
            assert np.all(np.abs(got[a].astype(np.float64) - ref) <= 1e-6 * np.abs(ref) + 1e-7 * np.abs(p)), (t, a)
    for (buf, view, off), src in zip(dev, (P[0], P[1], G[0], G[1], gstat)):   # the inputs are untouched
        assert np.array_equal(view.cpu().numpy(), src.reshape(-1))
