"""The oracle's own clip VJP against finite differences (CPU, float64).

oracle/meta.py differentiates the regularised meta-loss through K clipped-SGD updates with torch autograd
(create_graph).  The GPU tests take its gradient as the truth, also where clip_by_global_norm is live
(tests/test_gpu_clip.py), so its wiring is pinned here: the autograd directional derivative of
train_agent_meta's `reg` along random unit directions of eta against a central difference, with
stop_gradient=False (a finite difference cannot see the reference's stop_gradient) and max_grad_norm
chosen so that no update clips, only the critic table clips, and both tables clip -- the branch asserted from the
gradient norms, each at least 2 % away from max_grad_norm so that the perturbed evaluations stay on the same branch.
"""
import numpy as np
import pytest
import torch

from oracle import lpg as olpg
from oracle import meta as ometa

W, T, D, K, F = 2, 4, 7, 3, 5
_STEPS = (1e-3, 1e-4, 1e-5, 1e-6)


def _inputs():
    rs = np.random.RandomState(0)

    def traj():
        return {"idx": rs.randint(0, D, (W, T + 1)), "time": rs.randint(0, 200, (W, T + 1)),
                "action": rs.randint(0, 5, (W, T)).astype(np.int64), "reward": rs.randn(W, T),
                "done": rs.rand(W, T) < 0.2}
    trajs = [traj() for _ in range(K)]
    ev = traj()
    theta0 = rs.randn(D, 5)
    phi0 = rs.randn(D, 8)
    vcrit = rs.randn(D, 1)
    # a flax-like init (zero biases, O(1/16) head weights), scaled so that pi_hat and y_hat move the tables; the
    # policy head a quarter of that, which puts the actor table's gradient norm below the critic table's
    eta = olpg.init_params(1, F, dtype=np.float64) * 1.5
    off = 0
    for name, shape in olpg.layout(F).items():
        n = int(np.prod(shape))
        if name == "pi_w":
            eta[off:off + n] *= 0.25
        off += n
    dirs = rs.randn(3, eta.size)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return trajs, ev, theta0, phi0, vcrit, eta, dirs


class _Case:
    def __init__(self, max_norm, lifetime=2500, frozen_norm=False):
        self.trajs, self.ev, self.theta0, self.phi0, self.vcrit, self.eta, self.dirs = _inputs()
        self.hyp = ometa.Hypers(max_grad_norm=max_norm, stop_gradient=False)
        self.lifetime = lifetime
        self.frozen_norm = frozen_norm

    def reg(self, eta_np, grad=False):
        """reg at eta; with grad also d reg / d eta and the (actor, critic) gradient norms of the K updates."""
        eta = torch.tensor(eta_np, dtype=torch.float64, requires_grad=grad)
        theta = torch.tensor(self.theta0, dtype=torch.float64, requires_grad=True)
        phi = torch.tensor(self.phi0, dtype=torch.float64, requires_grad=True)
        norms = []
        clip_sgd = ometa.clip_sgd

        def recording_clip_sgd(params, g, lr, max_norm):
            gn = torch.sqrt(torch.sum(g * g))
            norms.append(float(gn.detach()))
            if self.frozen_norm:      # the clip with its norm held constant: what dropping the beta term computes
                gn = gn.detach()
                return params - lr * (g if bool(gn < max_norm) else (g / gn) * max_norm)
            return clip_sgd(params, g, lr, max_norm)
        ometa.clip_sgd = recording_clip_sgd
        try:
            reg, aux = ometa.train_agent_meta(eta, theta, phi, 0, self.lifetime, torch.tensor(self.vcrit), self.trajs,
                                              self.ev, self.hyp, K)
        finally:
            ometa.clip_sgd = clip_sgd
        if not grad:
            return float(reg.detach())
        g = torch.autograd.grad(reg, eta)[0].numpy()
        return float(reg.detach()), g, np.array(norms).reshape(K, 2), int(aux["step"])

    def errors(self, h, g):
        """relative error of the central difference with step h against g . d, per direction."""
        out = []
        for d in self.dirs:
            fd = (self.reg(self.eta + h * d) - self.reg(self.eta - h * d)) / (2.0 * h)
            out.append(abs(fd - g @ d) / abs(g @ d))
        return np.array(out)


def _branches(norms, max_norm):
    assert np.all(np.abs(norms / max_norm - 1.0) >= 0.02), norms / max_norm
    return (norms >= max_norm).sum(axis=0).tolist()     # clipped updates of the K: [actor, critic]


@pytest.fixture(scope="module")
def fd_step():
    """The central difference's step, from a sweep on the unclipped case: the one with the smallest error there
    (truncation ~ h^2 against rounding ~ 1e-16 / h)."""
    case = _Case(max_norm=1e9)
    _, g, norms, _ = case.reg(case.eta, grad=True)
    assert _branches(norms, 1e9) == [0, 0]
    sweep = {h: case.errors(h, g).max() for h in _STEPS}
    print("unclipped: central-difference relative error per step", {h: f"{e:.1e}" for h, e in sweep.items()})
    h = min(sweep, key=sweep.get)
    assert sweep[h] <= 1e-6, sweep
    return h


# max_grad_norm, lifetime, clipped updates of the K (actor, critic), applied updates
@pytest.mark.parametrize("max_norm,lifetime,clipped,applied", [
    (1e9, 2500, [0, 0], 3),
    (0.065, 2500, [0, 3], 3),
    (0.03, 2500, [3, 3], 3),
    (0.03, 2, [3, 3], 2),
], ids=["unclipped", "critic-only", "both-clipped", "both-clipped-lifetime-2"])
def test_oracle_clip_vjp_matches_central_difference(fd_step, max_norm, lifetime, clipped, applied):
    case = _Case(max_norm, lifetime)
    _, g, norms, step = case.reg(case.eta, grad=True)
    print(f"max_grad_norm {max_norm}: |G_theta|, |G_phi| per update\n{norms}")
    assert _branches(norms, max_norm) == clipped and step == applied
    err = case.errors(fd_step, g)
    print(f"h = {fd_step}: relative error of the autograd directional derivatives {err}")
    assert err.max() <= 1e-6, err
    if sum(clipped):
        # the check has power: with the norm inside the clip held constant (no beta term) the same derivative is off
        # by at least a hundred times the bound
        _, g0, _, _ = _Case(max_norm, lifetime, frozen_norm=True).reg(case.eta, grad=True)
        err0 = case.errors(fd_step, g0)
        print(f"with the clip's norm frozen: {err0}")
        assert err0.max() > 1e-4, err0
