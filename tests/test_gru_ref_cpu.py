"""tests/gru_ref.py (the kernel tests' GRU reference) pinned to the oracle: with x built the way
oracle.lpg.lpg_apply builds it, the float64 heads equal lpg_apply's, and the saved states equal its states."""
import numpy as np
import pytest
import torch

from gru_ref import gru_forward_ref
from oracle import lpg as olpg


def _inputs(F, B, T, seed):
    rs = np.random.RandomState(seed)
    flat = torch.tensor(olpg.init_params(seed, F, dtype=np.float64))
    flat = flat + 0.05 * torch.tensor(rs.randn(flat.numel()))   # non-zero biases
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    r, pi = t64(rs.randn(B, T)), t64(rs.randn(B, T))
    d = torch.tensor(rs.rand(B, T) < 0.3)
    yt, yt1 = torch.softmax(t64(rs.randn(B, T, 8)), -1), torch.softmax(t64(rs.randn(B, T, 8)), -1)
    step = lifetime = None
    if F == 7:
        lifetime = torch.tensor(rs.randint(250, 2500, size=B))
        step = torch.tensor((rs.rand(B) * lifetime.numpy()).astype(np.int64))
    return flat, r, d, pi, yt, yt1, step, lifetime


@pytest.mark.parametrize("F", [5, 7])
def test_gru_ref_equals_lpg_apply(F):
    B, T = 6, 5
    flat, r, d, pi, yt, yt1, step, lifetime = _inputs(F, B, T, 11 + F)
    pi_ref, y_ref, hs, x, states = olpg.lpg_apply(flat, r, d, pi, yt, yt1, step, lifetime, return_states=True)
    assert x.shape == (B, T, F)
    out = gru_forward_ref(olpg.unflatten(flat, F), x, d, torch.float64)
    assert out["pi_hat"].dtype == torch.float64
    assert float((out["pi_hat"] - pi_ref).abs().max()) <= 1e-12
    assert float((out["y_hat"] - y_ref).abs().max()) <= 1e-12
    for t in range(T):
        for name, ref in zip(("h_in", "r", "z", "hn", "n"), states[t]):
            assert float((out[name][:, t] - ref).abs().max()) <= 1e-12, (name, t)
    # the done reset is taken: some carries are zeroed, some are not
    assert bool(d.any()) and not bool(d.all())
    assert float(out["h_in"][d].abs().max()) == 0.0


def test_gru_ref_float32_is_an_f32_evaluation():
    """dtype=float32 returns float32 tensors close to, and different from, the float64 ones (the yardstick is a real f32
    run, not a cast of the float64 result)."""
    F, B, T = 5, 6, 5
    flat, r, d, pi, yt, yt1, _, _ = _inputs(F, B, T, 3)
    flat = flat.float().double()    # f32-representable parameters, as on the device
    _, _, _, x, _ = olpg.lpg_apply(flat, r, d, pi, yt, yt1, return_states=True)
    x = x.float()
    P = olpg.unflatten(flat, F)
    o64, o32 = gru_forward_ref(P, x, d, torch.float64), gru_forward_ref(P, x, d, torch.float32)
    for k in ("pi_hat", "y_hat", "h_in", "r", "z", "n", "hn"):
        assert o32[k].dtype == torch.float32 and o64[k].dtype == torch.float64
        e = float((o32[k].double() - o64[k]).abs().max())
        assert e < 1e-5, (k, e)
    assert not torch.equal(o32["pi_hat"], o64["pi_hat"].float())
