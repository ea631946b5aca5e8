"""Plain torch-on-CPU restatement of the LPG GRU forward (models/lpg.py:11-36 LPGGRU + :79-85 heads) with the inputs
x given directly: the reference of the kernel tests (tests/test_gpu_gru_fwd.py, test_gpu_meta.py, test_gpu_es.py,
tools/gru_accuracy.py), independent of the kernels.

    float64: the reference.
    float32: the yardstick -- an ordinary f32 evaluation of the same recurrence (parameters and inputs are f32 values
             already, so only the arithmetic differs); its error against float64 is what "f32-class accuracy" means for
             the inputs at hand.

The recurrence (reverse time, the carry zeroed where done):
    h_in(t) = where(done(t), 0, h_out(t + 1)),  h_out(T) = 0
    r = sigmoid(x W_ir + b_ir + h_in W_hr),  z = sigmoid(x W_iz + b_iz + h_in W_hz),  hn = h_in W_hn + b_hn
    n = tanh(x W_in + b_in + r * hn),  h_out(t) = (1 - z) n + z h_in
    pi_hat = relu(h_out) W_pi + b_pi,  y_hat = softmax(relu(h_out) W_y + b_y)
"""
import torch

_GRU_PARAMS = ("ir_w", "ir_b", "iz_w", "iz_b", "in_w", "in_b", "hr_w", "hz_w", "hn_w", "hn_b", "pi_w", "pi_b", "y_w",
               "y_b")


def gru_forward_ref(P, x, done, dtype=torch.float64):
    """P: name -> tensor (oracle.lpg.unflatten of the flat parameters); x [R, T, F]; done [R, T] (bool or 0/1).

    Returns a dict of `dtype` tensors: pi_hat [R, T], y_hat [R, T, 8] and the per-step h_in, r, z, n,
    hn = W_hn h + b_hn, each [R, T, 256]."""
    P = {k: torch.as_tensor(P[k]).detach().to(dtype) for k in _GRU_PARAMS}
    x = torch.as_tensor(x).to(dtype)
    d = torch.as_tensor(done).bool()
    R, T, _ = x.shape
    h = torch.zeros(R, P["hr_w"].shape[0], dtype=dtype)
    names = ("h_in", "r", "z", "n", "hn")
    steps = {k: [None] * T for k in names}
    outs = [None] * T
    for t in reversed(range(T)):
        h = torch.where(d[:, t, None], torch.zeros_like(h), h)
        xt = x[:, t]
        rg = torch.sigmoid(xt @ P["ir_w"] + P["ir_b"] + h @ P["hr_w"])
        zg = torch.sigmoid(xt @ P["iz_w"] + P["iz_b"] + h @ P["hz_w"])
        hn = h @ P["hn_w"] + P["hn_b"]
        ng = torch.tanh(xt @ P["in_w"] + P["in_b"] + rg * hn)
        for k, v in zip(names, (h, rg, zg, ng, hn)):
            steps[k][t] = v
        h = (1 - zg) * ng + zg * h
        outs[t] = h
    hs = torch.relu(torch.stack(outs, 1))
    res = {k: torch.stack(v, 1) for k, v in steps.items()}
    res["pi_hat"] = (hs @ P["pi_w"] + P["pi_b"])[..., 0]
    res["y_hat"] = torch.softmax(hs @ P["y_w"] + P["y_b"], -1)
    return res
