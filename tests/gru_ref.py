"""Plain torch-on-CPU restatement of the LPG GRU forward (models/lpg.py:11-36 LPGGRU + :79-85 heads) with the inputs
x given directly, and its VJP by autograd (gru_backward_ref): the reference of the kernel tests
(tests/test_gpu_gru_fwd.py, test_gpu_gru_bwd.py, test_gpu_meta.py, test_gpu_es.py, tools/gru_accuracy.py), independent
of the kernels.

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


def gru_backward_ref(P, x, done, d_pi, d_y, relu_mask=None, dtype=torch.float64, y_hat=None):
    """VJP of the recurrence above under the loss sum(pi_hat * d_pi) + sum(y_hat * d_y): torch autograd over a forward
    that keeps every pre-activation, evaluated wholly in `dtype` (float32: the yardstick, as in gru_forward_ref).

    x [R, T, F]; done [R, T]; d_pi [R, T]; d_y [R, T, 8]; relu_mask [R, T, 256] bool: when given, relu(h_out) is
    where(mask, h_out, 0) (the branch decisions of a float32 implementation).  y_hat [R, T, 8], when given, replaces
    softmax(logits) in the softmax VJP y (dy - sum y dy) (a caller's own y_hat, one-hot rows for instance).

    Returns a dict of `dtype` tensors:
        "grads"     name -> gradient of the 14 GRU / head parameters
        "dx"        [R, T, F]
        "dr_pre", "dz_pre", "dn_pre"   cotangents of the arguments of the two sigmoids and of the tanh, [R, T, 256]
        "dhn"       cotangent of hn = h_in W_hn + b_hn, [R, T, 256]
        "dh_heads"  [R, T, 9]: d pi_hat, then the cotangent of the y logits
        "relu_out"  [R, T, 256]
        "h_out"     [R, T, 256]
        "flips"     |h_out| of every element where relu_mask differs from h_out > 0 (empty without a mask)"""
    P = {k: torch.as_tensor(P[k]).detach().to(dtype).clone().requires_grad_(True) for k in _GRU_PARAMS}
    x = torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True)
    d = torch.as_tensor(done).bool()
    d_pi = torch.as_tensor(d_pi).to(dtype)
    d_y = torch.as_tensor(d_y).to(dtype)
    R, T, _ = x.shape
    h = torch.zeros(R, P["hr_w"].shape[0], dtype=dtype)
    pre = {k: [None] * T for k in ("a_r", "a_z", "hn", "a_n")}
    outs = [None] * T
    for t in reversed(range(T)):
        h = torch.where(d[:, t, None], torch.zeros_like(h), h)
        xt = x[:, t]
        a_r = xt @ P["ir_w"] + P["ir_b"] + h @ P["hr_w"]
        a_z = xt @ P["iz_w"] + P["iz_b"] + h @ P["hz_w"]
        hn = h @ P["hn_w"] + P["hn_b"]
        rg, zg = torch.sigmoid(a_r), torch.sigmoid(a_z)
        a_n = xt @ P["in_w"] + P["in_b"] + rg * hn
        for k, v in zip(("a_r", "a_z", "hn", "a_n"), (a_r, a_z, hn, a_n)):
            pre[k][t] = v
        h = (1 - zg) * torch.tanh(a_n) + zg * h
        outs[t] = h
    h_out = torch.stack(outs, 1)
    if relu_mask is None:
        hs = torch.relu(h_out)
        flips = torch.zeros(0, dtype=dtype)
    else:
        mk = torch.as_tensor(relu_mask).bool()
        hs = torch.where(mk, h_out, torch.zeros_like(h_out))
        flips = h_out.detach()[mk != (h_out.detach() > 0)].abs()
    pi_hat = (hs @ P["pi_w"] + P["pi_b"])[..., 0]
    logits = hs @ P["y_w"] + P["y_b"]
    y = torch.softmax(logits.detach(), -1) if y_hat is None else torch.as_tensor(y_hat).to(dtype)
    d_logits = y * (d_y - (y * d_y).sum(-1, keepdim=True))
    names = list(_GRU_PARAMS)
    flat_pre = [v for k in ("a_r", "a_z", "hn", "a_n") for v in pre[k]]
    g = torch.autograd.grad([pi_hat, logits], [P[k] for k in names] + [x] + flat_pre, [d_pi, d_logits],
                            allow_unused=True)
    zero = lambda v, like: torch.zeros_like(like) if v is None else v
    res = {"grads": {k: zero(v, P[k]) for k, v in zip(names, g[:len(names)])}, "dx": zero(g[len(names)], x)}
    gp = g[len(names) + 1:]
    for i, k in enumerate(("dr_pre", "dz_pre", "dhn", "dn_pre")):
        res[k] = torch.stack([zero(v, h_out[:, 0]) for v in gp[i * T:(i + 1) * T]], 1)
    res["dh_heads"] = torch.cat([d_pi[..., None], d_logits], -1)
    res["relu_out"] = hs.detach()
    res["h_out"] = h_out.detach()
    res["flips"] = flips
    return res
