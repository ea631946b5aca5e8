"""Shared plumbing of the GRU forward parity tests (tests/test_gpu_gru_fwd.py and its TOUED_GRU_F32=1 child
tests/gru_f32_worker.py): seeded parameters and inputs, pack + forward through the C ABI into NaN-prefilled outputs,
read-back of the saves as [R, T, 256], and the achieved-error / bound table against tests/gru_ref.py.

Bound of every output (the contract of tests/test_gpu_meta.py, set for unsaturated gates, or a small multiple of what
a plain f32 evaluation achieves on the same inputs, whichever is larger):

    heads  max(5e-6,                  4 e32)        e32 = max |gru_forward_ref(f32) - gru_forward_ref(f64)|
    saves  max(5e-6 (1 + max |ref|),  4 e32)

The factor 4 covers the kernels' different summation order.
"""
import numpy as np
import torch

from gru_ref import gru_forward_ref
from oracle import lpg as olpg

CONTRACT = 5e-6
HEADS = ("pi_hat", "y_hat")
NAN = float("nan")


def make_eta(F, seed):
    """(layout, flat f32 parameters on the host): init_lpg_params + 0.05 randn, both seeded."""
    from toued.lpg import LPGLayout, init_lpg_params
    lay = LPGLayout(F, kernel_test=True)
    eta = init_lpg_params(seed, F, device="cpu")
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return lay, eta + 0.05 * torch.randn(eta.shape, generator=g)


def scale_recurrent(lay, eta, wscale):
    for name in ("hr_w", "hz_w", "hn_w"):
        lay.view(eta, name).mul_(wscale)
    return eta


def make_inputs(N, W, T, K, F, seed, p_done=0.15):
    """xs f32 [F, K, T, R] randn, done u8 [K, N, T, W]."""
    rs = np.random.RandomState(seed)
    xs = rs.randn(F, K, T, N * W).astype(np.float32)
    done = (rs.rand(K, N, T, W) < p_done).astype(np.uint8)
    return xs, done


def refs(eta, F, xs_k, done_k):
    """(float64, float32) gru_forward_ref of one update: xs_k [F, T, R], done_k [N, T, W] (row r = agent * W + worker)."""
    N, T, W = done_k.shape
    P = olpg.unflatten(eta.double(), F)
    x = torch.from_numpy(np.array(xs_k)).permute(2, 1, 0)          # (copies: the inputs may be read-only)
    d = torch.from_numpy(np.array(done_k.transpose(0, 2, 1).reshape(N * W, T))).bool()
    return gru_forward_ref(P, x, d, torch.float64), gru_forward_ref(P, x, d, torch.float32)


class SaveRun:
    """LPGGRU (the SAVE instances) with every output NaN-prefilled: pack, then forward(k) per update."""

    def __init__(self, lay, eta, N, W, T, K, xs):
        from toued.lpg import LPGGRU
        self.N, self.W, self.T, self.K, self.R = N, W, T, K, N * W
        self.gru = gru = LPGGRU(lay, self.R, T, K, W, "cuda")
        self.eta = eta.cuda()
        gru.pack(self.eta)
        gru.X.copy_(torch.from_numpy(np.array(xs, order="C")))     # (a copy: the inputs may be read-only)
        gru.A[:256].fill_(NAN)
        gru.S.fill_(NAN)
        self.pi = torch.full((K, T, self.R), NAN, device="cuda")
        self.y = torch.full((K, T, 8, self.R), NAN, device="cuda")

    def forward(self, k, done_k, X=None, xs_f=None, xs_col=1):
        """Update k through LPGGRU.forward, or (X given: a strided device buffer, K = 1) through toued_gru_fwd itself."""
        gru = self.gru
        dk = torch.from_numpy(np.array(done_k, order="C")).cuda()
        if X is None:
            gru.forward(k, gru.X, dk, self.eta, self.pi, self.y)
        else:
            from toued import _lib
            assert self.K == 1 and k == 0
            S = gru.S
            _lib.call("toued_gru_fwd", self.R, self.T, self.W, gru.lay.F, _lib.ptr(X), xs_f, xs_col, _lib.ptr(dk),
                      _lib.ptr(gru.fwdA), _lib.ptr(self.eta), gru.lay.c_offsets, _lib.ptr(self.pi[0]),
                      _lib.ptr(self.y[0]), _lib.ptr(gru.A), _lib.ptr(S[0]), _lib.ptr(S[1]), _lib.ptr(S[2]),
                      _lib.ptr(S[3]), gru.M, _lib.stream_ptr())
        torch.cuda.synchronize()

    def save_names(self):
        # (the split-precision pair saves no n: its backward recomputes it, gru.hip gate_n)
        return ("h_in", "r", "z", "hn") + (() if self.gru.slab else ("n",))

    def outputs(self, k):
        """Update k's heads [R, T], [R, T, 8] and saves [R, T, 256] as host arrays, read back through hin_rows() /
        s_rows()."""
        gru, K, T, R = self.gru, self.K, self.T, self.R

        def tr(rows):
            return rows.reshape(256, K, T, R)[:, k].permute(2, 1, 0).cpu().numpy()
        out = {"pi_hat": self.pi[k].t().cpu().numpy(), "y_hat": self.y[k].permute(2, 0, 1).cpu().numpy(),
               "h_in": tr(gru.hin_rows()), "r": tr(gru.s_rows(0)), "z": tr(gru.s_rows(1)), "hn": tr(gru.s_rows(3))}
        if not gru.slab:
            out["n"] = tr(gru.S[2])
        return out


def run_multi(lay, etas, R, T, W, rpc, X, xs_f, xs_col, done):
    """toued_gru_pack_fwd_multi + toued_gru_fwd_multi (the per-candidate instances): etas [C, size] on the host,
    X a device buffer read as X[f * xs_f + (t * R + r) * xs_col], done u8 [R / W, T, W].  Heads [R, T], [R, T, 8]."""
    from toued import _lib
    C = etas.shape[0]
    assert C * rpc == R
    ed = etas.cuda().contiguous()
    fwdA = torch.zeros(C, _lib.lib().toued_gru_packed_floats(2), device="cuda")
    _lib.call("toued_gru_pack_fwd_multi", _lib.ptr(ed), lay.size, C, lay.c_offsets, lay.F, _lib.ptr(fwdA),
              _lib.stream_ptr())
    pi = torch.full((T, R), NAN, device="cuda")
    y = torch.full((T, 8, R), NAN, device="cuda")
    dk = torch.from_numpy(np.array(done, order="C")).cuda()
    _lib.call("toued_gru_fwd_multi", R, T, W, lay.F, rpc, _lib.ptr(X), xs_f, xs_col, _lib.ptr(dk), _lib.ptr(fwdA),
              _lib.ptr(ed), lay.size, lay.c_offsets, _lib.ptr(pi), _lib.ptr(y), _lib.stream_ptr())
    torch.cuda.synchronize()
    return {"pi_hat": pi.t().cpu().numpy(), "y_hat": y.permute(2, 0, 1).cpu().numpy()}


def multi_refs(lay, etas, xs, done, rpc):
    """Per-candidate references of a multi run joined along the rows: xs [F, T, R], done [R / W, T, W]; rows
    [c * rpc, (c + 1) * rpc) under candidate c's parameters."""
    F, T, R = xs.shape
    d_rows = done.transpose(0, 2, 1).reshape(R, T)       # row r = agent * W + worker
    r64, r32 = [], []
    for c in range(etas.shape[0]):
        sl = slice(c * rpc, (c + 1) * rpc)
        a, b = refs(etas[c], F, xs[:, :, sl], d_rows[sl].T[None])
        r64.append(a)
        r32.append(b)
    cat = lambda rs: {k: torch.cat([r[k] for r in rs]) for k in HEADS}
    return cat(r64), cat(r32)


def table(tag, got, r64, r32):
    """{output: (achieved max abs error vs float64, bound)} of the outputs in `got`, printed as "achieved / bound";
    every element of `got` must be finite (so: written)."""
    res = {}
    for name, g in got.items():
        ref = r64[name].numpy()
        assert g.shape == ref.shape, (tag, name, g.shape, ref.shape)
        assert np.isfinite(g).all(), f"{tag} {name}: {np.count_nonzero(~np.isfinite(g))} non-finite elements"
        e32 = float(np.abs(r32[name].double().numpy() - ref).max())
        contract = CONTRACT if name in HEADS else CONTRACT * (1.0 + float(np.abs(ref).max()))
        bound = max(contract, 4.0 * e32)
        err = float(np.abs(g.astype(np.float64) - ref).max())
        print(f"[gru_fwd {tag}] {name}: achieved {err:.2e} / bound {bound:.2e} (contract {contract:.2e}, "
              f"e32 {e32:.2e})")
        res[name] = (err, bound)
    return res


def save_case(tag, N, W, T, F, seed, K=1, lay_eta=None, inputs=None):
    """One SAVE case end to end: K updates of N x W rows, heads and every save of every update against the
    references.  Returns ({output (of update k): (achieved, bound)}, the SaveRun)."""
    lay, eta = lay_eta or make_eta(F, seed)
    xs, done = inputs or make_inputs(N, W, T, K, F, seed)
    run = SaveRun(lay, eta, N, W, T, K, xs)
    for k in range(K):
        run.forward(k, done[k])
    res = {}
    for k in range(K):
        r64, r32 = refs(eta, F, xs[:, k], done[k])
        got = run.outputs(k)
        assert set(got) == set(HEADS + run.save_names())
        sfx = f" k={k}" if K > 1 else ""
        res.update({name + sfx: v for name, v in table(tag + sfx, got, r64, r32).items()})
    return res, run


def assert_within(tag, res):
    bad = {k: v for k, v in res.items() if not v[0] <= v[1]}
    assert not bad, f"{tag}: achieved error above bound (achieved, bound): {bad}"
