"""GPU parity of the LPG GRU forward (csrc/gru.hip) on every kernel instance and at its index edges, against the
plain float64 restatement tests/gru_ref.py.

Dispatch (gru_fwd_launch): with nt2 = R % 64 == 0 and (rows_per_cand == 0 or rows_per_cand % 64 == 0),

    nt2 and not TOUED_GRU_F32=1   k_gru_fwd6<true>  (toued_gru_fwd)   k_gru_fwd6<false>  (toued_gru_fwd_multi)
    nt2 and TOUED_GRU_F32=1       k_gru_fwd<true,2>                   k_gru_fwd<false,2>
    not nt2                       k_gru_fwd<true,1>                   k_gru_fwd<false,1>

Which case runs which instance:

    k_gru_fwd6<true>    a b c d e f g h i m n     (SAVE: heads + saves h_in, r, z, W_hn h + b_hn)
    k_gru_fwd6<false>   i l m n                   (per-candidate: heads)
    k_gru_fwd<true,1>   j n                       (SAVE: heads + the five saves, n included, in [256][M] rows)
    k_gru_fwd<false,1>  k n
    k_gru_fwd<true,2>   a, c (T = 3) and the repeat n, in the child process of test_f32_fallback_process (the switch
                        is read once per process), which also runs one backward case under the switch
    k_gru_fwd<false,2>  the child's per-candidate run (two candidates of 64 rows, F = 7)

Every case packs and runs through the C ABI into NaN-prefilled outputs, checks pi_hat, y_hat and (SAVE) every save the
instance writes, and prints "achieved / bound" per output; the bound is tests/gru_fwd_cases.py's: the contract of
tests/test_gpu_meta.py (heads 5e-6, saves 5e-6 (1 + max |ref|)) or four times the error of a plain f32 evaluation of the
same inputs, whichever is larger.  DESIGN.md §6 records a run.
"""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import gru_fwd_cases as gc

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NAN = float("nan")


def _fwd6(run):
    """The case must have run the split-precision SAVE instance (its saves are in slab / unit-quad blocks)."""
    assert run.gru.slab and "n" not in run.save_names()


# ---------------------------------------------------------------------------------------------- a, b, c, e: shapes
@pytest.mark.parametrize("tag,N,W,T,F", [
    ("a", 4, 32, 6, 5),      # two agents per workgroup: each 32-row tile reads its own agent's done row
    ("b", 2, 96, 6, 5),      # the agent boundary falls between the two tiles of workgroup 1
    ("c-T1", 1, 64, 1, 5),   # single workgroup; T = 1: only the flush after the loop writes heads
    ("c-T2", 1, 64, 2, 5),   # one deferred head reduce + the flush, both parities of the double buffer
    ("c-T3", 1, 64, 3, 5),   # parity 0 reused
    ("e-F1", 1, 64, 4, 1),   # input-width clamp fc = min(f, F - 1) at its extreme, bias at slot 1
    ("e-F6", 1, 64, 4, 6),   # bias at slot 6
    ("e-F7", 1, 64, 4, 7),   # all eight augmented slots in use, bias at slot 7
])
def test_save_shapes(tag, N, W, T, F):
    res, run = gc.save_case(tag, N, W, T, F, seed=sum(map(ord, tag)))
    _fwd6(run)
    gc.assert_within(tag, res)


# ---------------------------------------------------------------------------------------------- d: K = 2
def test_save_offsets_of_second_update():
    """d: update 1's saves start at slab block 256 * T * R; update 0's saves, read back before and after the second
    call, are bit-identical, and both updates' saves match their references."""
    N, W, T, K, F = 2, 64, 4, 2, 5
    lay, eta = gc.make_eta(F, 41)
    xs, done = gc.make_inputs(N, W, T, K, F, 41)
    run = gc.SaveRun(lay, eta, N, W, T, K, xs)
    _fwd6(run)
    run.forward(0, done[0])
    before = run.outputs(0)
    run.forward(1, done[1])
    after = run.outputs(0)
    for name in before:
        assert np.array_equal(before[name], after[name]), f"update 0's {name} changed by the forward of update 1"
    res = {}
    for k in range(K):
        r64, r32 = gc.refs(eta, F, xs[:, k], done[k])
        res.update({f"{n} k={k}": v for n, v in gc.table(f"d k={k}", run.outputs(k), r64, r32).items()})
    gc.assert_within("d", res)


# ---------------------------------------------------------------------------------------------- f: done patterns
@pytest.mark.parametrize("pattern", ["ones", "zeros", "last", "first"])
def test_save_done_patterns(pattern):
    """f: all ones (every output depends on x(t) alone: every saved h_in is exactly 0); all zeros; ones only at
    t = T - 1 (no effect on the recurrence: the carry into T - 1 is 0 anyway, and no other step may see the flag); ones
    only at t = 0 (the carry into the last step of the scan)."""
    N, W, T, F = 2, 64, 6, 5
    xs, done = gc.make_inputs(N, W, T, 1, F, 51)
    done[:] = 0
    if pattern == "ones":
        done[:] = 1
    elif pattern == "last":
        done[:, :, T - 1] = 1
    elif pattern == "first":
        done[:, :, 0] = 1
    res, run = gc.save_case(f"f-{pattern}", N, W, T, F, seed=51, inputs=(xs, done))
    _fwd6(run)
    gc.assert_within(f"f-{pattern}", res)
    h_in = run.outputs(0)["h_in"]
    if pattern == "ones":
        assert not h_in.any()
    else:
        assert not h_in[:, T - 1].any() and h_in[:, :T - 1].any()
    if pattern == "first":
        assert not h_in[:, 0].any() and h_in[:, 1].any()


# ---------------------------------------------------------------------------------------------- g: weight scales
@pytest.mark.parametrize("zero_gate", ["hr_w", "hz_w", "hn_w"])
def test_save_heterogeneous_weight_scales(zero_gate):
    """g: k_fwd6_scales' clamp to [-30, 20] and its zero-row branch.  Column u (output unit u) of each recurrent
    matrix is multiplied by 2^k(u), k drawn from {-40, -20, -8, 0, 2} (2^-40: the scale exponent 14 - e clamps at 20);
    five columns of each gate are exactly zero; one whole gate's recurrent weights are zero."""
    N, W, T, F = 2, 64, 6, 5
    lay, eta = gc.make_eta(F, 61)
    rs = np.random.RandomState(61)
    for name in ("hr_w", "hz_w", "hn_w"):
        w = lay.view(eta, name)                                    # [k (input unit), u (output unit)]
        k = rs.choice([-40, -20, -8, 0, 2], size=256)
        w.mul_(torch.from_numpy(np.ldexp(1.0, k).astype(np.float32))[None, :])
        w[:, torch.from_numpy(rs.choice(256, 5, replace=False))] = 0.0
    lay.view(eta, zero_gate).zero_()
    res, run = gc.save_case(f"g-{zero_gate}", N, W, T, F, seed=61, lay_eta=(lay, eta))
    _fwd6(run)
    gc.assert_within(f"g-{zero_gate}", res)


# ---------------------------------------------------------------------------------------------- h: recurrent scale
@pytest.mark.parametrize("wscale", [4.0, 1e-3])
def test_save_recurrent_weight_scale(wscale):
    """h: the forward side of test_gru_backward_matches_autograd's wscale cases, checked directly."""
    N, W, T, F = 2, 64, 6, 5
    lay, eta = gc.make_eta(F, 71)
    gc.scale_recurrent(lay, eta, wscale)
    res, run = gc.save_case(f"h-{wscale:g}", N, W, T, F, seed=71, lay_eta=(lay, eta))
    _fwd6(run)
    gc.assert_within(f"h-{wscale:g}", res)


# ---------------------------------------------------------------------------------------------- i: lifetime inputs
def _lifetime_eta(seed):
    """Input rows 5 (step) and 6 (lifetime) of W_ir, W_iz, W_in: row 5 times 1e-3, row 6 = -row 5 times a per-unit
    factor in [0.9, 1.1] -- each term reaches +-25 at lifetime 25000 and the two cancel."""
    lay, eta = gc.make_eta(7, seed)
    rs = np.random.RandomState(seed)
    for name in ("ir_w", "iz_w", "in_w"):
        w = lay.view(eta, name)                                    # [7, 256]
        w[5] *= 1e-3
        w[6] = -w[5] * torch.from_numpy(rs.uniform(0.9, 1.1, size=256).astype(np.float32))
    return lay, eta


@functools.lru_cache(maxsize=None)
def _lifetime_inputs(integer):
    """randn inputs with X[6] an integer lifetime in [250, 25000] and X[5] an integer step in [0, lifetime) per row
    (--lifetime_conditioning: k_lpg_inputs writes the raw counters); integer=False adds U[0, 1) to both at every step,
    so the f32 values need all three bf16 pieces."""
    N, W, T, F = 2, 64, 6, 7
    xs, done = gc.make_inputs(N, W, T, 1, F, 81)
    rs = np.random.RandomState(82)
    life = rs.randint(250, 25001, size=N * W)
    step = np.floor(rs.rand(N * W) * life)
    assert (step < life).all() and life.max() > 20000
    frac = (lambda: 0.0) if integer else (lambda: rs.rand(T, N * W))
    xs[5, 0] = (step[None, :] + frac()).astype(np.float32)
    xs[6, 0] = (life[None, :] + frac()).astype(np.float32)
    xs.setflags(write=False)
    done.setflags(write=False)
    return xs, done


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "fractional"])
def test_save_lifetime_inputs(integer):
    """i, SAVE instance (the three-piece bf16 split of 2^14 x in the augmented k-step)."""
    N, W, T, F = 2, 64, 6, 7
    lay, eta = _lifetime_eta(83)
    xs, done = _lifetime_inputs(integer)
    tag = "i-save-" + ("int" if integer else "frac")
    res, run = gc.save_case(tag, N, W, T, F, seed=83, lay_eta=(lay, eta), inputs=(xs, done))
    _fwd6(run)
    gc.assert_within(tag, res)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "fractional"])
def test_multi_lifetime_inputs(integer):
    """i, per-candidate instance (the f32-MFMA augmented k-step), two candidates of 64 rows."""
    N, W, T, F = 2, 64, 6, 7
    etas = []
    for c in range(N):
        lay, e = _lifetime_eta(83 + c)
        etas.append(e)
    etas = torch.stack(etas)
    xs, done = _lifetime_inputs(integer)
    X = torch.from_numpy(xs[:, 0].copy()).cuda()
    tag = "i-multi-" + ("int" if integer else "frac")
    got = gc.run_multi(lay, etas, N * W, T, W, W, X, T * N * W, 1, done[0])
    gc.assert_within(tag, gc.table(tag, got, *gc.multi_refs(lay, etas, xs[:, 0], done[0], W)))


# ---------------------------------------------------------------------------------------------- j: f32 SAVE
@pytest.mark.parametrize("N,W,F", [(3, 32, 5), (3, 32, 7), (1, 32, 5), (1, 32, 7)])
def test_f32_save_instance(N, W, F):
    """j: k_gru_fwd<true,1> (R an odd multiple of 32): heads and the five saves, n included, in [256][M] rows."""
    tag = f"j-N{N}-F{F}"
    res, run = gc.save_case(tag, N, W, 6, F, seed=90 + N + F)
    assert not run.gru.slab and "n" in run.save_names() and any(k.startswith("n") for k in res)
    gc.assert_within(tag, res)


# ---------------------------------------------------------------------------------------------- k, l: per candidate
def _multi_case(C, W, T, F, seed):
    etas = []
    for c in range(C):
        lay, e = gc.make_eta(F, seed + c)
        etas.append(e)
    xs, done = gc.make_inputs(C, W, T, 1, F, seed)
    return lay, torch.stack(etas), xs[:, 0], done[0]


def test_f32_multi_instance():
    """k: k_gru_fwd<false,1> (rows_per_cand = 32): four candidates with their own parameters, each against its own
    float64."""
    C, W, T, F = 4, 32, 6, 7
    lay, etas, xs, done = _multi_case(C, W, T, F, 100)
    assert not torch.equal(etas[0], etas[1])
    got = gc.run_multi(lay, etas, C * W, T, W, 32, torch.from_numpy(xs).cuda(), T * C * W, 1, done)
    gc.assert_within("k", gc.table("k", got, *gc.multi_refs(lay, etas, xs, done, 32)))


def test_multi_stagger_grid():
    """l: k_gru_fwd6<false> on 18 workgroups, so workgroups 8-15 take the start-up stagger: per-candidate parity, and
    candidates 2 and 17 (undelayed workgroups) and 11 (a delayed one) rerun alone are bit-identical to their rows in
    the batch."""
    C, W, T, F = 18, 64, 3, 7
    lay, etas, xs, done = _multi_case(C, W, T, F, 110)
    got = gc.run_multi(lay, etas, C * W, T, W, W, torch.from_numpy(xs).cuda(), T * C * W, 1, done)
    gc.assert_within("l", gc.table("l", got, *gc.multi_refs(lay, etas, xs, done, W)))
    for c in (2, 11, 17):
        sl = slice(c * W, (c + 1) * W)
        xc = torch.from_numpy(np.ascontiguousarray(xs[:, :, sl])).cuda()
        alone = gc.run_multi(lay, etas[c:c + 1], W, T, W, W, xc, T * W, 1, done[c:c + 1])
        for name in gc.HEADS:
            assert np.isfinite(alone[name]).all()
            assert np.array_equal(alone[name], got[name][sl]), f"candidate {c} {name}: alone != in the batch"


# ---------------------------------------------------------------------------------------------- m: strides
def _strided(xs, xs_f, xs_col):
    """xs [F, T, R] laid out as X[f * xs_f + (t * R + r) * xs_col] in a NaN-filled device buffer."""
    F, T, R = xs.shape
    buf = np.full(F * xs_f, NAN, np.float32)
    for f in range(F):
        buf[f * xs_f:f * xs_f + T * R * xs_col:xs_col] = xs[f].reshape(-1)
    return torch.from_numpy(buf).cuda()


def test_input_strides():
    """m: xs_col = 2 and xs_f = 2 T R + 64 with NaN between the used elements: the SAVE instance's heads and saves and
    the per-candidate instance's heads are bit-identical to the dense-stride run of the same values (and finite: no
    unused element is read)."""
    N, W, T, F = 2, 64, 4, 5
    R = N * W
    xs_f, xs_col = 2 * T * R + 64, 2
    lay, eta = gc.make_eta(F, 120)
    xs, done = gc.make_inputs(N, W, T, 1, F, 120)
    Xs = _strided(xs[:, 0], xs_f, xs_col)
    outs = []
    for strided in (False, True):
        run = gc.SaveRun(lay, eta, N, W, T, 1, xs)
        _fwd6(run)
        if strided:
            run.gru.X.fill_(NAN)     # the strided run must not read the dense copy
            run.forward(0, done[0], X=Xs, xs_f=xs_f, xs_col=xs_col)
        else:
            run.forward(0, done[0], X=run.gru.X, xs_f=run.gru.M, xs_col=1)
        outs.append(run.outputs(0))
    r64, r32 = gc.refs(eta, F, xs[:, 0], done[0])
    gc.assert_within("m-save", gc.table("m-save", outs[1], r64, r32))
    for name in outs[0]:
        assert np.array_equal(outs[0][name], outs[1][name]), f"SAVE {name}: strided != dense"
    etas = torch.stack([eta, gc.make_eta(F, 121)[1]])
    dense = gc.run_multi(lay, etas, R, T, W, W, torch.from_numpy(xs[:, 0].copy()).cuda(), T * R, 1, done[0])
    strided = gc.run_multi(lay, etas, R, T, W, W, Xs, xs_f, xs_col, done[0])
    gc.assert_within("m-multi", gc.table("m-multi", strided, *gc.multi_refs(lay, etas, xs[:, 0], done[0], W)))
    for name in gc.HEADS:
        assert np.array_equal(dense[name], strided[name]), f"multi {name}: strided != dense"


# ---------------------------------------------------------------------------------------------- n: repeats
@pytest.mark.parametrize("N,W,F,fwd6", [(2, 64, 5, True), (3, 32, 7, False)], ids=["fwd6", "f32"])
def test_save_repeat_bit_identical(N, W, F, fwd6):
    """n, SAVE instances: two runs into NaN-prefilled outputs are bit-identical, every element written and finite."""
    T, K = 4, 2
    lay, eta = gc.make_eta(F, 130)
    xs, done = gc.make_inputs(N, W, T, K, F, 130)
    outs = []
    for _ in range(2):
        run = gc.SaveRun(lay, eta, N, W, T, K, xs)
        assert run.gru.slab == fwd6
        for k in range(K):
            run.forward(k, done[k])
        outs.append([run.outputs(k) for k in range(K)])
    for k in range(K):
        assert set(outs[0][k]) == set(gc.HEADS + run.save_names())
        for name, a in outs[0][k].items():
            assert np.isfinite(a).all(), (k, name)
            assert np.array_equal(a, outs[1][k][name]), f"update {k} {name}: differs between identical runs"


@pytest.mark.parametrize("C,W,rpc", [(3, 64, 64), (4, 32, 32)], ids=["fwd6", "f32"])
def test_multi_repeat_bit_identical(C, W, rpc):
    """n, per-candidate instances."""
    T, F = 4, 7
    lay, etas, xs, done = _multi_case(C, W, T, F, 140)
    X = torch.from_numpy(xs).cuda()
    a = gc.run_multi(lay, etas, C * W, T, W, rpc, X, T * C * W, 1, done)
    b = gc.run_multi(lay, etas, C * W, T, W, rpc, X, T * C * W, 1, done)
    for name in gc.HEADS:
        assert np.isfinite(a[name]).all()
        assert np.array_equal(a[name], b[name]), name


# ---------------------------------------------------------------------------------------------- argument checks
def test_fwd_multi_argument_checks():
    from toued import _lib
    L = _lib.lib()
    R, T, W, F = 128, 2, 64, 7
    lay, etas, xs, done = _multi_case(2, W, T, F, 150)
    ed = etas.cuda().contiguous()
    fwdA = torch.zeros(2, L.toued_gru_packed_floats(2), device="cuda")
    X = torch.from_numpy(xs).cuda()
    dn = torch.from_numpy(done).cuda()
    pi, y = torch.zeros(T, R, device="cuda"), torch.zeros(T, 8, R, device="cuda")
    P, st = _lib.ptr, _lib.stream_ptr()
    assert L.toued_gru_pack_fwd_multi(P(ed), lay.size, 2, lay.c_offsets, F, P(fwdA), st) == 0
    good = dict(R=R, T=T, W=W, F=F, rpc=64)

    def call(**kw):
        a = dict(good, **kw)
        return L.toued_gru_fwd_multi(a["R"], a["T"], a["W"], a["F"], a["rpc"], P(X), T * R, 1, P(dn), P(fwdA), P(ed),
                                     lay.size, lay.c_offsets, P(pi), P(y), st)

    assert call() == 0
    # rows_per_cand not dividing R; not a multiple of 32 (dividing R or not); no rows; the input widths outside 1..7
    bad = [dict(rpc=96), dict(rpc=16), dict(rpc=48), dict(rpc=0), dict(rpc=-64), dict(F=0), dict(F=8), dict(T=0),
           dict(R=96 + 16, rpc=16), dict(W=48)]
    for kw in bad:
        # a fresh error text per case: another entry point's failure in between
        assert L.toued_gae(1, 0, 1, None, None, None, 0.5, 0.5, None, None, st) == -1
        assert "toued_gae" in L.toued_last_error().decode()
        assert call(**kw) == -1, kw
        msg = L.toued_last_error().decode()
        assert msg and "toued_gru_fwd_multi" in msg, (kw, msg)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- TOUED_GRU_F32=1
def test_f32_fallback_process():
    """The documented fallback switch TOUED_GRU_F32=1 (read once per process: a fresh child, tests/gru_f32_worker.py):
    k_gru_fwd<true,2> on cases a and c (T = 3), heads and the five saves, and its repeat; k_gru_fwd<false,2> on two
    candidates; k_gru_bwd<1> at R % 64 == 0 with the non-block-floating-point weight-gradient reduction on one
    _gru_bwd_case of tests/test_gpu_meta.py at that file's f32 bound of 1e-4, and on cases a and c (T = 1) of the
    backward matrix (tests/test_gpu_gru_bwd.py case o) at tests/gru_bwd_cases.py's bound."""
    env = dict(os.environ, TOUED_GRU_F32="1")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "gru_f32_worker.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["gru_f32"] is True and res["bwd_col_exp_128"] == 0
    assert set(res["cases"]) == {"c-T3", "a", "multi"}
    for tag, tab in res["cases"].items():
        want = set(gc.HEADS) if tag == "multi" else set(gc.HEADS + ("h_in", "r", "z", "n", "hn"))
        assert set(tab) == want, (tag, sorted(tab))
        gc.assert_within(f"TOUED_GRU_F32=1 {tag}", {k: tuple(v) for k, v in tab.items()})
    assert res["repeat_bit_identical"] is True
    assert len(res["bwd"]) == 16, sorted(res["bwd"])
    bad = {k: v for k, v in res["bwd"].items() if not v < 1e-4}
    assert not bad, res["bwd"]
    assert res["bwd_matrix_instance"] == {"a": "k_gru_bwd<1>", "c-T1": "k_gru_bwd<1>"}
    for tag, tab in res["bwd_matrix"].items():
        assert {"dr_pre/kt", "dz_pre/r", "dhn", "dn_pre/r", "dh_heads", "relu_out", "dX3/r", "dX4/kt", "GI_in/row",
                "GI_heads/row", "hr_w/row", "in_w/row", "pi_b", "y_b"} <= set(tab), (tag, sorted(tab))
        import gru_bwd_cases as bc
        bc.assert_within(f"TOUED_GRU_F32=1 bwd {tag}", {k: tuple(v) for k, v in tab.items()})
