"""GPU parity of the LPG GRU backward (csrc/gru.hip) on every kernel instance and at its index edges, against the plain
float64 VJP tests/gru_ref.py gru_backward_ref.

Dispatch (LPGGRU.backward -> toued_gru_bwd_fused / toued_gru_bwd):

    R % 64 == 0, F <= 6, not TOUED_GRU_F32=1   k_gru_bwd6n<true>   (the default: small products fused, DG in slab blocks)
    fused=False, or F = 7 (R % 64 == 0)        k_gru_bwd6n<false> + toued_gru_bwd_small
    R % 64 != 0, or TOUED_GRU_F32=1            k_gru_bwd<1> + toued_gru_bwd_small, bf16-triple main reduction

Which case runs which instance:

    k_gru_bwd6n<true>    a b c d e f (F = 1, 4, 6) g s h i j k m n
    k_gru_bwd6n<false>   a b c d e f (F = 1, 4, 6, 7, lifetime inputs) g s h i j k m n
    k_gru_bwd<1>         h (N = 3, W = 32) l m n (toued_gru_bwd's checks come before the dispatch)
    k_gru_bwd<1> at R % 64 == 0: cases a and c (T = 1) in the TOUED_GRU_F32=1 child of
                         tests/test_gpu_gru_fwd.py::test_f32_fallback_process (tests/gru_f32_worker.py, key "bwd_matrix")

Every case runs pack, the K forwards and the backward through LPGGRU into outputs prefilled with NaN bits, asserts which
instance ran (gru.fused, gru.slab, gru.bfp), and checks every output the instance writes against float64: the gate
cotangents dr_pre, dz_pre, d(W_hn h + b_hn) (+ dn_pre, relu(h_out), the head cotangents where they reach memory), dX3,
dX4, GI's two blocks and the 14 parameter gradients, whole and per slice, at tests/gru_bwd_cases.py's bound
max(C, 4 e32); the split-precision instances also the exact col_exp contract (case i), from the device's own DG.
Case s (the recurrent weights times 4 and times 1e-3) is the wscale pair of tests/test_gpu_meta.py.  DESIGN.md §6
records a run.

Time runs as in the kernel: the forward scans t = T - 1 .. 0 (h_in(t) = h_out(t + 1)), the backward t ascending, so a
cotangent entering at step t reaches the steps t' >= t only, until a done flag at t' zeroes the carry.
"""
import numpy as np
import pytest
import torch

import gru_bwd_cases as bc

pytestmark = pytest.mark.gpu

FUSED, UNFUSED, F32 = "k_gru_bwd6n<true>", "k_gru_bwd6n<false>", "k_gru_bwd<1>"
BOTH = pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
PER_ROW = ("dr_pre", "dz_pre", "dhn", "dn_pre", "dh_heads", "dX3", "dX4")      # linear in the row's cotangents


def _inst(run, fused):
    """The instance the case is meant for ran (fused: True / False on the split-precision pair, None: k_gru_bwd<1>)."""
    gru = run.gru
    want = F32 if fused is None else FUSED if fused else UNFUSED
    assert bc.instance(gru) == want, (bc.instance(gru), want)
    assert (gru.fused, gru.slab, gru.bfp) == {FUSED: (True, True, True), UNFUSED: (False, True, True),
                                             F32: (False, False, False)}[want]
    return want


def _case(tag, fused, **kw):
    res, run, got, rr = bc.run_case(tag, fused=fused, **kw)
    _inst(run, fused)
    bc.assert_within(tag, res)
    return run, got, rr


def _same(tag, a, b, names=None):
    for name in names or [n for n in a if n != "grads"]:
        if name in a:
            assert np.isfinite(a[name].astype(np.float64)).all(), (tag, name)
            assert np.array_equal(a[name], b[name]), f"{tag}: {name} differs"


# ---------------------------------------------------------------------------------------------- a, b, c: shapes
@BOTH
@pytest.mark.parametrize("tag", ["a", "b", "c-T1", "c-T2", "c-T3"])
def test_shapes(tag, fused):
    """a (4 x 32: two agents per workgroup, one per 32-row tile) and b (2 x 96: the agent boundary between the two tiles
    of workgroup 1), every agent with its own done pattern; c: T = 1 (only prologue and epilogue of the step pipeline
    run, the contraction's result is never consumed: the outputs depend on the head cotangents alone), T = 2, 3."""
    run, got, _ = _case(tag, fused)
    if tag == "c-T1":
        assert run.T == 1


# ---------------------------------------------------------------------------------------------- d: update offsets
@BOTH
def test_update_offsets(fused):
    """d: K = 3 with a (K + 1)-slot done_all whose last slot is 0xFF; update 1's columns are bit-identical to a K = 1
    run of update 1's inputs alone; the C ABI with done_stride_k > N T W and 0xFF between the updates is bit-identical
    to the dense call."""
    lay, eta, xs, done, d_pi, d_y = bc.build("d")
    K, N, T, W = done.shape
    res, run, got, _ = bc.run_case("d", fused=fused, done_slots=K + 1)
    _inst(run, fused)
    assert run.done_all.shape[0] == K + 1 and bool((run.done_all[K] == 0xFF).all())
    bc.assert_within("d", res)
    alone = bc.BwdRun(lay, eta, xs[:, 1:2], done[1:2], d_pi[1:2], d_y[1:2], fused=fused).step_outputs()
    for name, a in alone.items():
        assert np.isfinite(a.astype(np.float64)).all()
        assert np.array_equal(a[0], got[name][1]), f"update 1's {name}: alone != inside the K = 3 run"
    dense = run.abi_backward(run.done_all, N * T * W).outputs()
    _same("d dense ABI call", dense, got)
    stride = N * T * W + 200
    buf = torch.full((K * stride,), 0xFF, dtype=torch.uint8, device="cuda")
    for k in range(K):
        buf[k * stride:k * stride + N * T * W] = run.done_all[k].reshape(-1)
    padded = run.abi_backward(buf, stride).outputs()
    _same("d done_stride_k", padded, dense)


# ---------------------------------------------------------------------------------------------- e: done patterns
@BOTH
@pytest.mark.parametrize("pattern", ["ones", "zeros", "first", "last"])
def test_done_patterns(pattern, fused):
    """e: all ones (no carry anywhere: every step depends on its own head cotangents alone), all zeros, ones only at
    t = 0 (the first carry of the backward is cut), ones only at t = T - 1 (the backward's last carry, which nothing
    consumes; the forward's h_in(T - 1) is 0 either way)."""
    _case(f"e-{pattern}", fused)


@BOTH
def test_done_cut_separates_the_sides(fused):
    """e: done = 1 for every row at the interior step t0.  The backward runs t ascending and zeroes the carry after step
    t0, so the upstream side is t <= t0: changing the head cotangents there leaves DG, dX and col_exp of the downstream
    side t > t0 bit-identical (and does change the upstream side); without the cut the same change reaches t > t0."""
    t0 = bc.CUT_T0
    for tag, cut in (("e-cut", True), ("e-zeros", False)):
        lay, eta, xs, done, d_pi, d_y = bc.build(tag)
        run = bc.BwdRun(lay, eta, xs, done, d_pi, d_y, fused=fused)
        _inst(run, fused)
        base = run.step_outputs()
        d_pi2, d_y2 = d_pi.copy(), d_y.copy()
        d_pi2[:, :t0 + 1] *= -1.5
        d_y2[:, :t0 + 1] = d_y2[:, :t0 + 1, ::-1]
        new = run.backward(d_pi2, d_y2).step_outputs()
        for name in base:
            if name == "relu_out":
                continue
            down = np.array_equal(base[name][:, :, t0 + 1:], new[name][:, :, t0 + 1:])
            if cut:
                assert down, f"{name}: steps t > {t0} changed with the cotangents of t <= {t0} across a done cut"
            if name != "col_exp":
                assert not np.array_equal(base[name][:, :, :t0 + 1], new[name][:, :, :t0 + 1]), name
                # (the head cotangents of a step depend on that step alone)
                assert cut or name == "dh_heads" or not down, f"{name}: no carry across t = {t0} without a done flag"


# ---------------------------------------------------------------------------------------------- f: input widths
@pytest.mark.parametrize("F,fused", [(1, True), (1, False), (4, True), (4, False), (6, True), (6, False), (7, False)])
def test_input_widths(F, fused):
    """f: F = 1, 4, 6 (fused and unfused) and F = 7 (LPGGRU takes the unfused split-precision kernel whatever it is
    asked): dX4 exactly 0 at F <= 4, dX3 exactly 0 at F <= 3 (the wi34 table zeroes the inputs the layout lacks), else
    against dx[..., 3], dx[..., 4]; in_w, ir_w, iz_w row by row (bc.table)."""
    lay, eta, xs, done, d_pi, d_y = bc.build(f"f-F{F}")
    assert lay.F == F
    res, run, got, (r64, _) = bc.run_case(f"f-F{F}", fused=True if F == 7 else fused)
    _inst(run, fused)
    bc.assert_within(f"f-F{F}", res)
    assert {f"{g}/row" for g in ("in_w", "ir_w", "iz_w")} <= set(res)
    assert (F <= 3) == (not got["dX3"].any()) and (F <= 4) == (not got["dX4"].any())
    assert got["grads"]["in_w"].shape == (F, 256)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "fractional"])
def test_lifetime_inputs(integer):
    """f, F = 7 with the forward matrix's lifetime inputs (step and lifetime up to 25000, cancelling weight rows): the
    x rows of the main reduction's A operand and the [x; 1] . dn^T product on their unbounded-input path."""
    tag = "f-life-" + ("int" if integer else "frac")
    run, got, _ = _case(tag, False)
    assert float(np.abs(np.asarray(run.gru.X[6].cpu())).max()) > 20000


# ---------------------------------------------------------------------------------------------- g: weight scales
@BOTH
@pytest.mark.parametrize("zero_gate", bc.GATES)
@pytest.mark.parametrize("variant", ["shared", "own"])
def test_backward_weight_scales(variant, zero_gate, fused):
    """g: k_bwd6_scales takes one exponent per input unit i over row i of all three gates, 14 - e clamped to [-30, 20]
    (2^-40 rows clamp at 20; with each gate its own factor the row maximum belongs to one gate and the others' pieces
    sit up to 42 binades below it), its zero-row branch (five rows of all three gates zero), and one whole gate zero."""
    _case(f"g-{variant}-{zero_gate}", fused)


@BOTH
@pytest.mark.parametrize("wscale", ["4", "0.001"])
def test_recurrent_weight_scale(wscale, fused):
    """The wscale inputs of tests/test_gpu_meta.py's test_gru_backward_matches_autograd (W_hr, W_hz, W_hn times 4: gates
    near saturation; times 1e-3: a carry that all but vanishes), here with every intermediate and per slice."""
    _case(f"s-{wscale}", fused)


# ---------------------------------------------------------------------------------------------- h: cotangent scales
H_CASES = pytest.mark.parametrize("tag,fused", [("h", True), ("h", False), ("h-f32", None)],
                                  ids=["fused", "unfused", "f32"])


def _row_exponents(R):
    """j(r) in [-12, 12], neighbouring rows of one 32-row tile far apart."""
    return ((np.arange(R) * 7) % 25 - 12).astype(np.int64)


@H_CASES
def test_cotangent_scale_homogeneity(tag, fused):
    """h: row r's d_pi and d_y times 2^j(r).  The VJP is linear in the row's cotangents, every scale on the path is a
    power of two and round-to-nearest is scale-free, so row r of DG, dn_pre, DH, dX3, dX4 equals the unscaled run's
    times 2^j(r) bit for bit and col_exp shifts by -j(r), as long as the row scale 14 - e stays inside [-40, 40]
    (checked from the float64 reference).  The scaled run itself is compared with float64 per row, each row against its
    own norm."""
    lay, eta, xs, done, d_pi, d_y = bc.build(tag)
    R = xs.shape[3]
    j = _row_exponents(R)
    s = np.ldexp(1.0, j).astype(np.float32)
    base = bc.BwdRun(lay, eta, xs, done, d_pi, d_y, fused=fused)
    _inst(base, fused)
    b = base.step_outputs()
    res, run, got, (r64, _) = bc.run_case(tag, fused=fused, inputs=(lay, eta, xs, done, d_pi * s, d_y * s),
                                          own_row_norm=True)
    bc.assert_within(tag + " scaled", res)
    m = np.max([np.abs(r64[n]).max(-1) for n in ("dr_pre", "dz_pre", "dhn")], 0)      # [K, R, T]
    assert (m > 0).all()
    e = np.frexp(m)[1]
    assert (14 - e >= -40).all() and (14 - e <= 40).all()
    for name in PER_ROW:
        if name in got:
            sc = s.astype(np.float64)[None, :, None] if got[name].ndim == 3 else s.astype(np.float64)[None, :, None, None]
            assert np.array_equal(got[name].astype(np.float64), b[name].astype(np.float64) * sc), \
                f"{name}: row r of the scaled run != 2^j(r) times the unscaled run"
    if "col_exp" in got:
        assert np.array_equal(got["col_exp"].astype(np.int64), b["col_exp"].astype(np.int64) - j[None, :, None])


@H_CASES
def test_zero_cotangents(tag, fused):
    """h: one whole agent with zero cotangents gives exactly-zero rows in every output and col_exp = 127 in its columns
    (the others still match float64); all-zero cotangents give every output exactly zero, GI and the flat gradient
    included."""
    lay, eta, xs, done, d_pi, d_y = bc.build(tag)
    W = done.shape[3]
    rows = slice(W, 2 * W)      # agent 1
    d_pi, d_y = d_pi.copy(), d_y.copy()
    d_pi[:, :, rows] = 0
    d_y[:, :, :, rows] = 0
    res, run, got, _ = bc.run_case(tag, fused=fused, inputs=(lay, eta, xs, done, d_pi, d_y))
    _inst(run, fused)
    bc.assert_within(tag + " zero agent", res)
    for name in PER_ROW:
        if name in got:
            assert not got[name][:, rows].any(), f"{name}: rows of the agent with zero cotangents"
            assert got[name].any()
    if "col_exp" in got:
        assert (got["col_exp"][:, rows] == 127).all() and (got["col_exp"][:, :W] != 127).all()
    got = run.backward(np.zeros_like(d_pi), np.zeros_like(d_y)).outputs()
    for name, a in list(got.items()) + list(got["grads"].items()):
        if name in ("grads", "relu_out"):
            continue
        if name == "col_exp":
            assert (a == 127).all()
        else:
            assert np.isfinite(a).all() and not a.any(), f"{name}: not exactly zero under all-zero cotangents"


@H_CASES
def test_one_hot_y_hat(tag, fused):
    """h: y_hat given to the backward as one-hot rows (1 and seven exact 0s): the softmax VJP y (dy - sum y dy) is
    exactly 0 in every row; the reference is fed the same y_hat."""
    lay, eta, xs, done, d_pi, d_y = bc.build(tag)
    F, K, T, R = xs.shape
    hot = np.random.RandomState(5).randint(0, 8, size=(K, T, R))
    y_hat = (np.arange(8)[None, None, :, None] == hot[:, :, None, :]).astype(np.float32)
    res, run, got, (r64, _) = bc.run_case(tag, fused=fused, y_hat=y_hat)
    _inst(run, fused)
    bc.assert_within(tag + " one-hot", res)
    assert not r64["dh_heads"][..., 1:].any()
    if "dh_heads" in got:
        assert not got["dh_heads"][..., 1:].any() and got["dh_heads"][..., 0].any()
    assert not got["grads"]["y_w"].any() and not got["grads"]["y_b"].any() and got["grads"]["pi_w"].any()


# ---------------------------------------------------------------------------------------------- j: row independence
@BOTH
def test_row_permutation(fused):
    """j: the workers of each agent permuted consistently in x, done and the cotangents (y_hat follows from the forward),
    by a permutation that moves rows across the two 32-row tiles and across the four-row groups of the transposed
    loads: DG, DH, RH, dX and col_exp rows come back permuted and bit-identical; the weight gradients stay within the
    bound of the unpermuted run's reference."""
    lay, eta, xs, done, d_pi, d_y = bc.build("j")
    K, N, T, W = done.shape
    res, run, got, (r64, r32) = bc.run_case("j", fused=fused)
    _inst(run, fused)
    bc.assert_within("j", res)
    p = (np.arange(W) * 37 + 11) % W
    assert sorted(p) == list(range(W)) and ((p < 32) != (np.arange(W) < 32)).any() and (p % 4 != np.arange(W) % 4).any()
    rp = (np.arange(N)[:, None] * W + p[None, :]).reshape(-1)      # new row a W + i holds old row a W + p[i]
    prun = bc.BwdRun(lay, eta, xs[..., rp], done[..., p], d_pi[..., rp], d_y[..., rp], fused=fused)
    pgot = prun.outputs()
    for name, a in pgot.items():
        if name in bc.STEP_OUTS + ("col_exp",):
            assert np.isfinite(a.astype(np.float64)).all()
            assert np.array_equal(a, got[name][:, rp]), f"{name}: permuted rows differ"
    tab = bc.table("j permuted", {k: pgot[k] for k in ("GI_in", "GI_heads", "grads")}, r64, r32, bc.contract(run.gru))
    bc.assert_within("j permuted", tab)


# ---------------------------------------------------------------------------------------------- k: many workgroups
def test_many_workgroups():
    """k: 33 x 64 rows, K = 2: 66 workgroups, so k_small_part / k_small_final run two chunks, the last of 2 workgroups.
    Fused GI and the flat gradient against float64 (with every other output); fused DG, col_exp and dX bit-identical to
    the unfused run."""
    from toued import _lib
    N, W, T, K, F, _ = bc.CASES["k"]
    n_wg = K * N * W // 64
    assert n_wg == 66 and _lib.lib().toued_gru_bwd_fused_work_floats(N * W, K) == (n_wg + 2) * (16 * 256 + 9 * 64)
    run, got, _ = _case("k", True)
    lay, eta, xs, done, d_pi, d_y = bc.build("k")
    un = bc.BwdRun(lay, eta, xs, done, d_pi, d_y, fused=False)
    _inst(un, False)
    _same("k fused vs unfused", got, un.step_outputs(), ("dr_pre", "dz_pre", "dhn", "col_exp", "dX3", "dX4"))


# ---------------------------------------------------------------------------------------------- l: f32 kernel
@pytest.mark.parametrize("tag", ["l-T1", "l-F7", "l-W96"])
def test_f32_instance(tag):
    """l: k_gru_bwd<1> at (N, W, T, F) = (1, 32, 1, 5), (3, 32, 4, 7), (1, 96, 3, 5): all five cotangent rows, RH, DH
    and every gradient."""
    run, got, _ = _case(tag, None)
    assert run.R % 64 and {"dr_pre", "dz_pre", "dhn", "dn_pre", "dh_heads", "relu_out"} <= set(got)
    assert "col_exp" not in got


# ---------------------------------------------------------------------------------------------- m: repeats
@pytest.mark.parametrize("tag,fused", [("m", True), ("m", False), ("m-f32", None)], ids=["fused", "unfused", "f32"])
def test_repeat_bit_identical(tag, fused):
    """m: two runs into NaN-prefilled outputs are bit-identical, every element written and finite."""
    run = bc.BwdRun(*bc.build(tag), fused=fused)
    _inst(run, fused)
    a = run.outputs()
    b = run.backward().outputs()
    _same(tag, a, b)
    _same(tag, a["grads"], b["grads"])
    assert len(a["grads"]) == 14 and all(v.any() for v in a["grads"].values())


# ---------------------------------------------------------------------------------------------- n: argument checks
def test_bwd_argument_checks():
    from toued import _lib
    from toued.lpg import LPGLayout
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    lay, eta, xs, done, d_pi, d_y = bc.build("c-T2")
    runs = {True: bc.BwdRun(lay, eta, xs, done, d_pi, d_y, fused=True, run=False),
            False: bc.BwdRun(lay, eta, xs, done, d_pi, d_y, fused=False, run=False)}
    _inst(runs[True], True)
    _inst(runs[False], False)
    lay7 = LPGLayout(7)

    def call(fused, **kw):
        run = runs[fused]
        gru, S = run.gru, run.gru.S
        a = dict(R=run.R, T=run.T, W=run.W, K=run.K, M=gru.M, off=lay.c_offsets, ce=P(gru.CE),
                 wn=gru.wg_work.numel())
        a.update(kw)
        common = (a["R"], a["T"], a["W"], a["K"], P(run.done_all), done[0].size, P(gru.bwdA), P(run.eta), a["off"],
                  P(run.y_hat), P(run.d_pi), P(run.d_y), P(gru.A), P(S[0]), P(S[1]))
        if fused:
            return L.toued_gru_bwd_fused(*common, P(S[3]), a["M"], P(gru.DG), P(gru.dX3), P(gru.dX4), a["ce"], P(gru.GI),
                                         P(gru.wg_work), a["wn"], st)
        return L.toued_gru_bwd(*common, P(S[2]), P(S[3]), a["M"], P(gru.DG), P(gru.RH), P(gru.DH), P(gru.dX3),
                               P(gru.dX4), a["ce"], st)

    assert call(True) == 0 and call(False) == 0
    need = L.toued_gru_bwd_fused_work_floats(64, 1)
    assert runs[True].gru.wg_work.numel() >= need
    bad = [(False, "toued_gru_bwd", dict(R=48)), (False, "toued_gru_bwd", dict(W=48)),
           (False, "toued_gru_bwd", dict(R=16, W=16)),
           (True, "toued_gru_bwd_fused", dict(R=96, W=32)), (True, "toued_gru_bwd_fused", dict(M=2 * 64 + 32)),
           (True, "toued_gru_bwd_fused", dict(wn=need - 1)), (True, "toued_gru_bwd_fused", dict(ce=None)),
           (True, "toued_gru_bwd_fused", dict(off=lay7.c_offsets))]
    for fused, entry, kw in bad:
        # a fresh error text per case: another entry point's failure in between
        assert L.toued_gae(1, 0, 1, None, None, None, 0.5, 0.5, None, None, st) == -1
        assert "toued_gae" in L.toued_last_error().decode()
        assert call(fused, **kw) == -1, kw
        msg = L.toued_last_error().decode()
        assert msg and entry in msg and (entry == "toued_gru_bwd_fused" or "toued_gru_bwd_fused" not in msg), (kw, msg)
    torch.cuda.synchronize()
