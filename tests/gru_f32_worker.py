"""Worker for tests/test_gpu_gru_fwd.py::test_f32_fallback_process, started with TOUED_GRU_F32=1 in a fresh process
(the library reads the switch once).

Under the switch every GRU launch takes the f32-MFMA kernels: k_gru_fwd<true,2> / k_gru_fwd<false,2> at R % 64 == 0,
k_gru_bwd<1>, saves in [256][M] rows (n included) and the bf16-triple weight-gradient reduction instead of the
block-floating-point one.  Runs cases a and c (T = 3) of the forward matrix, heads and saves, one per-candidate run,
a repeat of case a and of the per-candidate run, one backward case of tests/test_gpu_meta.py, and cases a and c (T = 1)
of the backward matrix (tests/gru_bwd_cases.py, key "bwd_matrix"); prints one JSON line of achieved errors and bounds,
which the parent asserts on.
"""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT / "tests", ROOT / "to-ued_amd", ROOT):
    sys.path.insert(0, str(_p))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import gru_fwd_cases as gc
    from test_gpu_meta import _gru_bwd_case
    from toued import _lib
    L = _lib.lib()
    out = {"gru_f32": os.environ.get("TOUED_GRU_F32") == "1", "bwd_col_exp_128": int(L.toued_gru_bwd_col_exp(128)),
           "slab_saves_128": int(L.toued_gru_slab_saves(128)), "cases": {}}
    # the switch took effect: no lockstep split-precision kernel, no slab saves
    assert out["gru_f32"] and out["bwd_col_exp_128"] == 0 and out["slab_saves_128"] == 0, out
    runs = {}
    for tag, N, W, T, F in (("c-T3", 1, 64, 3, 5), ("a", 4, 32, 6, 5)):
        res, run = gc.save_case("F32=1 " + tag, N, W, T, F, seed=sum(map(ord, tag)))
        assert not run.gru.slab and not run.gru.bfp and not run.gru.fused
        out["cases"][tag] = res
        runs[tag] = run
    # the same inputs again: bit-identical
    _, again = gc.save_case("F32=1 a (repeat)", 4, 32, 6, 5, seed=ord("a"))
    a, b = runs["a"].outputs(0), again.outputs(0)
    out["repeat_bit_identical"] = all(np.array_equal(a[k], b[k]) for k in a)
    # per-candidate: two candidates of 64 rows
    C, W, T, F = 2, 64, 4, 7
    etas = []
    for c in range(C):
        lay, e = gc.make_eta(F, 160 + c)
        etas.append(e)
    etas = torch.stack(etas)
    xs, done = gc.make_inputs(C, W, T, 1, F, 160)
    X = torch.from_numpy(xs[:, 0].copy()).cuda()
    got = gc.run_multi(lay, etas, C * W, T, W, W, X, T * C * W, 1, done[0])
    rep = gc.run_multi(lay, etas, C * W, T, W, W, X, T * C * W, 1, done[0])
    out["repeat_bit_identical"] = out["repeat_bit_identical"] and all(np.array_equal(got[k], rep[k]) for k in got)
    out["cases"]["multi"] = gc.table("F32=1 multi", got, *gc.multi_refs(lay, etas, xs[:, 0], done[0], W))
    # backward: the (2, 64, 1.0, 1.0) inputs of test_gru_backward_matches_autograd
    from toued.lpg import init_lpg_params
    N, W, T, K, F = 2, 64, 6, 2, 5
    eta = init_lpg_params(5, F)
    eta += (torch.randn(eta.shape, generator=torch.Generator(device="cpu").manual_seed(0)) * 0.05).cuda()
    rs = np.random.RandomState(1)
    xs = rs.randn(F, K, T, N * W).astype(np.float32)
    done = (rs.rand(K, N, T, W) < 0.15).astype(np.uint8)
    d_pi = rs.randn(K, T, N * W).astype(np.float32)
    d_y = rs.randn(K, T, 8, N * W).astype(np.float32)
    errs, flips = _gru_bwd_case(N, W, T, K, F, eta, xs, done, d_pi, d_y)
    out["bwd"] = {k: float(v) for k, v in errs.items()}
    out["bwd_relu_flips"] = len(flips)
    # the backward matrix's cases a (4 x 32) and c (T = 1): k_gru_bwd<1> at R % 64 == 0, every output it writes
    import gru_bwd_cases as bc
    out["bwd_matrix"], out["bwd_matrix_instance"] = {}, {}
    for tag in ("a", "c-T1"):
        res, run, got, _ = bc.run_case(tag)
        assert {"dn_pre", "relu_out", "dh_heads"} <= set(got) and "col_exp" not in got
        out["bwd_matrix"][tag] = res
        out["bwd_matrix_instance"][tag] = bc.instance(run.gru)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
