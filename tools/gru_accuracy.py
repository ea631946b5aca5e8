"""Accuracy of the LPG GRU forward against float64 (the f32-accuracy check of the bf16-split kernels).

    python tools/gru_accuracy.py            # default kernels
    TOUED_GRU_F32=1 python tools/gru_accuracy.py   # the f32-MFMA kernel, for comparison

Prints the max abs error of pi_hat, y_hat and the saved activations over T=20 steps of 4 agents x 64 workers
on random inputs (same construction as tests/test_gpu_meta.py::test_gru_forward_matches_oracle)."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))   # gru_ref: the float64 restatement the tests use

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from gru_ref import gru_forward_ref
    from oracle import lpg as olpg
    from toued.lpg import LPGGRU, LPGLayout, init_lpg_params
    N, W, T, K = 4, 64, 20, 1
    R = N * W
    lay = LPGLayout(5)
    eta = init_lpg_params(3, 5)
    eta += torch.randn_like(eta) * 0.05
    gru = LPGGRU(lay, R, T, K, W, "cuda")
    gru.pack(eta)
    rs = np.random.RandomState(0)
    X = gru.X
    X.copy_(torch.from_numpy(rs.randn(5, K, T, R).astype(np.float32)))
    done = (rs.rand(K, N, T, W) < 0.1).astype(np.uint8)
    pi_hat = torch.zeros(K, T, R, device="cuda")
    y_hat = torch.zeros(K, T, 8, R, device="cuda")
    gru.forward(0, X, torch.from_numpy(done[0]).cuda(), eta, pi_hat, y_hat)
    torch.cuda.synchronize()
    P = olpg.unflatten(torch.tensor(eta.cpu().numpy(), dtype=torch.float64), 5)
    x = torch.tensor(X[:, 0].cpu().numpy(), dtype=torch.float64).permute(2, 1, 0)
    d = torch.tensor(done[0].transpose(0, 2, 1).reshape(R, T).astype(bool))
    ref = gru_forward_ref(P, x, d, torch.float64)
    pi_ref, y_ref = ref["pi_hat"].numpy(), ref["y_hat"].numpy()
    hin_gpu = gru.hin_rows().cpu().numpy().reshape(256, T, R).transpose(2, 1, 0)
    hin_ref = ref["h_in"].numpy()
    res = {"kernel": "f32" if os.environ.get("TOUED_GRU_F32") == "1" else "default",
           "pi_hat_max_abs": float(np.abs(pi_hat[0].cpu().numpy().T - pi_ref).max()),
           "y_hat_max_abs": float(np.abs(y_hat[0].cpu().numpy().transpose(2, 0, 1) - y_ref).max()),
           "h_in_max_abs": float(np.abs(hin_gpu - hin_ref).max()),
           "pi_hat_scale": float(np.abs(pi_ref).max())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
