"""The meta-gradient step without a dense parameter history (TOUED_HIST_SPARSE, toued/meta.py): one live pair of agent
tables updated in place by toued_agent_step_snap, the reverse pass reading per-update row snapshots
(toued_entropy_clip_hvp_snap, toued_embed_bwd_snap), against the ring of K + 1 dense table pairs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
K, W = 3, 64


def _child(tmp_path, sparse, mode, T, N, nmb):
    out = tmp_path / f"hist_{sparse}.npz"
    env = dict(os.environ, TOUED_HIST_SPARSE=sparse)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "hist_sparse_worker.py"), mode, str(T), str(N), str(nmb),
                        str(out)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    facts = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return facts, dict(np.load(out))


# N = 3 agents (ordinary, discarded, single-cell: tests/hist_sparse_worker.py); --num_mini_batches 2 needs an even
# number of agents with the three of them in one chunk: N = 6, two chunks of 3
@pytest.mark.parametrize("mode,T,N,nmb", [
    pytest.param("tabular", 1, 3, 1, id="tabular-T1"), pytest.param("tabular", 3, 3, 1, id="tabular-T3"),
    pytest.param("debug", 1, 3, 1, id="debug-T1"), pytest.param("debug", 3, 3, 1, id="debug-T3"),
    pytest.param("tabular", 3, 6, 2, id="tabular-T3-two-mini-batches")])
def test_sparse_history_bit_identical_to_ring(tmp_path, mode, T, N, nmb):
    """Two consecutive meta-steps with level_sampler.sample() between them, TOUED_HIST_SPARSE=1 against =0, each in a
    child process: the meta-gradient (and its embedding block), eta, the Adam moments, the agents' theta, phi, step
    and env state, d_pi_hat, d_y_hat, gstat and every metric bit-identical after each step.  K = 3 updates of W = 64
    workers; the chunk the step's buffers hold has an agent whose first step's updates are all discarded (already at
    its lifetime), one whose samples all share one row (rewritten by every update) and an ordinary one."""
    f1, a1 = _child(tmp_path, "1", mode, T, N, nmb)
    f0, a0 = _child(tmp_path, "0", mode, T, N, nmb)
    assert f1["hist_sparse"] is True and f0["hist_sparse"] is False
    assert f1["n_chunks"] == f0["n_chunks"] == nmb
    assert f1["D"] == (5409 if mode == "tabular" else 65)
    for f in (f0, f1):
        loc = f["local"]
        assert min(loc.values()) >= 0
        applied = np.array(f["applied"])                     # [K][chunk agents]
        assert not applied[:, loc["discarded"]].any() and applied[:, loc["ordinary"]].all() \
            and applied[:, loc["single"]].all(), applied
        assert f["rows_single"] == 1 and f["rows_ordinary"] > 1, f
    assert set(a0) == set(a1) and len(a0) >= 2 * 19, sorted(a0)
    for name in sorted(a0):
        assert a0[name].dtype == a1[name].dtype and a0[name].shape == a1[name].shape, name
        assert a0[name].tobytes() == a1[name].tobytes(), name
    assert np.abs(a1["s1_grad"]).max() > 0 and np.isfinite(a1["s1_grad"]).all()


@pytest.mark.parametrize("D", [65, 5409])
def test_in_place_update_and_snapshots(D):
    """toued_agent_step_snap on aliased tables against toued_agent_step_entropy into separate tables (copies made
    beforehand) on the same inputs: the tables, gradient rows, metrics, steps and gstat bit-identical, and the
    snapshots equal to the old / new rows gathered on the host.  Three agents, T W = 192 samples: random rows with
    repeats (and the time row D - 1 among them), every sample on one row, and an update past the lifetime."""
    from toued import _lib
    from toued.env import L_LIFETIME, LEVEL_WORDS
    L, ptr = _lib, _lib.ptr
    N, T = 3, 3
    TW, R = T * W, N * W
    g = torch.Generator(device="cuda").manual_seed(D)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    theta, phi = rnd(N, D, 5), rnd(N, D, 8)
    tidx = torch.randint(0, min(D - 1, 40), (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
    tidx[0, 1, :5] = D - 1
    tidx[1, :T] = 7
    ttime = torch.randint(0, 50, (N, T + 1, W), device="cuda", generator=g, dtype=torch.int32)
    tact = torch.randint(0, 5, (N, T, W), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    trew = rnd(N, T, W)
    tdone = torch.zeros(N, T, W, dtype=torch.uint8, device="cuda")
    pi_hat = rnd(T, R)
    y_hat = torch.softmax(rnd(T, 8, R), dim=1).contiguous()
    levels = torch.zeros(N, LEVEL_WORDS, dtype=torch.int32, device="cuda")
    levels[:, L_LIFETIME] = 10
    step0 = torch.tensor([0, 3, 10], dtype=torch.int32, device="cuda")    # the third: step + 1 > lifetime
    z = lambda *s: torch.zeros(*s, device="cuda")
    hyp = (0.5, 40.0, 4.0, 0.5)
    st = L.stream_ptr()
    # reference: separate tables
    th1, ph1, Gth, Gph, met, gstat, step_a = theta.clone(), phi.clone(), z(N, D, 5), z(N, D, 8), z(N, 8), z(N, 4), \
        step0.clone()
    L.call("toued_agent_step_entropy", N, W, T, D, ptr(theta), ptr(phi), ptr(th1), ptr(ph1), ptr(tidx), ptr(ttime),
           ptr(tact), ptr(trew), ptr(tdone), ptr(pi_hat), ptr(y_hat), *hyp, ptr(Gth), ptr(Gph), ptr(met),
           ptr(step_a), ptr(levels), ptr(gstat), st)
    # in place
    thl, phl, Gth2, Gph2, met2, gstat2, step_b = theta.clone(), phi.clone(), z(N, D, 5), z(N, D, 8), z(N, 8), \
        z(N, 4), step0.clone()
    s_th0, s_ph0, s_l0 = z(N, TW, 5), z(N, TW + W, 8), z(N, 16)
    s_th1, s_ph1, s_l1 = z(N, TW, 5), z(N, TW, 8), z(N, 16)
    L.call("toued_agent_step_snap", N, W, T, D, ptr(thl), ptr(phl), ptr(tidx), ptr(ttime), ptr(tact), ptr(trew),
           ptr(tdone), ptr(pi_hat), ptr(y_hat), *hyp, ptr(Gth2), ptr(Gph2), ptr(met2), ptr(step_b), ptr(levels),
           ptr(gstat2), ptr(s_th0), ptr(s_ph0), ptr(s_l0), ptr(s_th1), ptr(s_ph1), ptr(s_l1), st)
    torch.cuda.synchronize()
    assert step_a.tolist() == [1, 4, 10]
    assert not torch.equal(th1[:2], theta[:2]) and torch.equal(th1[2], theta[2])
    for name, a, b in (("theta", th1, thl), ("phi", ph1, phl), ("Gth", Gth, Gth2), ("Gph", Gph, Gph2),
                       ("met", met, met2), ("gstat", gstat, gstat2), ("step", step_a, step_b)):
        assert torch.equal(a, b), name
    ix = tidx.long().reshape(N, (T + 1) * W)
    rows = lambda tab, n: torch.gather(tab, 1, ix[:, :n, None].expand(-1, -1, tab.shape[-1]))
    assert torch.equal(s_th0, rows(theta, TW)) and torch.equal(s_ph0, rows(phi, TW + W))
    assert torch.equal(s_th1, rows(th1, TW)) and torch.equal(s_ph1, rows(ph1, TW))
    for s_l, ta, tc in ((s_l0, theta, phi), (s_l1, th1, ph1)):
        assert torch.equal(s_l[:, :5], ta[:, D - 1]) and torch.equal(s_l[:, 8:], tc[:, D - 1])
