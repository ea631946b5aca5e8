"""--score_function max_mc with the agent axis sharded over two ranks (gloo collectives staged through the host, both
ranks on the box's GPU) against a single-process run: every rank's replicated buffer, its max_return included, must
come out as the single process's.  Each agent's score and level maximum depend on its own key, level, actor and
critic only, and the maxima of both ranks' agents reach every rank's buffer through the all-gather: the -inf pattern is
bit-exact and the values agree within the 1e-6 that tests/test_gpu_dist.py allows the scores (the LPG parameters the
actors were trained under differ by the meta-gradient all-reduce's summation order)."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

FLAGS = ["--env_mode", "mazes", "--num_agents", "4", "--num_mini_batches", "1", "--num_agent_updates", "2",
         "--score_function", "max_mc", "--buffer_size", "32"]


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, out):
    env = dict(os.environ, TOUED_DIST_BACKEND="gloo", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), str(ROOT / "tests" / "maxmc_dist_worker.py"),
           "--out", str(out)] + FLAGS
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(out / f"rank{i}_of{nproc}.npz")) for i in range(nproc)]


def test_two_ranks_keep_the_single_process_buffer(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    one = _run(1, tmp_path / "a")[0]
    two = _run(2, tmp_path / "b")
    assert np.array_equal(np.concatenate([t["levels"] for t in two]), one["levels"])
    known = np.isfinite(one["buf_max_return"])
    # the forced round scored agents 1 and 3, one on each rank: both slots' maxima are on every rank
    assert known.sum() >= 2 and (one["buf_max_return"][~known] == -np.inf).all()
    assert np.count_nonzero(one["last_score"]) >= 2
    for t in two:
        assert np.array_equal(t["buf_active"], one["buf_active"])
        assert np.array_equal(t["buf_new"], one["buf_new"])
        np.testing.assert_allclose(t["buf_score"], one["buf_score"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(t["last_score"], one["last_score"], rtol=0, atol=1e-6)
        assert np.array_equal(np.isfinite(t["buf_max_return"]), known)
        assert (t["buf_max_return"][~known] == -np.inf).all()
        np.testing.assert_allclose(t["buf_max_return"][known], one["buf_max_return"][known], rtol=0, atol=1e-6)
