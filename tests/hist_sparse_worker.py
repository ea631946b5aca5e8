"""Child process of tests/test_gpu_hist_sparse.py (TOUED_HIST_SPARSE is read when the step is built: one value per
process): two consecutive meta-steps with level_sampler.sample() between them (train.Trainer.meta_step) on a small
batch, everything the step leaves its caller written to an .npz, and one JSON line of what the run was.

    python tests/hist_sparse_worker.py ENV_MODE T N NUM_MINI_BATCHES OUT.npz

The last three agents are: an ordinary one, one already at its lifetime (every update of the first step is
discarded; the sampler then replaces it), and one whose policy puts all its mass on the no-op action, so that every
worker stays on the start cell: all its samples fall in one segment of the sorted row kernel and the same row is
rewritten by all K updates.
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "to-ued_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

W, K = 64, 3


def main():
    mode, T, N, nmb, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    args = parse_args(["--env_mode", mode, "--num_agents", str(N), "--num_mini_batches", str(nmb),
                       "--score_function", "random", "--env_workers", str(W), "--train_rollout_len", str(T),
                       "--num_agent_updates", str(K)])
    tr = Trainer(args)
    step, ag = tr.step_fn, tr.agents
    disc, single = N - 2, N - 1
    ag.step[disc] = ag.levels[disc, L_LIFETIME].to(ag.step.dtype)
    ag.theta[single] = 0.0
    ag.theta[single, :, 4] = 1000.0
    lo = N - step.N                      # the last chunk's first agent (the step's buffers hold the last chunk)
    arrays, facts = {}, {"hist_sparse": bool(step.hist_sparse), "n_chunks": step.n_chunks, "D": step.D}
    o = step.lay.offsets["e1_b"]
    for i in range(2):
        m = tr.meta_step()
        torch.cuda.synchronize()
        got = {"grad": step.grad, "embed_grad": step.grad[o:o + 161], "eta": tr.eta, "adam_m": tr.adam.m,
               "adam_v": tr.adam.v, "theta": tr.agents.theta, "phi": tr.agents.phi, "step": tr.agents.step,
               "state": tr.agents.state, "d_pi_hat": step.d_pi_hat, "d_y_hat": step.d_y_hat, "gstat": step.gstat}

        def flat(prefix, d):
            for k, v in d.items():
                if isinstance(v, dict):
                    flat(prefix + k + "_", v)
                else:
                    got[prefix + k] = v
        flat("metric_", m)
        for k, v in got.items():
            arrays[f"s{i}_{k}"] = v.detach().cpu().numpy().copy()
        if i == 0:
            gs = step.gstat.cpu().numpy()                     # [K][chunk agents][4]
            idx = step.traj.obs_idx[:K, :, :T].cpu().numpy()  # [K][chunk agents][T][W]
            facts["applied"] = gs[:, :, 2].tolist()
            facts["rows_single"] = int(np.unique(idx[:, single - lo]).size)
            facts["rows_ordinary"] = int(np.unique(idx[:, disc - 1 - lo]).size)
            facts["local"] = {"ordinary": disc - 1 - lo, "discarded": disc - lo, "single": single - lo}
    np.savez(out, **arrays)
    print(json.dumps(facts), flush=True)


if __name__ == "__main__":
    main()
