"""Worker for tests/test_gpu_maxmc_dist.py (launched via torch.distributed.run).

Runs `--meta_steps` outer iterations of the training driver (toued.train.Trainer) with --score_function max_mc on
this rank's agent slice, then one more level_sampler.sample in which the odd (global) agents are terminated, and
saves what a single-process run must reproduce: this rank's agents' levels, and the replicated buffer with its
max_return.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "to-ued_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--meta_steps", type=int, default=2)
    a, rest = ap.parse_known_args()
    from toued import prng
    from toued.dist import init_from_env
    from toued.env import L_LIFETIME
    from toued.parse_args import parse_args
    from toued.train import Trainer
    world = init_from_env()
    tr = Trainer(parse_args(rest), world)
    for _ in range(a.meta_steps):
        tr.meta_step()
    lo = 0 if tr.sl is None else tr.sl[0]
    gid = torch.arange(lo, lo + tr.agents.n, device=tr.agents.step.device)
    tr.agents.step = torch.where(gid % 2 == 1, tr.agents.levels[:, L_LIFETIME], tr.agents.step)
    ks = prng.split(tr.rng, 2)
    tr.buffer, tr.agents = tr.sampler.sample(ks[1].contiguous(), tr.buffer, tr.agents, tr.sl)
    torch.cuda.synchronize()
    b = tr.buffer
    np.savez(os.path.join(a.out, f"rank{world.rank}_of{world.size}.npz"), levels=tr.agents.levels.cpu().numpy(),
             buf_score=b.score.cpu().numpy(), buf_active=b.active.cpu().numpy(), buf_new=b.new.cpu().numpy(),
             buf_max_return=b.max_return.cpu().numpy(), last_score=tr.sampler.last_plr["score"].cpu().numpy())
    if world.active:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
