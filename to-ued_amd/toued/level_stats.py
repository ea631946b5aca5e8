"""Complexity metrics of a checkpointed level buffer.

    python -m toued.level_stats --checkpoint_dir D --env_mode M [--step S] [--diversity]

Restores the level buffer checkpoint that ``toued.train --checkpoint_dir D`` writes after S steps (the file
``D/buffer_<S>``, save_checkpoint's ``prefix="buffer_"``; the newest without --step) and prints one JSON object: the means of
``toued.env.level_stats`` over the buffer's levels -- the keys of --level_metrics' ``levels`` dict -- the number of
levels, and ``nearest_reward_hist``, the histogram of the distance to the nearest positive reward ("-1": the levels
without a reachable one).  ``--diversity`` adds ``unique_frac``, ``nn_dist`` and ``pair_dist``, the keys of
--buffer_diversity's ``buffer`` dict.
"""
from __future__ import annotations

import argparse
import json
import sys

import torch

from .checkpoint import level_buffer_from_state_dict, restore_checkpoint
from .env import get_env_spec, level_nearest, level_stats


def buffer_metrics(levels: torch.Tensor, spec) -> dict:
    """The JSON object of the module docstring for packed ``levels`` int32 [n, 80] on the device."""
    st = level_stats(levels, spec)
    f = lambda x: x.to(torch.float64)
    near = st.nearest_pos
    has = near >= 0
    free = (st.cells - st.n_walls).clamp(min=1)
    n = levels.shape[0]
    # the histogram over -1 .. max_grid^2 - 1 (a distance is below the number of cells)
    hist = torch.bincount((near + 1).long(), minlength=spec.g2 + 1).cpu().tolist()
    mean = lambda x: float(x.mean()) if n else float("nan")
    return {"n_levels": n, "solvable": mean(f(st.solvable == 1)), "n_walls": mean(f(st.n_walls)),
            "reachable_frac": mean(f(st.n_reach) / f(free)), "ecc": mean(f(st.ecc)),
            "nearest_reward_dist": float(f(near[has]).mean()) if bool(has.any()) else float("nan"),
            "nearest_reward_hist": {str(d - 1): c for d, c in enumerate(hist) if c}}


def diversity_metrics(levels: torch.Tensor) -> dict:
    """The diversity of packed ``levels`` int32 [B, 80] (B <= 65536) from one level_nearest launch of the levels
    against themselves, as 0-d float64 device tensors: ``unique_frac`` the share of rows that are the first of their
    identity class (row i counts when its nearest other row is at a distance > 0 or has a higher index), ``nn_dist``
    the mean distance to the nearest other row, ``pair_dist`` sum(dist_sum) / (B (B - 1)).  NaN where there is no
    pair (B < 2)."""
    B = levels.shape[0]
    nn = level_nearest(levels, levels, eligible="others")
    i = torch.arange(B, dtype=torch.int32, device=levels.device)
    first = (nn.dist > 0) | (nn.idx > i)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=levels.device)
    return {"unique_frac": first.to(torch.float64).mean() if B else nan,
            "nn_dist": nn.dist.to(torch.float64).mean() if B > 1 else nan,
            "pair_dist": nn.dist_sum.to(torch.float64).sum() / (B * (B - 1)) if B > 1 else nan}


def main(cmd_args=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint_dir", type=str, required=True)
    ap.add_argument("--env_mode", type=str, required=True)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--diversity", action="store_true",
                    help="add unique_frac, nn_dist and pair_dist (level_nearest of the buffer against itself)")
    a = ap.parse_args(cmd_args)
    spec, _, _ = get_env_spec(a.env_mode)
    state = restore_checkpoint(a.checkpoint_dir, prefix="buffer_", step=a.step)
    buf = level_buffer_from_state_dict(state, spec, torch.device("cuda", torch.cuda.current_device()))
    out = buffer_metrics(buf.levels, spec)
    if a.diversity:
        out.update({k: float(v) for k, v in diversity_metrics(buf.levels).items()})
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
