"""RolloutWrapper on MI355X (environments/rollout.py:13-102), vmapped over agents.

The reference's ``RolloutWrapper`` works on one agent and is vmapped by its
callers (agents/a2c.py:98, agents/lpg_agent.py:109, meta/train.py:48,
agents/agents.py:101-105, level_sampler.py:276).  Here the agent axis is
explicit: every call takes N agent keys, N packed levels and N actor tables,
and runs one fused HIP launch (csrc/env.hip k_rollout).  Called with the reference's
single-agent arguments instead -- one key ``rng`` of shape [2], one level, one actor table
``[D, 5]`` -- ``batch_reset``/``batch_rollout`` run that one agent and return its results
without the agent axis, as ``RolloutWrapper.batch_reset(rng, env_params, num_workers)`` and
``batch_rollout(rng, train_state, env_params, init_obs, init_state)`` do.
"""
from __future__ import annotations

import os

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .env import STATE_FIELDS, EnvSpec, get_env_spec


@dataclass
class Transition:
    """util/data.py:37-44 in compact, lane-contiguous layout.

    obs_idx/obs_time: int32 [N, T+1, W] (obs_t for t<T; slot T is the end obs,
    so next_obs_t == obs_{t+1}); action/done: uint8 [N, T, W]; reward: f32 [N, T, W].
    """
    obs_idx: torch.Tensor
    obs_time: torch.Tensor
    action: torch.Tensor
    reward: torch.Tensor
    done: torch.Tensor


class PolicyOccupancy(NamedTuple):
    """RolloutWrapper.policy_occupancy's result: toued_policy_occupancy's eight summary columns, f32 [n] each (views
    of one [n, 8] tensor), then ``visits`` f32 [n, S], ``collected`` f32 [n, max_n_objs] and ``occ_all`` (None, or
    f32 [n, max_rollout_len, S])."""
    ret: torch.Tensor                 # sum d pi r = V^pi_0(start), policy_return's value from the other side
    length: torch.Tensor              # the expected number of steps of the first episode
    p_early_term: torch.Tensor        # the probability that it ends by termination, not by the time limit
    alive_end: torch.Tensor           # the probability that it is still running after the last step
    entropy: torch.Tensor             # mean over the visited steps of the policy's entropy over log 5
    least_confidence: torch.Tensor    # ... of 1 - max pi
    min_margin: torch.Tensor          # ... of 1 - (max pi - second-largest pi)
    ret_abs: torch.Tensor             # sum d pi |r|, the error scale of ``ret``
    visits: torch.Tensor
    collected: torch.Tensor
    occ_all: torch.Tensor | None


class EpisodeStats(NamedTuple):
    """RolloutWrapper.episode_stats's result: toued_episode_stats's six columns, f64 [N] each (views of one [N, 6]
    tensor, ``table``, which a later call can be given as ``out`` to go on adding to it)."""
    episodes: torch.Tensor        # episodes completed
    ret_sum: torch.Tensor         # sum of their undiscounted returns
    ret_sq_sum: torch.Tensor      # sum of their squared returns
    len_sum: torch.Tensor         # sum of their lengths
    reward_sum: torch.Tensor      # sum of all rewards, finished episode or not
    steps: torch.Tensor           # (worker, step) pairs seen

    @property
    def table(self) -> torch.Tensor:
        e = self.episodes
        if e.dim() == 1 and (e.shape[0] <= 1 or e.stride(0) == 6):      # a column of the [N, 6] table it came from
            return e.as_strided((e.shape[0], 6), (6, 1), e.storage_offset())
        return torch.stack(tuple(self), dim=1)


def _check_transition(name: str, transition: Transition):
    """(N, T, W) of a trajectory that the score kernels read, its shapes checked against one another."""
    N, T, W = transition.reward.shape
    if transition.obs_idx.shape != (N, T + 1, W) or transition.obs_time.shape != (N, T + 1, W) \
            or transition.done.shape != (N, T, W):
        raise ValueError(f"{name}: obs_idx {tuple(transition.obs_idx.shape)}, reward "
                         f"{tuple(transition.reward.shape)}, done {tuple(transition.done.shape)}")
    return N, T, W


def _critic_rows(vcrit: torch.Tensor, N: int) -> torch.Tensor:
    """The value critics as contiguous rows [N, D], from [N, D] or the critic table [N, D, 1]."""
    return vcrit.reshape(N, vcrit.shape[1]).contiguous()


def split_rollouts() -> bool:
    """Train rollouts as draws + env chain (toued_rollout_draws / toued_rollout_env) unless TOUED_ROLLOUT_FUSED=1
    (the single-kernel toued_rollout; bit-identical)."""
    return os.environ.get("TOUED_ROLLOUT_FUSED") != "1"


class RolloutWrapper:
    def __init__(self, env_mode: str, train_rollout_len: int, eval_rollout_len: int | None = None,
                 env_workers: int = 64):
        self.env_mode = env_mode
        self.spec, max_len, _ = get_env_spec(env_mode)
        self.train_rollout_len = train_rollout_len
        self.eval_rollout_len = max_len if eval_rollout_len is None else eval_rollout_len
        self.env_workers = env_workers
        self._c = _lib.env_spec_c(self.spec)

    @property
    def obs_dim(self) -> int:
        return self.spec.obs_dim

    def batch_reset(self, agent_keys: torch.Tensor, levels: torch.Tensor, num_workers: int | None = None):
        """rollout.py:38-42 per agent: split(rng, W); vmap(env.reset).  Returns ((idx, time) [N*W], state).
        A single key [2] and level resets that one agent's W workers (the reference's unvmapped call)."""
        if agent_keys.dim() == 1:
            return self.batch_reset(agent_keys.view(1, 2), levels.view(1, -1), num_workers)
        W = self.env_workers if num_workers is None else num_workers
        N = agent_keys.shape[0]
        dev = agent_keys.device
        n = N * W
        # zeroed: the kernel writes the mode's fields only (object slots past max_n_objs stay 0, not stale memory)
        state = torch.zeros((STATE_FIELDS, n), dtype=torch.int32, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        tm = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("toued_batch_reset", self._c, _lib.ptr(levels), _lib.ptr(agent_keys.contiguous()), N, W,
                  _lib.ptr(state), _lib.ptr(idx), _lib.ptr(tm), _lib.stream_ptr())
        return (idx, tm), state

    def batch_reset_into(self, agent_keys: torch.Tensor, levels: torch.Tensor, state: torch.Tensor,
                         mask: torch.Tensor):
        """``batch_reset`` in place into ``state`` [fields, N*W] for the agents with ``mask`` (u8 [N]) set."""
        N = agent_keys.shape[0]
        W = state.shape[1] // N
        n = N * W
        if getattr(self, "_obs_scratch", None) is None or self._obs_scratch.shape[1] < n:
            self._obs_scratch = torch.empty((2, n), dtype=torch.int32, device=state.device)
        _lib.call("toued_batch_reset_masked", self._c, _lib.ptr(levels), _lib.ptr(agent_keys.contiguous()), N, W,
                  _lib.ptr(state), _lib.ptr(self._obs_scratch[0]), _lib.ptr(self._obs_scratch[1]), _lib.ptr(mask),
                  _lib.stream_ptr())
        return state

    def batch_rollout(self, agent_keys: torch.Tensor, theta: torch.Tensor, levels: torch.Tensor,
                      state: torch.Tensor, eval: bool = False, out: Transition | None = None,
                      inplace_state: bool = False):
        """rollout.py:45-102.  theta: actor tables f32 [N, D, 5].

        Returns (Transition, end_state, cum_return f32 [N, W]).  With a single key [2] (one level, theta [D, 5]):
        the reference's single-agent batch_rollout, results without the agent axis (cum_return [W]).
        """
        if agent_keys.dim() == 1:
            o = None if out is None else Transition(*(x.unsqueeze(0) for x in (out.obs_idx, out.obs_time, out.action,
                                                                              out.reward, out.done)))
            tr, st, cum = self.batch_rollout(agent_keys.view(1, 2), theta.unsqueeze(0), levels.view(1, -1), state,
                                             eval=eval, out=o, inplace_state=inplace_state)
            return Transition(tr.obs_idx[0], tr.obs_time[0], tr.action[0], tr.reward[0], tr.done[0]), st, cum[0]
        N = agent_keys.shape[0]
        n = state.shape[1]
        W = n // N
        T = self.eval_rollout_len if eval else self.train_rollout_len
        D = theta.shape[1]
        dev = state.device
        if not inplace_state:
            state = state.clone()
        if out is None:
            out = Transition(
                torch.empty((N, T + 1, W), dtype=torch.int32, device=dev),
                torch.empty((N, T + 1, W), dtype=torch.int32, device=dev),
                torch.empty((N, T, W), dtype=torch.uint8, device=dev),
                torch.empty((N, T, W), dtype=torch.float32, device=dev),
                torch.empty((N, T, W), dtype=torch.uint8, device=dev),
            )
        cum = torch.empty((N, W), dtype=torch.float32, device=dev)
        if eval or not split_rollouts():
            _lib.call("toued_rollout", self._c, _lib.ptr(levels), _lib.ptr(theta), D,
                      _lib.ptr(agent_keys.contiguous()), _lib.ptr(state), N, W, T, _lib.ptr(out.obs_idx),
                      _lib.ptr(out.obs_time), _lib.ptr(out.action), _lib.ptr(out.reward), _lib.ptr(out.done),
                      _lib.ptr(cum), _lib.stream_ptr())
            return out, state, cum
        draws = self.train_draws(agent_keys.view(1, N, 2), levels, W)
        self.rollout_from_draws(draws, 0, theta, levels, state, out, cum)
        return out, state, cum

    def train_draws(self, keys: torch.Tensor, levels: torch.Tensor, n_workers: int,
                    bufs: tuple[torch.Tensor, torch.Tensor] | None = None, stream: int | None = None) -> torch.Tensor:
        """The state-independent draws of U batches of train rollouts (toued_rollout_draws): keys [U, N, 2] (batch u's
        rollout keys), levels [N, words].  Returns u32 [T, U * N * W, 4]: in ``bufs`` = (chain scratch, draws), each
        at least [T, U * N * W, 4] (the step stride is theirs), or in a buffer of this wrapper reused by the next
        call of the same shape.  ``stream``: a raw HIP stream to launch on (default: torch's current stream)."""
        U, N = keys.shape[0], keys.shape[1]
        T, W = self.train_rollout_len, n_workers
        n = U * N * W
        if bufs is not None:
            chain, draws = bufs
            if chain.shape[0] < T or chain.shape[1] < n or draws.shape != chain.shape:
                raise ValueError(f"train_draws: buffers {tuple(chain.shape)} for T={T}, {n} workers")
            n = chain.shape[1]
        else:
            key = (T, n, str(levels.device))
            if getattr(self, "_draw_bufs", None) is None or self._draw_bufs[0] != key:
                self._draw_bufs = (key, torch.empty((T, n, 4), dtype=torch.int32, device=levels.device),
                                   torch.empty((T, n, 4), dtype=torch.int32, device=levels.device))
            _, chain, draws = self._draw_bufs
        if n != U * N * W:
            raise ValueError("train_draws: the buffers' worker stride must equal U * N * W")
        _lib.call("toued_rollout_draws", self._c, _lib.ptr(levels), _lib.ptr(keys.contiguous()), N, U, W, T,
                  _lib.ptr(chain), _lib.ptr(draws), stream if stream is not None else _lib.stream_ptr())
        return draws

    def rollout_from_draws(self, draws: torch.Tensor, u: int, theta: torch.Tensor, levels: torch.Tensor,
                           state: torch.Tensor, out: Transition, cum: torch.Tensor | None = None):
        """Batch u of train_draws' rollouts (toued_rollout_env): trajectories into ``out``, ``state`` advanced in place;
        bit-identical to toued_rollout with the same keys."""
        N = theta.shape[0]
        n = state.shape[1]
        T = self.train_rollout_len
        _lib.call("toued_rollout_env", self._c, _lib.ptr(levels), _lib.ptr(theta), theta.shape[1], _lib.ptr(state), N,
                  n // N, T, _lib.ptr(draws) + 16 * u * n, draws.shape[1], _lib.ptr(out.obs_idx),
                  _lib.ptr(out.obs_time), _lib.ptr(out.action), _lib.ptr(out.reward), _lib.ptr(out.done),
                  _lib.ptr(cum) if cum is not None else None, _lib.stream_ptr())

    def eval_draws(self, agent_keys: torch.Tensor, levels: torch.Tensor, n_workers: int,
                   buf: torch.Tensor | None = None) -> torch.Tensor:
        """The state-independent draws of an eval-length returns-only rollout (toued_eval_keys, toued_eval_draws):
        u32 [T, N*W, 4], consumed by eval_returns_from_draws.  They depend on the keys and levels only, so they can
        be produced early, beside other work."""
        N = agent_keys.shape[0]
        n, T = N * n_workers, self.eval_rollout_len
        dev = levels.device
        chain = torch.empty((T, n, 4), dtype=torch.int32, device=dev)
        if buf is None or buf.shape != (T, n, 4):
            buf = torch.empty((T, n, 4), dtype=torch.int32, device=dev)
        st = _lib.stream_ptr()
        _lib.call("toued_eval_keys", _lib.ptr(agent_keys.contiguous()), N, n_workers, T, _lib.ptr(chain), st)
        _lib.call("toued_eval_draws", self._c, _lib.ptr(levels), N, n_workers, T, _lib.ptr(chain), _lib.ptr(buf), st)
        return buf

    def eval_returns_from_draws(self, draws: torch.Tensor, theta: torch.Tensor, levels: torch.Tensor,
                                state: torch.Tensor) -> torch.Tensor:
        """eval_returns on draws from eval_draws (same keys, levels and worker count): bit-identical.
        Returns f32 [N, W]."""
        N = theta.shape[0]
        n = state.shape[1]
        cum = torch.empty((N, n // N), dtype=torch.float32, device=state.device)
        _lib.call("toued_eval_returns", self._c, _lib.ptr(levels), _lib.ptr(theta), theta.shape[1], _lib.ptr(state),
                  N, n // N, self.eval_rollout_len, _lib.ptr(draws), _lib.ptr(cum), _lib.stream_ptr())
        return cum

    def optimal_return(self, levels: torch.Tensor, max_rollout_len: int, return_all: bool = False) -> torch.Tensor:
        """rollout.py:104-108: vmap(GridWorld.optimal_return) (gridworld.py:253-323), the exact optimal expected
        return of tabular levels over ``max_rollout_len`` steps (toued_optimal_return, no host synchronisation).

        levels int32 [n, 80] -> f32 [n]: v_0 at the start state.  ``return_all``: f32 [n, max_rollout_len, S] with
        S = obs_dim - 1 table states (the reference's shape: the observation's last entry is the time feature, not
        a state), v_t of every tabular state, -inf at the invalid ones and 0 from max_steps_in_episode on.  A single
        level [80] returns a 0-d tensor, or [max_rollout_len, S].  Non-tabular modes raise NotImplementedError."""
        return self._exact_returns("optimal_return", "Optimal return", levels, None, max_rollout_len, return_all, 1)[0]

    def policy_return(self, levels: torch.Tensor, theta: torch.Tensor, max_rollout_len: int,
                      return_all: bool = False) -> torch.Tensor:
        """The exact expected return of tabular agents' own policies over ``max_rollout_len`` steps
        (toued_policy_return, no host synchronisation): ``optimal_return``'s recursion with the expectation over the
        actor's softmax policy in place of the max.  With ``max_rollout_len = eval_rollout_len`` it is the expectation
        of ``eval_agent``'s per-worker return.  Not in the reference.

        levels int32 [n, 80], theta f32 [n, obs_dim, 5] -> f32 [n]; ``return_all``: f32 [n, max_rollout_len, S] with
        S = obs_dim - 1, the masks of ``optimal_return``'s table.  A single level [80] with theta [obs_dim, 5] returns
        a 0-d tensor, or [max_rollout_len, S].  Non-tabular modes raise NotImplementedError."""
        return self._exact_returns("policy_return", "Policy return", levels, theta, max_rollout_len, return_all, 1)[0]

    def policy_return_moments(self, levels: torch.Tensor, theta: torch.Tensor, max_rollout_len: int,
                              return_all: bool = False):
        """(mean, variance) of the first-episode return of tabular agents' own policies over ``max_rollout_len``
        steps (toued_policy_return_moments, one launch, no host synchronisation): ``policy_return``'s recursion with a
        second table for Var[G_t | s], by the law of total variance.  The mean is ``policy_return``'s, bit for bit.
        The variance is over everything an eval rollout draws, the policy's actions and the level's termination and
        respawn draws; with ``max_rollout_len = eval_rollout_len`` it is the variance of ``eval_agent``'s per-worker
        return.  It is not clamped: a zero variance may come out a rounding below zero.  Not in the reference.

        Shapes, the single-agent form and the errors are ``policy_return``'s, for each of the two results."""
        return tuple(self._exact_returns("policy_return_moments", "Policy return moments", levels, theta,
                                         max_rollout_len, return_all, 2))

    def _exact_returns(self, name: str, title: str, levels: torch.Tensor, theta: torch.Tensor | None,
                       max_rollout_len: int, return_all: bool, n_out: int) -> list:
        """optimal_return (``theta`` None), policy_return and policy_return_moments through their entry point
        toued_<name>: the tabular check, the single-level form, theta's validation, the outputs and the call.  The
        ``n_out`` results: v_0 (then var_0) f32 [n], or with ``return_all`` the tables f32 [n, max_rollout_len, S]."""
        if not self.spec.tabular:
            raise NotImplementedError(f"{title} not implemented for non-tabular environments.")
        if levels.dim() == 1:
            outs = self._exact_returns(name, title, levels.view(1, -1), None if theta is None else theta.unsqueeze(0),
                                       max_rollout_len, return_all, n_out)
            return [o[0] for o in outs]
        n, L = levels.shape[0], int(max_rollout_len)
        if theta is not None and (tuple(theta.shape) != (n, self.obs_dim, 5) or theta.dtype != torch.float32
                                  or theta.device != levels.device):
            raise ValueError(f"{name}: theta {theta.dtype} {tuple(theta.shape)} on {theta.device}, expected "
                             f"float32 {(n, self.obs_dim, 5)} on {levels.device}")
        S = self.obs_dim - 1
        v0 = [torch.zeros(n, dtype=torch.float32, device=levels.device) for _ in range(n_out)]
        v_all = [torch.empty((n, L, S), dtype=torch.float32, device=levels.device) if return_all else None
                 for _ in range(n_out)]
        th, d = ([], []) if theta is None else ([_lib.ptr(theta)], [self.obs_dim])     # the arguments a theta adds
        _lib.call("toued_" + name, _lib.ptr(levels), *th, n, *d, self.spec.max_grid_size, self.spec.max_n_objs,
                  int(self.spec.tabular), L, *map(_lib.ptr, v0), *map(_lib.ptr, v_all), _lib.stream_ptr())
        return v_all if return_all else v0

    def policy_occupancy(self, levels: torch.Tensor, theta: torch.Tensor, max_rollout_len: int,
                         return_all: bool = False) -> PolicyOccupancy:
        """The exact state occupancy of tabular agents' own policies over ``max_rollout_len`` steps
        (toued_policy_occupancy, one launch, no host synchronisation): d_t(s), the probability that the agent's first
        episode is still running at step t and is in state s, pushed forward from the start state under
        ``policy_return``'s policy, and what follows from it (``PolicyOccupancy``): the return from the other side,
        the episode's expected length and how it ends, the three policy scores as averages over the visited steps,
        every state's expected visits and every object's expected collections.  Deterministic, key-free, and a level's
        result does not depend on its batch.  Not in the reference.

        levels int32 [n, 80], theta f32 [n, obs_dim, 5] -> the summary fields f32 [n], ``visits`` f32 [n, S] with
        S = obs_dim - 1 (0 at the invalid states), ``collected`` f32 [n, max_n_objs] and ``occ_all``, None or with
        ``return_all`` f32 [n, max_rollout_len, S] (rows from max_steps_in_episode on are 0).  A single level [80]
        with theta [obs_dim, 5] returns every field without the leading axis.  Non-tabular modes raise
        NotImplementedError."""
        if not self.spec.tabular:
            raise NotImplementedError("Policy occupancy not implemented for non-tabular environments.")
        if levels.dim() == 1:
            out = self.policy_occupancy(levels.view(1, -1), theta.unsqueeze(0), max_rollout_len, return_all)
            return PolicyOccupancy(*(None if o is None else o[0] for o in out))
        n, L = levels.shape[0], int(max_rollout_len)
        if tuple(theta.shape) != (n, self.obs_dim, 5) or theta.dtype != torch.float32 or theta.device != levels.device:
            raise ValueError(f"policy_occupancy: theta {theta.dtype} {tuple(theta.shape)} on {theta.device}, expected "
                             f"float32 {(n, self.obs_dim, 5)} on {levels.device}")
        S, dev = self.obs_dim - 1, levels.device
        summary = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        visits = torch.zeros((n, S), dtype=torch.float32, device=dev)
        collected = torch.zeros((n, self.spec.max_n_objs), dtype=torch.float32, device=dev)
        occ_all = torch.empty((n, L, S), dtype=torch.float32, device=dev) if return_all else None
        _lib.call("toued_policy_occupancy", _lib.ptr(levels), _lib.ptr(theta), n, self.obs_dim,
                  self.spec.max_grid_size, self.spec.max_n_objs, int(self.spec.tabular), L, _lib.ptr(summary),
                  _lib.ptr(visits), _lib.ptr(collected), _lib.ptr(occ_all), _lib.stream_ptr())
        return PolicyOccupancy(*summary.unbind(dim=1), visits, collected, occ_all)

    def value_loss_scores(self, transition: Transition, vcrit: torch.Tensor, gamma: float, gae_lambda: float,
                          return_adv: bool = False):
        """The value-loss PLR scores of N agents' trajectories under their value critics ``vcrit`` f32 [N, D]
        (toued_value_loss_scores: value gather, GAE and both means in one launch, no host synchronisation):
        (positive value loss, L1 value loss), f32 [N] each, the means over workers and steps of max(GAE, 0) and |GAE|
        with the value of meta/train.py:61-100 and the scan of util/metrics.py:17-38.  ``return_adv``: also the
        advantages f32 [N, T, W], bit-identical to toued.metrics.gae on the gathered values."""
        N, T, W = _check_transition("value_loss_scores", transition)
        vcrit = _critic_rows(vcrit, N)
        dev = transition.reward.device
        pvl = torch.empty(N, dtype=torch.float32, device=dev)
        l1 = torch.empty(N, dtype=torch.float32, device=dev)
        adv = torch.empty((N, T, W), dtype=torch.float32, device=dev) if return_adv else None
        # discount * gae_lambda is a python-float product in the reference (weak-typed, rounded to f32 once)
        gl = float(np.float32(float(gamma) * float(gae_lambda)))
        _lib.call("toued_value_loss_scores", N, W, T, vcrit.shape[1], _lib.ptr(vcrit), _lib.ptr(transition.obs_idx),
                  _lib.ptr(transition.obs_time), _lib.ptr(transition.reward), _lib.ptr(transition.done), float(gamma),
                  gl, _lib.ptr(pvl), _lib.ptr(l1), _lib.ptr(adv), _lib.stream_ptr())
        return (pvl, l1, adv) if return_adv else (pvl, l1)

    def max_mc_scores(self, transition: Transition, vcrit: torch.Tensor, gamma: float,
                      rmax_in: torch.Tensor | None = None, return_worker_max: bool = False):
        """The MaxMC PLR score of N agents' trajectories under their value critics ``vcrit`` f32 [N, D] or [N, D, 1]
        (toued_max_mc_scores: value gather, per-worker returns and the mean in one launch, no host synchronisation):
        (score, rmax), f32 [N] each.  ``rmax`` = max(``rmax_in``, the best episode return of any worker), ``rmax_in``
        f32 [N] the best return each level has seen before (None: -inf); ``score`` = rmax - mean of V(s_t) over
        workers and steps, the unclipped mean of R_max - V(s_t) (Jiang et al. 2021, "Replay-Guided Adversarial
        Environment Design").  Returns are discounted with ``gamma`` so that they live on the value critic's scale;
        the episode still open at the trajectory's end counts with its truncated return.  ``return_worker_max``: also
        each worker's best return, f32 [N, W]."""
        N, T, W = _check_transition("max_mc_scores", transition)
        vcrit = _critic_rows(vcrit, N)
        dev = transition.reward.device
        if rmax_in is not None:
            if rmax_in.shape != (N,) or rmax_in.dtype != torch.float32 or rmax_in.device != dev:
                raise ValueError(f"max_mc_scores: rmax_in {rmax_in.dtype} {tuple(rmax_in.shape)} on {rmax_in.device}, "
                                 f"expected float32 {(N,)} on {dev}")
            rmax_in = rmax_in.contiguous()
        score = torch.empty(N, dtype=torch.float32, device=dev)
        rmax = torch.empty(N, dtype=torch.float32, device=dev)
        wmax = torch.empty((N, W), dtype=torch.float32, device=dev) if return_worker_max else None
        _lib.call("toued_max_mc_scores", N, W, T, vcrit.shape[1], _lib.ptr(vcrit), _lib.ptr(transition.obs_idx),
                  _lib.ptr(transition.obs_time), _lib.ptr(transition.reward), _lib.ptr(transition.done), float(gamma),
                  _lib.ptr(rmax_in), _lib.ptr(score), _lib.ptr(rmax), _lib.ptr(wmax), _lib.stream_ptr())
        return (score, rmax, wmax) if return_worker_max else (score, rmax)

    def policy_scores(self, transition: Transition, theta: torch.Tensor, return_steps: bool = False):
        """The policy PLR scores of N agents' trajectories under their actor tables ``theta`` f32 [N, D, 5]
        (toued_policy_scores: the softmax of the rollout's actor, the three terms and their means in one launch, no host
        synchronisation): (entropy, least confidence, min margin), f32 [N] each, the means over workers and steps
        t < T of the policy entropy (divided by log 5, its maximum), of 1 - max pi and of 1 - (max pi - second-largest
        pi) (Prioritized Level Replay, Jiang et al. 2021, Table 1).  Only the observations are read: no reward, no
        done flag, no value critic.  ``return_steps``: also the per-step terms f32 [N, 3, T, W] (entropy before the
        division by log 5, least confidence, min margin)."""
        N, T, W = _check_transition("policy_scores", transition)
        dev = transition.reward.device
        if theta.dim() != 3 or theta.shape[0] != N or theta.shape[2] != 5 or theta.dtype != torch.float32 \
                or theta.device != dev:
            raise ValueError(f"policy_scores: theta {theta.dtype} {tuple(theta.shape)} on {theta.device}, expected "
                             f"float32 {(N, 'D', 5)} on {dev}")
        theta = theta.contiguous()
        ent = torch.empty(N, dtype=torch.float32, device=dev)
        lc = torch.empty(N, dtype=torch.float32, device=dev)
        mm = torch.empty(N, dtype=torch.float32, device=dev)
        steps = torch.empty((N, 3, T, W), dtype=torch.float32, device=dev) if return_steps else None
        _lib.call("toued_policy_scores", N, W, T, theta.shape[1], _lib.ptr(theta), _lib.ptr(transition.obs_idx),
                  _lib.ptr(transition.obs_time), _lib.ptr(ent), _lib.ptr(lc), _lib.ptr(mm), _lib.ptr(steps),
                  _lib.stream_ptr())
        return (ent, lc, mm, steps) if return_steps else (ent, lc, mm)

    def episode_stats(self, transition: Transition, carry=None, out=None):
        """The episodes that N agents' workers complete in a train trajectory, tracked across calls
        (toued_episode_stats, one launch, no host synchronisation): episodes do not end where a train rollout ends,
        so ``carry`` = (run_ret f32 [N, W], run_len int32 [N, W]) holds every worker's unfinished episode, its
        undiscounted return and its length.  None starts a lifetime (zeros); the carry given is updated in place and
        returned.  ``out``: an ``EpisodeStats`` (or its f64 [N, 6] ``table``) to add to, so that a bucket of updates
        accumulates without a torch op per update; None starts from zero.  Only reward and done are read.

        Returns (EpisodeStats, carry).  The running return is an f32 sum in time order, so one call on T1 + T2 steps
        leaves the carry of a call on T1 steps followed by one on T2 steps, bit for bit.  Not in the reference."""
        N, T, W = transition.reward.shape
        if transition.done.shape != (N, T, W):
            raise ValueError(f"episode_stats: reward {tuple(transition.reward.shape)}, done "
                             f"{tuple(transition.done.shape)}")
        dev = transition.reward.device
        if carry is None:
            carry = (torch.zeros((N, W), dtype=torch.float32, device=dev),
                     torch.zeros((N, W), dtype=torch.int32, device=dev))
        run_ret, run_len = carry
        if run_ret.shape != (N, W) or run_ret.dtype != torch.float32 or run_len.shape != (N, W) \
                or run_len.dtype != torch.int32 or run_ret.device != dev or run_len.device != dev:
            raise ValueError(f"episode_stats: carry {run_ret.dtype} {tuple(run_ret.shape)}, {run_len.dtype} "
                             f"{tuple(run_len.shape)}, expected float32 and int32 {(N, W)} on {dev}")
        table = out.table if isinstance(out, EpisodeStats) else out
        if table is None:
            table = torch.zeros((N, 6), dtype=torch.float64, device=dev)
        elif table.shape != (N, 6) or table.dtype != torch.float64 or table.device != dev:
            raise ValueError(f"episode_stats: out {table.dtype} {tuple(table.shape)} on {table.device}, expected "
                             f"float64 {(N, 6)} on {dev}")
        _lib.call("toued_episode_stats", N, W, T, _lib.ptr(transition.reward), _lib.ptr(transition.done),
                  _lib.ptr(run_ret), _lib.ptr(run_len), _lib.ptr(table), _lib.stream_ptr())
        return EpisodeStats(*table.unbind(dim=1)), (run_ret, run_len)

    def eval_returns(self, agent_keys: torch.Tensor, theta: torch.Tensor, levels: torch.Tensor,
                     state: torch.Tensor) -> torch.Tensor:
        """batch_rollout(..., eval=True) when only cum_return is consumed (eval_agent): returns-only
        kernel mode, no trajectory stores; `state` is left unmodified.  Returns f32 [N, W]."""
        N = agent_keys.shape[0]
        n = state.shape[1]
        cum = torch.empty((N, n // N), dtype=torch.float32, device=state.device)
        _lib.call("toued_rollout", self._c, _lib.ptr(levels), _lib.ptr(theta), theta.shape[1],
                  _lib.ptr(agent_keys.contiguous()), _lib.ptr(state), N, n // N, self.eval_rollout_len, None, None,
                  None, None, None, _lib.ptr(cum), _lib.stream_ptr())
        return cum
