"""PLR / GROOVE level scoring on MI355X (environments/level_sampler.py:169-234, 293-408).

``plr_sample`` is the ``alg_regret`` branch of ``LevelSampler.sample``:
  1. ``_reset_lowest_scoring`` (:331-353): toued_plr_reset_ids (LDS bitonic argsort of the buffer)
     + the level generator for the reset slots; ``new = active.at[ids].set(True)`` kept.
  2. ``_compute_algorithmic_regret`` (:293-329) per agent: a fresh A2C antagonist trained for
     ``max_lifetime`` updates (toued.a2c), then eval(A2C) - eval(LPG) over ``env_workers`` workers.
  3. the terminated agents' scores / flags scattered into the buffer (:188-200).
  4. toued_plr_sample: replay ids (rank or proportional), random new ids, the bernoulli/permutation
     selection (:203-227); ``active[new_ids] = True`` (:232-234).

With ``score_function = positive_value_loss`` or ``l1_value_loss`` (not in the reference) step 2 is
``value_loss_scores``: one eval rollout of the LPG agent and the mean of max(GAE, 0) or |GAE| under the agent's own
value critic (toued_value_loss_scores), no antagonist; the rest is unchanged.

With ``score_function = max_mc`` (not in the reference) step 2 is ``max_mc_scores``: the same eval rollout, and
MaxMC, the maximum Monte Carlo regret estimate of Robust PLR and ACCEL (Jiang et al. 2021, "Replay-Guided Adversarial
Environment Design"): the mean over the trajectory of R_max - V(s_t), R_max the highest episode return ever achieved on
the level (toued_max_mc_scores).  Returns are discounted with --gamma so that they live on the value critic's scale.
The buffer then carries ``max_return`` (f32 [B], -inf where nothing was achieved yet): the slots' R_max is read before
the round, written back max-combined in step 3 and forgotten (-inf) for the slots step 1 refills, edited levels
included.  No antagonist and no tabular level: every env mode.

With ``score_function = policy_entropy``, ``least_confidence`` or ``min_margin`` (not in the reference) step 2 is
``policy_scores``: the same eval rollout, and the mean over the trajectory of the policy entropy (over log 5), of
1 - max pi or of 1 - (max pi - second-largest pi), the three scores of Prioritized Level Replay (Jiang et al. 2021,
Table 1) that read nothing but the agent's own policy (toued_policy_scores).  No antagonist, no value critic (so also
with --use_es), no tabular level and no buffer state: every env mode; the rest is unchanged.

With ``score_function = optimal_regret`` (tabular modes; not in the reference) step 2 is ``optimal_regret``: the
exact optimal return of the level (toued_optimal_return) minus eval(LPG), no antagonist; the rest is unchanged.

With ``score_function = return_variance`` (tabular modes; not in the reference) step 2 is ``return_variance``: the
exact variance of the agent's first-episode return on its level (toued_policy_return_moments), the learnability score
p (1 - p) of "Sampling for Learnability" (Rutherford et al. 2024) for real-valued returns.  One launch: no antagonist,
no value critic, no keys and no eval rollout.  It is not a regret; the rest is unchanged.

With ``--regret_eval exact`` (tabular modes; not in the reference) the two regret scores evaluate an agent by the exact
expected return of its policy (toued_policy_return) in place of the eval rollouts: ``optimal_regret`` is V* - V^pi,
deterministic and key-free, and ``alg_regret`` trains its antagonists on the same keys and returns
V^pi(A2C) - V^pi(LPG).  The default, ``sampled``, is the code path above, bit for bit.

With ``--policy_score_eval exact`` (tabular modes; not in the reference) the three policy scores average their terms
over the exact state occupancy of the agent's policy on its level (toued_policy_occupancy) in place of the eval
trajectory: ``exact_policy_scores``, deterministic and key-free, no eval rollout.  The default, ``sampled``, is the code
path above, bit for bit; ``--regret_eval`` stays the regret scores' switch and refuses these.

With ``--score_transform rank_sampled`` or ``--staleness_coeff`` > 0 (neither in the reference) step 4 is
toued_plr_sample_prio: Prioritized Level Replay's replay distribution (Jiang et al. 2021, section 3), the mixture
(1 - rho) P_S + rho P_C of a score part P_S (rank_sampled: weight rank^(-1/score_temperature) over the descending-score
ranks, sampled by Gumbel top-k; rank / proportional: the reference's) and a staleness part P_C proportional to the
rounds since a slot was last scored.  The buffer then carries ``stamp`` (the round of a slot's last score or reset,
written in steps 1 and 3) and ``clock`` (a host integer, +1 per round); ``sampler.last_plr["p"]`` keeps the
distribution and ``replay_distribution`` computes it for any buffer.  With the default flags the call is
toued_plr_sample and no stamp exists.

Multi-GPU: the buffer is replicated on every rank and updated identically; each rank scores
its own agents and the per-agent (term, score, buffer id) vectors are all-gathered, so every
rank runs the same single-workgroup sampler kernel on the same inputs.

Scores of agents that are not terminated are discarded by the reference (``term_mask_fn``);
by default they are not computed (``regret_all_agents=False``): the regret of agent i depends
only on its own key, level and actor, so skipping the masked-out ones changes no output.
"""
from __future__ import annotations

import os

import torch

from . import _lib, prng
from .a2c import A2CHyperparams, A2CTrainer
from .debug import nan_checker
from .agents import AgentBatch, create_agents, eval_agent, eval_agent_reset
from .env import L_BUFID
from .level_sampler import SCORE_TABLE, TRANSFORM_CODES, score_family
from .rollout import Transition


def _split2(rng):
    if rng.dim() == 2:                 # a batch of keys: both halves contiguous from one planar split
        ks = prng.split_planar(rng, 2)
        return ks[0], ks[1]
    ks = prng.split(rng, 2)
    return ks[..., 0, :].contiguous(), ks[..., 1, :].contiguous()


def parent_ids(buffer, reset_ids: torch.Tensor) -> torch.Tensor:
    """The level editor's parents for the reset slots ``reset_ids`` [N] (toued_plr_parent_ids): the buffer's scored
    slots (not new, active ones included) outside ``reset_ids``, highest score first, dealt round-robin; -1 everywhere
    when there is none.  Not in the reference."""
    N = reset_ids.shape[0]
    out = torch.empty(N, dtype=torch.int32, device=reset_ids.device)
    _lib.call("toued_plr_parent_ids", len(buffer), N, _lib.ptr(buffer.score), _lib.ptr(buffer.new),
              _lib.ptr(reset_ids.contiguous()), _lib.ptr(out), _lib.stream_ptr())
    return out


def reset_lowest_scoring(sampler, rng: torch.Tensor, buffer, n_new: int, now: int | None = None) -> torch.Tensor:
    """level_sampler.py:331-353, in place on ``buffer``; returns the reset ids [n_new].  A buffer with stamps
    (--staleness_coeff > 0) gets ``stamp[ids] = now``, one with ``max_return`` (--score_function max_mc)
    ``max_return[ids] = -inf``.

    With ``--level_editor accel`` (not in the reference) the generated levels then pass through the level editor:
    a row whose coin (``--edit_prob``) says so becomes an edited copy of a parent, a scored buffer level read before
    this round's copy and never one of the slots being reset; ``sampler.last_edit`` keeps the parents and the flags.
    The generator still runs on the same keys and nothing else in the round changes.  Multi-GPU: both kernels read
    only replicated state (the buffer and the rng), so every rank computes identical children and no collective is
    needed.  With ``--edit_require_solvable`` a child without a reachable positive reward is refused and the slot keeps
    the generator's level (LevelEditor(require_solvable=True): the stats kernel on the same stream and replicated
    state, no host sync, no collective); ``sampler.last_edit["rejected"]`` marks those rows.  With
    ``--edit_min_distance D`` a child closer than D (toued.env.level_nearest) to a buffer slot outside ``ids`` or to an
    earlier row of this round is refused in the same way (LevelEditor(min_distance=D): two more launches on the same
    stream and replicated state); ``sampler.last_edit["too_close"]`` marks those rows."""
    B = len(buffer)
    ids = torch.empty(n_new, dtype=torch.int32, device=buffer.score.device)
    _lib.call("toued_plr_reset_ids", B, n_new, _lib.ptr(buffer.score), _lib.ptr(buffer.active),
              _lib.ptr(buffer.new), _lib.ptr(ids), _lib.stream_ptr())
    keys = prng.split(rng, n_new)
    levels = sampler.gen(keys, buffer_ids=ids)
    editor = getattr(sampler, "editor", None)
    if editor is not None:
        parents = parent_ids(buffer, ids)
        if editor.min_distance > 0:     # --edit_min_distance: the filter compares with the slots outside ids
            flags = editor(buffer.levels, parents, keys, levels, reset_ids=ids)
        else:
            flags = editor(buffer.levels, parents, keys, levels)
        sampler.last_edit = {"parent": parents, "edited": flags}
        if editor.require_solvable:     # --edit_require_solvable: the rows whose child the filter refused
            sampler.last_edit["rejected"] = editor.last_rejected
        if editor.min_distance > 0:
            sampler.last_edit["too_close"] = editor.last_too_close
    il = ids.long()
    buffer.levels.index_copy_(0, il, levels)
    buffer.score.index_fill_(0, il, 0.0)
    new = buffer.active.clone()
    new.index_fill_(0, il, True)
    buffer.active.index_fill_(0, il, False)
    buffer.new = new
    if buffer.stamp is not None and now is not None:
        buffer.stamp.index_fill_(0, il, int(now))
    if buffer.max_return is not None:      # a refilled slot holds another level (an edited one too)
        buffer.max_return.index_fill_(0, il, float("-inf"))
    return ids


def algorithmic_regret(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor) -> torch.Tensor:
    """_compute_algorithmic_regret (level_sampler.py:293-329) for n agents (keys [n,2])."""
    n = keys.shape[0]
    if n == 0:
        return torch.zeros(0, device=keys.device)
    ro = sampler.rollout_manager
    W = sampler.env_workers
    rng, c = _split2(keys)
    w_rng, ag_rng = _split2(c)                       # _create_agent (:273-291)
    (_, _), state = ro.batch_reset(w_rng, levels, W)
    theta, vcrit = create_agents(ag_rng, ro.obs_dim, 1)   # value critic: critic_dims=1 (:280-281)
    vcrit = vcrit.reshape(n, ro.obs_dim).contiguous()
    rng, tr = _split2(rng)
    step = torch.zeros(n, dtype=torch.int32, device=keys.device)
    lpg_rng, a2c_rng = _split2(rng)
    if sampler.regret_eval == "exact":
        # the antagonists train on the keys above, without the eval draws (no eval rollout follows); then both
        # agents' exact returns in one launch
        sampler.a2c_trainer().train(tr, theta, vcrit, step, levels, state, sampler.max_lifetime)
        r = ro.policy_return(torch.cat([levels, levels]), torch.cat([lpg_theta, theta]), ro.eval_rollout_len)
        return r[n:] - r[:n]
    # both eval_agent calls as one batch of 2n agents (each agent's rollout depends only on its own key, level and
    # table: bit-identical to two calls, at about the latency of one -- the returns-only rollout is latency-bound).
    # eval_agent's keys, reset and draws do not depend on the tables: the draws are made beside the antagonist's
    # update chain, and after it only the env chain runs (eval_agent_reset / eval_returns_from_draws, bit-identical)
    ev_levels = torch.cat([levels, levels])
    ev_state, ev_keys = eval_agent_reset(ro, torch.cat([lpg_rng, a2c_rng]), ev_levels, W)
    split_eval = (os.environ.get("TOUED_REGRET_SPLIT_EVAL", "1") != "0"
                  and _eval_draw_bytes(ro, 2 * n, W) <= EVAL_DRAWS_MAX_BYTES)
    trainer = sampler.a2c_trainer()
    trainer.train(tr, theta, vcrit, step, levels, state, sampler.max_lifetime,
                  eval_keys=ev_keys if split_eval else None, eval_levels=ev_levels if split_eval else None)
    both = torch.cat([lpg_theta, theta])
    if split_eval:
        cum = ro.eval_returns_from_draws(trainer.eval_draws_out, both, ev_levels, ev_state)
    else:
        cum = ro.eval_returns(ev_keys, both, ev_levels, ev_state)
    r = cum.mean(dim=1)
    r_lpg, r_a2c = r[:n], r[n:]
    return r_a2c - r_lpg


def optimal_regret(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor) -> torch.Tensor:
    """The true regret of n LPG agents on tabular levels: V*(level) - eval(LPG), with V* the exact optimal return over
    the eval rollout length (RolloutWrapper.optimal_return) in place of the trained antagonist's return.  Same
    signature and return as ``algorithmic_regret``, and the LPG agent is evaluated with the same key (the splits of
    level_sampler.py:293-329), so its return is bit-identical between the two scores.  An extension: the reference's
    LevelSampler has no such score function."""
    n = keys.shape[0]
    if n == 0:
        return torch.zeros(0, device=keys.device)
    ro = sampler.rollout_manager
    if sampler.regret_eval == "exact":      # V* - V^pi: no keys, no rollout, >= 0 up to the two tables' rounding
        return ro.optimal_return(levels, ro.eval_rollout_len) - ro.policy_return(levels, lpg_theta,
                                                                                 ro.eval_rollout_len)
    rng, _ = _split2(keys)
    rng, _ = _split2(rng)
    lpg_rng, _ = _split2(rng)
    return ro.optimal_return(levels, ro.eval_rollout_len) - eval_agent(ro, lpg_rng, levels, lpg_theta,
                                                                      sampler.env_workers)


def return_variance(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor) -> torch.Tensor:
    """The exact variance of n LPG agents' first-episode returns on their tabular levels over the eval rollout length
    (RolloutWrapper.policy_return_moments): zero on a level the agent always or never solves, largest where the
    outcome is open.  The variance is over the policy's actions and the level's own termination and respawn draws
    alike.  Same signature and return as ``optimal_regret``; ``keys`` is unused (no rollout, no antagonist, no value
    critic).  A score, not a regret.  An extension: the reference's LevelSampler has no such score function."""
    if levels.shape[0] == 0:
        return torch.zeros(0, device=levels.device)
    ro = sampler.rollout_manager
    return ro.policy_return_moments(levels, lpg_theta, ro.eval_rollout_len)[1]


# value_loss_scores keeps one chunk of agents' eval trajectories at a time (14 bytes per worker and step) under this
VALUE_LOSS_SCRATCH_BYTES = 1 << 30


def value_loss_scores(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor,
                      vcrit: torch.Tensor, chunk_agents: int | None = None):
    """The value-loss PLR scores of n LPG agents: (positive value loss, L1 value loss), f32 [n] each, the means over
    the agent's eval trajectory (``env_workers`` workers, ``eval_rollout_len`` steps) of max(GAE, 0) and |GAE| under
    its value critic ``vcrit`` [n, obs_dim] (AgentBatch.vcrit, the critic of meta/train.py:61-100), with the
    sampler's --gamma and --gae_lambda.  No antagonist and no optimal return: one eval rollout and one kernel
    (RolloutWrapper.value_loss_scores).  The LPG agent's key is ``algorithmic_regret``'s ``lpg_rng`` (the splits of
    level_sampler.py:293-329) and the worker reset and rollout key are ``eval_agent``'s, so the scored trajectory
    is the one whose return the regret scores use.  An extension: the reference's LevelSampler has no such score.

    The agents go through in chunks whose trajectories fit VALUE_LOSS_SCRATCH_BYTES (``chunk_agents`` overrides the
    chunk size); an agent's scores depend on its own key, level, actor and critic only, so the chunking changes
    no bit."""
    ro = sampler.rollout_manager
    vcrit = vcrit.reshape(keys.shape[0], ro.obs_dim)
    return _chunked_scores(sampler, keys, levels, lpg_theta, chunk_agents, 2, lambda lo, hi, out: ro.value_loss_scores(
        out, vcrit[lo:hi].contiguous(), sampler.args.gamma, sampler.args.gae_lambda))


def _chunked_scores(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor,
                    chunk_agents: int | None, k: int, per_chunk) -> tuple:
    """``k`` scores f32 [n] of the n agents' eval trajectories, filled a chunk of agents at a time:
    ``per_chunk(lo, hi, Transition of agents lo..hi-1)`` gives the k scores of those agents."""
    outs = tuple(torch.empty(keys.shape[0], dtype=torch.float32, device=keys.device) for _ in range(k))
    for lo, hi, out in _eval_trajectory_chunks(sampler, keys, levels, lpg_theta, chunk_agents):
        for o, part in zip(outs, per_chunk(lo, hi, out)):
            o[lo:hi] = part
    return outs


def _eval_trajectory_chunks(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor,
                            chunk_agents: int | None):
    """The eval trajectories that the critic-based scores read, a chunk of agents at a time: yields (lo, hi,
    Transition of agents lo..hi-1); nothing for n = 0.  The keys, reset and rollout are ``value_loss_scores``'; the
    trajectory buffers are reused from chunk to chunk, so a chunk's Transition holds until the next one is asked
    for."""
    n = keys.shape[0]
    if n == 0:
        return
    ro = sampler.rollout_manager
    W = sampler.env_workers
    rng, _ = _split2(keys)
    rng, _ = _split2(rng)
    lpg_rng, _ = _split2(rng)
    if chunk_agents is None:
        chunk_agents = VALUE_LOSS_SCRATCH_BYTES // (14 * W * (ro.eval_rollout_len + 1))
    chunk_agents = max(1, min(int(chunk_agents), n))
    out = None
    for lo in range(0, n, chunk_agents):
        hi = min(lo + chunk_agents, n)
        lv = levels[lo:hi].contiguous()
        state, ro_keys = eval_agent_reset(ro, lpg_rng[lo:hi].contiguous(), lv, W)
        if out is not None and hi - lo < chunk_agents:       # the last, shorter chunk: the buffers' leading rows
            out = Transition(*(getattr(out, f)[:hi - lo] for f in ("obs_idx", "obs_time", "action", "reward", "done")))
        out, _, _ = ro.batch_rollout(ro_keys, lpg_theta[lo:hi].contiguous(), lv, state, eval=True, out=out,
                                     inplace_state=True)
        yield lo, hi, out


def positive_value_loss(sampler, keys, levels, lpg_theta, vcrit) -> torch.Tensor:
    return value_loss_scores(sampler, keys, levels, lpg_theta, vcrit)[0]


def l1_value_loss(sampler, keys, levels, lpg_theta, vcrit) -> torch.Tensor:
    return value_loss_scores(sampler, keys, levels, lpg_theta, vcrit)[1]


def max_mc_scores(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor, vcrit: torch.Tensor,
                  prior: torch.Tensor, chunk_agents: int | None = None):
    """The MaxMC PLR score of n LPG agents (the maximum Monte Carlo regret estimate of Jiang et al. 2021,
    "Replay-Guided Adversarial Environment Design"): (score, rmax), f32 [n] each.  ``rmax`` = max(``prior``, the best
    episode return of any worker on the agent's eval trajectory), ``prior`` f32 [n] the best return the agent's level
    has seen so far (LevelBuffer.max_return of its slot, -inf for a level never scored); ``score`` = rmax - the mean
    of the value critic ``vcrit`` [n, obs_dim] over the trajectory, the unclipped mean of R_max - V(s_t).  Returns are
    discounted with the sampler's --gamma so that they live on the value critic's scale; the episode still open at
    the trajectory's end counts with its truncated return (RolloutWrapper.max_mc_scores).  No antagonist and no
    tabular level: any env mode.  The keys, the eval trajectory and the chunking are ``value_loss_scores``', so the
    scored trajectory is the one the other scores use, and the chunking changes no bit.  An extension: the reference's
    LevelSampler has no such score."""
    ro = sampler.rollout_manager
    vcrit = vcrit.reshape(keys.shape[0], ro.obs_dim)
    return _chunked_scores(sampler, keys, levels, lpg_theta, chunk_agents, 2, lambda lo, hi, out: ro.max_mc_scores(
        out, vcrit[lo:hi].contiguous(), sampler.args.gamma, prior[lo:hi].contiguous()))


def policy_scores(sampler, keys: torch.Tensor, levels: torch.Tensor, lpg_theta: torch.Tensor,
                  chunk_agents: int | None = None):
    """The policy PLR scores of n LPG agents (Prioritized Level Replay, Jiang et al. 2021, Table 1): (policy entropy,
    least confidence, min margin), f32 [n] each, the means over the agent's eval trajectory (``env_workers`` workers,
    ``eval_rollout_len`` steps) of the entropy of its policy divided by log 5, of 1 - max pi and of
    1 - (max pi - second-largest pi) (RolloutWrapper.policy_scores).  They read the agent's actor table and the
    observations it visited, nothing else: no antagonist, no value critic (so also with --use_es), no tabular level
    and no buffer state.  The keys, the eval trajectory and the chunking are ``value_loss_scores``', so the scored
    trajectory is the one the other scores use, and the chunking changes no bit.  An extension: the reference's
    LevelSampler has no such score."""
    if getattr(sampler, "policy_score_eval", "sampled") == "exact":
        return exact_policy_scores(sampler, levels, lpg_theta)
    ro = sampler.rollout_manager
    return _chunked_scores(sampler, keys, levels, lpg_theta, chunk_agents, 3,
                           lambda lo, hi, out: ro.policy_scores(out, lpg_theta[lo:hi].contiguous()))


def exact_policy_scores(sampler, levels: torch.Tensor, lpg_theta: torch.Tensor):
    """``policy_scores``' three scores of n tabular LPG agents without an eval rollout (``--policy_score_eval exact``):
    (policy entropy, least confidence, min margin), f32 [n] each, the same per-state terms averaged over the exact
    state occupancy of the agent's policy on its level over ``eval_rollout_len`` steps
    (RolloutWrapper.policy_occupancy's ``entropy``, ``least_confidence`` and ``min_margin``, bit for bit), that is
    over the steps of the agent's first episode, each weighted by the probability that the episode reaches it.

    What it is next to the sampled score: the episodes of a tabular level are independent and identically
    distributed (reset is deterministic, at the start cell with all objects present), so the per-step average over the
    first episode is the long-run per-step average of the sampled score (the renewal-reward theorem).  The sampled
    score over T = ``eval_rollout_len`` steps and ``env_workers`` workers differs from it by the truncated last
    episode, an O(1/T) bias, and by sampling noise.  No keys, no antagonist, no value critic (so also with --use_es),
    one launch, deterministic.  An extension: the reference's LevelSampler has no such score."""
    if levels.shape[0] == 0:
        z = torch.zeros(0, dtype=torch.float32, device=levels.device)
        return z, z.clone(), z.clone()
    ro = sampler.rollout_manager
    occ = ro.policy_occupancy(levels, lpg_theta, ro.eval_rollout_len)
    return occ.entropy, occ.least_confidence, occ.min_margin


def policy_entropy(sampler, keys, levels, lpg_theta) -> torch.Tensor:
    return policy_scores(sampler, keys, levels, lpg_theta)[0]


def least_confidence(sampler, keys, levels, lpg_theta) -> torch.Tensor:
    return policy_scores(sampler, keys, levels, lpg_theta)[1]


def min_margin(sampler, keys, levels, lpg_theta) -> torch.Tensor:
    return policy_scores(sampler, keys, levels, lpg_theta)[2]


# every score function that is called (level_sampler.SCORE_TABLE says with what), and its views by family
SCORE_CALLS = {"alg_regret": algorithmic_regret, "positive_value_loss": positive_value_loss,
               "l1_value_loss": l1_value_loss, "optimal_regret": optimal_regret, "return_variance": return_variance,
               "max_mc": max_mc_scores, "policy_entropy": policy_entropy, "least_confidence": least_confidence,
               "min_margin": min_margin}
REGRET_FUNCTIONS, MOMENT_FUNCTIONS, VALUE_LOSS_FUNCTIONS, RETURN_FUNCTIONS, POLICY_FUNCTIONS = (
    {n: SCORE_CALLS[n] for n in score_family(f)} for f in ("regret", "moment", "value_loss", "return", "policy"))


# the regret round's eval draws ([eval_len][2n * W][4] u32, plus as much key-chain scratch) are made ahead when they fit
EVAL_DRAWS_MAX_BYTES = 4 << 30


def _eval_draw_bytes(ro, n_agents: int, W: int) -> int:
    return 2 * 16 * ro.eval_rollout_len * n_agents * W


def _scatter_into(dst: torch.Tensor, ids: torch.Tensor, val) -> None:
    """dst[ids] = val for ids in [0, B], where id B (= len(dst)) is a sink whose writes are dropped."""
    ext = torch.empty(dst.shape[0] + 1, dtype=dst.dtype, device=dst.device)
    ext[:-1].copy_(dst)
    if isinstance(val, torch.Tensor):
        ext.index_put_((ids,), val.to(dst.dtype))
    else:   # a Python scalar goes in as a kernel argument (a host tensor would be copied in behind a stream sync)
        ext.index_fill_(0, ids, val)
    dst.copy_(ext[:-1])


def replay_distribution(buffer, n: int, transform: str, temperature: float, staleness_coeff: float = 0.0,
                        now: int | None = None) -> torch.Tensor:
    """The distribution p [B] that a round of ``n`` agents would draw its replay levels from (toued_plr_sample_prio's
    ``p_out``; the ids it draws go to scratch): ``transform`` one of SCORE_TRANSFORMS, ``temperature`` the
    --score_temperature, ``staleness_coeff`` the --staleness_coeff (needs ``buffer.stamp``), ``now`` the round the
    staleness is measured at (default: the buffer's next round, ``buffer.clock + 1``).  Not in the reference."""
    if transform not in TRANSFORM_CODES:
        raise ValueError(f"Level score transform {transform} not in known transforms: {sorted(TRANSFORM_CODES)}")
    rho = float(staleness_coeff)
    if rho > 0.0 and buffer.stamp is None:
        raise ValueError("staleness_coeff > 0 needs a level buffer with stamps")
    B = len(buffer)
    dev = buffer.score.device
    now = buffer.clock + 1 if now is None else int(now)
    p = torch.empty(B, dtype=torch.float32, device=dev)
    if not 1 <= n <= B:
        raise ValueError(f"replay_distribution: need 1 <= n <= {B} (got {n})")
    ids = torch.empty((4, n), dtype=torch.int32, device=dev)
    keys = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    _lib.call("toued_plr_sample_prio", B, n, _lib.ptr(buffer.score), _lib.ptr(buffer.active), _lib.ptr(buffer.new),
              _lib.ptr(buffer.stamp if rho > 0.0 else None), now, _lib.ptr(keys), TRANSFORM_CODES[transform],
              float(temperature), rho, 0.5, _lib.ptr(ids[0]), _lib.ptr(ids[1]), _lib.ptr(ids[2]), _lib.ptr(ids[3]),
              _lib.ptr(p), _lib.stream_ptr())
    return p


def plr_sample(sampler, rng: torch.Tensor, buffer, agents: AgentBatch, term: torch.Tensor, sl=None):
    """Returns (rng, buffer, new_levels [n_local, 64]) — new_levels for terminated agents, the
    caller keeps the old level elsewhere (``term_mask_fn``)."""
    world = sampler.world
    needs, score_fn = SCORE_TABLE[sampler.score_function], SCORE_CALLS[sampler.score_function]
    if needs.critic and agents.vcrit is None:
        raise ValueError(f"Level score function {sampler.score_function} needs the agents' value critics "
                         f"(AgentBatch.vcrit is None)")
    N = agents.n if sl is None else sl[2]
    B = len(buffer)
    dev = agents.levels.device
    rng, sub = _split2(rng)
    # _reset_lowest_scoring touches only the buffer, which the regret round below does not read: it runs on a side
    # stream beside the antagonists' training, joined before the buffer update
    main = torch.cuda.current_stream()
    side = getattr(sampler, "_plr_side", None)
    if side is None:
        side = sampler._plr_side = torch.cuda.Stream(device=dev)
    prior = rmax = None
    if needs.max_return:
        if buffer.max_return is None:
            raise ValueError(f"Level score function {sampler.score_function} needs a level buffer with max_return "
                             f"(LevelSampler.initialize_buffer makes it; a checkpoint written without it has none)")
        # the slots' best returns so far, read on the main stream before the side stream is let go: its reset of
        # other slots' max_return can then never race this read
        prior = buffer.max_return[agents.levels[:, L_BUFID].long()]
        rmax = torch.full((agents.n,), float("-inf"), dtype=torch.float32, device=dev)
    side.wait_stream(main)
    # the side kernels read `sub` and the old `buffer.new` (both from main's allocator pool) after this function has
    # dropped them: keep their blocks from being reused by main until the side stream's work has passed them
    sub.record_stream(side)
    buffer.new.record_stream(side)
    now = buffer.clock + 1      # this round's number: a host integer, no device read
    with torch.cuda.stream(side):
        reset_lowest_scoring(sampler, sub, buffer, N, now)
    rng, sub = _split2(rng)
    keys = prng.split(sub, N)
    if sl is not None:
        keys = keys[sl[0]:sl[1]].contiguous()
    score = torch.zeros(agents.n, dtype=torch.float32, device=dev)
    # what the function takes per agent beside the regret functions' arguments (SCORE_TABLE)
    per_agent = ([agents.vcrit.reshape(agents.n, sampler.obs_dim)] if needs.critic else []) \
        + ([prior] if needs.max_return else [])

    def regret(s, k, lv, th, sel=slice(None)):
        sc = score_fn(s, k, lv, th, *(x[sel].contiguous() for x in per_agent))
        if needs.max_return:
            sc, rmax[sel] = sc
        return sc
    if sampler.regret_all_agents:
        score = regret(sampler, keys, agents.levels, agents.theta)
    else:
        sel = term.nonzero().flatten()
        if sel.numel():
            score[sel] = regret(sampler, keys[sel].contiguous(), agents.levels[sel].contiguous(),
                                agents.theta[sel].contiguous(), sel)
    nan_checker().check("regret_scores", score)
    old_ids = agents.levels[:, L_BUFID].contiguous()
    if world is not None and world.active:
        term_g = world.all_gather_cat(term.to(torch.int32)).bool()
        score_g = world.all_gather_cat(score)
        old_g = world.all_gather_cat(old_ids)
        rmax_g = world.all_gather_cat(rmax) if rmax is not None else None
    else:
        term_g, score_g, old_g, rmax_g = term, score, old_ids, rmax
    main.wait_stream(side)
    buffer.new.record_stream(main)     # allocated on the side stream
    # buffer update for terminated levels (:188-200), without a boolean-mask gather (a host sync that would hold the
    # host's launches of the rest of sample() until the regret round has finished): every agent scatters, the
    # non-terminated ones into a sink slot B past the buffer's end
    t_ids = torch.where(term_g, old_g.long(), B)
    _scatter_into(buffer.score, t_ids, score_g)
    _scatter_into(buffer.active, t_ids, False)
    _scatter_into(buffer.new, t_ids, False)
    if buffer.stamp is not None:       # the gathered ids: every rank's copy stays identical
        _scatter_into(buffer.stamp, t_ids, now)
    if rmax_g is not None:             # max-combined: two agents on one slot cannot lose the larger return
        ext = torch.cat([buffer.max_return, buffer.max_return.new_full((1,), float("-inf"))])
        ext.scatter_reduce_(0, t_ids, rmax_g, "amax", include_self=True)
        buffer.max_return.copy_(ext[:-1])
    # replay vs random (:203-227)
    ks = prng.split(rng, 3)                           # rng, replay_rng, random_rng
    kbuf = torch.stack([ks[1], ks[2], ks[0]]).contiguous()
    chosen = torch.empty(N, dtype=torch.int32, device=dev)
    rep, rnd, use = torch.empty_like(chosen), torch.empty_like(chosen), torch.empty_like(chosen)
    rho = float(getattr(sampler, "staleness_coeff", 0.0))
    sampler.last_plr = {"replay": rep, "random": rnd, "use": use, "chosen": chosen, "score": score_g}
    if sampler.score_transform == "rank_sampled" or rho > 0.0:
        if rho > 0.0 and buffer.stamp is None:
            raise ValueError("staleness_coeff > 0 needs a level buffer with stamps (LevelSampler.initialize_buffer "
                             "makes them; a checkpoint written without them has none)")
        p = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("toued_plr_sample_prio", B, N, _lib.ptr(buffer.score), _lib.ptr(buffer.active),
                  _lib.ptr(buffer.new), _lib.ptr(buffer.stamp if rho > 0.0 else None), now, _lib.ptr(kbuf),
                  TRANSFORM_CODES[sampler.score_transform], float(sampler.score_temperature), rho,
                  float(sampler.p_replay), _lib.ptr(chosen), _lib.ptr(rep), _lib.ptr(rnd), _lib.ptr(use), _lib.ptr(p),
                  _lib.stream_ptr())
        sampler.last_plr["p"] = p
    else:
        _lib.call("toued_plr_sample", B, N, _lib.ptr(buffer.score), _lib.ptr(buffer.active), _lib.ptr(buffer.new),
                  _lib.ptr(kbuf), int(sampler.score_transform == "proportional"), float(sampler.score_temperature),
                  float(sampler.p_replay), _lib.ptr(chosen), _lib.ptr(rep), _lib.ptr(rnd), _lib.ptr(use),
                  _lib.stream_ptr())
    buffer.clock = now
    r1, _ = _split2(ks[0].contiguous())               # bernoulli: rng, _rng = split(rng)
    rng, _ = _split2(r1)                              # permutation: rng, _rng = split(rng)
    new_ids = torch.where(term_g, chosen, old_g)
    buffer.active.index_fill_(0, new_ids.long(), True)   # (:232-234)
    lo, hi = (0, N) if sl is None else (sl[0], sl[1])
    new_levels = buffer.levels[new_ids[lo:hi].long()]
    return rng, buffer, new_levels
