"""Command-line flags of the reference (experiments/parse_args.py:5-204), same names and defaults.

Additions (all default to the reference's behaviour):
  --ref_quirk_steps10   reproduce train.py:55's hard-coded 10 meta-steps (default: honour --train_steps)
  --fix_value_critic    train the meta-gradient value critic (the reference discards its update)
  --ref_quirk_checkpoint_init  checkpoint the initial states, as the reference does (train.py:52-57)
  --checkpoint_dir DIR  write the final LPG train state (and the level buffer) as flax-msgpack checkpoints
                        (experiments/logging.py:31-46 writes them into the wandb run directory)
  --regret_eval {sampled,exact}  how alg_regret / optimal_regret evaluate an agent: ``sampled`` (the default) by the
                        reference's eval rollouts, ``exact`` by the exact expected return of the agent's own policy
                        (RolloutWrapper.policy_return; tabular modes)
  --score_function return_variance  PLR with the exact variance of the agent's first-episode return on its level
                        (RolloutWrapper.policy_return_moments), the learnability score p (1 - p) of "Sampling for
                        Learnability" (Rutherford et al. 2024) for real-valued returns: no antagonist, no value critic
                        (so also with --use_es), no keys, no eval rollout; tabular modes.  The variance includes the
                        level's own randomness (termination and respawn draws), not only the policy's
  --score_function max_mc  PLR with MaxMC, the maximum Monte Carlo regret estimate Robust PLR and ACCEL are run with
                        (Jiang et al. 2021, "Replay-Guided Adversarial Environment Design"): the mean over the agent's
                        eval trajectory of R_max - V(s_t) under its value critic, R_max the highest episode return ever
                        achieved on the level (kept per buffer slot, forgotten when the slot is refilled); returns are
                        discounted with --gamma, the critic's scale.  No antagonist, every env mode; not with --use_es
  --score_function policy_entropy | least_confidence | min_margin  PLR with the scores that read nothing but the
                        agent's own policy (Jiang et al. 2021, "Prioritized Level Replay", Table 1): the mean over the
                        agent's eval trajectory of the policy entropy -sum_a pi log pi divided by log 5 (its maximum),
                        of the least confidence 1 - max_a pi, or of the min margin 1 - (max_a pi - second-largest_a pi).
                        No antagonist, no value critic (so also with --use_es), no buffer state; every env mode
  --policy_score_eval {sampled,exact}  how the three policy scores average their per-state terms: ``sampled`` (the
                        default) over the agent's eval trajectory, ``exact`` over the exact state occupancy of its
                        policy on the level (RolloutWrapper.policy_occupancy): the per-step average over the first
                        episode, which is the long-run per-step average of the sampled score, since the episodes of a
                        tabular level are independent and identically distributed; the sampled score over T steps
                        differs from it by the truncated last episode, an O(1/T) bias, and by sampling noise.  No
                        keys, no eval rollout, also with --use_es; tabular modes and these three scores only
  --occupancy_metrics   add an ``occupancy`` dict to every log line, from one policy_occupancy launch on the agents and
                        their levels after the meta-step's sample, means over all agents: ``episode_len``,
                        ``p_early_term``, ``exact_return``, ``collect_pos`` / ``collect_neg`` (the expected collections
                        of objects with a positive / negative reward) and ``cell_coverage`` (exp of the entropy of the
                        visits per cell over the number of reachable cells: in (0, 1], 1 for a uniform visitation).
                        Tabular modes
  --level_editor {none,accel}  how the PLR scores' reset round refills a freed buffer slot: ``none`` (the default) by
                        the level generator, ``accel`` with probability --edit_prob by --num_edits small edits
                        (--edit_ops: walls, objects, start, rewards; a reward moves by at most --edit_reward_delta) of a
                        high-scoring buffer level (ACCEL, Parker-Holder et al. 2022)
  --edit_require_solvable  accel only: an edited level on which no positive-reward object can be reached from the start
                        within max_steps_in_episode moves (toued.env.level_stats' ``solvable`` == 0) is refused and the
                        slot keeps the generator's level; the key schedule is unchanged.  Refused without
                        --level_editor accel
  --edit_min_distance D  accel only: an edited level whose level distance (toued.env.level_nearest: wall bits that
                        differ plus the other words of the level's canonical record that differ, 0 to 302) to a level
                        the buffer keeps this round, or to an earlier child of the round, is below D is refused and the slot
                        keeps the generator's level; the key schedule is unchanged.  1 refuses exact duplicates of the
                        parent (every edit of a child can be a no-op); 0, the default, checks nothing.  Refused without
                        --level_editor accel
  --buffer_diversity    add a ``buffer`` dict to every log line, from one level_nearest launch of the level buffer
                        against itself: ``unique_frac`` (the share of slots that are the first of their identity
                        class), ``nn_dist`` (the mean distance to the nearest other slot), ``pair_dist`` (the mean
                        distance over all pairs) and, with a level editor, ``edit_too_close`` (the round's count of
                        children --edit_min_distance refused).  Refused with --score_function random (no buffer)
  --level_metrics       add a ``levels`` dict to every log line: ACCEL's complexity metrics (Parker-Holder et al. 2022)
                        of the levels the agents are on after the meta-step's sample -- ``solvable`` (share),
                        ``n_walls``, ``reachable_frac``, ``ecc`` and ``nearest_reward_dist`` (means; NaN when no level
                        has a reachable reward) -- and, with a level editor, the round's ``edited`` and
                        ``edit_rejected`` counts.  One stats launch per meta-step; also with --use_es
  --score_transform rank_sampled  Prioritized Level Replay's rank prioritisation (Jiang et al. 2021): replay levels are
                        sampled without replacement with weight rank^(-1/score_temperature), rank 1 the highest score
                        (the reference's ``rank`` takes the N best-scoring slots, nothing is sampled)
  --staleness_coeff RHO PLR's staleness mixture: the replay distribution becomes (1 - RHO) P_S + RHO P_C, P_S the
                        --score_transform's distribution and P_C proportional to the rounds since a slot was last
                        scored; 0 (the default) is the reference's behaviour, in [0, 1], not with random / frozen
  --eval_every M        after every M-th meta-step rank 0 runs the meta-test (toued.evaluate.MetaTest) on the current
                        LPG parameters (--use_es: the search mean): fresh agents on --eval_levels held-out levels of
                        --eval_mode drawn from PRNGKey(--eval_seed) are trained for their whole lifetime by the frozen
                        rule, and a ``meta_test`` dict (``final_normalised``, ``final_exact_return``, ``auc`` over
                        --curve_points points, ``n_degenerate``) is added to that log line.  It has its own keys,
                        buffers and RolloutWrapper: training with and without it is bit-identical.  0 (the default)
                        never runs it; a negative M or a non-tabular --eval_mode is refused.  Not sharded over ranks
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--debug", action="store_true", help="Debug mode (disable JIT)")
    p.add_argument("--debug_nans", action="store_true", help="Exit and stack trace when NaNs are encountered")
    # --- ENVIRONMENT ---
    p.add_argument("--env_name", help="Environment name", type=str, default="GridWorld-v0")
    p.add_argument("--env_mode", help="Environment mode", type=str, default="all_shortlife")
    p.add_argument("--env_workers", help="Number of environment workers per agent", type=int, default=64)
    # --- EXPERIMENT ---
    p.add_argument("--seed", type=int, default=0, help="Random seed")
    p.add_argument("--train_steps", help="Number of train steps", type=int, default=int(3e4))
    p.add_argument("--num_agents", help="Meta-train batch size, doubled for antithetic task sampling when using ES",
                   type=int, default=512)
    p.add_argument("--num_mini_batches", help="Number of meta-training mini-batches", type=int, default=16)
    p.add_argument("-br", "--best-response-length", dest="br", default=10, type=int,
                   help="Number of best response iterates, must be multiple of 20")
    p.add_argument("--log", action="store_true", help="Log with WandB")
    p.add_argument("--wandb_project", type=str, help="Wandb project")
    p.add_argument("--wandb_entity", type=str, help="Wandb entity")
    p.add_argument("--wandb_group", type=str, default="debug", help="WandB group")
    # --- AGENT ---
    p.add_argument("--train_rollout_len", help="Number of environment steps per agent update", type=int, default=20)
    p.add_argument("--gamma", help="Discount factor", type=float, default=0.99)
    p.add_argument("--gae_lambda", help="Lambda parameter for Generalized Advantage Estimation", type=float,
                   default=0.95)
    p.add_argument("--entropy_coeff", help="Actor entropy coefficient for A2C agents", type=float, default=0.01)
    # --- LPG ---
    p.add_argument("--lpg_embedding_net_width", help="Width of LPG embedding network", type=int, default=16)
    p.add_argument("--lpg_gru_width", help="Number of LPG LSTM units", type=int, default=256)
    p.add_argument("--lpg_target_width", help="Size of categorical prediction vector (target) generated by LPG",
                   type=int, default=8)
    p.add_argument("--lpg_agent_target_coeff", help="(alpha_y) Agent target KL divergence.", type=float, default=5e-1)
    p.add_argument("--lpg_opt", help="LPG optimizer", type=str, default="Adam")
    p.add_argument("--lpg_learning_rate", help="LPG learning rate", type=float, default=1e-4)
    p.add_argument("--num_agent_updates", help="(K) Number of agent updates per LPG train step", type=int, default=5)
    p.add_argument("--lpg_max_grad_norm", help="Max gradient norm for LPG optimisation", type=float, default=0.5)
    p.add_argument("--lpg_policy_entropy_coeff", help="(beta_0) Trained agent policy entropy.", type=float,
                   default=5e-2)
    p.add_argument("--lpg_target_entropy_coeff", help="(beta_1) Trained agent target entropy.", type=float,
                   default=1e-3)
    p.add_argument("--lpg_policy_l2_coeff", help="(beta_2) Policy update (pi_hat) L2 regularization.", type=float,
                   default=5e-3)
    p.add_argument("--lpg_target_l2_coeff", help="(beta_3) Target update (y_hat) L2 regularization.", type=float,
                   default=1e-3)
    # ES
    p.add_argument("--use_es", action="store_true", help="Optimize LPG with ES")
    p.add_argument("--es_lrate_decay", type=float, default=0.999)
    p.add_argument("--es_lrate_limit", type=float, default=1e-5)
    p.add_argument("--es_sigma_init", type=float, default=0.1)
    p.add_argument("--es_sigma_decay", type=float, default=1.0)
    p.add_argument("--es_sigma_limit", type=float, default=0.1)
    p.add_argument("--es_mean_decay", type=float, default=0.0)
    # TA-LPG
    p.add_argument("--lifetime_conditioning", help="Condition LPG on agent lifetime", action="store_true")
    # --- UED ---
    p.add_argument("--buffer_size", help="Size of level buffer", type=int, default=4000)
    p.add_argument("--score_function", help="UED level scoring function (random, frozen, alg_regret, "
                   "positive_value_loss or l1_value_loss: the mean of max(GAE, 0) or |GAE| under the agent's value "
                   "critic, not with --use_es; or optimal_regret: the true regret against the level's exact optimal "
                   "return, tabular modes; or return_variance: the exact variance of the agent's return on the level, "
                   "tabular modes; or max_mc: the mean of R_max - V(s_t) under the agent's value critic, R_max the "
                   "level's best return so far, not with --use_es; or policy_entropy, least_confidence or min_margin: "
                   "the mean over the agent's eval trajectory of its policy's entropy over log 5, of 1 - max pi, or "
                   "of 1 - (max pi - second-largest pi), no critic, also with --use_es; see --regret_eval for the regret scores' agent "
                   "evaluation)", type=str,
                   default="random")
    p.add_argument("--p_replay", help="Probability of replaying a level from the buffer (vs. random sampling)",
                   type=float, default=0.5)
    p.add_argument("--score_transform", help="Transform to apply to level score (rank: the N best-scoring slots; "
                   "proportional: softmax of the score; rank_sampled: sampled with weight rank^(-1/temperature))",
                   type=str, default="rank")
    p.add_argument("--score_temperature", help="Temperature of score transformation function", type=float,
                   default=1.0)
    # --- MI355X build additions ---
    p.add_argument("--checkpoint_dir", type=str, default=None,
                   help="Directory for the final checkpoint_<steps> / buffer_checkpoint_<steps> files")
    p.add_argument("--ref_quirk_steps10", action="store_true",
                   help="Run exactly 10 meta-steps like the reference's train.py:55 (ignores --train_steps)")
    p.add_argument("--regret_all_agents", action="store_true",
                   help="alg_regret: also score non-terminated agents (the reference computes and discards them)")
    p.add_argument("--regret_eval", type=str, choices=["sampled", "exact"], default="sampled",
                   help="alg_regret / optimal_regret: evaluate the agents by eval rollouts (sampled, the reference) or "
                        "by the exact expected return of their policies (exact: deterministic, no keys; tabular modes)")
    p.add_argument("--policy_score_eval", type=str, choices=["sampled", "exact"], default="sampled",
                   help="policy_entropy / least_confidence / min_margin: average the policy terms over the agent's "
                        "eval trajectory (sampled), or over the exact state occupancy of its policy on the level "
                        "(exact: deterministic, no keys, no eval rollout; tabular modes)")
    p.add_argument("--occupancy_metrics", action="store_true",
                   help="Log what the agents' exact state occupancy on their levels says each meta-step (an "
                        "'occupancy' dict: episode length, early-termination probability, exact return, collections "
                        "of positive and negative objects, cell coverage; tabular modes)")
    p.add_argument("--level_editor", type=str, choices=["none", "accel"], default="none",
                   help="How the reset round of the PLR scores refills a freed buffer slot: by the level generator "
                        "(none), or with probability --edit_prob by small edits of a high-scoring buffer level (accel)")
    p.add_argument("--staleness_coeff", type=float, default=0.0,
                   help="Weight of PLR's staleness distribution (rounds since a buffer slot was last scored) in the "
                        "replay distribution, in [0, 1]; 0 replays by score alone")
    p.add_argument("--edit_prob", type=float, default=0.5,
                   help="accel: probability that a reset slot takes an edited level instead of a generated one")
    p.add_argument("--num_edits", type=int, default=5, help="accel: edits applied to a parent level")
    p.add_argument("--edit_ops", type=str, default="walls,objects,start",
                   help="accel: comma list of the edit operations drawn from (walls, objects, start, rewards)")
    p.add_argument("--edit_reward_delta", type=float, default=0.1,
                   help="accel: the rewards op moves an object type's reward by uniform(-delta, delta)")
    p.add_argument("--edit_require_solvable", action="store_true",
                   help="accel: refuse an edited level without a positive reward reachable within its episode; the "
                        "slot keeps the generator's level (needs --level_editor accel)")
    p.add_argument("--edit_min_distance", type=int, default=0,
                   help="accel: refuse an edited level closer than this level distance to a level the buffer keeps or "
                        "to an earlier child of the round (1: exact duplicates; 0: no check; needs --level_editor "
                        "accel)")
    p.add_argument("--buffer_diversity", action="store_true",
                   help="Log the level buffer's diversity each meta-step (a 'buffer' dict: share of unique levels, "
                        "mean nearest-neighbour and pairwise level distance; not with --score_function random)")
    p.add_argument("--level_metrics", action="store_true",
                   help="Log the agents' levels' complexity metrics each meta-step (a 'levels' dict: share solvable, "
                        "walls, reachable share, eccentricity, distance to the nearest reward; edit counts)")
    p.add_argument("--ref_quirk_checkpoint_init", action="store_true",
                   help="Checkpoint the initial LPG train state and level buffer, as the reference's _train_fn returns "
                        "them (train.py:52-57: the scan carry is never unpacked)")
    p.add_argument("--fix_value_critic", action="store_true",
                   help="Actually train the meta-gradient value critic (reference discards the update)")
    p.add_argument("--eval_every", type=int, default=0,
                   help="Run the meta-test (toued.evaluate) on the current LPG after every this many meta-steps and "
                        "log it as a 'meta_test' dict (0: never; training itself is unchanged)")
    p.add_argument("--eval_mode", type=str, default="mazes",
                   help="eval_every: environment mode of the held-out levels (tabular modes)")
    p.add_argument("--eval_levels", type=int, default=64, help="eval_every: number of held-out levels")
    p.add_argument("--eval_seed", type=int, default=0,
                   help="eval_every: PRNGKey of the held-out levels and of the evaluation's own keys")
    p.add_argument("--curve_points", type=int, default=11,
                   help="eval_every: points of the learning curve, evenly spaced over the agents' lifetime")
    return p


def parse_args(cmd_args=None):
    args, rest = build_parser().parse_known_args(sys.argv[1:] if cmd_args is None else cmd_args)
    if rest:
        raise ValueError(f"Unknown args {rest}")
    if args.num_agents % args.num_mini_batches != 0:
        raise ValueError(f"Number of agents ({args.num_agents}) must be divisible by number of mini-batches "
                         f"({args.num_mini_batches})")
    if args.edit_require_solvable and args.level_editor != "accel":
        raise ValueError("--edit_require_solvable filters the level editor's children: it needs --level_editor accel")
    if args.edit_min_distance < 0:
        raise ValueError(f"--edit_min_distance {args.edit_min_distance} is negative")
    if args.edit_min_distance and args.level_editor != "accel":
        raise ValueError("--edit_min_distance filters the level editor's children: it needs --level_editor accel")
    if args.buffer_diversity and args.score_function == "random":
        raise ValueError("--buffer_diversity measures the level buffer: --score_function random has none")
    if args.eval_every < 0:
        raise ValueError(f"--eval_every {args.eval_every} is negative")
    if args.eval_every:
        from . import modes
        kw = modes.ENV_MODE_KWARGS.get(args.eval_mode)
        if kw is None or not kw["tabular"]:
            raise ValueError(f"--eval_every needs a tabular --eval_mode: the exact returns the meta-test normalises "
                             f"by are not defined for {args.eval_mode}")
        if args.eval_levels < 1 or args.curve_points < 1:
            raise ValueError(f"--eval_every needs --eval_levels >= 1 and --curve_points >= 1 (got {args.eval_levels}, "
                             f"{args.curve_points})")
    return args
