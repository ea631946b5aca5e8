"""Held-out evaluation of a trained update rule: the meta-test of LPG / GROOVE / TA-LPG, with learning curves.

    python -m toued.evaluate --checkpoint_dir D [--step S] [--es_member mean|best]
                             [--eval_mode M --eval_levels n --eval_seed s | --levels_from_buffer D2]
                             [--curve_points P] [--baseline a2c] [--env_workers W] [--train_rollout_len T]
                             [--lifetime_conditioning] [--out FILE.json]

Reads ``D/checkpoint_<S>`` (the newest without --step) as ``toued.train --checkpoint_dir`` writes it: the
meta-gradient train state's ``params``, or with an ES train state the search mean (``--es_member mean``) or the
tracked best member (``best``).  A fresh tabular agent per held-out level is then trained for its whole lifetime by
the FROZEN rule, forward only, and what it learns is reported: does it learn, how fast, how close to optimal.  Prints
one JSON line (the aggregates); ``--out`` receives the whole result, per level and curve point.  Tabular modes only.
The evaluation runs on one GPU: it is not sharded over ranks (``toued.train --eval_every`` runs it on rank 0).

``MetaTest(args, eta).run(levels, rng)``, for n levels [n, 80]:

Key schedule (this project's own: the reference has no meta-test).  Everything derives from ``rng`` alone:
    agents_rng, train_rng, base_rng = split(rng, 3)
    agent i:    key_i = split(agents_rng, n)[i];  worker_rng, agent_rng = split(key_i)        (as _create_agent)
                env state = batch_reset(worker_rng, level_i) over env_workers workers
                actor_rng, critic_rng = split(agent_rng): the lecun actor / target-critic tables   (create_agents)
    training:   t_i = split(train_rng, n)[i];  update u rolls out with the u-th ``_rng`` of the chain
                ``t_i, _rng = split(t_i)`` (toued_key_chain, as ESTrainStep chains its candidates' train keys)
    --baseline: a2c_rng, vcrit_rng = split(base_rng);  the A2C twins' train keys split(a2c_rng, n), their value
                critics' keys split(vcrit_rng, n); the twins start from the LPG agents' initial actor tables and
                env states
    CLI / --eval_every levels: level_i = generator(split(PRNGKey(eval_seed), n)[i]), rng = fold_in(PRNGKey(
                eval_seed), 0x6d657461): a seed names a fixed held-out set and a fixed evaluation.

Training.  U = the largest lifetime word of the levels.  Per update, one launch each: the train rollout
(toued_rollout_draws per 32 updates + toued_rollout_env, or toued_rollout), toued_lpg_inputs, toued_gru_fwd_multi with
one candidate over all n * W rows (nothing saved for a backward), toued_agent_update (or toued_agent_grad +
toued_agent_apply where the fused update does not fit) and toued_episode_stats.  An agent past its own lifetime keeps
its tables (agents/lpg_agent.py:77-80; the update kernels compare ``step`` with the level's lifetime word); its workers
keep acting, so its sampled statistics go on under the frozen tables.

Curve points.  P = --curve_points update counts evenly spaced over 0 .. U, both ends included (``curve_schedule``).  At
each the actor tables are snapshotted; afterwards batched RolloutWrapper.policy_return calls give every (level,
snapshot) pair's exact expected return over eval_rollout_len steps (as many points per call as fit a byte budget),
one optimal_return call V* and one policy_return call on zero tables V^0, the uniform policy's.  Per level and point:
``exact_return``, ``normalised`` = (V^pi - V^0) / (V* - V^0), and from toued_episode_stats over the updates since the
point before (the point's bucket): ``episode_return`` = ret_sum / episodes (NaN for an empty bucket, as the bucket
of point 0 is), its standard error ``episode_return_se``, ``episode_len`` and ``reward_per_step``.  A level with
V* - V^0 <= 1e-6 is degenerate: it is left out of every normalised mean, counted in ``n_degenerate`` and never
divided.  Aggregates: means and standard errors over levels of the final and of the curve values; ``auc`` = the mean
of ``normalised`` over the points.  Manual meta-modes (mazes, tabular) also get them per sub-mode.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, modes, prng
from .env import L_LIFETIME, LevelGenerator, get_agent_hypers, get_env_spec
from .lpg import LPGLayout
from .meta import lpg_inputs_fn

_Y = 8
DRAW_CHUNK = 32                 # updates whose rollout draws are made in one launch (as toued.es)
SNAPSHOT_BYTES = 1 << 30        # actor snapshots held before a policy_return call evaluates them
DEGENERATE_GAP = 1e-6           # V* - V^0 at or below this: the exact kernels' error scale, nothing to normalise
RUN_FOLD = 0x6d657461           # "meta": fold_in(PRNGKey(eval_seed), .) is the evaluation's rng
BASELINES = ("none", "a2c")
ES_MEMBERS = ("mean", "best")


def curve_schedule(U: int, P: int) -> list:
    """The update counts of the curve points: P counts evenly spaced over 0 .. U with both ends, rounded half up,
    duplicates dropped (P > U + 1 gives every count once).  P = 1 is the final point alone; U = 0 is [0]."""
    U, P = int(U), int(P)
    if P < 1 or U < 0:
        raise ValueError(f"curve_schedule: U={U}, P={P} (need U >= 0, P >= 1)")
    if P == 1 or U == 0:
        return [U]
    return sorted({(2 * i * U + (P - 1)) // (2 * (P - 1)) for i in range(P)})


def _mean_se(x: np.ndarray, axis=0):
    """nan-ignoring mean and standard error over ``axis``; NaN where nothing (mean) or fewer than two (se) count."""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x)
    cnt = ok.sum(axis=axis)
    s = np.where(ok, x, 0.0).sum(axis=axis)
    mean = np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)
    d = np.where(ok, x - np.expand_dims(mean, axis), 0.0)
    var = (d * d).sum(axis=axis) / np.maximum(cnt - 1, 1)
    se = np.where(cnt > 1, np.sqrt(var / np.maximum(cnt, 1)), np.nan)
    return mean, se


def normalise(exact: np.ndarray, v_opt: np.ndarray, v_uniform: np.ndarray):
    """(normalised [n, P] with NaN rows for the degenerate levels, degenerate bool [n]).  No degenerate level is
    divided."""
    gap = np.asarray(v_opt, np.float64) - np.asarray(v_uniform, np.float64)
    deg = ~(gap > DEGENERATE_GAP)
    out = np.full(np.shape(exact), np.nan, np.float64)
    keep = ~deg
    out[keep] = (np.asarray(exact, np.float64)[keep] - np.asarray(v_uniform, np.float64)[keep, None]) / gap[keep, None]
    return out, deg


def bucket_stats(stats: np.ndarray) -> dict:
    """toued_episode_stats' columns [n, P, 6] -> the sampled per-bucket values [n, P]."""
    st = np.asarray(stats, np.float64)
    eps, rs, rq, ls, rw, steps = (st[..., i] for i in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(eps > 0, rs / np.maximum(eps, 1), np.nan)
        var = np.where(eps > 1, (rq - eps * mean * mean) / np.maximum(eps - 1, 1), np.nan)
        se = np.sqrt(np.maximum(var, 0.0) / np.maximum(eps, 1))
        length = np.where(eps > 0, ls / np.maximum(eps, 1), np.nan)
        rps = np.where(steps > 0, rw / np.maximum(steps, 1), np.nan)
    return {"episode_return": mean, "episode_return_se": se, "episode_len": length, "reward_per_step": rps,
            "episodes": eps}


def _aggregate(exact, norm, sampled) -> dict:
    """Means and standard errors over levels (axis 0) of the final and the curve values."""
    out = {}
    for name, x in (("exact_return", exact), ("normalised", norm), ("episode_return", sampled["episode_return"]),
                    ("episode_len", sampled["episode_len"]), ("reward_per_step", sampled["reward_per_step"])):
        m, se = _mean_se(x, axis=0)
        out["curve_" + name] = m
        out["curve_" + name + "_se"] = se
        out["final_" + name] = float(m[-1])
        out["final_" + name + "_se"] = float(se[-1])
    # per level the mean over the points (a degenerate level's row is NaN and stays out), then over levels
    out["auc"], out["auc_se"] = (float(v) for v in _mean_se(np.asarray(norm, np.float64).mean(axis=1)))
    return out


@dataclass
class MetaTestResult:
    """What MetaTest.run reports.  Per level and point [n, P] (numpy f64): exact_return, normalised (NaN rows for
    degenerate levels), episode_return, episode_return_se, episode_len, reward_per_step, episodes; per level [n]:
    v_opt, v_uniform, degenerate, lifetime, sub_mode (or None); ``aggregates`` / ``per_mode`` from ``_aggregate``;
    ``baseline``: None or the A2C twins' final values."""
    env_mode: str
    points: list
    updates: int
    exact_return: np.ndarray
    normalised: np.ndarray
    sampled: dict
    v_opt: np.ndarray
    v_uniform: np.ndarray
    degenerate: np.ndarray
    lifetime: np.ndarray
    sub_mode: np.ndarray | None
    aggregates: dict
    per_mode: dict = field(default_factory=dict)
    baseline: dict | None = None

    @property
    def n_degenerate(self) -> int:
        return int(self.degenerate.sum())

    def summary(self) -> dict:
        """The aggregates as plain JSON values (the CLI's stdout line; ``meta_test`` of a training log line holds
        its final_normalised, final_exact_return, auc and n_degenerate)."""
        out = {"env_mode": self.env_mode, "n_levels": int(self.exact_return.shape[0]), "updates": int(self.updates),
               "points": [int(p) for p in self.points], "n_degenerate": self.n_degenerate,
               **_jsonable(self.aggregates)}
        if self.per_mode:
            out["per_mode"] = _jsonable(self.per_mode)
        if self.baseline is not None:
            out["baseline"] = _jsonable({k: v for k, v in self.baseline.items() if not isinstance(v, np.ndarray)})
        return out

    def to_json(self) -> dict:
        """The whole result: the summary and ``levels``, every per-level array."""
        lv = {"exact_return": self.exact_return, "normalised": self.normalised, **self.sampled, "v_opt": self.v_opt,
              "v_uniform": self.v_uniform, "degenerate": self.degenerate, "lifetime": self.lifetime}
        if self.sub_mode is not None:
            lv["sub_mode"] = self.sub_mode
        if self.baseline is not None:
            lv.update({"baseline_" + k: v for k, v in self.baseline.items() if isinstance(v, np.ndarray)})
        return {**self.summary(), "levels": _jsonable(lv)}

    def log_dict(self) -> dict:
        a = self.aggregates
        return {"final_normalised": _jsonable(a["final_normalised"]),
                "final_exact_return": _jsonable(a["final_exact_return"]), "auc": _jsonable(a["auc"]),
                "n_degenerate": self.n_degenerate}


def _jsonable(x):
    """numpy -> plain JSON values; a non-finite float becomes None (JSON has no NaN)."""
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, np.ndarray):
        return _jsonable(x.tolist())
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x) if math.isfinite(float(x)) else None
    return x


def summarise(env_mode, points, updates, exact, v_opt, v_uniform, stats, lifetime, sub_mode=None,
              baseline_exact=None) -> MetaTestResult:
    """The host side of MetaTest.run: exact [n, P], v_opt / v_uniform [n], stats [n, P, 6], all numpy."""
    exact = np.asarray(exact, np.float64)
    norm, deg = normalise(exact, v_opt, v_uniform)
    sampled = bucket_stats(stats)
    agg = _aggregate(exact, norm, sampled)
    per_mode = {}
    names = modes.ENV_MODE_PARAMS.get(env_mode, {}).get("modes") if sub_mode is not None else None
    if names:
        for j, name in enumerate(names):
            sel = np.asarray(sub_mode) == j
            if sel.any():
                per_mode[name] = {"n_levels": int(sel.sum()), "n_degenerate": int(deg[sel].sum()),
                                  **_aggregate(exact[sel], norm[sel], {k: v[sel] for k, v in sampled.items()})}
    baseline = None
    if baseline_exact is not None:
        be = np.asarray(baseline_exact, np.float64)
        bn, _ = normalise(be[:, None], v_opt, v_uniform)
        (me, se), (mn, sn) = _mean_se(be), _mean_se(bn[:, 0])
        baseline = {"name": "a2c", "final_exact_return": float(me), "final_exact_return_se": float(se),
                    "final_normalised": float(mn), "final_normalised_se": float(sn), "exact_return": be,
                    "normalised": bn[:, 0]}
    return MetaTestResult(env_mode, list(points), int(updates), exact, norm, sampled, np.asarray(v_opt, np.float64),
                          np.asarray(v_uniform, np.float64), deg, np.asarray(lifetime), sub_mode, agg, per_mode,
                          baseline)


def _require_tabular(mode: str, what: str):
    if mode not in modes.ENV_MODE_KWARGS:
        raise ValueError(f"{what}: environment mode {mode} is not registered")
    if not modes.ENV_MODE_KWARGS[mode]["tabular"]:
        raise ValueError(f"{what} needs a tabular environment mode: the exact returns it normalises by are not "
                         f"defined for {mode}")


class MetaTest:
    """The meta-test of the frozen rule ``eta`` on the levels of ``args.eval_mode`` (module docstring)."""

    def __init__(self, args, eta: torch.Tensor, device=None):
        from .rollout import RolloutWrapper
        self.mode = args.eval_mode
        _require_tabular(self.mode, "the meta-test")
        self.dev = torch.device(device) if device is not None else eta.device
        self.F = 7 if getattr(args, "lifetime_conditioning", False) else 5
        self.lay = LPGLayout(self.F)
        if eta.numel() != self.lay.size:
            other = LPGLayout(12 - self.F).size
            hint = (" (it is the size of a rule trained " + ("without" if self.F == 7 else "with")
                    + " the flag)") if eta.numel() == other else ""
            raise ValueError(f"eta has {eta.numel()} parameters, the LPG layout with F={self.F} has {self.lay.size}: "
                             f"--lifetime_conditioning must be given as the rule was trained{hint}")
        self.spec, self.max_rollout_len, _ = get_env_spec(self.mode)
        self.W, self.T = int(args.env_workers), int(args.train_rollout_len)
        if self.W % 32:
            raise ValueError(f"env_workers={self.W} must be a multiple of 32 for the MFMA GRU row blocks")
        self.ro = RolloutWrapper(self.mode, self.T, self.max_rollout_len, self.W)      # its own: no shared buffers
        self.D = self.ro.obs_dim
        self.P = int(getattr(args, "curve_points", 11))
        if self.P < 1:
            raise ValueError(f"--curve_points {self.P}: at least one point")
        self.baseline = getattr(args, "baseline", "none") or "none"
        if self.baseline not in BASELINES:
            raise ValueError(f"--baseline {self.baseline} not in {BASELINES}")
        h = get_agent_hypers(self.mode)
        from .agents import AgentHyperparams
        self.ah = AgentHyperparams(**h, critic_dims=_Y)
        self.ah.check_supported()
        self.alpha_y = float(getattr(args, "lpg_agent_target_coeff", 0.5))
        self.a2c_hyp = (float(getattr(args, "gamma", 0.99)), float(getattr(args, "gae_lambda", 0.95)),
                        float(getattr(args, "entropy_coeff", 0.01)))
        self.eta = eta.detach().to(self.dev, torch.float32).reshape(1, -1).contiguous().clone()
        self.fwdA = torch.zeros((1, _lib.lib().toued_gru_packed_floats(2)), dtype=torch.float32, device=self.dev)
        _lib.call("toued_gru_pack_fwd_multi", _lib.ptr(self.eta), self.lay.size, 1, self.lay.c_offsets, self.F,
                  _lib.ptr(self.fwdA), _lib.stream_ptr())
        self.fused_update = bool(_lib.lib().toued_agent_update_fits(self.W, self.T, self.D))
        # test hook: a list receives, per update, the device clones ESTrainStep.trace records: the tables and the env
        # state before the update's rollout, ``step`` and the trajectory
        self.trace = None
        self.timers = None          # a toued.meta.KernelTimers: HIP-event timing of the per-update launches
        self._bufs = {}

    def _alloc(self, n):
        if self._bufs.get("n") != n:
            W, T, D, dev = self.W, self.T, self.D, self.dev
            R = n * W
            f32, i32, u8 = torch.float32, torch.int32, torch.uint8
            z = lambda *s, dt=f32: torch.zeros(s, dtype=dt, device=dev)
            from .rollout import Transition
            self._bufs = {
                "n": n, "tr": Transition(z(n, T + 1, W, dt=i32), z(n, T + 1, W, dt=i32), z(n, T, W, dt=u8),
                                         z(n, T, W), z(n, T, W, dt=u8)),
                "X": z(self.F, T, R), "pi_hat": z(T, R), "y_hat": z(T, _Y, R), "met": z(n, 8), "gstat": z(n, 4),
                "G_th": None if self.fused_update else z(n, D, 5), "G_ph": None if self.fused_update else z(n, D, _Y),
                "draws": None,
            }
        return self._bufs

    def _draw_bufs(self, b, n, m):
        """(key-chain scratch, draws) of m <= DRAW_CHUNK updates' train rollouts, views of two [T][32 n W][4] buffers."""
        if b["draws"] is None:
            b["draws"] = tuple(torch.empty((self.T, DRAW_CHUNK * n * self.W, 4), dtype=torch.int32, device=self.dev)
                               for _ in range(2))
        k = self.T * m * n * self.W * 4
        return tuple(x.view(-1)[:k].view(self.T, m * n * self.W, 4) for x in b["draws"])

    def create_agents(self, rng: torch.Tensor, levels: torch.Tensor):
        """The fresh agents and keys of the module docstring: (theta, phi, env state, train keys [n, 2], base_rng)."""
        from .agents import create_agents
        n = levels.shape[0]
        ks = prng.split(rng.reshape(2), 3)
        agents_rng, train_rng, base_rng = (ks[i].contiguous() for i in range(3))
        kk = prng.split_planar(prng.split(agents_rng, n), 2)       # kk[0] worker_rng, kk[1] agent_rng
        (_, _), state = self.ro.batch_reset(kk[0], levels)
        theta, phi = create_agents(kk[1], self.D, _Y)
        return theta, phi, state, prng.split(train_rng, n).contiguous(), base_rng

    def run(self, levels: torch.Tensor, rng: torch.Tensor, sub_modes=None) -> MetaTestResult:
        """levels int32 [n, 80] of this mode, rng int32 [2].  ``sub_modes``: int [n] the levels' sub-mode indices of
        a manual meta-mode (LevelGenerator(..., with_sub_mode=True)), for the per-mode aggregates."""
        from .rollout import Transition, split_rollouts
        L, ptr = _lib, _lib.ptr
        levels = levels.to(self.dev).contiguous()
        n = levels.shape[0]
        if n == 0:
            raise ValueError("the meta-test needs at least one level")
        W, T, D, F = self.W, self.T, self.D, self.F
        R, nd = n * W, self.lay.size
        lifetime = levels[:, L_LIFETIME].cpu().numpy()
        U = int(lifetime.max())
        points = curve_schedule(U, self.P)
        Pn = len(points)
        theta, phi, state, train_keys, base_rng = self.create_agents(rng, levels)
        step = torch.zeros(n, dtype=torch.int32, device=self.dev)
        theta0, state0 = (theta.clone(), state.clone()) if self.baseline == "a2c" else (None, None)
        b = self._alloc(n)
        tr = b["tr"]
        b["met"].zero_()
        chain = torch.empty((max(U, 1), n, 2), dtype=torch.int32, device=self.dev)
        if U:
            L.call("toued_key_chain", ptr(train_keys), n, U, ptr(chain), L.stream_ptr())
        theta_alt = phi_alt = None
        if not self.fused_update:
            theta_alt, phi_alt = torch.empty_like(theta), torch.empty_like(phi)
        e1w, e1b, e2w, e2b = (self.eta.view(-1)[self.lay.offsets[k]:] for k in ("e1_w", "e1_b", "e2_w", "e2_b"))
        # snapshots: as many points as the byte budget holds, evaluated by one policy_return call when full
        cap = max(1, min(Pn, SNAPSHOT_BYTES // max(1, theta.numel() * 4)))
        snaps = torch.empty((cap, n, D, 5), dtype=torch.float32, device=self.dev)
        lev_rep = levels.repeat(cap, 1).contiguous()
        exact = torch.empty((Pn, n), dtype=torch.float32, device=self.dev)
        stats = torch.zeros((Pn, n, 6), dtype=torch.float64, device=self.dev)
        run_ret = torch.zeros((n, W), dtype=torch.float32, device=self.dev)
        run_len = torch.zeros((n, W), dtype=torch.int32, device=self.dev)
        held = [0, 0]           # points [held[0], held[1]) are in snaps

        def flush():
            m = held[1] - held[0]
            if m:
                exact[held[0]:held[1]] = self.ro.policy_return(lev_rep[:m * n], snaps[:m].reshape(m * n, D, 5),
                                                               self.max_rollout_len).view(m, n)
            held[0] = held[1]

        def snapshot(th):
            if held[1] - held[0] == cap:
                flush()
            snaps[held[1] - held[0]].copy_(th)
            held[1] += 1

        tm = self.timers
        timed = (lambda name: tm.start(name)) if tm is not None and tm.enabled else (lambda name: None)
        done_t = (lambda tok: tm.stop(tok)) if tm is not None and tm.enabled else (lambda tok: None)
        split = split_rollouts()
        draws = None
        pi = 0                  # the next curve point
        for u in range(U):
            if points[pi] == u:
                snapshot(theta)
                pi += 1
            if self.trace is not None:
                rec = {"theta": theta.clone(), "phi": phi.clone(), "state": state.clone(), "step": step.clone()}
            st = L.stream_ptr()
            tok = timed("rollout")
            if split:
                if u % DRAW_CHUNK == 0:
                    m = min(DRAW_CHUNK, U - u)
                    draws = self.ro.train_draws(chain[u:u + m], levels, W, self._draw_bufs(b, n, m))
                self.ro.rollout_from_draws(draws, u % DRAW_CHUNK, theta, levels, state, tr)
            else:
                self.ro.batch_rollout(chain[u], theta, levels, state, out=tr, inplace_state=True)
            done_t(tok)
            if self.trace is not None:
                rec["traj"] = Transition(tr.obs_idx.clone(), tr.obs_time.clone(), tr.action.clone(),
                                         tr.reward.clone(), tr.done.clone())
                self.trace.append(rec)
            tok = timed("lpg_inputs")
            L.call(lpg_inputs_fn(R, W), n, W, T, D, F, ptr(theta), ptr(phi), ptr(tr.obs_idx), ptr(tr.obs_time),
                   ptr(tr.action), ptr(tr.reward), ptr(tr.done), ptr(e1w), ptr(e1b), ptr(e2w), ptr(e2b), ptr(step),
                   ptr(levels), ptr(b["X"]), T * R, 1, 0, st)
            done_t(tok)
            tok = timed("gru_fwd_multi")
            L.call("toued_gru_fwd_multi", R, T, W, F, R, ptr(b["X"]), T * R, 1, ptr(tr.done), ptr(self.fwdA),
                   ptr(self.eta), nd, self.lay.c_offsets, ptr(b["pi_hat"]), ptr(b["y_hat"]), st)
            done_t(tok)
            tok = timed("agent_update")
            if self.fused_update:
                L.call("toued_agent_update", n, W, T, D, ptr(theta), ptr(phi), ptr(tr.obs_idx), ptr(tr.obs_time),
                       ptr(tr.action), ptr(tr.reward), ptr(tr.done), ptr(b["pi_hat"]), ptr(b["y_hat"]), self.alpha_y,
                       self.ah.actor_learning_rate, self.ah.critic_learning_rate, self.ah.max_grad_norm,
                       ptr(b["met"]), ptr(step), ptr(levels), ptr(b["gstat"]), st)
            else:
                b["G_th"].zero_()
                b["G_ph"].zero_()
                L.call("toued_agent_grad", n, W, T, D, ptr(theta), ptr(phi), ptr(tr.obs_idx), ptr(tr.obs_time),
                       ptr(tr.action), ptr(tr.reward), ptr(tr.done), ptr(b["pi_hat"]), ptr(b["y_hat"]), self.alpha_y,
                       ptr(b["G_th"]), ptr(b["G_ph"]), ptr(b["met"]), ptr(step), ptr(levels), ptr(b["gstat"]), st)
                L.call("toued_agent_apply", n, D, ptr(theta), ptr(phi), ptr(b["G_th"]), ptr(b["G_ph"]),
                       self.ah.actor_learning_rate, self.ah.critic_learning_rate, self.ah.max_grad_norm, ptr(step),
                       ptr(theta_alt), ptr(phi_alt), ptr(b["gstat"]), st)
                theta, theta_alt, phi, phi_alt = theta_alt, theta, phi_alt, phi
            done_t(tok)
            tok = timed("episode_stats")
            # the bucket of the next point: updates (points[pi - 1], points[pi]]
            L.call("toued_episode_stats", n, W, T, ptr(tr.reward), ptr(tr.done), ptr(run_ret), ptr(run_len),
                   ptr(stats[pi]), st)
            done_t(tok)
        assert points[pi] == U and pi == Pn - 1
        snapshot(theta)
        flush()
        v_opt = self.ro.optimal_return(levels, self.max_rollout_len)
        v_uni = self.ro.policy_return(levels, torch.zeros_like(theta), self.max_rollout_len)
        base = None
        if self.baseline == "a2c":
            base = self._a2c_twins(base_rng, theta0, state0, levels, U)
        self.theta, self.phi, self.step, self.state = theta, phi, step, state       # the trained agents
        cpu = lambda t: t.cpu().numpy()
        return summarise(self.mode, points, U, cpu(exact).T, cpu(v_opt), cpu(v_uni),
                         cpu(stats).transpose(1, 0, 2), lifetime,
                         None if sub_modes is None else np.asarray(cpu(sub_modes) if torch.is_tensor(sub_modes)
                                                                   else sub_modes),
                         None if base is None else cpu(base))

    def _a2c_twins(self, base_rng, theta0, state0, levels, U):
        """--baseline a2c: the agents' twins (same initial actor tables and env states) trained by the A2C antagonist's
        trainer for U updates (an agent past its lifetime keeps its tables there too); their exact returns f32 [n]."""
        from .a2c import A2CHyperparams, A2CTrainer
        from .agents import create_value_critics
        n = levels.shape[0]
        ks = prng.split(base_rng.reshape(2), 2)
        a2c_keys = prng.split(ks[0].contiguous(), n).contiguous()
        vcrit = create_value_critics(prng.split(ks[1].contiguous(), n).contiguous(), self.D)
        trainer = A2CTrainer(self.ro, A2CHyperparams(*self.a2c_hyp), self.ah, use_graph=False)
        step = torch.zeros(n, dtype=torch.int32, device=self.dev)
        trainer.train(a2c_keys, theta0, vcrit, step, levels, state0, U)
        return self.ro.policy_return(levels, theta0, self.max_rollout_len)


def draw_levels(mode: str, n: int, seed: int, device=None):
    """The held-out set a seed names: (levels [n, 80] = generator(split(PRNGKey(seed), n)), their sub-mode indices
    for a manual meta-mode or None, the evaluation's rng = fold_in(PRNGKey(seed), RUN_FOLD))."""
    _require_tabular(mode, "the meta-test")
    key = prng.PRNGKey(seed, device)
    gen = LevelGenerator(mode, key.device)
    levels, sub = gen(prng.split(key, n).contiguous(), with_sub_mode=True)
    manual = bool(modes.ENV_MODE_PARAMS[mode].get("manual"))
    return levels, (sub if manual else None), prng.fold_in(key, RUN_FOLD).contiguous()


def load_eta(checkpoint_dir: str, step, lifetime_conditioning: bool, es_member: str = "mean", device=None):
    """The rule of ``checkpoint_<step>`` as the flat f32 eta on the device: the meta-gradient train state's params, or
    an ES train state's search mean / tracked best member."""
    from .checkpoint import lpg_flat_from_tree, restore_checkpoint
    lay = LPGLayout(7 if lifetime_conditioning else 5)
    state = restore_checkpoint(checkpoint_dir, step=step)
    if "es_state" in state:
        if es_member not in ES_MEMBERS:
            raise ValueError(f"--es_member {es_member} not in {ES_MEMBERS}")
        flat = np.asarray(state["es_state"]["mean" if es_member == "mean" else "best_member"], np.float32).reshape(-1)
        if flat.size != lay.size:
            raise ValueError(f"the checkpoint's ES member has {flat.size} parameters, the LPG layout has {lay.size}: "
                             f"--lifetime_conditioning must be given as the rule was trained")
    else:
        try:
            flat = lpg_flat_from_tree(state["params"], lay)
        except ValueError as e:
            raise ValueError(f"{e}: --lifetime_conditioning must be given as the rule was trained") from None
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.array(flat, np.float32)).to(dev)      # (a copy: restored leaves are read-only views)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint_dir", type=str, required=True, help="directory of checkpoint_<step>")
    ap.add_argument("--step", type=int, default=None, help="the checkpoint's step (default: the newest)")
    ap.add_argument("--es_member", type=str, default="mean", help="ES checkpoints: the search mean, or the best member")
    ap.add_argument("--eval_mode", type=str, default="mazes", help="environment mode of the held-out levels (tabular)")
    ap.add_argument("--eval_levels", type=int, default=64, help="number of held-out levels drawn")
    ap.add_argument("--eval_seed", type=int, default=0, help="PRNGKey of the held-out levels and of the evaluation")
    ap.add_argument("--levels_from_buffer", type=str, default=None,
                    help="take the levels of this directory's newest buffer checkpoint instead of drawing them")
    ap.add_argument("--curve_points", type=int, default=11, help="points of the learning curve, 0 .. lifetime")
    ap.add_argument("--baseline", type=str, default="none", help="none, or a2c: also train A2C twins of the agents")
    ap.add_argument("--env_workers", type=int, default=64)
    ap.add_argument("--train_rollout_len", type=int, default=20)
    ap.add_argument("--lifetime_conditioning", action="store_true", help="the rule was trained with it (F = 7)")
    ap.add_argument("--lpg_agent_target_coeff", type=float, default=5e-1)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae_lambda", type=float, default=0.95)
    ap.add_argument("--entropy_coeff", type=float, default=0.01)
    ap.add_argument("--out", type=str, default=None, help="write the whole result (per level and point) as JSON")
    return ap


def parse_eval_args(cmd_args=None):
    a, rest = build_parser().parse_known_args(sys.argv[1:] if cmd_args is None else cmd_args)
    if rest:
        raise ValueError(f"Unknown args {rest}")
    _require_tabular(a.eval_mode, "the meta-test")
    if a.es_member not in ES_MEMBERS:
        raise ValueError(f"--es_member {a.es_member} not in {ES_MEMBERS}")
    if a.baseline not in BASELINES:
        raise ValueError(f"--baseline {a.baseline} not in {BASELINES}")
    if a.curve_points < 1:
        raise ValueError(f"--curve_points {a.curve_points}: at least one point")
    if a.eval_levels < 1:
        raise ValueError(f"--eval_levels {a.eval_levels}: at least one level")
    if a.env_workers < 1 or a.env_workers % 32:
        raise ValueError(f"--env_workers {a.env_workers} must be a positive multiple of 32")
    if a.train_rollout_len < 1:
        raise ValueError(f"--train_rollout_len {a.train_rollout_len}: at least one step")
    return a


def main(cmd_args=None):
    a = parse_eval_args(cmd_args)
    dev = torch.device("cuda", torch.cuda.current_device())
    eta = load_eta(a.checkpoint_dir, a.step, a.lifetime_conditioning, a.es_member, dev)
    mt = MetaTest(a, eta, dev)
    if a.levels_from_buffer:
        from .checkpoint import level_buffer_from_state_dict, restore_checkpoint
        buf = level_buffer_from_state_dict(restore_checkpoint(a.levels_from_buffer, prefix="buffer_"), mt.spec, dev)
        levels, sub = buf.levels, None
        rng = prng.fold_in(prng.PRNGKey(a.eval_seed, dev), RUN_FOLD).contiguous()
    else:
        levels, sub, rng = draw_levels(a.eval_mode, a.eval_levels, a.eval_seed, dev)
    res = mt.run(levels, rng, sub)
    _lib.check_device_errors(wait=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res.to_json(), f)
    print(json.dumps(res.summary()), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
