"""toued.evaluate on the MI355X: the meta-test of a frozen LPG.

  * trace certification: every update of MetaTest.run from the device's own tables before it -- the rollout
    regenerated bit-exactly by oracle/rollout.py from the documented key schedule, the table change within the
    relative-L2 bound tests/test_gpu_es.py holds these kernels to (2e-5 |d_ref| + 1e-7) of oracle/meta.lpg_agent_step,
    ``step`` exact -- with one level's lifetime word at 2 of 4, so discarded updates are covered; F = 5 and F = 7
  * curve points: exact_return is RolloutWrapper.policy_return on the traced tables bit for bit, the sampled
    episode_return is tests/episode_stats_ref.py on the traced trajectories
  * --eval_every leaves training bit-identical and puts ``meta_test`` on the log line
  * checkpoint round trip through the CLI, for a meta-gradient and an ES checkpoint
  * semantics on 16 ``mazes`` levels of --eval_seed 0 with a zero eta
"""
import json

import numpy as np
import pytest
import torch

import episode_stats_ref as er
from oracle import agents as oag
from oracle import jaxrand as jr
from oracle import levels as olv
from oracle import meta as ometa
from oracle import rollout as oro

pytestmark = pytest.mark.gpu

N, W, T, P = 3, 32, 6, 3


def dk(a):
    from toued.prng import from_uint32_numpy
    return from_uint32_numpy(a, "cuda")


def _eval_args(*extra):
    from toued import evaluate as ev
    return ev.parse_eval_args(["--checkpoint_dir", "unused", "--eval_mode", "debug", "--env_workers", str(W),
                               "--train_rollout_len", str(T), "--curve_points", str(P), *extra])


@pytest.fixture(scope="module", params=[5, 7], ids=["F5", "F7"])
def traced(request):
    """One traced meta-test in ``debug`` mode (lifetime 4), level 1's lifetime word overridden to 2 on both sides."""
    from toued import evaluate as ev
    from toued.lpg import init_lpg_params
    F = request.param
    spec = olv.env_spec("debug")
    p_lv, lt = olv.reset_env_params(jr.split(jr.PRNGKey(3), N), "debug")
    lt = np.array(lt, np.int32)
    assert lt.tolist() == [4, 4, 4]
    lt[1] = 2
    packed = olv.pack_levels(p_lv, lt, spec)
    levels = torch.from_numpy(packed).cuda()
    gen = torch.Generator(device="cuda").manual_seed(99)
    eta = init_lpg_params(20 + F, F) + torch.randn(ev.LPGLayout(F).size, device="cuda", generator=gen) * 0.05
    mt = ev.MetaTest(_eval_args(*(["--lifetime_conditioning"] if F == 7 else [])), eta, "cuda")
    mt.trace = []
    rng = jr.PRNGKey(17)
    res = mt.run(levels, dk(rng))
    torch.cuda.synchronize()
    return {"F": F, "spec": spec, "p_lv": p_lv, "lt": lt, "levels": levels, "eta": eta, "mt": mt, "rng": rng,
            "res": res}


def test_trace_certified(traced):
    from test_gpu_env import _state_np
    c = traced
    mt, spec, p_lv, lt, F = c["mt"], c["spec"], c["p_lv"], c["lt"], c["F"]
    D, U = mt.D, 4
    assert c["res"].updates == U and len(mt.trace) == U and c["res"].points == [0, 2, 4]
    # the documented key schedule, from rng alone
    agents_rng, train_rng, _ = jr.split(c["rng"], 3)
    kk = jr.split(jr.split(agents_rng, N), 2)
    ost = oro.batch_reset(spec, kk[:, 0], p_lv, W)
    got0 = _state_np(mt.trace[0]["state"], spec)
    for k in ("time", "pos", "obj_existss", "early_term", "obj_poss"):
        np.testing.assert_array_equal(got0[k], ost[k], err_msg=f"initial env state {k}")
    th0 = np.stack([oag.create_agent(kk[i, 1], D, 8)[0] for i in range(N)])
    ph0 = np.stack([oag.create_agent(kk[i, 1], D, 8)[1] for i in range(N)])
    assert np.array_equal(mt.trace[0]["theta"].cpu().numpy(), th0), "fresh actor tables"
    assert np.array_equal(mt.trace[0]["phi"].cpu().numpy(), ph0), "fresh target-critic tables"
    tk = jr.split(train_rng, N)
    hyp = ometa.Hypers(lifetime_conditioning=F == 7)
    eta64 = torch.tensor(c["eta"].cpu().numpy(), dtype=torch.float64)
    th_k = [r["theta"].cpu().numpy() for r in mt.trace] + [mt.theta.cpu().numpy()]
    ph_k = [r["phi"].cpu().numpy() for r in mt.trace] + [mt.phi.cpu().numpy()]
    st_k = [r["step"].cpu().numpy() for r in mt.trace] + [mt.step.cpu().numpy()]
    steps = np.zeros(N, np.int64)
    for u in range(U):
        s2 = jr.split(tk, 2)
        tk, rk = s2[:, 0], s2[:, 1]
        otr, ost, _ = oro.batch_rollout(spec, rk, th_k[u], p_lv, ost, T)
        tr = mt.trace[u]["traj"]
        for name, got in (("idx", tr.obs_idx), ("time", tr.obs_time), ("action", tr.action), ("reward", tr.reward),
                          ("done", tr.done)):
            g = got.cpu().numpy()
            np.testing.assert_array_equal(g, otr[name].transpose(0, 2, 1).astype(g.dtype),
                                          err_msg=f"rollout {u} {name}")
        assert np.array_equal(st_k[u], steps), ("step", u)
        for a in range(N):
            tr_a = {"idx": otr["idx"][a], "time": otr["time"][a], "action": otr["action"][a].astype(np.int64),
                    "reward": otr["reward"][a], "done": otr["done"][a].astype(bool)}
            th = torch.tensor(th_k[u][a], dtype=torch.float64, requires_grad=True)
            ph = torch.tensor(ph_k[u][a], dtype=torch.float64, requires_grad=True)
            th1, ph1, s1, _, _ = ometa.lpg_agent_step(th, ph, int(steps[a]), int(lt[a]), eta64, tr_a, hyp)
            for got0_, got1_, ref1, nm in ((th_k[u][a], th_k[u + 1][a], th1, "theta"),
                                           (ph_k[u][a], ph_k[u + 1][a], ph1, "phi")):
                d_ref = ref1.detach().numpy() - got0_
                d_dev = got1_.astype(np.float64) - got0_
                assert np.linalg.norm(d_dev - d_ref) <= 2e-5 * np.linalg.norm(d_ref) + 1e-7, (nm, a, u)
            if u >= lt[a]:      # past its lifetime the agent keeps its tables, bit for bit
                assert np.array_equal(th_k[u + 1][a], th_k[u][a]) and np.array_equal(ph_k[u + 1][a], ph_k[u][a])
            else:
                assert not np.array_equal(th_k[u + 1][a], th_k[u][a]), ("an applied update changes theta", a, u)
            steps[a] = s1
    assert np.array_equal(st_k[U], steps) and steps.tolist() == [4, 2, 4]


def test_curve_points(traced):
    c = traced
    mt, res, levels = c["mt"], c["res"], c["levels"]
    L = mt.max_rollout_len
    tables = [mt.trace[0]["theta"], mt.trace[2]["theta"], mt.theta]
    for j, th in enumerate(tables):
        want = mt.ro.policy_return(levels, th.contiguous(), L).cpu().numpy().astype(np.float64)
        assert np.array_equal(res.exact_return[:, j], want), f"point {j}"
    v_opt = mt.ro.optimal_return(levels, L).cpu().numpy().astype(np.float64)
    v_uni = mt.ro.policy_return(levels, torch.zeros_like(mt.theta), L).cpu().numpy().astype(np.float64)
    assert np.array_equal(res.v_opt, v_opt) and np.array_equal(res.v_uniform, v_uni)
    keep = ~res.degenerate
    assert np.array_equal(res.degenerate, ~(v_opt - v_uni > 1e-6))
    np.testing.assert_array_equal(res.normalised[keep],
                                  (res.exact_return[keep] - v_uni[keep, None]) / (v_opt - v_uni)[keep, None])
    # the sampled curve: the restatement on the traced trajectories, carried across the updates, per bucket
    ret = ln = None
    per_update = []
    for r in mt.trace:
        s, ret, ln, mag = er.episode_stats(r["traj"].reward.cpu().numpy(), r["traj"].done.cpu().numpy(), ret, ln)
        per_update.append((s, mag))
    assert np.isnan(res.sampled["episode_return"][:, 0]).all() and not res.sampled["episodes"][:, 0].any()
    for j, us in ((1, (0, 1)), (2, (2, 3))):
        s = sum(per_update[u][0] for u in us)
        mag = sum(per_update[u][1] for u in us)
        assert np.array_equal(res.sampled["episodes"][:, j], s[:, 0])
        has = s[:, 0] > 0
        assert has.any()
        tol = (len(us) * W * T + len(us)) * 2.0 ** -52 * mag[has, 1] / s[has, 0]
        assert np.all(np.abs(res.sampled["episode_return"][has, j] - s[has, 1] / s[has, 0]) <= tol + 1e-300)
        np.testing.assert_allclose(res.sampled["episode_len"][has, j], s[has, 3] / s[has, 0], rtol=1e-15)
        np.testing.assert_allclose(res.sampled["reward_per_step"][:, j], s[:, 4] / s[:, 5], rtol=0,
                                   atol=(len(us) * W * T + len(us)) * 2.0 ** -52 * np.max(mag[:, 4] / s[:, 5]))
    assert np.isfinite(res.exact_return).all()
    json.dumps(res.to_json())


def test_eta_of_the_other_layout_is_refused():
    from toued import evaluate as ev
    with pytest.raises(ValueError, match="--lifetime_conditioning"):
        ev.MetaTest(_eval_args(), torch.zeros(ev.LPGLayout(7).size, device="cuda"), "cuda")
    with pytest.raises(ValueError, match="--lifetime_conditioning"):
        ev.MetaTest(_eval_args("--lifetime_conditioning"), torch.zeros(ev.LPGLayout(5).size, device="cuda"), "cuda")


_TRAIN = ["--env_mode", "debug", "--num_agents", "4", "--num_mini_batches", "1", "--seed", "2", "--score_function",
          "alg_regret", "--buffer_size", "16"]
_EVAL = ["--eval_mode", "debug", "--eval_levels", "3", "--eval_seed", "4", "--curve_points", "3"]


def _train(extra, steps):
    from toued.parse_args import parse_args
    from toued.train import Trainer, reduce_metrics
    tr = Trainer(parse_args(_TRAIN + extra))
    lines = [reduce_metrics(tr.meta_step(), tr.world) for _ in range(steps)]
    tr.finish()
    torch.cuda.synchronize()
    return tr, lines


def test_eval_every_leaves_training_unchanged():
    a, la = _train(["--eval_every", "1"] + _EVAL, 3)
    b, lb = _train([], 3)
    for name, x, y in (("eta", a.eta, b.eta), ("theta", a.agents.theta, b.agents.theta),
                       ("phi", a.agents.phi, b.agents.phi), ("step", a.agents.step, b.agents.step),
                       ("vcrit", a.agents.vcrit, b.agents.vcrit), ("levels", a.agents.levels, b.agents.levels),
                       ("state", a.agents.state, b.agents.state), ("rng", a.rng, b.rng),
                       ("buffer levels", a.buffer.levels, b.buffer.levels), ("buffer score", a.buffer.score, b.buffer.score),
                       ("buffer active", a.buffer.active, b.buffer.active), ("buffer new", a.buffer.new, b.buffer.new),
                       ("adam m", a.adam.m, b.adam.m), ("adam v", a.adam.v, b.adam.v)):
        assert torch.equal(x, y), name
    assert not torch.equal(a.eta, a.eta_init)
    for m, plain in zip(la, lb):
        assert "meta_test" not in plain
        mt = m["meta_test"]
        assert set(mt) == {"final_normalised", "final_exact_return", "auc", "n_degenerate"}
        assert isinstance(mt["n_degenerate"], int) and np.isfinite(mt["final_exact_return"])
        json.dumps(m)
        rest = {k: v for k, v in m.items() if k != "meta_test"}
        assert json.dumps(rest, sort_keys=True) == json.dumps(plain, sort_keys=True)     # (NaN compares as text)
    # with M = 2 only every second line carries it
    _, lc = _train(["--eval_every", "2"] + _EVAL, 2)
    assert "meta_test" not in lc[0] and "meta_test" in lc[1]


@pytest.mark.parametrize("use_es", [False, True], ids=["metagrad", "es"])
def test_checkpoint_round_trip(use_es, tmp_path, capsys):
    from toued import evaluate as ev
    from toued.train import save_final_checkpoints
    extra = ["--use_es", "--lifetime_conditioning"] if use_es else []
    tr, _ = _train(extra + ["--checkpoint_dir", str(tmp_path)], 2)
    save_final_checkpoints(str(tmp_path), tr, 2)
    want = tr.step_fn.es.mean if use_es else tr.eta
    cond = ["--lifetime_conditioning"] if use_es else []
    eta = ev.load_eta(str(tmp_path), 2, use_es, "mean", "cuda")
    assert torch.equal(eta, want) and eta.abs().sum() > 0
    out = tmp_path / "result.json"
    cli = ["--checkpoint_dir", str(tmp_path), "--step", "2", "--env_workers", str(W), "--train_rollout_len", str(T),
           "--baseline", "a2c", "--out", str(out)] + _EVAL + cond
    res = ev.main(cli)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    direct = ev.MetaTest(ev.parse_eval_args(cli), want, "cuda").run(*_drawn(ev))
    for k in ("exact_return", "normalised", "v_opt", "v_uniform"):
        assert np.array_equal(getattr(res, k), getattr(direct, k), equal_nan=True), k
    for k in res.sampled:
        assert np.array_equal(res.sampled[k], direct.sampled[k], equal_nan=True), k
    assert np.array_equal(res.baseline["exact_return"], direct.baseline["exact_return"])
    assert line == json.loads(json.dumps(direct.summary())) and line["n_levels"] == 3 and "baseline" in line
    full = json.loads(out.read_text())
    assert full["levels"]["exact_return"] == direct.exact_return.tolist()
    # the newest checkpoint is found without --step; a wrong layout flag is refused by name
    assert torch.equal(ev.load_eta(str(tmp_path), None, use_es, "mean", "cuda"), want)
    with pytest.raises(ValueError, match="--lifetime_conditioning"):
        ev.load_eta(str(tmp_path), 2, not use_es, "mean", "cuda")


def _drawn(ev):
    levels, sub, rng = ev.draw_levels("debug", 3, 4, "cuda")
    return levels, rng, sub


def test_levels_from_buffer(tmp_path):
    """--levels_from_buffer evaluates on the levels of a checkpointed buffer."""
    from toued import evaluate as ev
    from toued.train import save_final_checkpoints
    tr, _ = _train(["--checkpoint_dir", str(tmp_path)], 1)
    save_final_checkpoints(str(tmp_path), tr, 1)
    res = ev.main(["--checkpoint_dir", str(tmp_path), "--levels_from_buffer", str(tmp_path), "--eval_mode", "debug",
                   "--env_workers", str(W), "--train_rollout_len", str(T), "--curve_points", "2"])
    assert res.exact_return.shape == (16, 2) and np.array_equal(res.lifetime, tr.buffer.levels[:, 5].cpu().numpy())


def test_semantics_zero_eta_on_mazes():
    """A zero eta on the 16 ``mazes`` levels of --eval_seed 0 (checked on the CPU with tests/optret_ref.py and
    tests/polret_ref.py: 1 of the 16 has V* = V^0, within the cap of 4): the run finishes, every return is finite,
    no policy beats the optimum by more than the exact kernels' error scale, and the sub-modes are reported."""
    from toued import evaluate as ev
    from toued.lpg import LPGLayout
    args = ev.parse_eval_args(["--checkpoint_dir", "unused", "--eval_mode", "mazes", "--eval_levels", "16",
                               "--eval_seed", "0", "--curve_points", "5"])
    levels, sub, rng = ev.draw_levels("mazes", 16, 0, "cuda")
    keys = jr.split(jr.PRNGKey(0), 16)
    p_lv, lt = olv.reset_env_params(keys, "mazes")
    assert np.array_equal(levels.cpu().numpy(), olv.pack_levels(p_lv, lt, olv.env_spec("mazes")))
    res = ev.MetaTest(args, torch.zeros(LPGLayout(5).size, device="cuda"), "cuda").run(levels, rng, sub)
    assert res.updates == 2500 and res.points == [0, 625, 1250, 1875, 2500]
    assert np.isfinite(res.exact_return).all() and np.isfinite(res.v_opt).all() and np.isfinite(res.v_uniform).all()
    assert res.n_degenerate <= 4
    keep = ~res.degenerate
    assert np.isfinite(res.normalised[keep]).all() and np.all(res.normalised[keep] <= 1.0 + 1e-6)
    assert np.isfinite(res.sampled["reward_per_step"][:, 1:]).all()
    assert np.all(res.sampled["episodes"][:, 1:] > 0) and np.isfinite(res.sampled["episode_return"][:, 1:]).all()
    assert res.per_mode and sum(m["n_levels"] for m in res.per_mode.values()) == 16
    assert np.isfinite(res.aggregates["final_normalised"]) and np.isfinite(res.aggregates["auc"])
    json.dumps(res.to_json())
