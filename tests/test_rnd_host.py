"""Random network distillation on the host: the cfg and its refusals, the weight
schedules, the plain path's reward pass and predictor step, the weight-zero invariance the forked
RNG is for, the checkpoints and the task registrations."""
import copy
import warnings

import pytest
import torch

from fake_env import FakeEnv
from rsl_rl.algorithms import PPO, Distillation
from rsl_rl.modules import ActorCritic, ActorCriticRecurrent, StudentTeacher
from rsl_rl.modules.rnd import RandomNetworkDistillation, parse_cfg, weight_at
from rsl_rl.runners import OnPolicyRunner

N, T, O, P, A = 16, 8, 6, 9, 3
RND = dict(weight=0.5, num_outputs=4, predictor_hidden_dims=[16, 8], target_hidden_dims=[8, 8], learning_rate=1e-2)


def _cfg(rnd=None, **runner):
    cfg = {"runner": {"policy_class_name": "ActorCritic", "algorithm_class_name": "PPO", "num_steps_per_env": T,
                      "save_interval": 50, **runner},
           "algorithm": {"num_learning_epochs": 2, "num_mini_batches": 2, "learning_rate": 1e-3},
           "policy": {"actor_hidden_dims": [16], "critic_hidden_dims": [16], "activation": "elu", "init_noise_std": 1.0}}
    if rnd is not None:
        cfg["algorithm"]["rnd_cfg"] = rnd
    return cfg


def _runner(rnd=None, priv=P, seed=3, log_dir=None, **runner):
    torch.manual_seed(seed)
    return OnPolicyRunner(FakeEnv(num_envs=N, num_obs=O, num_actions=A, num_privileged_obs=priv), _cfg(rnd, **runner),
                          log_dir=log_dir, device="cpu")


def _policy():
    return ActorCritic(O, P, A, actor_hidden_dims=[16], critic_hidden_dims=[16])


# ------------------------------------------------------------------------ cfg --
def test_unknown_key_raises():
    with pytest.raises(ValueError, match=r"rnd_cfg: unknown keys \['wieght'\]"):
        PPO(_policy(), rnd_cfg=dict(RND, wieght=1.0))
    with pytest.raises(ValueError, match="weight_schedule: unknown mode"):
        parse_cfg(dict(RND, weight_schedule={"mode": "cosine"}))
    with pytest.raises(ValueError, match="takes exactly the keys"):
        parse_cfg(dict(RND, weight_schedule={"mode": "step", "final_step": 3}))
    with pytest.raises(ValueError, match="rnd_cfg.state"):
        parse_cfg(dict(RND, state="rnd_state"))


@pytest.mark.parametrize("key", ["reward_normalization", "state_normalization"])
def test_normalisers_are_refused(key):
    with pytest.raises(ValueError, match=f"rnd_cfg.{key} is not supported"):
        PPO(_policy(), rnd_cfg=dict(RND, **{key: True}))


def test_recurrent_symmetry_and_distillation_are_refused():
    rec = ActorCriticRecurrent(O, P, A, actor_hidden_dims=[16], critic_hidden_dims=[16], rnn_type="lstm",
                               rnn_hidden_size=8, rnn_num_layers=1)
    with pytest.raises(ValueError, match="rnd_cfg is not supported for recurrent policies"):
        PPO(rec, rnd_cfg=RND)
    ident = (list(range(O)), [1.0] * O), (list(range(P)), [1.0] * P), (list(range(A)), [1.0] * A)
    with pytest.raises(ValueError, match="rnd_cfg with symmetry_cfg.use_data_augmentation is not supported"):
        PPO(_policy(), symmetry_cfg={"use_data_augmentation": True}, symmetry_tables=ident, rnd_cfg=RND)
    st = StudentTeacher(O, P, A, student_hidden_dims=[16, 8], teacher_hidden_dims=[8, 8])
    with pytest.raises(ValueError, match="Distillation does not support rnd_cfg"):
        Distillation(st, rnd_cfg=RND)
    Distillation(st, rnd_cfg=dict(RND, weight=0.0))  # switched off: nothing to refuse


def test_world_size_above_one_is_refused(monkeypatch):
    from rsl_rl.algorithms import ppo
    monkeypatch.setattr(ppo, "_dist_world", lambda: 2)
    alg = ppo.PPO.__new__(ppo.PPO)  # (the constructor would go on to broadcast the parameters)
    alg._sym = None
    with pytest.raises(ValueError, match="torch.distributed world size above 1"):
        alg._rnd_refusals(_policy(), RND)
    monkeypatch.setattr(ppo, "_dist_world", lambda: 1)
    assert alg._rnd_refusals(_policy(), RND)["weight"] == 0.5


@pytest.mark.parametrize("cfg", [None, {}, {"weight": 0.0}, dict(RND, weight=0.0, weight_schedule=None)])
def test_weight_zero_without_a_schedule_builds_nothing(cfg):
    assert parse_cfg(cfg) is None
    alg = PPO(_policy(), rnd_cfg=cfg)
    alg.init_storage(N, T, [O], [P], [A])
    assert alg.rnd is None and alg.rnd_optimizer is None
    runner = _runner(cfg)
    assert runner.alg.rnd is None


def test_defaults():
    cfg = parse_cfg({"weight": 1.0})
    assert cfg["learning_rate"] == 1e-3 and cfg["num_outputs"] == 16 and cfg["state"] == "critic"
    assert cfg["predictor_hidden_dims"] == cfg["target_hidden_dims"] == [256, 128, 64] and cfg["seed"] == 0


# ------------------------------------------------------------------ schedules --
def test_schedules():
    assert weight_at(0.5, None, 10 ** 6) == 0.5
    assert weight_at(0.5, {"mode": "constant"}, 10 ** 6) == 0.5
    step = {"mode": "step", "final_step": 10, "final_value": 0.125}
    assert [weight_at(0.5, step, s) for s in (0, 9, 10, 11)] == [0.5, 0.5, 0.125, 0.125]
    lin = {"mode": "linear", "initial_step": 4, "final_step": 12, "final_value": 0.0}
    assert [weight_at(0.5, lin, s) for s in (0, 3, 4, 6, 8, 12, 13, 100)] == [0.5, 0.5, 0.5, 0.375, 0.25, 0.0, 0.0, 0.0]
    rnd = RandomNetworkDistillation(O, parse_cfg(dict(RND, weight_schedule=step)))
    x = torch.randn(5, O)
    for k in range(12):  # the per-step statement advances the counter
        want = rnd.error(x) * (0.5 if k < 10 else 0.125)
        assert torch.equal(rnd.get_intrinsic_reward(x), want)
    assert rnd.update_counter == 12


def test_forked_rng_and_seed():
    torch.manual_seed(11)
    before = torch.get_rng_state()
    a = RandomNetworkDistillation(O, parse_cfg(RND))
    assert torch.equal(torch.get_rng_state(), before)
    b = RandomNetworkDistillation(O, parse_cfg(RND))
    c = RandomNetworkDistillation(O, parse_cfg(dict(RND, seed=1)))
    for p, q, r in zip(a.parameters(), b.parameters(), c.parameters()):
        assert torch.equal(p, q)
    assert not torch.equal(next(a.parameters()), next(c.parameters()))
    assert all(not p.requires_grad for p in a.target.parameters())
    assert all(p.requires_grad for p in a.predictor.parameters())


# ------------------------------------------------------------ the plain path --
def _collect(runner):
    """One eager rollout; returns (obs, critic_obs) at its end."""
    obs = runner.env.get_observations()
    cobs = runner.env.get_privileged_observations()
    cobs = obs if cobs is None else cobs
    for _ in range(T):
        obs, cobs, *_ = runner._collect_step(obs, cobs)
    return obs, cobs


@pytest.mark.parametrize("state,priv", [("critic", P), ("policy", P), ("critic", None)])
def test_reward_pass_is_the_torch_statement(state, priv):
    sched = {"mode": "linear", "initial_step": 2, "final_step": 3 * T, "final_value": 0.0}
    runner = _runner(dict(RND, state=state, weight_schedule=sched), priv=priv)
    alg = runner.alg
    assert alg.rnd is not None and alg._rnd_fused is None
    want_width = P if (state == "critic" and priv) else O
    assert alg.rnd.num_states == want_width
    for it in range(2):
        _, cobs = _collect(runner)
        st = alg.storage
        before = st.rewards.clone()
        rows = (st.privileged_observations if want_width == P else st.observations).flatten(0, 1)
        with torch.no_grad():
            d = alg.rnd.target(rows) - alg.rnd.predictor(rows)
            r = torch.sqrt((d * d).sum(dim=1))
        w = torch.tensor([weight_at(0.5, sched, it * T + t) for t in range(T)]).repeat_interleave(N)
        alg.compute_returns(cobs)
        assert torch.equal(st.rewards, before + (w * r).view(T, N, 1))
        assert not torch.equal(st.rewards, before)
        torch.testing.assert_close(alg._rnd_stats, torch.stack([(w * r).mean(), r.mean()]))
        alg.update()
    assert alg.rnd.update_counter == 2 * T


def test_target_frozen_predictor_trained_policy_untouched():
    runner = _runner(RND)
    alg = runner.alg
    tgt0 = copy.deepcopy(alg.rnd.target.state_dict())
    pred0 = copy.deepcopy(alg.rnd.predictor.state_dict())
    seen = []
    plain = alg._rnd_minibatch_step

    def spy(batch):
        grads = [None if p.grad is None else p.grad.clone() for p in alg.actor_critic.parameters()]
        plain(batch)
        after = [None if p.grad is None else p.grad for p in alg.actor_critic.parameters()]
        seen.append(all((a is None and b is None) or torch.equal(a, b) for a, b in zip(grads, after)))
    alg._rnd_minibatch_step = spy
    losses = []
    for _ in range(2):
        _, cobs = _collect(runner)
        alg.compute_returns(cobs)
        alg.update()
        losses.append(float(alg.rnd_loss_mean))
    assert len(seen) == 2 * 2 * 2 and all(seen)  # 2 updates x 2 epochs x 2 mini-batches
    for k, v in alg.rnd.target.state_dict().items():
        assert torch.equal(v, tgt0[k]), k
    for k, v in alg.rnd.predictor.state_dict().items():
        assert not torch.equal(v, pred0[k]), k
    assert all(p.grad is None for p in alg.rnd.target.parameters())
    assert losses[0] > 0 and losses[1] < losses[0]  # the predictor learns the target on these rows
    # the loss is the mean over mb x E entries, averaged over the update's steps
    assert set(alg.rnd_optimizer.state[p]["step"] if not torch.is_tensor(alg.rnd_optimizer.state[p]["step"])
               else float(alg.rnd_optimizer.state[p]["step"]) for p in alg.rnd.predictor.parameters()) == {8.0}


def test_weight_zero_invariance():
    """RND on under a schedule that holds the weight at 0 trains the policy of an RND-off run,
    bit for bit: the nets are initialised under a forked RNG and nothing else draws."""
    zero = dict(RND, weight=0.0, weight_schedule={"mode": "constant"})
    off = _runner(None)  # (each seeds the global stream, builds and trains before the other starts)
    off.learn(2)
    on = _runner(zero)
    on.learn(2)
    assert on.alg.rnd is not None and off.alg.rnd is None
    for p, q in zip(off.alg.actor_critic.parameters(), on.alg.actor_critic.parameters()):
        assert torch.equal(p, q)
    assert float(on.alg.rnd_loss_mean) > 0  # the predictor trained all the same


def test_empirical_normalization_rows():
    """With empirical_normalization on, the rows RND sees are the storage's (normalised) rows."""
    runner = _runner(RND, empirical_normalization=True)
    alg = runner.alg
    _, cobs = _collect(runner)
    assert alg._rnd_states().data_ptr() == alg.storage.privileged_observations.data_ptr()
    seen = []
    err = alg.rnd.error
    alg.rnd.error = lambda rows: (seen.append(rows.clone()), err(rows))[1]
    alg.compute_returns(cobs)
    assert len(seen) == 1 and torch.equal(seen[0], alg.storage.privileged_observations.flatten(0, 1))


# ---------------------------------------------------------------- checkpoints --
def test_checkpoint_round_trip(tmp_path):
    runner = _runner(RND, log_dir=str(tmp_path))
    runner.learn(2)
    ck = torch.load(tmp_path / "model_2.pt", weights_only=True)
    assert {"rnd_state_dict", "rnd_optimizer_state_dict"} <= set(ck)
    r2 = _runner(RND, seed=9)
    assert not torch.equal(next(r2.alg.actor_critic.parameters()), next(runner.alg.actor_critic.parameters()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r2.load(str(tmp_path / "model_2.pt"))
    for (k, v), (_, u) in zip(r2.alg.rnd.state_dict().items(), runner.alg.rnd.state_dict().items()):
        assert torch.equal(v, u), k
    for p, q in zip(r2.alg.rnd.predictor.parameters(), runner.alg.rnd.predictor.parameters()):
        s2, s1 = r2.alg.rnd_optimizer.state[p], runner.alg.rnd_optimizer.state[q]
        assert torch.equal(s2["exp_avg"], s1["exp_avg"]) and torch.equal(s2["exp_avg_sq"], s1["exp_avg_sq"])
        assert float(s2["step"]) == float(s1["step"]) == 8.0
        assert s1["exp_avg"].abs().sum() > 0
    assert r2.alg.rnd_iteration == 2  # the schedule's counter follows the loaded iteration


def test_checkpoint_without_rnd_loads_with_a_warning(tmp_path):
    old = _runner(None, log_dir=str(tmp_path))
    old.learn(1)
    ck = torch.load(tmp_path / "model_1.pt", weights_only=True)
    assert "rnd_state_dict" not in ck
    r2 = _runner(RND, seed=9)
    fresh = copy.deepcopy(r2.alg.rnd.state_dict())
    with pytest.warns(UserWarning, match="holds no rnd_state_dict"):
        r2.load(str(tmp_path / "model_1.pt"))
    for p, q in zip(r2.alg.actor_critic.parameters(), old.alg.actor_critic.parameters()):
        assert torch.equal(p, q)
    for k, v in r2.alg.rnd.state_dict().items():
        assert torch.equal(v, fresh[k])
    r2.learn(1)


def test_logging(tmp_path, monkeypatch, capsys):
    import json
    from rsl_rl.runners import on_policy_runner as opr
    monkeypatch.setattr(opr, "_make_writer", opr._JsonlWriter)  # whichever writer is installed: this one is read
    sched = {"mode": "linear", "initial_step": 0, "final_step": 4 * T, "final_value": 0.0}
    runner = _runner(dict(RND, weight=1.5e-5, weight_schedule=sched), log_dir=str(tmp_path))
    runner.learn(2)
    runner.writer.flush()
    rows = [json.loads(line) for line in (tmp_path / "scalars.jsonl").read_text().splitlines()]
    for tag in ("Loss/rnd", "Rnd/mean_intrinsic_reward", "Rnd/weight"):
        vals = [r["value"] for r in rows if r["tag"] == tag]
        assert len(vals) == 2 and all(v > 0 for v in vals), tag
    # the logged weight is the schedule's at the counter after each rollout
    assert [r["value"] for r in rows if r["tag"] == "Rnd/weight"] == [weight_at(1.5e-5, sched, T),
                                                                       weight_at(1.5e-5, sched, 2 * T)]
    out = capsys.readouterr().out
    assert "RND loss:" in out and "(weight 1.125e-05)" in out and "(weight 7.500e-06)" in out  # small weights stay legible


# ---------------------------------------------------------------------- tasks --
def test_tasks_are_registered():
    import isaacgym  # noqa: F401
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    for new, base in (("go2_robust_rnd", "go2_robust_asym"), ("go2_terrain_robust_rnd", "go2_terrain_robust_asym")):
        assert task_registry.get_task_class(new) is task_registry.get_task_class(base)
        assert class_to_dict(task_registry.get_cfgs(new)[0]) == class_to_dict(task_registry.get_cfgs(base)[0])
        tc = class_to_dict(task_registry.get_cfgs(new)[1])
        assert tc["runner"]["experiment_name"] == new
        cfg = parse_cfg(tc["algorithm"]["rnd_cfg"])
        assert cfg is not None and cfg["state"] == "critic" and cfg["weight"] > 0
        sched = cfg["weight_schedule"]
        assert sched["mode"] == "linear" and sched["final_value"] == 0.0
        assert sched["final_step"] == tc["runner"]["max_iterations"] // 2 * tc["runner"]["num_steps_per_env"]
        assert parse_cfg(class_to_dict(task_registry.get_cfgs(base)[1])["algorithm"]["rnd_cfg"]) is None
