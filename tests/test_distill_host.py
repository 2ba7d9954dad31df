"""Teacher-student distillation on the host: StudentTeacher, Distillation's plain
path against a literal loop, the checkpoint rule, the refusals and the task registrations."""
import copy

import pytest
import torch
import torch.nn as nn

from fake_env import FakeEnv
from rsl_rl.algorithms import Distillation
from rsl_rl.modules import ActorCritic, StudentTeacher
from rsl_rl.runners import OnPolicyRunner

N, T, G, A, O, P = 8, 4, 2, 3, 6, 5


def _policy(seed=0, **kw):
    torch.manual_seed(seed)
    return StudentTeacher(O, P, A, student_hidden_dims=[16, 8], teacher_hidden_dims=[8, 8], **kw)


def _filled(alg, seed=1):
    """A hand-built storage: T steps of N rows through Distillation.act / process_env_step."""
    g = torch.Generator().manual_seed(seed)
    alg.init_storage(N, T, [O], [P], [A])
    for _ in range(T):
        obs, tobs = torch.randn(N, O, generator=g), 2.0 * torch.randn(N, P, generator=g)
        act = alg.act(obs, tobs)
        assert act.shape == (N, A)
        alg.process_env_step(torch.zeros(N), torch.zeros(N, dtype=torch.bool), {})
    assert alg.storage.step == T
    alg.storage.privileged_actions.mul_(6.0)  # (labels on both sides of the huber's delta)
    return alg


def _literal_update(student, obs, target, loss_type, epochs, lr, max_norm):
    """rsl_rl 2.x Distillation.update, written out."""
    fn = nn.functional.mse_loss if loss_type == "mse" else (lambda a, b: nn.functional.huber_loss(a, b, delta=1.0))
    opt = torch.optim.Adam(student.parameters(), lr=lr)
    mean, cnt, loss = 0.0, 0, 0
    for _ in range(epochs):
        for t in range(obs.shape[0]):
            bl = fn(student(obs[t]), target[t])
            loss = loss + bl
            mean += bl.item()
            cnt += 1
            if cnt % G == 0:
                opt.zero_grad()
                loss.backward()
                if max_norm:
                    nn.utils.clip_grad_norm_(student.parameters(), max_norm)
                opt.step()
                loss = 0
    return mean / cnt


@pytest.mark.parametrize("max_norm", [None, 0.05])
@pytest.mark.parametrize("epochs", [1, 2])
@pytest.mark.parametrize("loss_type", ["mse", "huber"])
def test_plain_update_is_the_literal_loop(loss_type, epochs, max_norm):
    pol = _policy()
    pol.load_state_dict({"actor." + k: v for k, v in _policy(5).teacher.state_dict().items()})
    alg = _filled(Distillation(pol, num_learning_epochs=epochs, gradient_length=G, learning_rate=1e-2,
                               max_grad_norm=max_norm, loss_type=loss_type, device="cpu"))
    st = alg.storage
    # the storage holds the student's rows and the teacher's actions on the privileged rows
    assert st.observations.shape == (T, N, O) and st.privileged_actions.shape == (T, N, A)
    if loss_type == "huber":  # both branches of the huber are exercised
        d = (pol.student(st.observations) - st.privileged_actions).abs()
        assert (d > 1).any() and (d < 1).any()
    ref = copy.deepcopy(pol.student)
    teacher0 = copy.deepcopy(pol.teacher.state_dict())
    std0 = pol.std.detach().clone()
    want = _literal_update(ref, st.observations.clone(), st.privileged_actions.clone(), loss_type, epochs, 1e-2,
                           max_norm)
    got = alg.update()
    assert isinstance(got, float)
    torch.testing.assert_close(torch.tensor(got), torch.tensor(want), rtol=1e-6, atol=0)
    for p, q in zip(pol.student.parameters(), ref.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-9)
    assert alg.storage.step == 0
    # std and the teacher are untouched, and neither is in the optimizer
    assert torch.equal(pol.std.detach(), std0) and pol.std.grad is None
    for k, v in pol.teacher.state_dict().items():
        assert torch.equal(v, teacher0[k])
    held = {id(p) for g in alg.optimizer.param_groups for p in g["params"]}
    assert held == {id(p) for p in pol.student.parameters()}
    assert all(not p.requires_grad for p in pol.teacher.parameters())


def test_storage_rows_are_the_teachers_actions():
    pol = _policy()
    pol.load_state_dict({"actor." + k: v for k, v in _policy(5).teacher.state_dict().items()})
    alg = Distillation(pol, gradient_length=G, device="cpu")
    alg.init_storage(N, T, [O], [P], [A])
    obs, tobs = torch.randn(N, O), torch.randn(N, P)
    alg.act(obs, tobs)
    alg.process_env_step(torch.zeros(N), torch.zeros(N, dtype=torch.bool), {})
    assert torch.equal(alg.storage.observations[0], obs)
    assert torch.equal(alg.storage.privileged_actions[0], pol.teacher(tobs))
    assert torch.equal(pol.evaluate(tobs), pol.teacher(tobs)) and not pol.evaluate(tobs).requires_grad
    assert torch.equal(pol.act_inference(obs), pol.student(obs))
    assert pol.actor is pol.student and pol.is_recurrent is False
    assert alg.compute_returns(obs) is None
    assert alg.actor_critic is pol and alg.learning_rate == pytest.approx(1e-3)


def test_act_samples_around_the_student():
    pol = _policy(init_noise_std=0.1)
    obs = torch.randn(4096, O)
    a = pol.act(obs)
    r = (a - pol.student(obs)).detach()
    assert abs(r.std().item() - 0.1) < 0.01 and abs(r.mean().item()) < 0.01


def test_load_state_dict_rule():
    ppo = ActorCritic(P, P, A, actor_hidden_dims=[8, 8], critic_hidden_dims=[8, 8])
    pol = _policy()
    student0 = copy.deepcopy(pol.student.state_dict())
    std0 = pol.std.detach().clone()
    assert pol.loaded_teacher is False
    resumed = pol.load_state_dict(ppo.state_dict())
    assert resumed is False and pol.loaded_teacher is True
    for k, v in ppo.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k], v)
    for k, v in pol.student.state_dict().items():  # a PPO checkpoint leaves the student and std alone
        assert torch.equal(v, student0[k])
    assert torch.equal(pol.std.detach(), std0)
    # a distillation checkpoint loads everything and resumes
    sd = pol.state_dict()
    assert any(k.startswith("student.") for k in sd) and any(k.startswith("teacher.") for k in sd)
    assert not any(k.startswith("actor.") for k in sd)
    other = _policy(9)
    assert other.load_state_dict(sd) is True and other.loaded_teacher is True
    for k, v in sd.items():
        assert torch.equal(other.state_dict()[k], v)
    with pytest.raises(ValueError):
        _policy().load_state_dict({"weight": torch.zeros(1)})


def test_update_raises_before_a_teacher_is_loaded():
    alg = _filled(Distillation(_policy(), gradient_length=G, device="cpu"))
    with pytest.raises(ValueError, match="teacher model parameters not loaded"):
        alg.update()


def _train_cfg(**runner):
    cfg = dict(policy=dict(student_hidden_dims=[16, 8], teacher_hidden_dims=[8, 8], activation="elu",
                           init_noise_std=0.1),
               algorithm=dict(num_learning_epochs=1, gradient_length=G, learning_rate=1e-3, max_grad_norm=None,
                              loss_type="mse"),
               runner=dict(policy_class_name="StudentTeacher", algorithm_class_name="Distillation",
                           num_steps_per_env=T, save_interval=50, defer_env_extras=False))
    cfg["runner"].update(runner)
    return cfg


def test_refusals(monkeypatch):
    env = FakeEnv(num_envs=N, num_obs=O, num_actions=A, num_privileged_obs=O + 2)
    # 1. empirical normalisation
    with pytest.raises(ValueError, match="empirical_normalization"):
        OnPolicyRunner(env, _train_cfg(empirical_normalization=True), device="cpu")
    # 2. symmetry augmentation
    cfg = _train_cfg()
    cfg["algorithm"]["symmetry_cfg"] = dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.0)
    with pytest.raises(ValueError, match="symmetry"):
        OnPolicyRunner(env, cfg, device="cpu")
    with pytest.raises(ValueError, match="symmetry"):
        Distillation(_policy(), symmetry_cfg=dict(use_mirror_loss=True), device="cpu")
    # (the cfg's default, everything off, is taken)
    Distillation(_policy(), symmetry_cfg=dict(use_data_augmentation=False, use_mirror_loss=False), device="cpu")
    # 3. a recurrent student or teacher
    with pytest.raises(ValueError, match="recurrent"):
        OnPolicyRunner(env, _train_cfg(policy_class_name="ActorCriticRecurrent"), device="cpu")
    rec = _policy()
    rec.memory = nn.LSTM(O, 8)
    with pytest.raises(ValueError, match="recurrent"):
        Distillation(rec, device="cpu")
    rec2 = _policy()
    rec2.is_recurrent = True
    with pytest.raises(ValueError, match="recurrent"):
        Distillation(rec2, device="cpu")
    # 4. a torch.distributed world size above 1
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a, **k: 0)
    with pytest.raises(ValueError, match="world size"):
        Distillation(_policy(), device="cpu")
    with pytest.raises(ValueError, match="world size"):
        OnPolicyRunner(env, _train_cfg(), device="cpu")


def test_runner_on_the_plain_path(tmp_path):
    """The runner end to end on the CPU: a PPO run's checkpoint is the teacher, the student
    learns, the checkpoint round-trips and resumes; a PPO checkpoint through load() does not."""
    env = FakeEnv(num_envs=N, num_obs=O, num_actions=A, num_privileged_obs=O + 2)
    ppo_cfg = dict(policy=dict(actor_hidden_dims=[8, 8], critic_hidden_dims=[8, 8], activation="elu",
                               init_noise_std=1.0),
                   algorithm=dict(num_learning_epochs=1, num_mini_batches=1),
                   runner=dict(policy_class_name="ActorCritic", algorithm_class_name="PPO", num_steps_per_env=T,
                               save_interval=50))
    tenv = FakeEnv(num_envs=N, num_obs=O + 2, num_actions=A)  # the teacher task: one (privileged) row
    teacher = OnPolicyRunner(tenv, ppo_cfg, device="cpu")
    tpath = str(tmp_path / "teacher" / "model_0.pt")
    teacher.save(tpath)

    runner = OnPolicyRunner(env, _train_cfg(), device="cpu")
    assert isinstance(runner.alg, Distillation) and isinstance(runner.alg.actor_critic, StudentTeacher)
    with pytest.raises(ValueError, match="teacher"):
        runner.learn(1)
    runner = OnPolicyRunner(env, _train_cfg(), device="cpu")
    runner.load_teacher(tpath)
    pol = runner.alg.actor_critic
    for k, v in teacher.alg.actor_critic.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k], v)
    s0 = copy.deepcopy(pol.student.state_dict())
    t0 = copy.deepcopy(pol.teacher.state_dict())
    runner.learn(2)
    assert runner.current_learning_iteration == 2
    assert any(not torch.equal(v, s0[k]) for k, v in pol.student.state_dict().items())
    assert all(torch.equal(v, t0[k]) for k, v in pol.teacher.state_dict().items())
    spath = str(tmp_path / "student" / "model_2.pt")
    runner.save(spath)
    again = OnPolicyRunner(env, _train_cfg(), device="cpu")
    again.load(spath)
    assert again.current_learning_iteration == 2 and again.alg.actor_critic.loaded_teacher
    for k, v in pol.state_dict().items():
        assert torch.equal(again.alg.actor_critic.state_dict()[k], v)
    again.learn(1)
    # a distillation run's checkpoint also serves as a teacher source
    third = OnPolicyRunner(env, _train_cfg(), device="cpu")
    third.load_teacher(spath)
    assert all(torch.equal(v, t0[k]) for k, v in third.alg.actor_critic.teacher.state_dict().items())
    # a PPO checkpoint through load(): fills the teacher, does not resume
    fourth = OnPolicyRunner(env, _train_cfg(), device="cpu")
    fourth.load(tpath)
    assert fourth.current_learning_iteration == 0 and fourth.alg.actor_critic.loaded_teacher


def test_logging_writes_the_behaviour_loss(tmp_path):
    import json
    import os
    env = FakeEnv(num_envs=N, num_obs=O, num_actions=A, num_privileged_obs=O + 2)
    runner = OnPolicyRunner(env, _train_cfg(), log_dir=str(tmp_path / "log"), device="cpu")
    runner.writer = __import__("rsl_rl.runners.on_policy_runner", fromlist=["_JsonlWriter"])._JsonlWriter(
        str(tmp_path / "log"))
    runner.alg.actor_critic.loaded_teacher = True  # (a random teacher)
    runner.learn(1)
    runner.writer.flush()
    tags = {json.loads(line)["tag"] for line in open(os.path.join(str(tmp_path / "log"), "scalars.jsonl"))}
    assert "Loss/behavior" in tags and "Loss/value_function" not in tags and "Loss/surrogate" not in tags


TASKS = {  # name: (student / policy inputs, teacher / privileged inputs presented to the runner)
    "go2_robust_teacher": (87, None),
    "go2_terrain_robust_teacher": (274, None),
    "go2_robust_distill": (240, 87),
    "go2_terrain_robust_distill": (427, 274),
}


@pytest.mark.parametrize("name", sorted(TASKS))
def test_tasks_are_registered_with_their_widths(name):
    import isaacgym  # noqa: F401
    from legged_gym.envs import task_registry
    from legged_gym.envs.base.privileged_actor import PrivilegedActorRobot, presented_widths
    from legged_gym.utils.helpers import class_to_dict
    env_cfg, train_cfg = task_registry.get_cfgs(name)
    assert presented_widths(env_cfg) == TASKS[name]
    cfg = class_to_dict(train_cfg)
    if name.endswith("_teacher"):
        assert env_cfg.env.privileged_as_observations is True
        assert task_registry.get_task_class(name) is PrivilegedActorRobot
        # the inner env is the _asym task's: the native step still builds both rows
        asym, asym_train = task_registry.get_cfgs(name.replace("_teacher", "_asym"))
        assert (env_cfg.env.num_observations, env_cfg.env.num_privileged_obs) == \
            (asym.env.num_observations, asym.env.num_privileged_obs)
        assert asym.env.privileged_as_observations is False
        assert cfg["runner"]["algorithm_class_name"] == "PPO" and cfg["runner"]["policy_class_name"] == "ActorCritic"
        assert cfg["algorithm"] == class_to_dict(asym_train)["algorithm"]
        assert cfg["runner"]["experiment_name"] == name
    else:
        assert getattr(env_cfg.env, "privileged_as_observations", False) is False
        assert cfg["runner"]["algorithm_class_name"] == "Distillation"
        assert cfg["runner"]["policy_class_name"] == "StudentTeacher"
        assert cfg["runner"]["defer_env_extras"] is False
        assert cfg["runner"]["teacher_experiment_name"] == name.replace("_distill", "_teacher")
        assert cfg["runner"]["teacher_load_run"] == -1 and cfg["runner"]["teacher_checkpoint"] == -1
        assert cfg["algorithm"] == dict(num_learning_epochs=1, gradient_length=6, learning_rate=1e-3,
                                        max_grad_norm=None, loss_type="mse",
                                        symmetry_cfg=dict(use_data_augmentation=False, use_mirror_loss=False,
                                                          mirror_loss_coeff=0.0))
        assert cfg["policy"]["student_hidden_dims"] == [512, 256, 128]
        assert cfg["policy"]["teacher_hidden_dims"] == [512, 256, 128]
        assert cfg["runner"]["num_steps_per_env"] % cfg["algorithm"]["gradient_length"] == 0
        # the policy the runner would build
        pol = StudentTeacher(*presented_widths(env_cfg), env_cfg.env.num_actions, **cfg["policy"])
        assert pol.student[0].in_features == TASKS[name][0] and pol.teacher[0].in_features == TASKS[name][1]
        Distillation(pol, device="cpu", **cfg["algorithm"])  # (the cfg as the runner passes it)


def test_the_switch_is_off_by_default():
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    from legged_gym.envs.base.privileged_actor import presented_widths
    assert LeggedRobotCfg.env.privileged_as_observations is False
    assert presented_widths(LeggedRobotCfg) == (48, None)

    class NoRow(LeggedRobotCfg):
        class env(LeggedRobotCfg.env):
            privileged_as_observations = True
    with pytest.raises(ValueError):
        presented_widths(NoRow)
