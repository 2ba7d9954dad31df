"""The launch prologue of the env-step kernels (csrc/leggedsim.hip): the model cache copied
from the image lgs_create_sim builds once per sim, the per-env loads issued together before the
first LDS write, and the PD law's task vectors staged in LDS for the substep loop.

None of it is arithmetic, so every check is exact: the kernels against the CPU oracle through
the bridge (orc_step, orc_simulate, orc_body_states_env, orc_reset_idx).  Where the oracle does
not know a feature (the clamped PD target, the actuator rows and action delay) the reference is
its substep fed by the fp32 restatement of the PD law, as in test_gpu_actuator_rand.py.

Shapes: 2 and 6 envs (one wave of two envs and three of them for the 32-row Go2 kernels; an odd
wave count and the grid's last wave for the one-env-per-wave ones), on the Go2 32-row entry,
its exact 48-row entry and a padded generic entry (H1 with the ankles locked, 8 DOFs on the
(16, 24) shape).  At most 8 control steps per run.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import isaacgym  # noqa: F401,E402
import bridge  # noqa: E402
import legged_gym.envs.base.legged_robot as lr  # noqa: E402
from legged_gym.envs import task_registry  # noqa: E402
from leggedsim import cabi  # noqa: E402
from test_gpu_actuator_rand import ON, fill_rows, physics_half, restate_physics, restate_step  # noqa: E402
from test_gpu_padded import lock_dofs  # noqa: E402
from test_gpu_parity import (POST, STATE, assert_exact, env_arrays, fused_vs_oracle, make, restore, save,  # noqa: E402
                             writes_body_states)
from test_gpu_post_physics_branches import split_step, tilt  # noqa: E402
from test_self_collision import crossed_pose  # noqa: E402

SHAPES = ["go2", "go2_48", "h1_padded"]
P = lambda a: a.ctypes.data  # noqa: E731


def rand_actions(env, g, scale=0.5):
    return scale * torch.randn(env.num_envs, env.num_actions, device="cuda", generator=g)


@pytest.fixture
def build(monkeypatch):
    """build(shape, n, **edits): a reset env on the shape's instantiation, closed at teardown."""
    envs = []

    def _build(shape, n, **edits):
        task = shape
        if shape == "go2_48":
            task = "go2"
            cls = task_registry.get_task_class(task)
            monkeypatch.setattr(cls, "max_contacts", 12)
            monkeypatch.setattr(cls, "max_rows", 48)
        elif shape == "h1_padded":
            task, D = "h1", 8
            real = lr.load_model
            monkeypatch.setattr(lr, "load_model", lambda *a, **k: lock_dofs(
                real(*a, **k), ["left_ankle_joint", "right_ankle_joint"]))
            edits.update(env__num_actions=D, env__num_observations=11 + 3 * D, env__num_privileged_obs=14 + 3 * D)
        env = make(task, n, **edits)
        envs.append(env)
        want = {"go2": (12, 19, 32), "go2_48": (12, 19, 48), "h1_padded": (16, 24, 48)}.get(shape)
        if want:
            assert env.sim.instantiation() == want
        env.reset()
        return env
    yield _build
    for env in envs:
        env.close()
    lib = bridge.ensure_built()
    bridge.set_ground(lib)
    bridge.set_self_collision(lib, None)


# ------------------------------------------- 1. every kernel that copies the image ---
@pytest.mark.parametrize("n", [2, 6])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_kernel_family_matches_the_oracle_bitwise(build, shape, n):
    """lgs_step, lgs_simulate, lgs_forward_kinematics and lgs_reset_idx, each against the oracle."""
    env = build(shape, n)
    g = torch.Generator(device="cuda").manual_seed(n)
    lib = bridge.ensure_built()
    mh = cabi.ModelHandle(env.model)
    fused_vs_oracle(env, g, 3, f"{shape} x{n} lgs_step")
    # lgs_simulate: one substep on caller torques
    tau = (3.0 * torch.randn(n, env.num_dof, device="cuda", generator=g)).contiguous()
    snap = bridge.snapshot(env)
    env.sim.simulate(tau)
    torch.cuda.synchronize()
    bridge.set_env(lib, env)
    root, dofs, cf, rbs = (snap[k].copy() for k in ("root", "dofs", "cforce", "rbs"))
    t = tau.cpu().numpy()
    lib.orc_simulate(C.byref(mh.desc), C.byref(env._lgs_params), n, P(root), P(dofs), P(t), P(cf), P(rbs),
                     P(snap["added_mass"]), P(snap["friction"]))
    got = dict(root=env.root_states.cpu().numpy(), dofs=env.dof_state.cpu().numpy(),
               cforce=env._contact_forces.cpu().numpy(), rbs=env.rigid_body_states.cpu().numpy())
    assert_exact(got, dict(root=root, dofs=dofs, cforce=cf, rbs=rbs), ["root", "dofs", "cforce", "rbs"], n,
                 f"{shape} x{n} lgs_simulate")
    # lgs_reset_idx on the last env (the grid's last wave), then lgs_forward_kinematics
    snap = bridge.snapshot(env)
    snap["reset"] = env._reset_bufs[env._buf_idx].cpu().numpy().astype(np.uint8)
    step = env.common_step_counter
    env.reset_idx(torch.tensor([n - 1], device="cuda"))
    got = env_arrays(env)
    b = {k: (None if v is None else np.ascontiguousarray(v).copy()) for k, v in snap.items()}
    b["episode_acc"][:] = 0
    mask = np.zeros(n, np.uint8)
    mask[n - 1] = 1
    E = bridge._env_struct(b)
    lib.orc_reset_idx(C.byref(mh.desc), C.byref(env.task_params), n, P(b["root"]), P(b["dofs"]), C.byref(E), P(mask),
                      int(step))
    assert_exact(got, b, ["root", "dofs", "commands", "actions", "last_actions", "last_dof_vel", "feet_air_time",
                          "episode_length", "episode_sums", "reset"], n, f"{shape} x{n} lgs_reset_idx")
    env.rigid_body_states.fill_(7.0)
    env.gym.refresh_rigid_body_state_tensor(env.sim)
    torch.cuda.synchronize()
    B = env.num_bodies
    have = env.rigid_body_states.view(n, B, 13).cpu().numpy()
    root = env.root_states.cpu().numpy()
    dofs = env.dof_state.cpu().numpy().reshape(n, -1)
    want = np.zeros((n, B, 13), np.float32)
    for e in range(n):
        r, d = np.ascontiguousarray(root[e]), np.ascontiguousarray(dofs[e])
        lib.orc_body_states_env(C.byref(mh.desc), P(r), P(d), P(want[e]))
    np.testing.assert_array_equal(have, want, err_msg=f"{shape} x{n} lgs_forward_kinematics")
    # and the step after the reset
    fused_vs_oracle(env, g, 1, f"{shape} x{n} lgs_step after reset_idx")


def test_two_sims_of_different_robots_step_alternately(build):
    """The image belongs to the sim: Go2 (12 DOFs, 19 bodies) and H1 (10, 11) alive together."""
    a, b = build("go2", 2), build("h1", 2)
    ga, gb = (torch.Generator(device="cuda").manual_seed(s) for s in (1, 2))
    for it in range(3):
        fused_vs_oracle(a, ga, 1, f"go2 beside h1, round {it}")
        fused_vs_oracle(b, gb, 1, f"h1 beside go2, round {it}")


def test_self_collision_set_after_create_and_steps(build):
    """lgs_set_self_collision after the sim has stepped (off, then on again): the steps from a
    crossed-leg pose match the oracle given the same setting, and the setting matters."""
    env = build("h1", 2)
    sc = env.self_collision
    assert sc is not None and len(sc.pairs) > 0
    g = torch.Generator(device="cuda").manual_seed(5)
    fused_vs_oracle(env, g, 1, "h1 x2 as created")
    q, _, _ = crossed_pose(env.model, sc, env.default_dof_pos.cpu().numpy())
    n, D = env.num_envs, env.num_dof
    env._sync_stream()
    env.dof_state.view(n, D, 2)[:, :, 0] = torch.tensor(q, device="cuda").repeat(n, 1)
    env.dof_state.view(n, D, 2)[:, :, 1] = 0.0
    env.root_states[:, 2] = env.env_origins[:, 2] + 2.5
    env.root_states[:, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    env.root_states[:, 7:13] = 0.0
    hold = torch.zeros(n, env.num_actions, device="cuda")
    hold[:] = torch.tensor((q - env.default_dof_pos.cpu().numpy().reshape(-1)) / env.cfg.control.action_scale, device="cuda")
    st = save(env)
    out = {}
    for setting in (None, sc):
        restore(env, st)
        env.sim.set_self_collision(setting)
        env.self_collision = setting  # (what bridge.set_env hands the oracle)
        snap = bridge.snapshot(env)
        ref = bridge.step(env, snap, hold.cpu().numpy(), env.common_step_counter)
        env.step(hold)
        out[setting is None] = env_arrays(env)
        assert_exact(out[setting is None], ref, STATE + POST, n, f"h1 x2 self-collision {'off' if setting is None else 'on'}",
                     skip_body_states=not writes_body_states(env))
    assert (out[True]["dofs"] != out[False]["dofs"]).any(), "the crossed legs never touched"


# ------------------------------------------------------------ 2. the PD section ---
@pytest.mark.parametrize("control", ["P", "V", "T"])
def test_control_modes_match_the_oracle_bitwise(build, control):
    more = dict(control__action_scale=0.5) if control == "T" else {}
    env = build("go2", 2, control__control_type=control, **more)
    assert env.task_params.control_type == {"P": 0, "V": 1, "T": 2}[control]
    fused_vs_oracle(env, torch.Generator(device="cuda").manual_seed(3), 4, f"go2 x2 control {control}")


@pytest.mark.parametrize("task", ["go2", "go2_handstand"])
def test_pd_law_on_staged_vectors_matches_the_restatement_bitwise(build, task):
    """The actuator rows with a non-zero delay, and with them the clamped target (handstand):
    lgs_step_physics against decimation x { restated PD law -> orc_simulate }; for the walking
    task the fused step against orc_post_physics on that."""
    n = 2
    env = build(task, n, **ON, domain_rand__actuator_resample_on_reset=False)
    T = env.task_params
    assert T.clamp_pd_targets == (1 if task == "go2_handstand" else 0)
    g = torch.Generator(device="cuda").manual_seed(11)
    delays, clipped_any = set(), False
    for it in range(4):
        delays.update(fill_rows(env, it))
        a = rand_actions(env, g, 0.5 if it < 3 else 8.0)  # (the last step: targets past the clamp and the effort limit)
        st = save(env)
        snap = bridge.snapshot(env)
        want, clipped = restate_physics(env, snap, a.cpu().numpy())
        clipped_any |= clipped
        got = physics_half(env, a)
        keys = ["root", "dofs", "cforce", "actions"] + ([] if T.record_unclipped_torques else ["torques"])
        assert_exact(got, want, keys, n, f"{task} x{n} step {it}: lgs_step_physics vs the restatement")
        restore(env, st)
        k = env.common_step_counter
        env.step(a)
        if task == "go2":
            ref = restate_step(env, snap, want, k)
            assert_exact(env_arrays(env), ref, STATE + POST, n, f"{task} x{n} step {it}: lgs_step vs the restatement",
                         skip_body_states=not writes_body_states(env))
    assert clipped_any and max(delays) > 0


def test_set_task_between_two_steps_shows_in_the_next_launch(build):
    """The staged default_dof_pos / torque_limits are per launch, not cached across launches."""
    env = build("go2", 2)
    g = torch.Generator(device="cuda").manual_seed(7)
    fused_vs_oracle(env, g, 2, "go2 x2 before lgs_set_task")
    st = save(env)
    a = rand_actions(env, g)
    env.step(a)
    old = env_arrays(env)["torques"].copy()
    restore(env, st)
    T2 = cabi.TaskParams.from_buffer_copy(env.task_params)
    for j in range(env.num_dof):
        T2.default_dof_pos[j] += 0.2
        T2.torque_limits[j] *= 0.25
    env.sim.set_task(T2)
    env.task_params = T2
    snap = bridge.snapshot(env)
    ref = bridge.step(env, snap, a.cpu().numpy(), env.common_step_counter)
    env.step(a)
    got = env_arrays(env)
    assert_exact(got, ref, STATE + POST, 2, "go2 x2 after lgs_set_task")
    assert (got["torques"] != old).any()
    lim = np.array(T2.torque_limits[:env.num_dof], np.float32)
    assert (np.abs(got["torques"]) <= lim).all()
    fused_vs_oracle(env, g, 1, "go2 x2, the step after")


@pytest.mark.parametrize("shape,n", [("go2", 2), ("go2", 6), ("h1_padded", 2)])
def test_physics_then_post_is_the_fused_step_bitwise(build, shape, n):
    env = build(shape, n)
    g = torch.Generator(device="cuda").manual_seed(n)
    for it in range(3):
        a = rand_actions(env, g)
        st = save(env)
        env.step(a)
        fused = copy.deepcopy(env_arrays(env))
        for three in (False, True):
            restore(env, st)
            assert_exact(split_step(env, a, three), fused, STATE + POST, n, f"{shape} x{n} step {it} split ({three})")


# ------------------------------------------------------ 3. the post-physics block ---
def nonzero_scales(name):
    """The task's reward terms (legged_gym drops a zero scale), the termination term aside."""
    from legged_gym.utils.helpers import class_to_dict
    sc = class_to_dict(task_registry.get_cfgs(name)[0].rewards.scales)
    return sorted(k for k, v in sc.items() if v != 0 and k != "termination")


def test_most_and_fewest_reward_terms_match_the_oracle_bitwise(build):
    """The registry task with the most reward terms among those the oracle knows, and Go2 with
    one term alone (no termination term, no optional one)."""
    known = ["go2", "h1", "h1_2", "g1"]
    most = max(known, key=lambda k: len(nonzero_scales(k)))
    env = build(most, 2)
    assert env.task_params.num_rewards == len(nonzero_scales(most))
    fused_vs_oracle(env, torch.Generator(device="cuda").manual_seed(1), 3, f"{most} x2, the most terms")
    sc = copy.deepcopy(task_registry.get_cfgs("go2")[0].rewards.scales)
    for k in nonzero_scales("go2") + ["termination"]:
        setattr(sc, k, 0.0)
    sc.tracking_lin_vel = 1.0
    env = build("go2", 2, rewards__scales=sc)
    T = env.task_params
    assert (T.num_rewards, T.has_termination_reward) == (1, 0)
    fused_vs_oracle(env, torch.Generator(device="cuda").manual_seed(2), 3, "go2 x2, one term")


def test_one_env_of_the_wave_resets_and_the_other_does_not(build):
    env = build("go2", 2)
    g = torch.Generator(device="cuda").manual_seed(9)
    fused_vs_oracle(env, g, 1, "go2 x2 warm")
    tilt(env, 1)
    snap = bridge.snapshot(env)
    a = rand_actions(env, g)
    ref = bridge.step(env, snap, a.cpu().numpy(), env.common_step_counter)
    env.step(a)
    assert_exact(env_arrays(env), ref, STATE + POST, 2, "go2 x2, env 1 terminates")
    assert list(ref["reset"].astype(int).ravel()) == [0, 1]
    fused_vs_oracle(env, g, 2, "go2 x2 after the reset")
