"""Host side of PPO's symmetry augmentation: the tables of leggedsim/task.py
symmetry_tables (involution, the Go2 frame against a hand-written expectation, the history
tiling, the scan on the point list, the privileged tail), every refusal by message, the switch's
default, the doubled storage, the torch statement of the augmented update against a restatement
written here, and the tables against the simulator's own symmetry: the CPU oracle's control step
on mirrored pairs of envs (tests/symmetry_case.py).  No GPU."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
import symmetry_case as sc
from legged_gym.utils import task_registry
from legged_gym.utils.helpers import class_to_dict
from leggedsim import cabi
from leggedsim.model import MODELS_DIR, Model
from leggedsim.task import joint_symmetry, priv_params, scan_points, symmetry_tables
from rsl_rl.algorithms import PPO
from rsl_rl.modules import ActorCritic, ActorCriticRecurrent
from rsl_rl.storage import RolloutStorage
from test_height_obs_host import _spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# task -> (policy row, critic row) widths; the two new tasks last
SUPPORTED = {"go2": (48, 48), "go2_terrain": (235, 235), "go2_robust": (48, 48), "go2_robust_history": (240, 240),
             "go2_terrain_robust": (427, 427), "go2_robust_asym": (240, 87), "go2_terrain_robust_asym": (427, 274),
             "go2_robust_sym": (240, 87), "go2_terrain_robust_sym": (427, 274)}
ON = dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.0)


def env_like(task, model="go2", edit=None):
    """What symmetry_tables reads of an env: the task's spec on its bundled model."""
    spec, _ = _spec(task, model, edit)
    spec.model = Model.load(os.path.join(MODELS_DIR, model + ".npz"))
    spec._hooks = task_registry.get_task_class(task).python_step_hooks()
    return spec


def apply(x, table):
    return sc.mirror(x, table)


# ------------------------------------------------------------------ tables ---
@pytest.mark.parametrize("task", list(SUPPORTED))
def test_tables_have_the_rows_widths_and_mirror_twice_is_the_identity(task):
    env = env_like(task)
    tabs = symmetry_tables(env)
    assert [len(t[0]) for t in tabs] == list(SUPPORTED[task]) + [12]
    assert (env.num_obs, env.num_privileged_obs or env.num_obs) == SUPPORTED[task]
    rng = np.random.default_rng(0)
    for perm, sign in tabs:
        K = len(perm)
        assert perm.dtype == np.int32 and sign.dtype == np.float32 and sign.shape == (K,)
        assert np.array_equal(perm[perm], np.arange(K)) and np.array_equal(sign * sign[perm], np.ones(K, F))
        assert set(np.unique(sign)) <= {-1.0, 1.0}
        x = rng.standard_normal((3, K)).astype(F)
        x[0, ::5] = 0.0
        twice = apply(apply(x, (perm, sign)), (perm, sign))
        assert np.array_equal(twice.view(np.uint32), x.view(np.uint32))
    if not env.num_privileged_obs:
        assert tabs[1] is tabs[0] or all(np.array_equal(a, b) for a, b in zip(tabs[0], tabs[1]))


def test_go2_frame_is_the_hand_written_table():
    env = env_like("go2")
    names = list(env.model.dof_names)
    assert names == [f"{leg}_{j}_joint" for leg in ("FL", "FR", "RL", "RR") for j in ("hip", "thigh", "calf")]
    policy, critic, action = symmetry_tables(env)
    # the joint pairs by DOF name, -1 on the hip abduction joints (x axis), +1 on thigh and calf (y axis)
    other = {"FL": "FR", "FR": "FL", "RL": "RR", "RR": "RL"}
    for j, n in enumerate(names):
        assert names[action[0][j]] == other[n[:2]] + n[2:]
        assert action[1][j] == (-1.0 if "hip" in n else 1.0)
    assert list(action[0]) == [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]
    # the twelve base entries: lin vel (+,-,+), ang vel (-,+,-), gravity (+,-,+), commands (+,-,-)
    assert list(policy[0][:12]) == list(range(12))
    assert list(policy[1][:12]) == [1, -1, 1, -1, 1, -1, 1, -1, 1, 1, -1, -1]
    for b in range(3):  # joint positions, velocities, previous actions
        assert list(policy[0][12 + 12 * b:24 + 12 * b]) == [12 + 12 * b + int(p) for p in action[0]]
        assert list(policy[1][12 + 12 * b:24 + 12 * b]) == list(action[1])
    assert all(np.array_equal(a, b) for a, b in zip(policy, critic))


def test_history_table_is_the_frame_table_tiled():
    frame = symmetry_tables(env_like("go2_robust"))[0]
    hist = symmetry_tables(env_like("go2_robust_history"))[0]
    assert len(hist[0]) == 5 * 48
    for h in range(5):  # the frame order is untouched
        assert np.array_equal(hist[0][48 * h:48 * (h + 1)], frame[0] + 48 * h)
        assert np.array_equal(hist[1][48 * h:48 * (h + 1)], frame[1])
    both = symmetry_tables(env_like("go2_terrain_robust"))[0]
    assert np.array_equal(both[0][:240], hist[0]) and np.array_equal(both[1][:240], hist[1])


@pytest.mark.parametrize("task,head", [("go2_terrain", 48), ("go2_terrain_robust", 240)])
def test_scan_maps_each_point_to_its_mirror_image_on_the_point_list(task, head):
    env = env_like(task)
    pts = scan_points(env.cfg)
    assert pts.shape == (187, 3)
    perm, sign = (t[head:] for t in symmetry_tables(env)[0])
    assert np.array_equal(pts[perm - head], pts * (1, -1, 1)) and np.array_equal(sign, np.ones(187, F))
    # the order of the list is the scan's: point k = ix * len(y) + iy
    tc = env.cfg.terrain
    assert pts[1][0] == tc.measured_points_x[0] and pts[1][1] == tc.measured_points_y[1]


def test_privileged_row_is_frame_fixed_scalars_permuted_actuator_rows_and_scan():
    env = env_like("go2_terrain_robust_asym")
    policy, critic, action = symmetry_tables(env)
    frame = symmetry_tables(env_like("go2"))[0]
    assert priv_params(env).num_tail == 39
    perm, sign = critic
    assert np.array_equal(perm[:48], frame[0]) and np.array_equal(sign[:48], frame[1])   # the clean frame
    assert list(perm[48:50]) == [48, 49] and list(sign[48:50]) == [1, 1]                 # friction, added mass
    for g in range(3):  # kp, kd, strength: the joint pairing, sign +1
        lo = 50 + 12 * g
        assert np.array_equal(perm[lo:lo + 12], action[0] + lo) and np.array_equal(sign[lo:lo + 12], np.ones(12, F))
    assert perm[86] == 86 and sign[86] == 1                                              # the delay
    assert np.array_equal(perm[87:], policy[0][240:] - 240 + 87) and np.array_equal(sign[87:], np.ones(187, F))
    # without the actuator rows the tail is friction and mass alone
    def edit(cfg):
        cfg.env.privileged_parameters, cfg.env.num_privileged_obs = True, 50
    c = symmetry_tables(env_like("go2", edit=edit))[1]
    assert len(c[0]) == 50 and list(c[0][48:]) == [48, 49] and list(c[1][48:]) == [1, 1]


# ---------------------------------------------------------------- refusals ---
def test_layouts_and_python_observations_are_refused():
    with pytest.raises(ValueError, match="handstand layout is not supported"):
        symmetry_tables(env_like("go2_handstand"))
    with pytest.raises(ValueError, match="humanoid layout is not supported yet"):
        symmetry_tables(env_like("h1", "h1"))
    env = env_like("go2")
    env._hooks = frozenset({"compute_observations"})
    with pytest.raises(ValueError, match="overrides compute_observations"):
        symmetry_tables(env)


def test_asymmetric_default_pose_gains_and_scan_are_refused_with_the_joint_named():
    def pose(cfg):
        cfg.init_state.default_joint_angles = dict(cfg.init_state.default_joint_angles, FR_thigh_joint=0.9)
    with pytest.raises(ValueError, match=r"default angle .* of joint FL_thigh_joint \(0\.8\) is not the mirror image of "
                                         r"FR_thigh_joint's \(0\.9\)"):
        symmetry_tables(env_like("go2", edit=pose))

    def hip(cfg):  # the hips mirror with sign -1: equal angles are asymmetric
        cfg.init_state.default_joint_angles = dict(cfg.init_state.default_joint_angles, FR_hip_joint=0.1)
    with pytest.raises(ValueError, match="of joint FL_hip_joint"):
        symmetry_tables(env_like("go2", edit=hip))
    env = env_like("go2")
    env.p_gains = np.array(env.p_gains, F)
    env.p_gains[7] = 25.0
    with pytest.raises(ValueError, match=r"stiffness .* of joint RL_thigh_joint"):
        symmetry_tables(env)
    env = env_like("go2")
    env.d_gains = np.array(env.d_gains, F)
    env.d_gains[2] = 0.7
    with pytest.raises(ValueError, match=r"damping .* of joint FL_calf_joint"):
        symmetry_tables(env)
    env = env_like("go2")
    env.cfg.control.action_scale = [0.25] * 11 + [0.3]
    with pytest.raises(ValueError, match=r"action scale .* of joint RL_calf_joint"):
        symmetry_tables(env)

    def scan(cfg):
        cfg.terrain.measured_points_y = [-0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.6]
    with pytest.raises(ValueError, match="measured_points_y is not symmetric about 0"):
        symmetry_tables(env_like("go2_terrain", edit=scan))


def test_a_model_that_does_not_pair_is_refused():
    env = env_like("go2")
    env.model.joint_pos = env.model.joint_pos.copy()
    b = int(env.model.dof_body[list(env.model.dof_names).index("FR_hip_joint")])
    env.model.joint_pos[b, 0] += 0.02
    with pytest.raises(ValueError, match="does not pair left-right"):
        joint_symmetry(env)
    env = env_like("go2")
    env.model.axis = env.model.axis.copy()
    env.model.axis[int(env.model.dof_body[4])] = (0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="axes of joints .* are not mirror images"):
        joint_symmetry(env)


def _tables(task="go2"):
    return symmetry_tables(env_like(task))


def test_ppo_refusals_at_construction():
    ac = ActorCritic(48, 48, 12, [32], [32])
    with pytest.raises(ValueError, match="use_mirror_loss is not supported"):
        PPO(ac, symmetry_cfg=dict(ON, use_mirror_loss=True), symmetry_tables=_tables())
    with pytest.raises(ValueError, match="unknown keys"):
        PPO(ac, symmetry_cfg=dict(ON, mirror=True), symmetry_tables=_tables())
    with pytest.raises(ValueError, match="needs symmetry_tables"):
        PPO(ac, symmetry_cfg=ON)
    rec = ActorCriticRecurrent(48, 48, 12, [32], [32], rnn_hidden_size=16)
    with pytest.raises(ValueError, match="not supported for recurrent policies"):
        PPO(rec, symmetry_cfg=ON, symmetry_tables=_tables())
    alg = PPO(ac, symmetry_cfg=ON, symmetry_tables=_tables())
    with pytest.raises(ValueError, match="symmetry_tables of widths"):
        alg.init_storage(4, 4, [60], [None], [12])
    # off, by either spelling: no tables needed, nothing kept
    for cfg in (None, {}, dict(ON, use_data_augmentation=False)):
        assert PPO(ac, symmetry_cfg=cfg)._sym is None


def test_runner_refuses_empirical_normalization_and_hands_the_tables_over():
    from rsl_rl.runners import OnPolicyRunner
    calls = []

    class Env:
        num_envs, num_obs, num_privileged_obs, num_actions = 4, 48, None, 12

        def symmetry_tables(self):
            calls.append(1)
            return _tables()

        def reset(self):
            return None, None

    _, train_cfg = task_registry.get_cfgs("go2_robust_sym")
    cfg = copy.deepcopy(class_to_dict(train_cfg))
    assert cfg["algorithm"]["symmetry_cfg"] == ON
    cfg["policy"] = dict(cfg["policy"], actor_hidden_dims=[32], critic_hidden_dims=[32])
    bad = copy.deepcopy(cfg)
    bad["runner"]["empirical_normalization"] = True
    with pytest.raises(ValueError, match="use_data_augmentation with empirical_normalization is not supported"):
        OnPolicyRunner(Env(), bad, device="cpu")
    runner = OnPolicyRunner(Env(), cfg, device="cpu")
    assert calls == [1] and runner.alg._sym is not None and runner.alg.storage.doubled is not None
    off = copy.deepcopy(cfg)
    off["algorithm"]["symmetry_cfg"]["use_data_augmentation"] = False
    runner = OnPolicyRunner(Env(), off, device="cpu")
    assert calls == [1] and runner.alg._sym is None and runner.alg.storage.doubled is None


# --------------------------------------------------------------- off is off --
def test_the_default_is_off_and_only_the_two_new_tasks_switch_it_on():
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfgPPO
    assert class_to_dict(LeggedRobotCfgPPO.algorithm.symmetry_cfg) == dict(ON, use_data_augmentation=False)
    for task in task_registry.task_classes:
        _, train_cfg = task_registry.get_cfgs(task)
        on = class_to_dict(train_cfg)["algorithm"]["symmetry_cfg"]["use_data_augmentation"]
        assert on == (task in ("go2_robust_sym", "go2_terrain_robust_sym")), task
    for new, base in (("go2_robust_sym", "go2_robust_asym"), ("go2_terrain_robust_sym", "go2_terrain_robust_asym")):
        assert task_registry.get_task_class(new) is task_registry.get_task_class(base)
        assert class_to_dict(task_registry.get_cfgs(new)[0]) == class_to_dict(task_registry.get_cfgs(base)[0])
        assert task_registry.get_cfgs(new)[1].runner.experiment_name == new


def test_storage_without_the_switch_is_todays_and_with_it_the_first_half_keeps_names_shapes_and_contiguity():
    off = RolloutStorage(6, 4, [48], [87], [12])
    assert off.doubled is None
    on = RolloutStorage(6, 4, [48], [87], [12], mirrored_half=True)
    assert sorted(on.doubled) == sorted(RolloutStorage.DOUBLED)
    for name in RolloutStorage.DOUBLED:
        a, b, whole = getattr(off, name), getattr(on, name), on.doubled[name]
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and b.is_contiguous()
        assert a.untyped_storage().nbytes() == a.numel() * 4   # today's allocation
        assert whole.shape == (8,) + a.shape[1:] and b.data_ptr() == whole.data_ptr()
    for name in ("rewards", "dones"):
        assert getattr(on, name).shape == getattr(off, name).shape and name not in on.doubled
    assert RolloutStorage(6, 4, [48], [None], [12], mirrored_half=True).doubled.get("privileged_observations") is None
    ac = ActorCritic(48, 48, 12, [32], [32])
    alg = PPO(ac)
    alg.init_storage(6, 4, [48], [None], [12])
    assert alg.storage.doubled is None and alg._sym is None


# ------------------------------------------------------ torch path, CPU ------
def _rollout(alg, T, N, O, CO, A, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(T):
        obs, cobs = torch.randn(N, O, generator=g), torch.randn(N, CO, generator=g)
        alg.act(obs, cobs if alg.storage.privileged_observations is not None else obs)
        done = torch.rand(N, generator=g) < 0.1
        alg.process_env_step(0.3 * torch.randn(N, generator=g), done, {"time_outs": done & (torch.rand(N, generator=g) < 0.5)})
    alg.compute_returns(torch.randn(N, CO, generator=g))


@pytest.mark.parametrize("schedule,CO", [("fixed", None), ("adaptive", 50)])
def test_torch_update_with_augmentation_is_the_update_on_the_explicitly_mirrored_batch(schedule, CO):
    """O = 48, A = 12, 64 envs x 4 steps.  The restatement: every mini-batch of the plain generator
    followed by its mirror image -- rows through the tables by fancy indexing, the scalar columns
    repeated (rsl_rl 2.x) -- through the plain PPO's own optimizer step.  Same torch ops in fp32."""
    O, A, N, T = 48, 12, 64, 4

    def edit(cfg):
        cfg.env.privileged_parameters, cfg.env.num_privileged_obs = True, 50
    tabs = symmetry_tables(env_like("go2", edit=edit if CO else None))
    torch.manual_seed(0)
    ac = ActorCritic(O, CO or O, A, [64, 32], [64, 32])
    kw = dict(num_learning_epochs=2, num_mini_batches=2, learning_rate=1e-3, schedule=schedule, device="cpu")
    aug = PPO(copy.deepcopy(ac), symmetry_cfg=ON, symmetry_tables=tabs, **kw)
    ref = PPO(copy.deepcopy(ac), **kw)
    for alg in (aug, ref):
        alg.init_storage(N, T, [O], [CO], [A])
        torch.manual_seed(3)
        _rollout(alg, T, N, O, CO or O, A, seed=1)
    assert torch.equal(aug.storage.observations, ref.storage.observations)
    torch.manual_seed(7)
    l_aug = aug.update()
    # the restatement
    (po, so), (pc, sg), (pa, sa) = [(torch.from_numpy(p.astype(np.int64)), torch.from_numpy(s)) for p, s in tabs]
    torch.manual_seed(7)
    acc = torch.zeros(2)
    for b in ref.storage.mini_batch_generator(2, 2):
        obs, cobs, act, val, adv, ret, logp, mu, sigma = b[:9]
        both = (torch.cat([obs, obs[:, po] * so]), torch.cat([cobs, cobs[:, pc] * sg]), torch.cat([act, act[:, pa] * sa]),
                val.repeat(2, 1), adv.repeat(2, 1), ret.repeat(2, 1), logp.repeat(2, 1),
                torch.cat([mu, mu[:, pa] * sa]), torch.cat([sigma, sigma[:, pa]]))
        ref._minibatch_step(*both, (None, None), None, acc)
    l_ref = (acc / 4).tolist()
    np.testing.assert_allclose(l_aug, l_ref, rtol=1e-6, atol=0)
    assert aug.learning_rate == pytest.approx(ref.learning_rate, rel=1e-6)
    moved = False
    for a, b, c in zip(aug.actor_critic.parameters(), ref.actor_critic.parameters(), ac.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9)
        moved |= bool((a - c).abs().max() > 0)
    assert moved
    # and it is not the plain update
    plain = PPO(copy.deepcopy(ac), **kw)
    plain.init_storage(N, T, [O], [CO], [A])
    torch.manual_seed(3)
    _rollout(plain, T, N, O, CO or O, A, seed=1)
    torch.manual_seed(7)
    plain.update()
    assert any(not torch.equal(a, b) for a, b in zip(aug.actor_critic.parameters(), plain.actor_critic.parameters()))


# ------------------------------------------------------------ entry point ----
def test_the_entry_point_is_declared_exported_and_mirrored():
    import ctypes as C
    from rsl_rl.modules import mfma_mlp as mm
    hdr = open(os.path.join(ROOT, "include", "ppo_mlp.h")).read()
    assert re.search(r"PMLP_API int pmlp_mirror_rows\(int32_t njobs, const pmlp_mirror_rows_job\* jobs, int64_t R,\s*"
                     r"void\* stream\);", hdr)
    lib = C.CDLL(mm.lib_path())
    assert hasattr(lib, "pmlp_mirror_rows")
    assert [n for n, _ in mm.MirrorRowsJob._fields_] == ["src", "dst", "ld", "K", "perm", "sign", "perm_host"]
    assert C.sizeof(mm.MirrorRowsJob) == 48
    assert int(re.search(r"#define PMLP_MIRROR_MAX_JOBS (\d+)", hdr).group(1)) == mm.PMLP_MIRROR_MAX_JOBS
    assert int(re.search(r"#define PMLP_MIRROR_MAX_K (\d+)", hdr).group(1)) == mm.PMLP_MIRROR_MAX_K
    assert "mirror_rows.hip" in open(os.path.join(ROOT, "unitree-rl-gym_amd", "csrc", "Makefile")).read()


# ----------------------------------------------------------- equivariance ----
def test_the_tables_are_the_oracle_steps_own_symmetry(oracle_lib):
    """4 airborne Go2 envs as two mirrored pairs through the oracle's control step (orc_step, the C
    ABI; state set as tests/test_oracle_physics.py sets it: written into the host arrays): after
    each of 4 control steps env 2k + 1's row is the mirror image of env 2k's within BOUND = 4 x the
    largest deviation the oracle itself shows here (symmetry_case.ORACLE_DEVIATION; the test prints
    the figure it sees).  The oracle's step writes no parameter tail, so its privileged row is not
    in this test: tests/test_gpu_symmetry.py checks the privileged row on k_step."""
    import bridge
    from hostspec import host_buffers, make_spec
    s = make_spec("go2", sc.cfg_edit)
    s._hooks = frozenset()
    policy, _, joints = symmetry_tables(s)
    b = host_buffers(s, sc.N)
    b["env_origins"][:] = 0
    root, q, qd = sc.initial_state(s.default_dof_pos, joints, kp=float(s.p_gains[0]), kd=float(s.d_gains[0]),
                                   action_scale=s.cfg.control.action_scale)
    assert (root[:, 2] == 3.0).all()  # airborne: the contact sweep's order is not mirror-symmetric
    b["root"][:] = root
    dofs = b["dofs"].reshape(sc.N, s.num_dof, 2)
    dofs[:, :, 0], dofs[:, :, 1] = q, qd
    worst = 0.0
    for step in range(sc.STEPS):
        act, cmd = sc.step_inputs(step, joints, dt=s.dt, action_scale=s.cfg.control.action_scale)
        b["commands"][:] = cmd
        b["actions"][:] = act
        b["episode_acc"][:] = 0
        bridge.step_raw(s.model, s.sim_params, s.task, sc.N, b, step, lib=oracle_lib)
        assert not b["reset"].any() and (b["root"][:, 2] > 2.5).all() and not b["cforce"].any()
        for a in (0, 2):  # the state cannot pass with a wrong table
            sep = sc.separation(b["obs"][a], policy)
            assert sep >= sc.SEPARATION, (step, a, sep)
        dev = sc.deviation(b["obs"], policy)
        print(f"step {step}: max |obs_B - mirror(obs_A)| = {dev:.4e}")
        worst = max(worst, dev)
        # a wrong table is far outside: one flipped sign, one pair left unswapped
        wrong = (policy[0].copy(), policy[1].copy())
        wrong[1][13] = -wrong[1][13]
        assert sc.deviation(b["obs"], wrong) > 100 * sc.BOUND
        wrong = (policy[0].copy(), policy[1].copy())
        wrong[0][[24, 27]] = [24, 27]
        assert sc.deviation(b["obs"], wrong) > 100 * sc.BOUND
    print(f"largest deviation {worst:.4e}; recorded {sc.ORACLE_DEVIATION:.4e}; bound {sc.BOUND:.4e}")
    assert worst <= sc.BOUND
