"""The Go2 handstand task on the host: registration, the native-only class, and the full
lgs_task_params derived with no GPU from the bundled go2 model (derive_env_spec ->
build_task_params), against the reference task's constants
(go2_handstand_config.py / go2_handstand_env.py)."""
import copy
import os

import numpy as np
import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from hostspec import make_spec
from legged_gym.envs.base.env_spec import derive_env_spec
from legged_gym.envs.base.legged_robot import LeggedRobot
from legged_gym.utils import task_registry
from leggedsim import cabi
from leggedsim.model import MODELS_DIR, Model
from leggedsim.task import build_task_params

TASK = "go2_handstand"
NEW_IDS = ["handstand_orientation", "handstand_base_height", "front_feet_contact", "hind_feet_no_contact", "pose",
           "stability", "stay_still", "lin_vel_xy", "energy", "front_hip_neutral", "front_feet_together"]


def handstand_spec(cfg_edit=None):
    """hostspec.make_spec for the handstand task: the bundled go2 model, the task class's own
    constants (task_cls)."""
    env_cfg, _ = task_registry.get_cfgs(TASK)
    cfg = copy.deepcopy(env_cfg)
    if cfg_edit:
        cfg_edit(cfg)
    cls = task_registry.get_task_class(TASK)
    model = Model.load(os.path.join(MODELS_DIR, "go2.npz"))
    model.reorder_points({model.body_names.index(n) for n in model.body_names if cfg.asset.foot_name in n})
    spec = derive_env_spec(cfg, model, cfg.sim.dt, cls.obs_layout, cls.hip_dof_indices, verbose=False, task_cls=cls)
    spec.model = model
    spec.task = build_task_params(spec)
    spec.sim_params = cabi.sim_params_from_cfg(cfg.sim, cfg.asset, max_contacts=cls.max_contacts,
                                               max_rows=cls.max_rows, ground_friction=float(cfg.terrain.static_friction))
    return spec


@pytest.fixture(scope="module")
def spec():
    return handstand_spec()


def test_registered_and_native_only():
    assert TASK in task_registry.task_classes
    cls = task_registry.get_task_class(TASK)
    assert issubclass(cls, LeggedRobot)
    assert cls.python_step_hooks() == frozenset()
    assert cls._overridden(cls.NATIVE_STEP_METHODS) == []
    cls._refuse_native_step_overrides()
    for name in cls.PYTHON_STEP_HOOKS + cls.NATIVE_STEP_METHODS:
        assert name not in vars(cls), name
    assert not [n for n in vars(cls) if n.startswith("_reward_")]  # every term is the kernel's
    _, train_cfg = task_registry.get_cfgs(TASK)
    assert train_cfg.runner.experiment_name == "go2_handstand"


def test_header_ids_follow_the_python_list():
    assert cabi.REWARD_IDS[-len(NEW_IDS):] == NEW_IDS
    assert len(cabi.REWARD_IDS) == 23 + len(NEW_IDS) and cabi.MAX_REWARDS == 24
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "leggedsim.h")).read()
    enum = hdr[hdr.index("enum lgs_reward_id"):hdr.index("LGS_REW_COUNT")]
    names = [t.strip().split()[0].rstrip(",") for t in enum.replace("\n", " ").split("LGS_REW_")[1:]]
    assert [n.lower() for n in names] == cabi.REWARD_IDS
    assert "LGS_OBS_HANDSTAND = 2" in hdr and cabi.OBS_HANDSTAND == 2


def test_bodies_and_layout(spec):
    T, names = spec.task, spec.model.body_names
    assert T.obs_layout == cabi.OBS_HANDSTAND and T.num_obs == 46 and T.num_privileged_obs == 46
    assert T.num_actions == 12 and T.decimation == 5 and T.control_type == 0
    assert T.action_scale == pytest.approx(0.3) and list(T.p_gains)[:12] == [35.0] * 12
    assert list(T.d_gains)[:12] == [0.5] * 12
    assert [names[i] for i in list(T.feet_idx)[:T.num_feet]] == ["FL_foot", "FR_foot", "RL_foot", "RR_foot"]
    assert T.num_front_feet == 2
    term = [names[i] for i in list(T.termination_idx)[:T.num_termination]]
    assert len(term) == 15
    assert sorted(term) == sorted(["base", "Head_lower", "Head_upper"] +
                                  [f"{leg}_{part}" for leg in ("FL", "FR", "RL", "RR") for part in ("hip", "thigh", "calf")])
    assert T.num_penalised == 12
    assert T.base_init_state[2] == pytest.approx(0.28) and T.base_height_target == pytest.approx(0.65)
    assert T.only_positive_rewards == 0 and T.has_termination_reward == 1
    assert T.termination_mode == 1 and T.fallen_band == pytest.approx(0.2)
    assert T.contact_flag_threshold == 5.0 and T.contact_flip_prob == pytest.approx(0.01)
    assert T.feet_together_target == pytest.approx(0.12)
    assert T.record_unclipped_torques == 1
    # front_feet_together reads the front feet's rigid-body rows: the step refreshes the feet
    assert T.write_body_states == 1
    assert T.body_state_mask == sum(1 << i for i in list(T.feet_idx)[:4])
    dofs = spec.dof_names
    assert [dofs[i] for i in list(T.hip_dofs)[:T.num_hip]] == ["FL_hip_joint", "FR_hip_joint"]


def test_reward_ids_resolve_per_task(spec):
    T = spec.task
    ids = {n: cabi.REWARD_IDS[T.reward_ids[k]] for k, n in enumerate(spec.reward_names)}
    assert T.num_rewards == 17 == len(ids)
    assert ids["orientation"] == "handstand_orientation" and ids["base_height"] == "handstand_base_height"
    for n, i in ids.items():
        if n not in ("orientation", "base_height"):
            assert i == n
    assert set(NEW_IDS) - {"energy"} <= set(ids.values())
    scale = dict(zip(spec.reward_names, list(T.reward_scales)))
    dt = 5 * 0.005
    assert scale["pose"] == pytest.approx(10.0 * dt) and scale["lin_vel_xy"] == pytest.approx(-3 * dt)
    assert T.termination_scale == pytest.approx(-5.0 * dt)
    # the same cfg names on the Go2 walking task are the base terms, as before
    assert cabi.REWARD_ALIASES == {"stumble": "feet_stumble"}
    go2 = make_spec("go2", lambda c: (setattr(c.rewards.scales, "orientation", -1.0),
                                      setattr(c.rewards.scales, "base_height", -2.0)))
    gid = {n: cabi.REWARD_IDS[go2.task.reward_ids[k]] for k, n in enumerate(go2.reward_names)}
    assert gid["orientation"] == "orientation" and gid["base_height"] == "base_height"
    assert cabi.reward_id("orientation") == cabi.REWARD_ID["orientation"]
    assert cabi.reward_id("stumble") == cabi.REWARD_ID["feet_stumble"] and cabi.reward_id("no_such_term") is None


def test_clamp_pose_and_noise(spec):
    T, dofs = spec.task, spec.dof_names
    pose = {"hip": 0.0, "thigh_front": -0.89, "calf_front": -1.5, "thigh_rear": 1.7, "calf_rear": -1.853}
    lo, hi = np.array(list(T.pd_target_lower)[:12]), np.array(list(T.pd_target_upper)[:12])
    target, weight = np.array(list(T.pose_target)[:12]), np.array(list(T.pose_weight)[:12])
    assert T.clamp_pd_targets == 1
    for j, n in enumerate(dofs):
        rear = n[:2] in ("RL", "RR")
        part = n.split("_")[1]
        want = pose["hip"] if part == "hip" else pose[f"{part}_{'rear' if rear else 'front'}"]
        assert target[j] == np.float32(want), n
        assert np.isfinite(lo[j]) == np.isfinite(hi[j]) == rear, n
        if rear:
            assert lo[j] == np.float32(want) - np.float32(0.15) and hi[j] == np.float32(want) + np.float32(0.15), n
            assert weight[j] == np.float32(0.3)
        else:
            assert lo[j] == -np.inf and hi[j] == np.inf and weight[j] == 1.0
    assert int(np.isfinite(lo).sum()) == 6
    nv = np.array(list(T.noise_vec)[:46])
    assert T.add_noise == 1
    np.testing.assert_allclose(nv[:3], 0.2 * 0.25, rtol=1e-6)
    np.testing.assert_allclose(nv[3:6], 0.05, rtol=1e-6)
    np.testing.assert_allclose(nv[6:18], 0.01, rtol=1e-6)
    np.testing.assert_allclose(nv[18:30], 1.5 * 0.05, rtol=1e-6)
    assert not nv[-16:].any()
    np.testing.assert_array_equal(spec.noise_scale_vec, nv.astype(np.float32))
    assert not np.array(list(T.noise_vec)[46:]).any()


@pytest.mark.parametrize("task", ["go2", "h1", "g1", "h1_2"])
def test_other_tasks_have_every_new_switch_off(task):
    T = make_spec(task).task
    assert T.obs_layout in (cabi.OBS_QUADRUPED, cabi.OBS_HUMANOID)
    for f in ("clamp_pd_targets", "record_unclipped_torques", "termination_mode", "num_front_feet"):
        assert getattr(T, f) == 0, f
    for f in ("fallen_band", "contact_flag_threshold", "contact_flip_prob", "feet_together_target"):
        assert getattr(T, f) == 0.0, f
    for f in ("pd_target_lower", "pd_target_upper", "pose_target", "pose_weight"):
        assert not any(getattr(T, f)), f
    assert all(i < cabi.REWARD_ID["handstand_orientation"] for i in list(T.reward_ids)[:T.num_rewards])
