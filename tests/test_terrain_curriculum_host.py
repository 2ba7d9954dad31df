"""Host side of the rough-terrain path of the fused step: the cfg switches
`terrain.level_curriculum`, `terrain.scan_heights`, `rewards.ground_relative_heights`, the task
parameters they become (leggedsim/task.py), the `g1_terrain` registration and the ctypes mirrors
of the appended ABI fields.  No GPU."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from hostspec import make_spec
from legged_gym.envs.base.env_spec import derive_env_spec
from legged_gym.utils import task_registry
from leggedsim import cabi
from leggedsim.model import MODELS_DIR, Model
from leggedsim.task import build_task_params, terrain_switches
from rsl_rl.modules import mfma_mlp as mm

SWITCH_FIELDS = ("terrain_curriculum", "terrain_rows", "terrain_cols", "terrain_half_length_sq", "measure_heights",
                 "num_height_x", "num_height_y", "ground_relative_heights")


def _task_params(task, model_file, cfg_edit=None):
    """build_task_params of a registered task on its bundled model (hostspec.make_spec's recipe,
    for tasks it has no model entry for)."""
    env_cfg, _ = task_registry.get_cfgs(task)
    cfg = copy.deepcopy(env_cfg)
    if cfg_edit:
        cfg_edit(cfg)
    cls = task_registry.get_task_class(task)
    model = Model.load(os.path.join(MODELS_DIR, model_file + ".npz"))
    feet = {model.body_names.index(n) for n in model.body_names if cfg.asset.foot_name in n}
    model.reorder_points(feet)
    spec = derive_env_spec(cfg, model, cfg.sim.dt, cls.obs_layout, cls.hip_dof_indices, verbose=False,
                           task_cls=cls)
    return build_task_params(spec), cfg


def test_g1_terrain_is_registered_like_g1_rough_with_the_switches_on():
    from legged_gym.envs.g1.g1_config import G1HeightfieldCfg, G1RoughCfgPPO, G1TerrainCfg
    from legged_gym.envs.g1.g1_env import G1Robot
    assert task_registry.get_task_class("g1_terrain") is G1Robot
    env_cfg, train_cfg = task_registry.get_cfgs("g1_terrain")
    assert isinstance(env_cfg, G1TerrainCfg) and isinstance(env_cfg, G1HeightfieldCfg)
    assert isinstance(train_cfg, G1RoughCfgPPO)
    assert env_cfg.terrain.mesh_type == "heightfield"
    assert env_cfg.terrain.level_curriculum and env_cfg.terrain.scan_heights
    assert env_cfg.rewards.ground_relative_heights
    # g1_rough is left alone
    rough, _ = task_registry.get_cfgs("g1_rough")
    assert not rough.terrain.level_curriculum and not rough.terrain.scan_heights
    assert not rough.rewards.ground_relative_heights
    assert terrain_switches(rough) == (False, False, False)
    assert terrain_switches(env_cfg) == (True, True, True)


def _default_map(cfg):
    """legged_gym's default map, set on the instance (class attributes may have been edited by
    whoever ran before)."""
    cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.terrain_length = 10, 20, 8.0


def _plane(cfg):
    cfg.terrain.mesh_type = "plane"


def test_g1_terrain_task_params_carry_the_switches_grid_and_tile_table():
    T, cfg = _task_params("g1_terrain", "g1_12dof", _default_map)
    tc = cfg.terrain
    assert T.terrain_curriculum == 1
    assert (T.terrain_rows, T.terrain_cols) == (tc.num_rows, tc.num_cols) == (10, 20)
    assert T.terrain_half_length_sq == np.float32(16.0)  # (8 m / 2)^2
    assert T.measure_heights == 1 and T.ground_relative_heights == 1
    assert (T.num_height_x, T.num_height_y) == (17, 11)  # legged_gym's 187-point scan
    np.testing.assert_array_equal(np.array(T.height_points_x[:17], np.float32),
                                  np.array(tc.measured_points_x, np.float32))
    np.testing.assert_array_equal(np.array(T.height_points_y[:11], np.float32),
                                  np.array(tc.measured_points_y, np.float32))
    assert not any(T.height_points_x[17:]) and not any(T.height_points_y[11:])
    # everything else is g1_rough's
    R, _ = _task_params("g1_rough", "g1_12dof", _default_map)
    skip = set(SWITCH_FIELDS) | {"height_points_x", "height_points_y"}
    for name, _ in cabi.TaskParams._fields_:
        if name in skip:
            continue
        a, b = getattr(T, name), getattr(R, name)
        if hasattr(a, "__len__"):
            a, b = list(a), list(b)
        assert a == b, name


@pytest.mark.parametrize("task,model", [("go2", "go2"), ("go2_handstand", "go2"), ("h1", "h1"), ("h1_2", "h1_2_12dof"),
                                        ("g1", "g1_12dof"), ("g1_rough", "g1_12dof")])
def test_every_existing_task_has_the_new_fields_zero(task, model):
    T, _ = _task_params(task, model)
    for name in SWITCH_FIELDS:
        assert getattr(T, name) == 0, name
    assert not any(T.height_points_x) and not any(T.height_points_y)


def _on(sec, attr):
    def edit(cfg):
        setattr(getattr(cfg, sec), attr, True)
    return edit


@pytest.mark.parametrize("sec,attr", [("terrain", "level_curriculum"), ("terrain", "scan_heights"),
                                      ("rewards", "ground_relative_heights")])
def test_a_switch_on_a_plane_is_refused(sec, attr):
    def edit(cfg):
        _plane(cfg)
        _on(sec, attr)(cfg)
        if attr == "ground_relative_heights":  # (with its scan, so that only the plane is at fault)
            cfg.terrain.scan_heights = True
    with pytest.raises(ValueError, match="need a terrain map"):
        make_spec("go2", edit)
    with pytest.raises(ValueError, match="need a terrain map"):
        _task_params("g1", "g1_12dof", edit)


def test_ground_relative_heights_without_the_scan_is_refused():
    def edit(cfg):
        cfg.terrain.mesh_type = "heightfield"
        cfg.rewards.ground_relative_heights = True
    with pytest.raises(ValueError, match="needs terrain.scan_heights"):
        _task_params("g1_rough", "g1_12dof", edit)

    def both(cfg):
        edit(cfg)
        cfg.terrain.scan_heights = True
    T, _ = _task_params("g1_rough", "g1_12dof", both)
    assert T.ground_relative_heights == 1 and T.measure_heights == 1 and T.terrain_curriculum == 0


def test_a_scan_grid_past_32_points_a_side_is_refused():
    def edit(cfg):
        cfg.terrain.scan_heights = True
        cfg.terrain.measured_points_x = [0.01 * i for i in range(33)]
    with pytest.raises(ValueError, match="1 to 32 entries"):
        _task_params("g1_rough", "g1_12dof", edit)


def test_appended_abi_fields_are_last_and_mirrored():
    """The new fields are appended (nothing before them moved) and the Python mirrors name them in
    the header's order."""
    names = [n for n, _ in cabi.TaskParams._fields_]
    assert names[-10:] == ["terrain_curriculum", "terrain_rows", "terrain_cols", "terrain_half_length_sq",
                           "measure_heights", "num_height_x", "num_height_y", "height_points_x", "height_points_y",
                           "ground_relative_heights"]
    assert names[-11] == "feet_together_target"
    env = [n for n, _ in cabi.EnvBuffers._fields_]
    assert env[-6:] == ["episode_acc_next", "terrain_levels", "terrain_types", "terrain_origins",
                        "terrain_level_sum", "measured_heights"]
    ex = [n for n, _ in mm.EnvExtras._fields_]
    assert ex[-3:] == ["step_counter", "level_sum", "num_envs"]
    assert C.sizeof(mm.EnvExtras) % 8 == 0
    assert cabi.STREAM_TERRAIN == 6 and cabi.MAX_HEIGHT_POINTS == 32
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "leggedsim.h")).read()
    assert "#define LGS_STREAM_TERRAIN 6u" in header and "#define LGS_MAX_HEIGHT_POINTS 32" in header
