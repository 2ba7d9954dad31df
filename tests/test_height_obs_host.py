"""Host side of the height scan in the policy input: the cfg switch
`terrain.scan_in_observations`, what it becomes (leggedsim/task.py: the head of the noise vector
in lgs_task_params, the tail's one scale in lgs_height_obs), the refusals, the `go2_terrain`
registration, the new entry point's declaration / export / mirror, and the fused MLP forward's
input-width limit.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from legged_gym.utils import task_registry
from leggedsim import cabi, native
from leggedsim.task import build_task_params, height_obs_params, scan_in_observations, terrain_switches
from rsl_rl.modules import mfma_mlp as mm
from test_terrain_curriculum_host import _default_map, _task_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXISTING = [("go2", "go2"), ("go2_handstand", "go2"), ("h1", "h1"), ("h1_2", "h1_2_12dof"), ("g1", "g1_12dof"),
            ("g1_rough", "g1_12dof"), ("g1_terrain", "g1_12dof")]


def _spec(task, model, cfg_edit=None):
    """(spec, cfg) of a task on its bundled model: what build_task_params / height_obs_params read."""
    import copy
    from legged_gym.envs.base.env_spec import derive_env_spec
    from leggedsim.model import MODELS_DIR, Model
    env_cfg, _ = task_registry.get_cfgs(task)
    cfg = copy.deepcopy(env_cfg)
    _default_map(cfg)
    if cfg_edit:
        cfg_edit(cfg)
    cls = task_registry.get_task_class(task)
    m = Model.load(os.path.join(MODELS_DIR, model + ".npz"))
    m.reorder_points({m.body_names.index(n) for n in m.body_names if cfg.asset.foot_name in n})
    return derive_env_spec(cfg, m, cfg.sim.dt, cls.obs_layout, cls.hip_dof_indices, verbose=False, task_cls=cls), cfg


def test_go2_terrain_is_registered_with_the_four_switches_and_235_observations():
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from legged_gym.envs.go2.go2_config import GO2RoughCfg, GO2RoughCfgPPO, GO2TerrainCfg
    assert task_registry.get_task_class("go2_terrain") is LeggedRobot  # no Python step method of its own
    env_cfg, train_cfg = task_registry.get_cfgs("go2_terrain")
    assert isinstance(env_cfg, GO2TerrainCfg) and isinstance(env_cfg, GO2RoughCfg)
    assert isinstance(train_cfg, GO2RoughCfgPPO) and train_cfg.runner.experiment_name == "go2_terrain"
    assert train_cfg.policy.actor_hidden_dims == [512, 256, 128] and not hasattr(train_cfg.policy, "rnn_type")
    assert env_cfg.terrain.mesh_type == "heightfield"
    assert terrain_switches(env_cfg) == (True, True, True) and scan_in_observations(env_cfg)
    assert env_cfg.env.num_observations == 235 and not env_cfg.env.num_privileged_obs
    # the plain go2 task is left alone
    go2, go2_train = task_registry.get_cfgs("go2")
    assert go2.env.num_observations == 48 and not scan_in_observations(go2)
    assert go2_train.runner.experiment_name == "rough_go2"


def test_go2_terrain_task_params_and_height_obs():
    spec, cfg = _spec("go2_terrain", "go2")
    T, H = build_task_params(spec), height_obs_params(spec)
    assert (T.num_obs, T.num_privileged_obs, T.obs_layout) == (235, 0, cabi.OBS_QUADRUPED)
    assert (T.measure_heights, T.num_height_x, T.num_height_y) == (1, 17, 11)
    assert T.terrain_curriculum == 1 and T.ground_relative_heights == 1
    ns, sc = cfg.noise.noise_scales, cfg.normalization.obs_scales
    tail = np.float32(ns.height_measurements * cfg.noise.noise_level * sc.height_measurements)
    assert (H.enabled, H.offset, H.clip) == (1, 0.5, 1.0)
    assert H.scale == np.float32(sc.height_measurements) and H.noise_scale == tail and tail > 0
    # the full-length vector as legged_gym builds it: go2's head, then 187 copies of the tail scale
    go2, _ = _spec("go2", "go2")
    v = np.asarray(spec.noise_scale_vec, np.float32)
    assert v.shape == (235,)
    np.testing.assert_array_equal(v[:48], np.asarray(go2.noise_scale_vec, np.float32))
    np.testing.assert_array_equal(v[48:], np.full(187, tail, np.float32))
    # lgs_task_params keeps the head only (noise_vec stays LGS_MAX_OBS long)
    assert len(T.noise_vec) == cabi.MAX_OBS == 128
    np.testing.assert_array_equal(np.array(T.noise_vec[:48], np.float32), v[:48])
    assert not any(T.noise_vec[48:])


def test_g1_with_the_switch_on_has_the_humanoid_rows_plus_the_scan():
    def edit(cfg):
        cfg.terrain.scan_in_observations = True
        cfg.env.num_observations, cfg.env.num_privileged_obs = 47 + 187, 50 + 187
    spec, _ = _spec("g1_terrain", "g1_12dof", edit)
    T, H = build_task_params(spec), height_obs_params(spec)
    assert (T.num_obs, T.num_privileged_obs, H.enabled) == (234, 237, 1)
    off, _ = _spec("g1_terrain", "g1_12dof")
    np.testing.assert_array_equal(np.array(T.noise_vec[:47], np.float32), np.asarray(off.noise_scale_vec, np.float32))
    assert not any(T.noise_vec[47:])


@pytest.mark.parametrize("task,model", EXISTING)
def test_every_existing_task_has_the_call_disabled_and_its_task_params_unchanged(task, model):
    """lgs_height_obs is off, and lgs_task_params is, byte for byte (so field for field), what the
    tree before this feature built (tests/golden/task_params_before_height_obs.npz)."""
    spec, cfg = _spec(task, model)
    H = height_obs_params(spec)
    assert (H.enabled, H.offset, H.clip, H.scale, H.noise_scale) == (0, 0.0, 0.0, 0.0, 0.0)
    assert not scan_in_observations(cfg)
    T = build_task_params(spec)
    want = np.load(os.path.join(ROOT, "tests", "golden", "task_params_before_height_obs.npz"))[task]
    got = np.frombuffer(bytes(T), dtype=np.uint8)
    assert got.size == want.size == C.sizeof(cabi.TaskParams)
    if not np.array_equal(got, want):
        W = cabi.TaskParams.from_buffer_copy(want.tobytes())
        for name, _ in cabi.TaskParams._fields_:
            a, b = getattr(T, name), getattr(W, name)
            if hasattr(a, "__len__"):
                a, b = list(a), list(b)
            assert a == b, name
        raise AssertionError("lgs_task_params differs outside its named fields")


def _scan_on(cfg):
    cfg.terrain.mesh_type = "heightfield"
    cfg.terrain.scan_heights = True
    cfg.terrain.scan_in_observations = True
    cfg.env.num_observations = 235


def test_refused_on_a_plane():
    def edit(cfg):
        _scan_on(cfg)
        cfg.terrain.mesh_type = "plane"
    with pytest.raises(ValueError, match="need a terrain map"):
        _task_params("go2", "go2", edit)


def test_refused_for_the_handstand_layout():
    def edit(cfg):
        _scan_on(cfg)
        cfg.env.num_observations = 46 + 187
    with pytest.raises(ValueError, match="quadruped or the humanoid observation layout"):
        _task_params("go2_handstand", "go2", edit)


def test_refused_without_scan_heights():
    def edit(cfg):
        _scan_on(cfg)
        cfg.terrain.scan_heights = False
    with pytest.raises(ValueError, match="scan_in_observations needs terrain.scan_heights"):
        _task_params("go2", "go2", edit)
    # terrain.measure_heights (True in every config, inert) is not the switch
    plain, _ = task_registry.get_cfgs("go2")
    assert plain.terrain.measure_heights and not scan_in_observations(plain)


@pytest.mark.parametrize("num_obs", [48, 234, 236])
def test_refused_when_num_observations_is_not_head_plus_scan(num_obs):
    def edit(cfg):
        _scan_on(cfg)
        cfg.env.num_observations = num_obs
    with pytest.raises(ValueError, match=r"num_observations must be 48 \+ 187 scan points = 235"):
        _task_params("go2", "go2", edit)

    def hum(cfg):
        cfg.terrain.scan_in_observations = True
        cfg.env.num_observations, cfg.env.num_privileged_obs = 234, 50
    with pytest.raises(ValueError, match=r"num_privileged_obs must be 50 \+ 187 scan points = 237"):
        _task_params("g1_terrain", "g1_12dof", hum)


def test_refused_for_a_grid_of_more_than_256_points():
    def edit(cfg):
        _scan_on(cfg)
        cfg.terrain.measured_points_x = [0.05 * i for i in range(24)]  # 24 x 11 = 264
        cfg.env.num_observations = 48 + 264
    with pytest.raises(ValueError, match="264 scan points, the rows take 1 to 256"):
        _task_params("go2", "go2", edit)

    def fits(cfg):
        _scan_on(cfg)
        cfg.terrain.measured_points_x = [0.05 * i for i in range(16)]  # 16 x 16 = 256
        cfg.terrain.measured_points_y = [0.05 * i for i in range(16)]
        cfg.env.num_observations = 48 + 256
    T, _ = _task_params("go2", "go2", fits)
    assert T.num_obs == 304


def test_refused_for_a_non_uniform_tail_noise():
    spec, _ = _spec("go2_terrain", "go2")
    v = np.array(spec.noise_scale_vec, np.float32)
    v[100] *= 2  # a task's _get_noise_scale_vec override
    spec.noise_scale_vec = v
    with pytest.raises(ValueError, match="must share one noise scale"):
        build_task_params(spec)
    v[48:] = v[100]  # uniform again, another value: taken
    assert height_obs_params(spec).noise_scale == v[100]


def test_the_new_entry_point_is_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert re.search(r"LGS_API int lgs_set_height_observations\(lgs_sim\* sim, const lgs_height_obs\* desc\);", header)
    m = re.search(r"typedef struct lgs_height_obs \{(.*?)\} lgs_height_obs;", header, re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(cabi.HeightObs._fields_)
    assert [n for n, _ in cabi.HeightObs._fields_] == ["enabled", "offset", "clip", "scale", "noise_scale"]
    assert "#define LGS_MAX_SCAN_OBS 256" in header and cabi.MAX_SCAN_OBS == 256
    assert "#define LGS_MAX_OBS 128" in header and cabi.MAX_OBS == 128
    assert "lgs_set_height_observations" in native.EXPORTED_SYMBOLS
    import torch  # noqa: F401  (the HIP runtime before the library)
    lib = native.load()
    assert hasattr(lib, "lgs_set_height_observations")
    assert lib.lgs_set_height_observations.restype is C.c_int
    # a NULL sim is a status and an error text, not a crash
    assert lib.lgs_set_height_observations(None, None) != 0 and lib.lgs_last_error()


def test_the_pinned_structs_keep_their_last_fields():
    assert [n for n, _ in cabi.TaskParams._fields_][-3:] == ["height_points_x", "height_points_y",
                                                             "ground_relative_heights"]
    assert [n for n, _ in cabi.EnvBuffers._fields_][-2:] == ["terrain_level_sum", "measured_heights"]
    assert [n for n, _ in mm.EnvExtras._fields_][-3:] == ["step_counter", "level_sum", "num_envs"]
    assert C.sizeof(cabi.TaskParams) == 2632


def test_mlp_forward_supported_takes_inputs_up_to_256_in_multiples_of_16():
    import torch.nn as nn
    lins = [nn.Linear(235, 512), nn.Linear(512, 256), nn.Linear(256, 128), nn.Linear(128, 12)]
    assert mm.mlp_forward_supported(lins, 240) and mm.mlp_forward_supported(lins, 256)
    assert not mm.mlp_forward_supported(lins, 248) and not mm.mlp_forward_supported(lins, 272)
    assert mm.mlp_forward_supported(lins, 48) and mm.mlp_forward_supported(lins, 64)
    header = open(os.path.join(ROOT, "include", "ppo_mlp.h")).read()
    assert re.search(r"K0 a multiple of 16,\s*\n?\s*\*?\s*<= 256", header)
