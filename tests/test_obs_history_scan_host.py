"""Host side of the observation history with the height scan: the policy row is a
history of the layout's head alone, then one current scan (H * F + P entries).  The
`go2_terrain_robust` registration, the widths the cfg checks accept and refuse, the noise vector
(the head tiled, then the scan's one scale), the unchanged lgs_task_params of every existing
task, and the fused forward's second width class (multiples of 64 up to 512).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch.nn as nn

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from legged_gym.utils import task_registry
from leggedsim import cabi
from leggedsim.task import (actuator_rand_params, build_task_params, check_scan_observations, height_obs_params,
                            obs_history_params, scan_in_observations, terrain_switches)
from rsl_rl.modules import mfma_mlp as mm
from test_actuator_rand_host import SWITCHES
from test_height_obs_host import EXISTING, _spec  # (EXISTING: the tasks of the golden record)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _pair(H, num_obs, priv=None):
    def edit(cfg):
        cfg.env.history_length = H
        cfg.env.num_observations = num_obs
        if priv is not None:
            cfg.env.num_privileged_obs = priv
    return edit


def test_go2_terrain_robust_is_registered_with_427_inputs_and_the_switches_on():
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from legged_gym.envs.go2.go2_config import GO2TerrainCfg, GO2TerrainCfgPPO, GO2TerrainRobustCfg
    assert task_registry.get_task_class("go2_terrain_robust") is LeggedRobot  # no Python step method of its own
    env_cfg, train_cfg = task_registry.get_cfgs("go2_terrain_robust")
    assert isinstance(env_cfg, GO2TerrainRobustCfg) and isinstance(env_cfg, GO2TerrainCfg)
    assert isinstance(train_cfg, GO2TerrainCfgPPO) and train_cfg.runner.experiment_name == "go2_terrain_robust"
    assert train_cfg.policy.actor_hidden_dims == [512, 256, 128] == train_cfg.policy.critic_hidden_dims
    assert not hasattr(train_cfg.policy, "rnn_type")
    assert env_cfg.env.history_length == 5 and env_cfg.env.num_observations == 427 == 5 * 48 + 187
    assert not env_cfg.env.num_privileged_obs
    assert terrain_switches(env_cfg) == (True, True, True) and scan_in_observations(env_cfg)
    assert all(getattr(env_cfg.domain_rand, s) for s in SWITCHES)
    # the tasks it is made of are left alone
    terrain, _ = task_registry.get_cfgs("go2_terrain")
    assert terrain.env.history_length == 1 and terrain.env.num_observations == 235
    assert not any(getattr(terrain.domain_rand, s, False) for s in SWITCHES)


def test_the_task_becomes_both_descriptors_and_the_actuator_ranges():
    spec, cfg = _spec("go2_terrain_robust", "go2")
    R, Hobs, A = obs_history_params(spec), height_obs_params(spec), actuator_rand_params(spec)
    assert (R.enabled, R.frames, R.num_frame) == (1, 5, 48)
    assert Hobs.enabled == 1 and Hobs.num_points == 187
    assert A.enabled == 1 and A.resample_on_reset == 1
    assert check_scan_observations(cfg, cabi.OBS_QUADRUPED, 12) == 187
    T = build_task_params(spec)
    assert (T.num_obs, T.num_privileged_obs, T.measure_heights) == (427, 0, 1)
    assert T.num_height_x * T.num_height_y == 187
    assert C.sizeof(cabi.TaskParams) == 2632


@pytest.mark.parametrize("task,model", EXISTING)
def test_every_existing_tasks_task_params_are_the_golden_record(task, model):
    spec, _ = _spec(task, model)
    want = np.load(os.path.join(ROOT, "tests", "golden", "task_params_before_height_obs.npz"))[task]
    got = np.frombuffer(bytes(build_task_params(spec)), dtype=np.uint8)
    assert got.size == want.size == C.sizeof(cabi.TaskParams)
    np.testing.assert_array_equal(got, want)


def test_the_noise_vector_is_the_head_tiled_then_the_scans_scale():
    spec, _ = _spec("go2_terrain_robust", "go2")
    one, _ = _spec("go2_terrain", "go2")
    v, w = np.asarray(spec.noise_scale_vec, F32), np.asarray(one.noise_scale_vec, F32)
    assert v.shape == (427,) and w.shape == (235,)
    np.testing.assert_array_equal(v[:240], np.tile(w[:48], 5))
    np.testing.assert_array_equal(v[240:], w[48:])
    assert (v[240:] == v[240]).all() and v[240] > 0
    # the kernel's copy: the head's 48 scales, nothing after them; the scan's scale in lgs_height_obs
    T, T1 = build_task_params(spec), build_task_params(one)
    assert list(T.noise_vec) == list(T1.noise_vec) and not any(list(T.noise_vec)[48:])
    assert height_obs_params(spec).noise_scale == height_obs_params(one).noise_scale == float(v[240])
    # the humanoid: 47-entry frames, the privileged row without a history
    hum, _ = _spec("g1_terrain", "g1_12dof", _scan_on(_pair(2, 2 * 47 + 187, 50 + 187)))
    hv = np.asarray(hum.noise_scale_vec, F32)
    assert hv.shape == (281,)
    np.testing.assert_array_equal(hv[:94], np.tile(hv[:47], 2))
    assert (hv[94:] == hv[94]).all()
    Th = build_task_params(hum)
    assert (Th.num_obs, Th.num_privileged_obs) == (281, 237)


def _scan_on(then):
    def edit(cfg):
        cfg.terrain.scan_in_observations = True
        then(cfg)
    return edit


def test_overrides_that_break_the_tiling_or_the_tail_are_still_refused():
    spec, _ = _spec("go2_terrain_robust", "go2")
    v = np.asarray(spec.noise_scale_vec, F32).copy()
    bad = v.copy()
    bad[48 + 5] *= 2  # an older frame with a scale of its own
    spec.noise_scale_vec = bad
    with pytest.raises(ValueError, match="tiled 5 times"):
        build_task_params(spec)
    bad = v.copy()
    bad[240 + 3] *= 2  # a scan point with a scale of its own
    spec.noise_scale_vec = bad
    with pytest.raises(ValueError, match="share one noise scale"):
        build_task_params(spec)
    spec.noise_scale_vec = v
    spec._hooks = frozenset({"compute_observations"})
    with pytest.raises(ValueError, match="compute_observations"):
        obs_history_params(spec)


@pytest.mark.parametrize("H,num_obs,want", [(5, 426, 427), (5, 283, 427), (2, 96, 283), (5, 240, 427), (5, 235, 427)])
def test_a_wrong_width_of_the_pair_is_refused_with_the_width_it_must_be(H, num_obs, want):
    spec, cfg = _spec("go2_terrain", "go2")
    cfg.env.history_length, cfg.env.num_observations = H, num_obs
    with pytest.raises(ValueError, match=rf"do not combine.*must be {want}"):
        obs_history_params(spec)
    with pytest.raises(ValueError, match=rf"do not combine.*must be {want}"):
        check_scan_observations(cfg, cabi.OBS_QUADRUPED, 12)


def test_the_right_widths_are_accepted_and_h1_keeps_the_scans_own_text():
    for H in (2, 5, 8):
        spec, cfg = _spec("go2_terrain", "go2", _pair(H, 48 * H + 187))
        assert obs_history_params(spec).frames == H
        assert check_scan_observations(cfg, cabi.OBS_QUADRUPED, 12) == 187
        assert build_task_params(spec).num_obs == 48 * H + 187
    spec, cfg = _spec("go2_terrain", "go2")
    cfg.env.num_observations = 234
    with pytest.raises(ValueError, match=r"must be 48 \+ 187 scan points = 235, not 234"):
        check_scan_observations(cfg, cabi.OBS_QUADRUPED, 12)
    # the humanoid's privileged row takes the scan and no history
    spec, cfg = _spec("g1_terrain", "g1_12dof", _scan_on(_pair(2, 281, 237)))
    cfg.env.num_privileged_obs = 2 * 50 + 187
    with pytest.raises(ValueError, match=r"num_privileged_obs must be 50 \+ 187 scan points = 237"):
        check_scan_observations(cfg, cabi.OBS_HUMANOID, 12)
    # the handstand layout takes no scan, with or without a history
    with pytest.raises(ValueError, match="quadruped or the humanoid"):
        check_scan_observations(cfg, cabi.OBS_HANDSTAND, 12)


def test_mlp_forward_supported_takes_multiples_of_64_up_to_512():
    lins = [nn.Linear(427, 512), nn.Linear(512, 256), nn.Linear(256, 128), nn.Linear(128, 12)]
    for k0 in (320, 384, 448, 512):
        assert mm.mlp_forward_supported(lins, k0), k0
    for k0 in (272, 288, 432, 576, 640):
        assert not mm.mlp_forward_supported(lins, k0), k0
    assert mm.mlp_forward_supported(lins, 240) and mm.mlp_forward_supported(lins, 256)  # (as before)
    # the first layer's padding: to 8 up to 256, to 64 above
    assert [mm._pad_k0(n) for n in (45, 48, 235, 250, 256)] == [48, 48, 240, 256, 256]
    assert [mm._pad_k0(n) for n in (257, 300, 320, 427, 428, 448, 500, 512)] == [320, 320, 320, 448, 448, 448, 512, 512]
    assert mm.mlp_forward_supported(lins, mm._pad_k0(427))


def test_the_header_states_both_width_classes_and_the_pair():
    header = open(os.path.join(ROOT, "include", "ppo_mlp.h")).read()
    assert re.search(r"K0 a multiple of 16,\s*\n?\s*\*?\s*<= 256", header)
    assert re.search(r"or a multiple of 64, 256 < K0 <= 512", header)
    assert "pmlp_mlp_forward_ppo_loss_parts_k0(int32_t M, int32_t A, int32_t K0);" in header
    lgs = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert "num_obs = H * F + P" in lgs
    assert "observation history and\n * height observations do not combine" in lgs
    assert "LGS_MAX_OBS_FRAMES * LGS_MAX_OBS + LGS_MAX_SCAN_OBS" in lgs
