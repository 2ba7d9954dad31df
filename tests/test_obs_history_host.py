"""Host side of the observation history: the numpy restatement of "shift, append,
fill after reset" that tests/test_gpu_obs_history.py holds the kernel to, the cfg switch
`env.history_length`, what it becomes (leggedsim/task.py obs_history_params -> lgs_obs_history),
the refusals, the `go2_robust_history` registration, the entry point's declaration / export /
mirror and the tiled noise vector.  No GPU."""
import copy
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from legged_gym.utils import task_registry
from leggedsim import cabi, native
from leggedsim.task import actuator_rand_params, build_task_params
from test_actuator_rand_host import EXISTING, SWITCHES
from test_height_obs_host import _spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------- restatement --
def stack_row(prev_row, frame, fresh, H):
    """The policy row of a control step under a history of H frames (include/leggedsim.h,
    lgs_obs_history).  prev_row [N, H * F]: the env's last row; frame [N, F]: the row the step
    writes without the feature; fresh [N] bool: the env reset since its last row was written (in
    this step's launch or between the steps).  Shift the older frames down, append the frame; a
    fresh env's row is its frame in every slot."""
    frame = np.asarray(frame)
    Fw = frame.shape[1]
    out = np.concatenate([np.asarray(prev_row)[:, Fw:], frame], axis=1)
    fresh = np.asarray(fresh, bool)
    out[fresh] = np.tile(frame[fresh], (1, H))
    return out


def test_restatement_agrees_with_hand_written_rows_across_a_reset():
    f = [np.array([[10 * t + 1, 10 * t + 2, 10 * t + 3]], F32) for t in range(5)]  # F = 3, one env
    # H = 2: first row fills; then [t-1 | t]; a reset at t = 3 fills again
    r = stack_row(np.zeros((1, 6), F32), f[0], [True], 2)
    np.testing.assert_array_equal(r, [[1, 2, 3, 1, 2, 3]])
    r = stack_row(r, f[1], [False], 2)
    np.testing.assert_array_equal(r, [[1, 2, 3, 11, 12, 13]])
    r = stack_row(r, f[2], [False], 2)
    np.testing.assert_array_equal(r, [[11, 12, 13, 21, 22, 23]])
    r = stack_row(r, f[3], [True], 2)
    np.testing.assert_array_equal(r, [[31, 32, 33, 31, 32, 33]])
    r = stack_row(r, f[4], [False], 2)
    np.testing.assert_array_equal(r, [[31, 32, 33, 41, 42, 43]])
    # H = 3, oldest first
    r = stack_row(np.full((1, 9), 7, F32), f[0], [True], 3)
    np.testing.assert_array_equal(r, [[1, 2, 3, 1, 2, 3, 1, 2, 3]])
    r = stack_row(r, f[1], [False], 3)
    np.testing.assert_array_equal(r, [[1, 2, 3, 1, 2, 3, 11, 12, 13]])
    r = stack_row(r, f[2], [False], 3)
    np.testing.assert_array_equal(r, [[1, 2, 3, 11, 12, 13, 21, 22, 23]])
    r = stack_row(r, f[3], [False], 3)
    np.testing.assert_array_equal(r, [[11, 12, 13, 21, 22, 23, 31, 32, 33]])
    r = stack_row(r, f[4], [True], 3)
    np.testing.assert_array_equal(r, [[41, 42, 43, 41, 42, 43, 41, 42, 43]])
    # two envs, one of them fresh: the other's history is untouched by it
    two = stack_row(np.array([[1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12]], F32),
                    np.array([[20, 21, 22], [30, 31, 32]], F32), [False, True], 2)
    np.testing.assert_array_equal(two, [[4, 5, 6, 20, 21, 22], [30, 31, 32, 30, 31, 32]])
    assert two.dtype == F32


# ------------------------------------------------------------------- cfg ----
def test_defaults_are_off():
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    assert LeggedRobotCfg.env.history_length == 1
    assert cabi.MAX_OBS_FRAMES == 8


@pytest.mark.parametrize("task,model", EXISTING + [("go2_robust", "go2")])
def test_every_existing_task_has_the_feature_off_and_no_tensors(task, model):
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from leggedsim.task import obs_history_params
    spec, cfg = _spec(task, model)
    assert cfg.env.history_length == 1
    R = obs_history_params(types.SimpleNamespace(cfg=cfg))
    assert (R.enabled, R.frames) == (0, 0) and not (R.history or R.fill)
    env = types.SimpleNamespace(cfg=cfg, num_obs=cfg.env.num_observations)  # (off: neither the device nor the sim)
    LeggedRobot._build_observation_history(env)
    assert env.obs_history is None and env._obs_history_fill is None
    assert env.num_obs_frame == cfg.env.num_observations


@pytest.mark.parametrize("task,model", [t for t in EXISTING if t[0] in ("go2", "go2_handstand", "h1", "h1_2", "g1",
                                                                       "g1_rough", "g1_terrain")])
def test_every_existing_tasks_task_params_are_the_golden_record(task, model):
    """lgs_task_params gained no field and no task's bytes moved (the record of the tree before the
    height observations, which every later feature has been held to)."""
    spec, _ = _spec(task, model)
    T = build_task_params(spec)
    want = np.load(os.path.join(ROOT, "tests", "golden", "task_params_before_height_obs.npz"))[task]
    got = np.frombuffer(bytes(T), dtype=np.uint8)
    assert got.size == want.size == C.sizeof(cabi.TaskParams)
    np.testing.assert_array_equal(got, want)


def _history(H, num_obs):
    def edit(cfg):
        cfg.env.history_length = H
        cfg.env.num_observations = num_obs
    return edit


def test_history_on_gives_the_descriptor_and_the_frame_width():
    from leggedsim.task import obs_history_params
    for task, model, Fw in (("go2", "go2", 48), ("g1", "g1_12dof", 47), ("go2_handstand", "go2", 46)):
        spec, _ = _spec(task, model, _history(5, 5 * Fw))
        R = obs_history_params(spec)
        assert (R.enabled, R.frames, R.num_frame) == (1, 5, Fw), task
        assert not (R.history or R.fill)  # the env's tensors, not the builder's
        T = build_task_params(spec)
        assert T.num_obs == 5 * Fw
        assert T.num_privileged_obs == (spec.num_privileged_obs or 0)  # the privileged row is untouched


@pytest.mark.parametrize("bad", [0, -1, 9, 2.5, True])
def test_a_history_length_outside_1_to_8_is_refused(bad):
    from leggedsim.task import obs_history_params
    spec, _ = _spec("go2", "go2", _history(bad, 48))
    with pytest.raises(ValueError, match="env.history_length must be"):
        obs_history_params(spec)


def test_num_observations_must_be_the_frames_times_the_head():
    from leggedsim.task import obs_history_params
    for num_obs in (48, 239, 241, 5 * 47):
        spec, _ = _spec("go2", "go2", _history(5, num_obs))
        with pytest.raises(ValueError, match=r"must be 5 x the layout's 48 = 240"):
            obs_history_params(spec)
    spec, _ = _spec("g1", "g1_12dof", _history(2, 96))
    with pytest.raises(ValueError, match=r"must be 2 x the layout's 47 = 94"):
        obs_history_params(spec)
    # H = 8, the bound itself: 384 entries
    spec, _ = _spec("go2", "go2", _history(8, 384))
    assert obs_history_params(spec).frames == 8


def test_the_height_scan_in_the_rows_and_a_history_do_not_combine():
    from leggedsim.task import obs_history_params

    def edit(cfg):
        cfg.env.history_length = 2
        cfg.env.num_observations = 96
    spec, cfg = _spec("go2_terrain", "go2")
    assert cfg.terrain.scan_in_observations
    cfg.env.history_length, cfg.env.num_observations = 2, 96
    with pytest.raises(ValueError, match="do not combine"):
        obs_history_params(spec)


def test_a_python_compute_observations_is_refused():
    from leggedsim.task import obs_history_params
    spec, _ = _spec("go2", "go2", _history(5, 240))
    spec._hooks = frozenset({"compute_observations"})
    with pytest.raises(ValueError, match="compute_observations"):
        obs_history_params(spec)
    spec._hooks = frozenset({"check_termination"})  # the other hooks edit no row
    assert obs_history_params(spec).enabled == 1


def test_go2_robust_history_is_registered_with_240_inputs_and_the_four_switches_on():
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from legged_gym.envs.go2.go2_config import GO2RobustCfg, GO2RobustCfgPPO
    from leggedsim.task import obs_history_params
    assert task_registry.get_task_class("go2_robust_history") is LeggedRobot  # no Python step method of its own
    env_cfg, train_cfg = task_registry.get_cfgs("go2_robust_history")
    assert isinstance(env_cfg, GO2RobustCfg) and isinstance(train_cfg, GO2RobustCfgPPO)
    assert train_cfg.runner.experiment_name == "go2_robust_history"
    assert train_cfg.policy.actor_hidden_dims == [512, 256, 128] and not hasattr(train_cfg.policy, "rnn_type")
    assert (env_cfg.env.history_length, env_cfg.env.num_observations) == (5, 240)
    assert not env_cfg.env.num_privileged_obs  # the critic reads the same 240-wide row
    assert all(getattr(env_cfg.domain_rand, s) for s in SWITCHES)
    assert actuator_rand_params(types.SimpleNamespace(cfg=env_cfg)).enabled == 1
    spec, _ = _spec("go2_robust_history", "go2")
    R = obs_history_params(spec)
    assert (R.enabled, R.frames, R.num_frame) == (1, 5, 48)
    # go2_robust is left alone
    robust, robust_train = task_registry.get_cfgs("go2_robust")
    assert (robust.env.history_length, robust.env.num_observations) == (1, 48)
    assert robust_train.runner.experiment_name == "go2_robust"


# ----------------------------------------------------------------- noise ----
def test_the_noise_vector_is_the_head_tiled_and_task_params_keep_the_head():
    for task, model, Fw in (("go2", "go2", 48), ("g1", "g1_12dof", 47), ("go2_handstand", "go2", 46)):
        off, _ = _spec(task, model)
        head = np.asarray(off.noise_scale_vec, F32)
        assert head.shape == (Fw,) and head.any()
        spec, _ = _spec(task, model, _history(3, 3 * Fw))
        v = np.asarray(spec.noise_scale_vec, F32)
        np.testing.assert_array_equal(v, np.tile(head, 3))
        T = build_task_params(spec)
        np.testing.assert_array_equal(np.array(T.noise_vec[:Fw], F32), head)
        assert not any(T.noise_vec[Fw:])
        # everything but num_obs is the task without the history, byte for byte
        T0 = build_task_params(off)
        T0.num_obs = T.num_obs
        assert bytes(T0) == bytes(T), task


def test_a_noise_override_that_is_not_the_tiling_is_refused():
    spec, _ = _spec("go2", "go2", _history(3, 144))
    v = np.asarray(spec.noise_scale_vec, F32).copy()
    v[48 + 5] *= 2  # an older frame with a scale of its own: the kernel never re-noises it
    spec.noise_scale_vec = v
    with pytest.raises(ValueError, match="tiled 3 times"):
        build_task_params(spec)
    spec.noise_scale_vec = v[:100]
    with pytest.raises(ValueError, match="tiled 3 times"):
        build_task_params(spec)


# ------------------------------------------------------------------- ABI ----
def test_the_entry_point_is_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert re.search(r"LGS_API int lgs_set_observation_history\(lgs_sim\* sim, const lgs_obs_history\* desc\);", header)
    assert "#define LGS_MAX_OBS_FRAMES 8" in header
    m = re.search(r"typedef struct lgs_obs_history \{(.*?)\} lgs_obs_history;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for stmt in body.split(";"):
        d = re.match(r"\s*(int32_t|float)(\*?)\s+(\w+)\s*$", stmt.strip())
        if not d:
            assert not stmt.strip(), stmt
            continue
        fields.append((d.group(3), C.c_void_p if d.group(2) else {"int32_t": C.c_int32, "float": C.c_float}[d.group(1)]))
    mirror = list(cabi.ObsHistory._fields_)
    assert fields == mirror
    assert [n for n, _ in mirror] == ["enabled", "frames", "history", "fill"]
    assert C.sizeof(cabi.ObsHistory) == 24
    assert [getattr(cabi.ObsHistory, n).offset for n, _ in mirror] == [0, 4, 8, 16]
    assert "lgs_set_observation_history" in native.EXPORTED_SYMBOLS
    import torch  # noqa: F401  (the HIP runtime before the library)
    lib = native.load()
    assert hasattr(lib, "lgs_set_observation_history")
    assert lib.lgs_set_observation_history.restype is C.c_int
    # a NULL sim, with or without a descriptor, is a status and an error text, not a crash
    assert lib.lgs_set_observation_history(None, None) == -1 and b"null" in lib.lgs_last_error()
    R = cabi.ObsHistory()
    assert lib.lgs_set_observation_history(None, C.byref(R)) == -1 and lib.lgs_last_error()


def test_the_pinned_structs_and_ids_are_untouched():
    header = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert C.sizeof(cabi.TaskParams) == 2632
    assert [n for n, _ in cabi.TaskParams._fields_][-1] == "ground_relative_heights"
    assert [n for n, _ in cabi.EnvBuffers._fields_][-2:] == ["terrain_level_sum", "measured_heights"]
    assert [n for n, _ in cabi.ActuatorRand._fields_][-1] == "delay" and C.sizeof(cabi.ActuatorRand) == 72
    assert [n for n, _ in cabi.HeightObs._fields_][-1] == "noise_scale" and C.sizeof(cabi.HeightObs) == 20
    assert cabi.MAX_REWARDS == 24 and cabi.MAX_OBS == 128
    ids = re.search(r"enum lgs_reward_id \{(.*?)LGS_REW_COUNT", header, re.S).group(1)
    ids = re.sub(r"/\*.*?\*/", "", ids, flags=re.S)
    assert len([x for x in ids.split(",") if x.strip()]) == 34  # LGS_REW_COUNT
    assert len(cabi.REWARD_ID) == 34
