"""Host side of the actuator randomisation and action latency: the cfg switches under
`domain_rand`, what they become (leggedsim/task.py actuator_rand_params -> lgs_actuator_rand), the
refusals, the `go2_robust` registration, the entry point's declaration / export / mirror, and the
numpy fp32 restatements of the PD law and of the reset draws that tests/test_gpu_actuator_rand.py
holds the kernel to.  No GPU."""
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
from leggedsim.task import actuator_rand_params
from test_height_obs_host import _spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EXISTING = [("go2", "go2"), ("go2_terrain", "go2"), ("go2_handstand", "go2"), ("h1", "h1"), ("h1_2", "h1_2_12dof"),
            ("g1", "g1_12dof"), ("g1_rough", "g1_12dof"), ("g1_terrain", "g1_12dof"), ("g1_terrain_scan", "g1_12dof")]
SWITCHES = ("randomize_kp", "randomize_kd", "randomize_motor_strength", "randomize_action_delay")


# ------------------------------------------------------------ restatements --
# include/leggedsim.h (lgs_actuator_rand), operation by operation in numpy float32: every
# elementwise numpy op rounds once to fp32, like the kernel's uncontracted arithmetic.
def actuator_gains(T, D, kp_scale, kd_scale, strength):
    """(kp, kd) [N, D] of a control step: (gain * scale) * strength."""
    pg, dg = np.array(T.p_gains[:D], F), np.array(T.d_gains[:D], F)
    return (pg[None, :] * kp_scale.astype(F)) * strength.astype(F), (dg[None, :] * kd_scale.astype(F)) * strength.astype(F)


def actuator_torques(T, D, kp, kd, strength, delay, it, a_prev, a, q, qd, last_qd, sim_dt):
    """Substep `it`'s joint torques: (tau after the effort clip, t before it), each [N, D]."""
    a_used = np.where((it < np.asarray(delay))[:, None], a_prev.astype(F), a.astype(F))
    as_ = a_used * F(T.action_scale)
    lim = np.array(T.torque_limits[:D], F)[None, :]
    if T.control_type == 0:
        tg = as_ + np.array(T.default_dof_pos[:D], F)[None, :]
        if T.clamp_pd_targets:
            tg = np.minimum(np.maximum(tg, np.array(T.pd_target_lower[:D], F)), np.array(T.pd_target_upper[:D], F))
        t = kp * (tg - q) - kd * qd
    elif T.control_type == 1:
        t = kp * (as_ - qd) - kd * (qd - last_qd) / F(sim_dt)
    else:
        t = as_ * strength.astype(F)
    t = t.astype(F)
    return np.minimum(np.maximum(t, -lim), lim).astype(F), t


def rand_range(lo, hi, u):
    """The kernel's rand_range: (hi - lo) * u + lo in fp32."""
    return (F(hi) - F(lo)) * F(u) + F(lo)


def actuator_draws(uniform, R, D, e, step):
    """A resetting env's rows: (kp_scale [D], kd_scale [D], strength [D], delay).  `uniform(e, step,
    stream, index)` is the step's counter-based draw (lgs_uniform with the task's seed); R the
    lgs_actuator_rand."""
    u = lambda k: F(uniform(e, step, cabi.STREAM_ACTUATOR, k))  # noqa: E731
    kp = np.array([rand_range(R.kp_range[0], R.kp_range[1], u(j)) for j in range(D)], F)
    kd = np.array([rand_range(R.kd_range[0], R.kd_range[1], u(cabi.MAX_DOFS + j)) for j in range(D)], F)
    st = np.array([rand_range(R.strength_range[0], R.strength_range[1], u(2 * cabi.MAX_DOFS + j)) for j in range(D)], F)
    n = R.delay_range[1] - R.delay_range[0] + 1
    delay = R.delay_range[0] + min(int(u(3 * cabi.MAX_DOFS) * F(n)), n - 1)
    return kp, kd, st, delay


def _task(control_type, **kw):
    T = cabi.TaskParams()
    T.control_type, T.action_scale = control_type, 0.25
    T.p_gains[:2] = [20.0, 40.0]
    T.d_gains[:2] = [0.5, 1.0]
    T.default_dof_pos[:2] = [0.125, -1.5]
    T.torque_limits[:2] = [23.7, 45.0]
    for k, v in kw.items():
        setattr(T, k, v)
    return T


def test_restated_gains_and_p_law_agree_with_hand_computed_values():
    T = _task(0)
    ks, ds, st = (np.array([[1.25, 0.5]], F), np.array([[0.5, 2.0]], F), np.array([[2.0, 0.75]], F))
    kp, kd = actuator_gains(T, 2, ks, ds, st)
    np.testing.assert_array_equal(kp, np.array([[50.0, 15.0]], F))   # (20 * 1.25) * 2, (40 * 0.5) * 0.75
    np.testing.assert_array_equal(kd, np.array([[0.5, 1.5]], F))     # (0.5 * 0.5) * 2, (1 * 2) * 0.75
    a, a_prev = np.array([[2.0, -4.0]], F), np.array([[0.0, 4.0]], F)
    q, qd = np.array([[0.375, -2.0]], F), np.array([[1.0, -2.0]], F)
    # no delay: as = (0.5, -1); tg = (0.625, -2.5); t = 50 * 0.25 - 0.5 * 1 = 12, 15 * -0.5 - 1.5 * -2 = -4.5
    tau, raw = actuator_torques(T, 2, kp, kd, st, [0], 0, a_prev, a, q, qd, qd, 0.005)
    np.testing.assert_array_equal(raw, np.array([[12.0, -4.5]], F))
    np.testing.assert_array_equal(tau, raw)
    # substep 0 of a delay of 1 uses a_prev: as = (0, 1); tg = (0.125, -0.5); t = 50 * -0.25 - 0.5 = -13, 15 * 1.5 + 3 = 25.5
    tau, raw = actuator_torques(T, 2, kp, kd, st, [1], 0, a_prev, a, q, qd, qd, 0.005)
    np.testing.assert_array_equal(raw, np.array([[-13.0, 25.5]], F))
    # substep 1 of the same delay is back on a
    _, raw1 = actuator_torques(T, 2, kp, kd, st, [1], 1, a_prev, a, q, qd, qd, 0.005)
    np.testing.assert_array_equal(raw1, np.array([[12.0, -4.5]], F))
    # the effort clip: 8x the gains -> t = (96, -36), limits (23.7, 45)
    tau, raw = actuator_torques(T, 2, kp * F(8), kd * F(8), st, [0], 0, a_prev, a, q, qd, qd, 0.005)
    np.testing.assert_array_equal(raw, np.array([[96.0, -36.0]], F))
    np.testing.assert_array_equal(tau, np.array([[F(23.7), -36.0]], F))


def test_restated_clamped_target_v_and_t_laws_agree_with_hand_computed_values():
    kp, kd, st = np.array([[50.0, 15.0]], F), np.array([[0.5, 1.5]], F), np.array([[2.0, 0.75]], F)
    a, z = np.array([[2.0, -4.0]], F), np.zeros((1, 2), F)
    q, qd, lqd = np.array([[0.375, -2.0]], F), np.array([[1.0, -2.0]], F), np.array([[0.5, -1.0]], F)
    T = _task(0, clamp_pd_targets=1)
    T.pd_target_lower[:2] = [0.0, -2.0]
    T.pd_target_upper[:2] = [0.5, 2.0]
    # tg = clip((0.625, -2.5)) = (0.5, -2): t = 50 * 0.125 - 0.5, 15 * 0 + 3
    _, raw = actuator_torques(T, 2, kp, kd, st, [0], 0, z, a, q, qd, lqd, 0.005)
    np.testing.assert_array_equal(raw, np.array([[5.75, 3.0]], F))
    # V: kp * (as - qd) - kd * (qd - lqd) / dt, dt = 0.5: 50 * -0.5 - 0.5 * 0.5 / 0.5 = -25.5, 15 * 1 - 1.5 * -1 / 0.5 = 18
    _, raw = actuator_torques(_task(1), 2, kp, kd, st, [0], 0, z, a, q, qd, lqd, 0.5)
    np.testing.assert_array_equal(raw, np.array([[-25.5, 18.0]], F))
    # T: as * strength = 0.5 * 2, -1 * 0.75
    tau, raw = actuator_torques(_task(2), 2, kp, kd, st, [0], 0, z, a, q, qd, lqd, 0.005)
    np.testing.assert_array_equal(raw, np.array([[1.0, -0.75]], F))
    np.testing.assert_array_equal(tau, raw)


def test_restated_draws_follow_the_stream_layout_and_a_unit_range_draws_exactly_one():
    asked = []
    table = {0: 0.5, 1: 0.25, cabi.MAX_DOFS: 0.75, cabi.MAX_DOFS + 1: 0.0, 2 * cabi.MAX_DOFS: 1.0 - 2.0 ** -24,
             2 * cabi.MAX_DOFS + 1: 0.5, 3 * cabi.MAX_DOFS: 0.999}

    def uniform(e, step, stream, index):
        asked.append((e, step, stream, index))
        return table[index]

    R = cabi.ActuatorRand()
    R.kp_range[:], R.kd_range[:], R.strength_range[:], R.delay_range[:] = (0.5, 1.5), (1.0, 1.0), (0.0, 2.0), (1, 3)
    kp, kd, st, delay = actuator_draws(uniform, R, 2, 5, 77)
    np.testing.assert_array_equal(kp, np.array([1.0, 0.75], F))
    np.testing.assert_array_equal(kd, np.array([1.0, 1.0], F))          # [1, 1]: exactly 1.0f whatever u
    np.testing.assert_array_equal(st, np.array([F(2.0) * F(1.0 - 2.0 ** -24), 1.0], F))
    assert delay == 3                                                   # 1 + min(int(0.999 * 3), 2)
    assert all(a[:3] == (5, 77, 7) for a in asked) and cabi.STREAM_ACTUATOR == 7
    assert [a[3] for a in asked] == [0, 1, 26, 27, 52, 53, 78]
    table[3 * cabi.MAX_DOFS] = 0.34
    assert actuator_draws(uniform, R, 2, 5, 77)[3] == 2                 # 1 + int(1.02)
    R.delay_range[:] = (2, 2)
    assert actuator_draws(uniform, R, 2, 5, 77)[3] == 2


# ------------------------------------------------------------------- cfg ----
def test_defaults_are_off():
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    dr = LeggedRobotCfg.domain_rand
    assert not any(getattr(dr, s) for s in SWITCHES)
    assert dr.kp_range == [0.9, 1.1] and dr.kd_range == [0.9, 1.1] and dr.motor_strength_range == [0.9, 1.1]
    assert dr.action_delay_range == [0, 2] and dr.actuator_resample_on_reset is True


@pytest.mark.parametrize("task,model", EXISTING)
def test_every_existing_task_has_the_feature_off_and_no_tensors(task, model):
    from legged_gym.envs.base.legged_robot import LeggedRobot
    spec, cfg = _spec(task, model)
    R = actuator_rand_params(types.SimpleNamespace(cfg=cfg))
    assert (R.enabled, R.resample_on_reset) == (0, 0)
    assert list(R.kp_range) == list(R.kd_range) == list(R.strength_range) == [1.0, 1.0] and list(R.delay_range) == [0, 0]
    assert not (R.kp_scale or R.kd_scale or R.strength or R.delay)
    env = types.SimpleNamespace(cfg=cfg)  # (off: the method touches neither the device nor the sim)
    LeggedRobot._build_actuator_randomization(env)
    assert env.actuator_rand.enabled == 0
    assert env.kp_factors is None and env.kd_factors is None and env.motor_strengths is None
    assert env.action_delay_substeps is None


def _cfg(task="go2", **dr):
    cfg = copy.deepcopy(task_registry.get_cfgs(task)[0])
    for k, v in dr.items():
        setattr(cfg.domain_rand, k, v)
    return types.SimpleNamespace(cfg=cfg)


def test_each_group_passes_its_range_and_the_others_the_neutral_one():
    R = actuator_rand_params(_cfg(randomize_kp=True, kp_range=[0.8, 1.3]))
    assert (R.enabled, R.resample_on_reset) == (1, 1)
    assert list(R.kp_range) == [F(0.8), F(1.3)] and list(R.kd_range) == list(R.strength_range) == [1.0, 1.0]
    assert list(R.delay_range) == [0, 0]
    R = actuator_rand_params(_cfg(randomize_kd=True, randomize_motor_strength=True, kd_range=[0.5, 0.5],
                                  actuator_resample_on_reset=False))
    assert (R.enabled, R.resample_on_reset) == (1, 0)
    assert list(R.kp_range) == [1.0, 1.0] and list(R.kd_range) == [0.5, 0.5] and list(R.strength_range) == [F(0.9), F(1.1)]
    R = actuator_rand_params(_cfg(randomize_action_delay=True, action_delay_range=[1, 4]))  # go2: decimation 4
    assert R.enabled == 1 and list(R.delay_range) == [1, 4] and list(R.kp_range) == [1.0, 1.0]
    # a range of a group that is off is not read
    assert actuator_rand_params(_cfg(kp_range=[3, 1], action_delay_range=[9, 1])).enabled == 0


@pytest.mark.parametrize("switch,name", [("randomize_kp", "kp_range"), ("randomize_kd", "kd_range"),
                                         ("randomize_motor_strength", "motor_strength_range")])
@pytest.mark.parametrize("bad", [[1.1, 0.9], [-0.1, 1.0], [0.9, float("inf")], [float("nan"), 1.0], [1.0]])
def test_a_bad_factor_range_is_refused(switch, name, bad):
    with pytest.raises(ValueError, match=f"domain_rand.{name} must be"):
        actuator_rand_params(_cfg(**{switch: True, name: bad}))


@pytest.mark.parametrize("bad", [[-1, 2], [3, 2], [0, 5], [5, 5], [0.5, 2], [0]])
def test_an_action_delay_outside_the_decimation_loop_is_refused(bad):
    with pytest.raises(ValueError, match=r"0 <= lo <= hi <= control.decimation = 4"):
        actuator_rand_params(_cfg(randomize_action_delay=True, action_delay_range=bad))
    R = actuator_rand_params(_cfg(randomize_action_delay=True, action_delay_range=[4, 4]))  # the bound itself
    assert R.enabled == 1 and list(R.delay_range) == [4, 4]


def test_go2_robust_is_registered_with_the_four_switches_on():
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from legged_gym.envs.go2.go2_config import GO2RobustCfg, GO2RoughCfg, GO2RoughCfgPPO
    assert task_registry.get_task_class("go2_robust") is LeggedRobot  # no Python step method of its own
    env_cfg, train_cfg = task_registry.get_cfgs("go2_robust")
    assert isinstance(env_cfg, GO2RobustCfg) and isinstance(env_cfg, GO2RoughCfg)
    assert isinstance(train_cfg, GO2RoughCfgPPO) and train_cfg.runner.experiment_name == "go2_robust"
    assert all(getattr(env_cfg.domain_rand, s) for s in SWITCHES)
    R = actuator_rand_params(types.SimpleNamespace(cfg=env_cfg))
    assert (R.enabled, R.resample_on_reset) == (1, 1)
    assert list(R.kp_range) == list(R.kd_range) == list(R.strength_range) == [F(0.9), F(1.1)]
    assert list(R.delay_range) == [0, 2] and env_cfg.control.decimation == 4
    assert env_cfg.env.num_observations == 48
    # the plain go2 task is left alone
    go2, go2_train = task_registry.get_cfgs("go2")
    assert not any(getattr(go2.domain_rand, s) for s in SWITCHES) and go2_train.runner.experiment_name == "rough_go2"


# ------------------------------------------------------------------- ABI ----
def test_the_entry_point_is_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert re.search(r"LGS_API int lgs_set_actuator_randomization\(lgs_sim\* sim, const lgs_actuator_rand\* desc\);",
                     header)
    assert "#define LGS_STREAM_ACTUATOR 7u" in header and cabi.STREAM_ACTUATOR == 7
    m = re.search(r"typedef struct lgs_actuator_rand \{(.*?)\} lgs_actuator_rand;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    fields = []
    for stmt in body.split(";"):
        d = re.match(r"\s*(int32_t|float)(\*?)\s+(.*)$", stmt.strip(), re.S)
        if not d:
            assert not stmt.strip(), stmt
            continue
        for name in d.group(3).split(","):
            arr = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            t = C.c_void_p if d.group(2) else ctype[d.group(1)]
            fields.append((arr.group(1), t * int(arr.group(2)) if arr.group(2) else t))
    mirror = list(cabi.ActuatorRand._fields_)
    assert [n for n, _ in fields] == [n for n, _ in mirror] == [
        "enabled", "resample_on_reset", "kp_range", "kd_range", "strength_range", "delay_range", "kp_scale",
        "kd_scale", "strength", "delay"]
    for (n, a), (_, b) in zip(fields, mirror):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0), n
        assert getattr(a, "_type_", a) == getattr(b, "_type_", b), n
    assert C.sizeof(cabi.ActuatorRand) == 8 + 6 * 4 + 2 * 4 + 4 * 8
    assert "lgs_set_actuator_randomization" in native.EXPORTED_SYMBOLS
    import torch  # noqa: F401  (the HIP runtime before the library)
    lib = native.load()
    assert hasattr(lib, "lgs_set_actuator_randomization")
    assert lib.lgs_set_actuator_randomization.restype is C.c_int
    # a NULL sim, with or without a descriptor, is a status and an error text, not a crash
    assert lib.lgs_set_actuator_randomization(None, None) == -1 and b"null" in lib.lgs_last_error()
    R = cabi.ActuatorRand()
    assert lib.lgs_set_actuator_randomization(None, C.byref(R)) == -1 and lib.lgs_last_error()


def test_the_pinned_structs_and_ids_are_untouched():
    assert C.sizeof(cabi.TaskParams) == 2632
    assert [n for n, _ in cabi.EnvBuffers._fields_][-2:] == ["terrain_level_sum", "measured_heights"]
    assert cabi.MAX_REWARDS == 24
