"""Host side of the asymmetric critic's privileged row: the cfg switch
`env.privileged_parameters`, what it becomes (leggedsim/task.py priv_params -> lgs_priv_params), the
widths per layout, the refusals and their numbers, the two registered tasks, the entry point's
declaration / export / mirror, the padded first-layer widths of an actor and a critic of different
widths, and the numpy fp32 restatement of the parameter tail that tests/test_gpu_priv_params.py
holds the kernel to.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from legged_gym.utils import task_registry
from leggedsim import cabi, native
from leggedsim.task import actuator_rand_params, build_task_params, priv_params
from rsl_rl.modules import mfma_mlp as mm
from test_height_obs_host import _spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ACT = ("randomize_kp", "randomize_kd", "randomize_motor_strength", "randomize_action_delay")


# ------------------------------------------------------------- restatement --
# include/leggedsim.h (lgs_priv_params), operation by operation in numpy float32: every elementwise
# numpy op rounds once to fp32, like the kernel's uncontracted arithmetic.
def priv_tail(R, clip, friction, added_mass, kp=None, kd=None, strength=None, delay=None):
    """The parameter tail [N, Wp] of envs with these rows: friction, added mass and, with the
    actuator rows, kp [N, D], kd, strength and the delay [N]; each clip((v - offset) * scale, +-clip)
    with its group's {offset, scale} of the lgs_priv_params R."""
    c = F(clip)

    def entry(v, group):
        v = np.asarray(v, F)
        v = v.reshape(len(v), -1)
        return np.minimum(np.maximum((v - F(group[0])) * F(group[1]), -c), c).astype(F)

    cols = [entry(friction, R.friction), entry(added_mass, R.added_mass)]
    if kp is not None:
        cols += [entry(kp, R.kp), entry(kd, R.kd), entry(strength, R.strength),
                 entry(np.asarray(delay).astype(F), R.delay)]
    return np.concatenate(cols, axis=1)


def test_restated_tail_agrees_with_hand_computed_values():
    R = cabi.PrivParams()
    R.friction[:], R.added_mass[:] = (0.75, 2.0), (1.0, 0.5)
    R.kp[:], R.kd[:], R.strength[:], R.delay[:] = (1.0, 8.0), (1.0, 4.0), (0.5, 2.0), (1.0, 1.0)
    fr, ms = np.array([1.0, 0.25], F), np.array([3.0, -1.0], F)
    t = priv_tail(R, 100.0, fr, ms)
    np.testing.assert_array_equal(t, np.array([[0.5, 1.0], [-1.0, -1.0]], F))
    kp = np.array([[1.125, 0.875], [1.0, 1.25]], F)
    kd = np.array([[0.75, 1.0], [1.25, 1.5]], F)
    st = np.array([[0.5, 1.0], [0.25, 0.0]], F)
    t = priv_tail(R, 1.5, fr, ms, kp, kd, st, np.array([2, 0], np.int32))
    assert t.shape == (2, 2 + 3 * 2 + 1) and t.dtype == F
    #                      fr    mass  kp          kd          strength     delay
    want = np.array([[0.5, 1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 1.0, 1.0],
                     [-1.0, -1.0, 0.0, 1.5, 1.0, 1.5, -0.5, -1.0, -1.0]], F)   # kp 2.0 and kd 2.0 meet the clip 1.5
    np.testing.assert_array_equal(t, want)
    # one rounding per operation: (v - offset) rounds before the product
    R.friction[:] = (0.1, 3.0)
    v = np.array([0.3], F)
    assert priv_tail(R, 100.0, v, np.zeros(1, F))[0, 0] == F(F(v[0] - F(0.1)) * F(3.0))


# ------------------------------------------------------------------- cfg ----
def _env(task, model, **edits):
    def edit(cfg):
        for k, v in edits.items():
            sec, attr = k.split("__")
            setattr(getattr(cfg, sec), attr, v)
    return _spec(task, model, edit)[0]


def test_the_default_is_off_and_every_other_task_has_no_tail():
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg
    assert LeggedRobotCfg.env.privileged_parameters is False
    for task, model in (("go2", "go2"), ("go2_robust_history", "go2"), ("go2_terrain_robust", "go2"),
                        ("go2_handstand", "go2"), ("h1", "h1"), ("g1", "g1_12dof"), ("g1_terrain_scan", "g1_12dof")):
        R = priv_params(_env(task, model))
        assert (R.enabled, R.num_tail, R.num_priv) == (0, 0, 0), task
        assert not any(list(getattr(R, g)) != [0.0, 0.0] for g in cabi.PRIV_GROUPS)


def test_offsets_and_scales_of_randomised_and_fixed_groups():
    env = _env("go2_robust_asym", "go2", domain_rand__randomize_friction=True, domain_rand__friction_range=[0.1, 1.25],
               domain_rand__randomize_base_mass=False, domain_rand__kp_range=[0.8, 1.3],
               domain_rand__randomize_kd=False, domain_rand__action_delay_range=[1, 3])
    R = priv_params(env)
    assert (R.enabled, R.num_head, R.num_tail, R.num_priv) == (1, 48, 39, 87)
    assert list(R.friction) == [F((0.1 + 1.25) / 2), F(2 / (1.25 - 0.1))]     # randomised: onto [-1, 1]
    assert list(R.added_mass) == [0.0, 1.0]                                     # fixed at 0: offset 0, scale 1
    # (the actuator ranges are the fp32 ones actuator_rand_params resolved; the arithmetic on them is double)
    lo, hi = float(F(0.8)), float(F(1.3))
    assert list(R.kp) == [F((lo + hi) / 2), F(2 / (hi - lo))]
    assert list(R.kd) == [1.0, 1.0]                                             # the group is off: [1, 1] -> 0
    lo, hi = float(F(0.9)), float(F(1.1))
    assert list(R.strength) == [F((lo + hi) / 2), F(2 / (hi - lo))]
    assert list(R.delay) == [2.0, 1.0]
    # a randomised parameter lands in [-1, 1]: the range's ends
    t = priv_tail(R, 100.0, np.array([0.1, 1.25], F), np.zeros(2, F))
    np.testing.assert_allclose(t[:, 0], [-1.0, 1.0], rtol=0, atol=2e-7)
    # friction off: the terrain's static friction, a fixed group
    env = _env("go2_robust_asym", "go2", domain_rand__randomize_friction=False, terrain__static_friction=0.75,
               domain_rand__randomize_base_mass=True, domain_rand__added_mass_range=[-1.0, 3.0])
    R = priv_params(env)
    assert list(R.friction) == [0.75, 1.0] and list(R.added_mass) == [1.0, 0.5]


def test_widths_per_layout_and_width_stability_under_the_play_switches():
    assert priv_params(_env("go2_robust_asym", "go2")).num_priv == 87
    assert priv_params(_env("go2_terrain_robust_asym", "go2")).num_priv == 274
    # no actuator group: friction and mass alone
    R = priv_params(_env("go2", "go2", env__privileged_parameters=True, env__num_privileged_obs=50))
    assert (R.enabled, R.num_tail, R.num_priv) == (1, 2, 50)
    on = {"domain_rand__" + s: True for s in ACT}
    for task, model, head, D in (("h1", "h1", 44, 10), ("g1", "g1_12dof", 50, 12)):
        R = priv_params(_env(task, model, env__privileged_parameters=True, env__num_privileged_obs=head + 2))
        assert (R.num_head, R.num_tail, R.num_priv) == (head, 2, head + 2)
        Wp = 2 + 3 * D + 1
        R = priv_params(_env(task, model, env__privileged_parameters=True, env__num_privileged_obs=head + Wp, **on))
        assert (R.num_tail, R.num_priv) == (Wp, head + Wp) and head + Wp in (77, 89)
    R = priv_params(_env("g1_terrain_scan", "g1_12dof", env__privileged_parameters=True,
                         env__num_privileged_obs=50 + 2 + 187))
    assert (R.num_head, R.num_tail, R.num_priv) == (50, 2, 239)
    # what play.py flips moves no width
    for task, n in (("go2_robust_asym", 87), ("go2_terrain_robust_asym", 274)):
        env = _env(task, "go2", domain_rand__randomize_friction=False, domain_rand__push_robots=False,
                   noise__add_noise=False)
        R = priv_params(env)
        assert R.num_priv == n and list(R.friction) == [F(env.cfg.terrain.static_friction), 1.0]
        assert build_task_params(env).num_privileged_obs == n


def test_python_refusals_name_the_width_the_row_would_have():
    with pytest.raises(ValueError, match=r"num_privileged_obs must be 48 \+ 39 parameters \+ 0 scan points = 87, not 88"):
        priv_params(_env("go2_robust_asym", "go2", env__num_privileged_obs=88))
    with pytest.raises(ValueError, match=r"48 \+ 39 parameters \+ 187 scan points = 274, not 87"):
        priv_params(_env("go2_terrain_robust_asym", "go2", env__num_privileged_obs=87))
    with pytest.raises(ValueError, match=r"must be 48 \+ 2 parameters \+ 0 scan points = 50, not None"):
        priv_params(_env("go2", "go2", env__privileged_parameters=True))
    with pytest.raises(ValueError, match=r"must be 44 \+ 2 parameters \+ 0 scan points = 46, not 44"):
        priv_params(_env("h1", "h1", env__privileged_parameters=True))
    with pytest.raises(ValueError, match="quadruped or the humanoid observation layout"):
        priv_params(_env("go2_handstand", "go2", env__privileged_parameters=True))
    # the 23-DOF G1 with the actuator group: 83 + 72 does not fit
    from test_gpu_parity import _register_g1_23dof
    _register_g1_23dof()
    on = {"domain_rand__" + s: True for s in ACT}
    with pytest.raises(ValueError, match=r"head \(83\) \+ the parameter tail \(72\) = 155 exceed the 128"):
        priv_params(_env("g1_23dof", "g1_23dof", env__privileged_parameters=True, env__num_privileged_obs=155, **on))
    R = priv_params(_env("g1_23dof", "g1_23dof", env__privileged_parameters=True, env__num_privileged_obs=85))
    assert (R.num_head, R.num_tail) == (83, 2)
    with pytest.raises(ValueError, match="the friction range must be finite"):
        priv_params(_env("go2_robust_asym", "go2", domain_rand__friction_range=[0.5, float("inf")]))


def test_both_tasks_are_registered_with_87_and_274():
    from legged_gym.envs.base.legged_robot import LeggedRobot
    from legged_gym.envs.go2.go2_config import (GO2RobustAsymCfg, GO2RobustHistoryCfg, GO2TerrainRobustAsymCfg,
                                                GO2TerrainRobustCfg)
    for task, base, cls, O, P in (("go2_robust_asym", GO2RobustHistoryCfg, GO2RobustAsymCfg, 240, 87),
                                  ("go2_terrain_robust_asym", GO2TerrainRobustCfg, GO2TerrainRobustAsymCfg, 427, 274)):
        assert task_registry.get_task_class(task) is LeggedRobot
        env_cfg, train_cfg = task_registry.get_cfgs(task)
        assert isinstance(env_cfg, cls) and isinstance(env_cfg, base) and train_cfg.runner.experiment_name == task
        assert env_cfg.env.privileged_parameters is True
        assert (env_cfg.env.num_observations, env_cfg.env.num_privileged_obs, env_cfg.env.history_length) == (O, P, 5)
        assert actuator_rand_params(_env(task, "go2")).enabled == 1
        T = build_task_params(_env(task, "go2"))
        assert (T.num_obs, T.num_privileged_obs, T.obs_layout) == (O, P, cabi.OBS_QUADRUPED)
    # the tasks they extend are left alone
    for task in ("go2_robust_history", "go2_terrain_robust"):
        c = task_registry.get_cfgs(task)[0]
        assert not c.env.privileged_parameters and not c.env.num_privileged_obs


# ------------------------------------------------------------------- ABI ----
def test_the_entry_point_is_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "leggedsim.h")).read()
    assert re.search(r"LGS_API int lgs_set_privileged_parameters\(lgs_sim\* sim, const lgs_priv_params\* desc\);", header)
    m = re.search(r"typedef struct lgs_priv_params \{(.*?)\} lgs_priv_params;", header, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    fields = []
    for stmt in body.split(";"):
        d = re.match(r"\s*(int32_t|float)\s+(.*)$", stmt.strip(), re.S)
        if not d:
            assert not stmt.strip(), stmt
            continue
        for name in d.group(2).split(","):
            arr = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            t = ctype[d.group(1)]
            fields.append((arr.group(1), t * int(arr.group(2)) if arr.group(2) else t))
    mirror = list(cabi.PrivParams._fields_)
    assert [n for n, _ in fields] == [n for n, _ in mirror] == ["enabled"] + list(cabi.PRIV_GROUPS)
    assert cabi.PRIV_GROUPS == ("friction", "added_mass", "kp", "kd", "strength", "delay")
    for (n, a), (_, b) in zip(fields, mirror):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0), n
        assert getattr(a, "_type_", a) == getattr(b, "_type_", b), n
    assert C.sizeof(cabi.PrivParams) == 4 + 6 * 2 * 4
    assert "lgs_set_privileged_parameters" in native.EXPORTED_SYMBOLS
    assert "has no history in any layout" in header and "the quadruped has none, so its" not in header
    import torch  # noqa: F401  (the HIP runtime before the library)
    lib = native.load()
    assert hasattr(lib, "lgs_set_privileged_parameters") and lib.lgs_set_privileged_parameters.restype is C.c_int
    # a NULL sim, with or without a descriptor, is a status and an error text, not a crash
    assert lib.lgs_set_privileged_parameters(None, None) == -1 and b"null" in lib.lgs_last_error()
    assert lib.lgs_set_privileged_parameters(None, C.byref(cabi.PrivParams())) == -1 and lib.lgs_last_error()
    assert C.sizeof(cabi.TaskParams) == 2632  # (the task struct is untouched)


# ------------------------------------------------------------ policy side ---
def test_first_layer_widths_of_an_actor_and_a_critic_of_different_widths():
    import torch.nn as nn
    lins = [nn.Linear(8, 512), nn.Linear(512, 256), nn.Linear(256, 128), nn.Linear(128, 1)]
    # the pinned single-net rule is untouched
    assert [mm._pad_k0(n) for n in (45, 48, 235, 250, 256)] == [48, 48, 240, 256, 256]
    assert [mm._pad_k0(n) for n in (257, 300, 320, 427, 428, 448, 500, 512)] == [320, 320, 320, 448, 448, 448, 512, 512]
    assert mm._pad_k0(87) == 88 and not mm.mlp_forward_supported(lins, 88)
    assert mm._pad_k0(274) == 320 and mm.mlp_forward_supported(lins, 320)
    # nets of different widths: a padding to 8 that is no multiple of 16 goes to 16
    assert mm._pad_k0_nets([240, 87]) == [240, 96] and mm._pad_k0_nets([427, 274]) == [448, 320]
    assert all(mm.mlp_forward_supported(lins, k) for k in (240, 96, 448, 320))
    assert mm._pad_k0_nets([300, 235]) == [320, 240]          # (tests/test_gpu_wider_mlp.py's pair)
    assert mm._pad_k0_nets([47, 50]) == [48, 64] and mm._pad_k0_nets([41, 44]) == [48, 48]
    # nets of one width keep the single-net rule, whatever it pads to
    for n in (45, 48, 50, 87, 235, 240, 427):
        assert mm._pad_k0_nets([n, n]) == [mm._pad_k0(n)] * 2
