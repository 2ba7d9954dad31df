"""env configuration -> ``lgs_task_params`` (everything post_physics_step reads).

Takes any env-like object (the live LeggedRobot, or a host-only namespace in
tests) exposing the attributes the reference env derives in _parse_cfg /
_init_buffers / _prepare_reward_function (legged_robot.py:52-186, 817-840).
"""
from __future__ import annotations

import os

import numpy as np

from . import cabi


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _put(arr, values):
    v = _np(values).astype(np.float32).reshape(-1)
    arr[: len(v)] = v.tolist()


def build_task_params(env) -> cabi.TaskParams:
    T = cabi.TaskParams()
    cfg = env.cfg
    A, D = env.num_actions, env.num_dof
    if A != D:
        raise ValueError("num_actions must equal the number of DOFs")
    T.obs_layout = env.obs_layout
    T.num_obs = env.num_obs
    T.num_privileged_obs = env.num_privileged_obs or 0
    T.num_actions = A
    T.decimation = cfg.control.decimation
    T.control_type = {"P": 0, "V": 1, "T": 2}.get(cfg.control.control_type, -1)
    if T.control_type < 0:
        raise NameError(f"Unknown controller type: {cfg.control.control_type}")
    T.action_scale = cfg.control.action_scale
    T.clip_actions = cfg.normalization.clip_actions
    T.clip_observations = cfg.normalization.clip_observations
    T.control_dt = env.dt
    _put(T.p_gains, env.p_gains)
    _put(T.d_gains, env.d_gains)
    _put(T.default_dof_pos, _np(env.default_dof_pos).reshape(-1))
    _put(T.torque_limits, env.torque_limits)
    lim = _np(env.dof_pos_limits)
    _put(T.soft_dof_pos_lower, lim[:, 0])
    _put(T.soft_dof_pos_upper, lim[:, 1])
    _put(T.dof_vel_limits, env.dof_vel_limits)
    s = env.obs_scales
    T.obs_scale_lin_vel, T.obs_scale_ang_vel = s.lin_vel, s.ang_vel
    T.obs_scale_dof_pos, T.obs_scale_dof_vel = s.dof_pos, s.dof_vel
    _put(T.commands_scale, env.commands_scale)
    T.add_noise = int(bool(env.add_noise))
    # (with the height scan observed the vector's tail is the scan's one scale, in lgs_height_obs:
    # height_obs_params, which also refuses a cfg the tail cannot honour)
    # (with an observation history it is the newest frame's head: history_noise_head)
    # (with both, DESIGN 3.13: the head tiled, then the scan's entries)
    hist = obs_history_params(env)
    if hist.enabled:
        height_obs_params(env)  # (refuses a tail that is not one scale)
        _put(T.noise_vec, history_noise_head(env, hist))
    else:
        _put(T.noise_vec, _np(env.noise_scale_vec).reshape(-1)[:env.num_obs - height_obs_params(env).num_points])
    T.max_episode_length = float(env.max_episode_length)
    T.max_episode_length_s = float(env.max_episode_length_s)
    T.resample_interval = int(cfg.commands.resampling_time / env.dt)
    T.heading_command = int(bool(cfg.commands.heading_command))
    r = env.command_ranges
    _put(T.cmd_lin_vel_x, r["lin_vel_x"])
    _put(T.cmd_lin_vel_y, r["lin_vel_y"])
    _put(T.cmd_ang_vel_yaw, r["ang_vel_yaw"])
    _put(T.cmd_heading, r["heading"])
    T.push_robots = int(bool(cfg.domain_rand.push_robots))
    T.push_interval = int(cfg.domain_rand.push_interval)
    T.max_push_vel_xy = cfg.domain_rand.max_push_vel_xy
    _put(T.base_init_state, env.base_init_state)
    fi = [int(x) for x in _np(env.feet_indices).tolist()]
    if len(fi) > cabi.MAX_FEET:
        raise ValueError("too many feet bodies for the native step")
    T.num_feet = len(fi)
    T.feet_idx[: len(fi)] = fi
    pi_ = [int(x) for x in _np(env.penalised_contact_indices).tolist()][: cabi.MAX_CONTACT_BODIES]
    T.num_penalised = len(pi_)
    T.penalised_idx[: len(pi_)] = pi_
    ti = [int(x) for x in _np(env.termination_contact_indices).tolist()][: cabi.MAX_CONTACT_BODIES]
    T.num_termination = len(ti)
    T.termination_idx[: len(ti)] = ti
    hip = list(env.hip_dof_indices)
    T.num_hip = len(hip)
    T.hip_dofs[: len(hip)] = hip
    native = list(getattr(env, "_native_reward_names", env.reward_names))
    py = [n for n, _ in getattr(env, "_py_rewards", [])]
    hooks = getattr(env, "_hooks", frozenset())
    T.num_rewards = len(native)
    # the reward total (only_positive_rewards, the termination term) is finished in Python when
    # Python terms add to it or a Python check_termination decides the resets
    T.defer_reward_total = int(bool(py) or "check_termination" in hooks)
    T.num_extra_sums = len(py)
    aliases = getattr(env, "reward_aliases", None)  # the task class's own names for native terms
    for k, n in enumerate(native):
        T.reward_ids[k] = cabi.reward_id(n, aliases)
        T.reward_scales[k] = float(env.reward_scales[n])
    T.has_termination_reward = int("termination" in env.reward_scales)
    T.termination_scale = float(env.reward_scales.get("termination", 0.0))
    rw = cfg.rewards
    T.only_positive_rewards = int(bool(rw.only_positive_rewards))
    T.tracking_sigma = rw.tracking_sigma
    T.base_height_target = rw.base_height_target
    T.max_contact_force = rw.max_contact_force
    T.soft_dof_vel_limit = rw.soft_dof_vel_limit
    T.soft_torque_limit = rw.soft_torque_limit
    # gait phase constants of the humanoid envs (h1_env.py:58-59, :101, :109)
    T.phase_period, T.phase_offset, T.stance_threshold, T.swing_height_target = 0.8, 0.5, 0.55, 0.08
    seed = int(getattr(cfg, "seed", 1))
    rank = int(os.environ.get("RANK", "0"))
    T.seed = (seed & 0xFFFFFFFF) | (rank << 32)
    # the rows the step refreshes: the feet (all the reference's humanoid envs read, h1_env.py:34-52)
    # unless the task asks for every body (rigid_body_state_bodies = "all"); by default every
    # body when the task has Python reward terms or step hooks, which may read any row
    bodies = getattr(env, "rigid_body_state_bodies", None)
    if bodies is None:
        bodies = "all" if (py or hooks) else "feet"
    if bodies not in ("all", "feet"):
        raise ValueError(f"rigid_body_state_bodies must be 'all', 'feet' or None, not {bodies!r}")
    T.write_body_states = int(bool(getattr(env, "uses_rigid_body_states", env.obs_layout == cabi.OBS_HUMANOID)) or
                              bool(py) or bool(hooks))
    if bodies == "all":
        T.body_state_mask = 0
    else:
        T.body_state_mask = sum(1 << b for b in fi) if fi else 0
    T.custom_origins = int(bool(getattr(env, "custom_origins", False)))
    _native_task_switches(T, env, A)
    _terrain_switches(T, env)
    return T


def terrain_switches(cfg):
    """(level_curriculum, scan_heights, ground_relative_heights) of a cfg, refusing the combinations
    the step cannot honour: any of them on a plane (there is no map to move on or to scan), and
    ground-relative height terms without the scan they average."""
    tc, rw = cfg.terrain, cfg.rewards
    cur = bool(getattr(tc, "level_curriculum", False))
    scan = bool(getattr(tc, "scan_heights", False))
    rel = bool(getattr(rw, "ground_relative_heights", False))
    if tc.mesh_type not in ("heightfield", "trimesh"):
        on = [n for n, v in (("terrain.level_curriculum", cur), ("terrain.scan_heights", scan),
                             ("rewards.ground_relative_heights", rel)) if v]
        if on:
            raise ValueError(f"{', '.join(on)} need a terrain map (terrain.mesh_type 'heightfield' or 'trimesh'), "
                             f"not {tc.mesh_type!r}")
    if rel and not scan:
        raise ValueError("rewards.ground_relative_heights needs terrain.scan_heights (base_height averages the scan)")
    return cur, scan, rel


def scan_in_observations(cfg):
    """terrain.scan_in_observations of a cfg (the height scan is the tail of the
    observation rows), refusing it without the scan it observes.  (terrain.measure_heights is
    True in every config and inert: it is not the switch.)"""
    on = bool(getattr(cfg.terrain, "scan_in_observations", False))
    if on and not terrain_switches(cfg)[1]:
        raise ValueError("terrain.scan_in_observations needs terrain.scan_heights (the scan it observes)")
    return on


def layout_head(obs_layout, A):
    """(observation, privileged observation) widths of a layout's own rows for A actions."""
    if obs_layout == cabi.OBS_QUADRUPED:
        return 12 + 3 * A, 0
    if obs_layout == cabi.OBS_HUMANOID:
        return 11 + 3 * A, 14 + 3 * A
    raise ValueError("terrain.scan_in_observations needs the quadruped or the humanoid observation layout")


def _history_length(cfg):
    """cfg.env.history_length as a frame count, 1 where it is absent or not a valid count (the
    value itself is refused by obs_history_params)."""
    H = getattr(cfg.env, "history_length", 1)
    ok = not isinstance(H, bool) and isinstance(H, (int, float)) and int(H) == H and 1 <= H <= cabi.MAX_OBS_FRAMES
    return int(H) if ok else 1


def check_scan_observations(cfg, obs_layout, A):
    """The constructor's checks of terrain.scan_in_observations: the layout, the grid's size and
    cfg.env.num_observations / num_privileged_obs = the layout's head + the scan's points; with
    env.history_length = H > 1 the policy row is H heads, then the scan's points.
    Returns the number of scan points in the rows (0: the switch is off)."""
    if not scan_in_observations(cfg):
        return 0
    head, head_priv = layout_head(obs_layout, A)
    tc = cfg.terrain
    P = len(tc.measured_points_x) * len(tc.measured_points_y)
    if not 1 <= P <= cabi.MAX_SCAN_OBS:
        raise ValueError(f"terrain.scan_in_observations: {P} scan points, the rows take 1 to {cabi.MAX_SCAN_OBS}")
    H = _history_length(cfg)
    if H > 1 and cfg.env.num_observations != H * head + P:
        raise ValueError(f"env.history_length = {H} and terrain.scan_in_observations do not combine at "
                         f"env.num_observations = {cfg.env.num_observations}: the row is {H} x the layout's {head} "
                         f"+ {P} scan points, so it must be {H * head + P}")
    if cfg.env.num_observations != H * head + P:
        raise ValueError(f"terrain.scan_in_observations: env.num_observations must be {head} + {P} scan points = "
                         f"{head + P}, not {cfg.env.num_observations}")
    priv = cfg.env.num_privileged_obs
    # (with env.privileged_parameters the privileged row's width is priv_params' to check)
    if priv and head_priv and not bool(getattr(cfg.env, "privileged_parameters", False)) and priv != head_priv + P:
        raise ValueError(f"terrain.scan_in_observations: env.num_privileged_obs must be {head_priv} + {P} scan points "
                         f"= {head_priv + P}, not {priv}")
    return P


def height_obs_params(env) -> cabi.HeightObs:
    """lgs_height_obs of an env: off, or legged_gym's tail constants and the one noise scale of
    the tail of env.noise_scale_vec (a task override that makes it non-uniform is refused)."""
    H = cabi.HeightObs()
    P = check_scan_observations(env.cfg, env.obs_layout, env.num_actions)
    H.num_points = P  # (not a field of the C struct)
    if not P:
        return H
    tail = _np(env.noise_scale_vec).astype(np.float32).reshape(-1)[env.num_obs - P:]
    if len(tail) != P or not (tail == tail[0]).all():
        raise ValueError("_get_noise_scale_vec: the height scan's entries must share one noise scale "
                         "(the kernel's tail has a single scale)")
    H.enabled = 1
    H.offset, H.clip = cabi.HEIGHT_OBS_OFFSET, cabi.HEIGHT_OBS_CLIP
    H.scale = float(env.obs_scales.height_measurements)
    H.noise_scale = float(tail[0])
    return H


def actuator_rand_params(env) -> cabi.ActuatorRand:
    """lgs_actuator_rand of an env's cfg.domain_rand, without its buffers (the env
    allocates them when `enabled`).  A group that is off passes the neutral range ([1, 1]; delay
    [0, 0]); every group off: enabled = 0.  A range that is not finite 0 <= lo <= hi, or a delay
    outside 0 .. control.decimation substeps, is refused."""
    dr = env.cfg.domain_rand
    R = cabi.ActuatorRand()

    def factor_range(switch, name):
        if not bool(getattr(dr, switch, False)):
            return 1.0, 1.0
        r = getattr(dr, name)
        lo, hi = (float(r[0]), float(r[1])) if len(r) == 2 else (np.nan, np.nan)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= hi):
            raise ValueError(f"domain_rand.{name} must be [lo, hi] with finite 0 <= lo <= hi, not {list(r)!r}")
        return lo, hi

    R.kp_range[:] = factor_range("randomize_kp", "kp_range")
    R.kd_range[:] = factor_range("randomize_kd", "kd_range")
    R.strength_range[:] = factor_range("randomize_motor_strength", "motor_strength_range")
    delay = (0, 0)
    if bool(getattr(dr, "randomize_action_delay", False)):
        r = dr.action_delay_range
        dec = int(env.cfg.control.decimation)
        ok = len(r) == 2 and all(float(x) == int(x) for x in r) and 0 <= int(r[0]) <= int(r[1]) <= dec
        if not ok:
            raise ValueError(f"domain_rand.action_delay_range must be [lo, hi] in whole physics substeps with "
                             f"0 <= lo <= hi <= control.decimation = {dec}, not {list(r)!r}")
        delay = (int(r[0]), int(r[1]))
    R.delay_range[:] = delay
    R.enabled = int(any(bool(getattr(dr, s, False)) for s in
                        ("randomize_kp", "randomize_kd", "randomize_motor_strength", "randomize_action_delay")))
    R.resample_on_reset = int(bool(R.enabled and getattr(dr, "actuator_resample_on_reset", True)))
    return R


def priv_params(env) -> cabi.PrivParams:
    """lgs_priv_params of an env's cfg.env.privileged_parameters: the randomised
    parameters as a tail of the privileged row.  A group with range [lo, hi] passes
    offset = (lo + hi) / 2 and scale = 2 / (hi - lo) (1 when hi == lo), computed in double: a
    randomised parameter lands in [-1, 1], a fixed one at 0.  Ranges: friction_range with
    randomize_friction, else the terrain's static friction; added_mass_range with
    randomize_base_mass, else [0, 0]; the actuator groups the ranges actuator_rand_params resolves.
    The friction and mass entries are always there and the actuator entries follow the actuator
    switches alone, so the width does not move with randomize_friction, push_robots or add_noise
    (a checkpoint's critic still loads in play.py).  `num_tail`, `num_head` and `num_priv` (not
    fields of the C struct): the tail's, the head's and the whole row's width.  Refused: the
    handstand layout, a head + tail above cabi.MAX_OBS, and an env.num_privileged_obs other than the
    row's width."""
    R = cabi.PrivParams()
    R.num_tail = R.num_head = R.num_priv = 0
    cfg = env.cfg
    if not bool(getattr(cfg.env, "privileged_parameters", False)):
        return R
    A = env.num_actions
    if env.obs_layout == cabi.OBS_QUADRUPED:
        head = 12 + 3 * A
    elif env.obs_layout == cabi.OBS_HUMANOID:
        head = 14 + 3 * A
    else:
        raise ValueError("env.privileged_parameters needs the quadruped or the humanoid observation layout (the "
                         "handstand task's privileged row is its noisy frame)")
    act = actuator_rand_params(env)
    Wp = 2 + (3 * A + 1 if act.enabled else 0)
    if head + Wp > cabi.MAX_OBS:
        raise ValueError(f"env.privileged_parameters: the privileged head ({head}) + the parameter tail ({Wp}) = "
                         f"{head + Wp} exceed the {cabi.MAX_OBS} entries the step's observation stage holds")
    S = check_scan_observations(cfg, env.obs_layout, A)
    if cfg.env.num_privileged_obs != head + Wp + S:
        raise ValueError(f"env.privileged_parameters: env.num_privileged_obs must be {head} + {Wp} parameters + "
                         f"{S} scan points = {head + Wp + S}, not {cfg.env.num_privileged_obs}")
    dr = cfg.domain_rand
    fr = list(dr.friction_range) if bool(dr.randomize_friction) else [cfg.terrain.static_friction] * 2
    mr = list(dr.added_mass_range) if bool(dr.randomize_base_mass) else [0.0, 0.0]
    ranges = {"friction": fr, "added_mass": mr, "kp": list(act.kp_range), "kd": list(act.kd_range),
              "strength": list(act.strength_range), "delay": list(act.delay_range)}
    for name in cabi.PRIV_GROUPS:
        r = ranges[name]
        lo, hi = (float(r[0]), float(r[1])) if len(r) == 2 else (np.nan, np.nan)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"env.privileged_parameters: the {name} range must be finite [lo, hi] with lo <= hi, "
                             f"not {r!r}")
        getattr(R, name)[:] = ((lo + hi) / 2.0, 2.0 / (hi - lo) if hi > lo else 1.0)
    R.enabled, R.num_tail, R.num_head, R.num_priv = 1, Wp, head, head + Wp + S
    return R


def obs_frame_width(obs_layout, A, num_feet=0):
    """The width of a layout's own policy row (one frame of an observation history): what
    lgs_set_task accepts as num_obs for the layout without a history."""
    if obs_layout == cabi.OBS_HANDSTAND:
        return 6 + 3 * A + num_feet
    return (11 if obs_layout == cabi.OBS_HUMANOID else 12) + 3 * A


def obs_history_params(env) -> cabi.ObsHistory:
    """lgs_obs_history of an env's cfg.env.history_length, without its buffers (the env
    allocates them when `enabled`).  1 is off.  With H >= 2 the policy row is the last H frames,
    oldest first, each the layout's own row; `num_frame` (not a field of the C struct) is that
    row's width.  With terrain.scan_in_observations the row is those H frames, then
    the one current scan: H * F + P entries.  Refused: a length outside 1 .. 8, num_observations
    that is not H frames (+ the scan's points), and a task class with a Python
    compute_observations (it would edit a row whose older frames the kernel has already stored)."""
    R = cabi.ObsHistory()
    R.num_frame = 0
    H = getattr(env.cfg.env, "history_length", 1)
    if isinstance(H, bool) or int(H) != H or not 1 <= H <= cabi.MAX_OBS_FRAMES:
        raise ValueError(f"env.history_length must be a whole number of frames from 1 (off) to "
                         f"{cabi.MAX_OBS_FRAMES}, not {H!r}")
    H = int(H)
    if H == 1:
        return R
    F = obs_frame_width(env.obs_layout, env.num_actions, len(_np(env.feet_indices).reshape(-1)))
    if scan_in_observations(env.cfg):
        tc = env.cfg.terrain
        P = len(tc.measured_points_x) * len(tc.measured_points_y)
        if env.cfg.env.num_observations != H * F + P:
            raise ValueError(f"env.history_length = {H} and terrain.scan_in_observations do not combine at "
                             f"env.num_observations = {env.cfg.env.num_observations}: the row is {H} x the layout's "
                             f"{F} + {P} scan points, so it must be {H * F + P}")
    elif env.cfg.env.num_observations != H * F:
        raise ValueError(f"env.history_length = {H}: env.num_observations must be {H} x the layout's {F} = "
                         f"{H * F}, not {env.cfg.env.num_observations}")
    if "compute_observations" in getattr(env, "_hooks", frozenset()):
        raise ValueError("env.history_length > 1 with a Python compute_observations: the override would edit "
                         "a row whose older frames the kernel has already stored (INTEGRATION.md)")
    R.enabled, R.frames, R.num_frame = 1, H, F
    return R


def history_noise_head(env, R):
    """The one frame's noise scales of env.noise_scale_vec under an observation history R: the
    vector is that head tiled R.frames times (older frames are copied, never re-noised, so the
    kernel reads the head alone); an override that is not that tiling is refused.  With the
    height scan observed the scan's entries follow the tiling (height_obs_params reads them)."""
    v = _np(env.noise_scale_vec).astype(np.float32).reshape(-1)
    F, H = R.num_frame, R.frames
    P = check_scan_observations(env.cfg, env.obs_layout, env.num_actions)
    if len(v) != H * F + P or not (v[:H * F].reshape(H, F) == v[:F]).all():
        raise ValueError(f"_get_noise_scale_vec: with env.history_length = {H} the vector must be the frame's "
                         f"{F} scales tiled {H} times (the kernel noises the newest frame only)")
    return v[:F]


def _terrain_switches(T, env):
    """The rough-terrain switches: the level curriculum's tile table and threshold, the
    height scan's grid, the ground-relative height terms."""
    cfg = env.cfg
    cur, scan, rel = terrain_switches(cfg)
    tc = cfg.terrain
    if cur:
        T.terrain_curriculum = 1
        T.terrain_rows, T.terrain_cols = int(tc.num_rows), int(tc.num_cols)
        T.terrain_half_length_sq = float(np.float32(0.5 * tc.terrain_length) ** 2)
    if scan:
        px, py = list(tc.measured_points_x), list(tc.measured_points_y)
        if not (1 <= len(px) <= cabi.MAX_HEIGHT_POINTS and 1 <= len(py) <= cabi.MAX_HEIGHT_POINTS):
            raise ValueError(f"terrain.measured_points_x / _y: 1 to {cabi.MAX_HEIGHT_POINTS} entries each")
        T.measure_heights = 1
        T.num_height_x, T.num_height_y = len(px), len(py)
        _put(T.height_points_x, px)
        _put(T.height_points_y, py)
    T.ground_relative_heights = int(rel)


def _native_task_switches(T, env, A):
    """The task switches past the base env's behaviour (all off for a plain LeggedRobot):
    a per-DOF clamp of the PD target (LeggedRobot._pd_target_limits), and the handstand
    task's constants (`handstand` namespace of the env spec, envs/go2/go2_handstand_env.py)."""
    lim = env._pd_target_limits() if hasattr(env, "_pd_target_limits") else getattr(env, "pd_target_limits", None)
    if lim is not None:
        lo, hi = (_np(x).astype(np.float32).reshape(-1) for x in lim)
        if len(lo) != A or len(hi) != A:
            raise ValueError(f"_pd_target_limits must return two vectors of {A} entries")
        if T.control_type != 0:
            raise ValueError("_pd_target_limits needs control_type 'P' (the clamp is on the position target)")
        T.clamp_pd_targets = 1
        _put(T.pd_target_lower, lo)
        _put(T.pd_target_upper, hi)
    T.record_unclipped_torques = int(bool(getattr(env, "record_unclipped_torques", False)))
    hs = getattr(env, "handstand", None)
    if hs is None:
        hs = getattr(getattr(env, "spec", None), "handstand", None)
    if hs is not None:
        T.termination_mode = 1
        T.fallen_band = hs.fallen_band
        _put(T.pose_target, hs.pose_target)
        _put(T.pose_weight, hs.pose_weight)
        T.num_front_feet = hs.num_front_feet
        T.contact_flag_threshold = hs.contact_flag_threshold
        T.contact_flip_prob = hs.contact_flip_prob
        T.feet_together_target = hs.feet_together_target


# ----------------------------------------------------------------- symmetry ----
def scan_points(cfg):
    """The height scan's points [P, 3] in the robot's yaw frame, in the order of the scan's entries
    (legged_gym's _init_height_points: point k = ix * len(measured_points_y) + iy, z = 0)."""
    tc = cfg.terrain
    x, y = np.asarray(tc.measured_points_x, np.float64), np.asarray(tc.measured_points_y, np.float64)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(gx.size)], axis=1)


def _zero_pose_frames(model):
    """World rotation and origin of every body's joint frame with every joint at zero."""
    B = model.num_bodies
    rot, pos = np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b in range(B):
        jr = np.asarray(model.joint_rot[b], np.float64).reshape(3, 3)
        jp = np.asarray(model.joint_pos[b], np.float64)
        p = int(model.parent[b])
        if p < 0:
            rot[b], pos[b] = jr, jp
        else:
            rot[b], pos[b] = rot[p] @ jr, pos[p] + rot[p] @ jp
    return rot, pos


def joint_symmetry(env, tol=1e-4):
    """The joint table of the reflection across the robot's sagittal (x-z) plane:
    (perm int32 [D], sign float32 [D]) with mirror(q)[j] = sign[j] * q[perm[j]].  DOF j pairs with
    the DOF whose joint origin, all joints at zero, is j's with y -> -y (a joint in the plane
    pairs with itself), and whose axis is j's mirrored: a rotation about a mirrors to a rotation
    about (-ax, ay, -az), so the pair's axes agree up to that map and a sign, and that sign is the
    table's: -1 for an x or z axis, +1 for a y axis.  Refused: a model that does not pair
    completely, and a cfg whose default pose, PD gains or action scale are not the mirror image of
    themselves (the observation subtracts the default pose and the action is scaled into a PD
    target around it, so the row's mirror would not be a signed permutation)."""
    model = env.model
    D = model.num_dofs
    names = list(model.dof_names)
    rot, pos = _zero_pose_frames(model)
    body = [int(b) for b in model.dof_body]
    org = np.array([pos[b] for b in body])
    axw = np.array([rot[b] @ np.asarray(model.axis[b], np.float64) for b in body])
    perm, sign = np.zeros(D, np.int32), np.zeros(D, np.float32)
    for j in range(D):
        want = org[j] * (1.0, -1.0, 1.0)
        hits = [k for k in range(D) if np.abs(org[k] - want).max() < tol]
        if len(hits) != 1:
            raise ValueError(f"symmetry: joint {names[j]} has {len(hits)} mirror partners across the sagittal plane "
                             "(the model does not pair left-right)")
        k = hits[0]
        m = axw[k] * (-1.0, 1.0, -1.0)  # the partner's rotation, mirrored
        if np.abs(m - axw[j]).max() < tol:
            s = 1.0
        elif np.abs(m + axw[j]).max() < tol:
            s = -1.0
        else:
            raise ValueError(f"symmetry: the axes of joints {names[j]} and {names[k]} are not mirror images")
        perm[j], sign[j] = k, s
    if not (perm[perm] == np.arange(D)).all() or not (sign * sign[perm] == 1).all():
        raise ValueError("symmetry: the joint pairing is not an involution")
    f = lambda v: np.asarray(_np(v), np.float64).reshape(-1)  # noqa: E731

    def check(what, v, signed):
        v = f(v)
        m = v[perm] * (sign if signed else 1.0)
        bad = np.nonzero(np.abs(m - v) > 1e-6 * np.maximum(1.0, np.abs(v)))[0]
        if len(bad):
            j = int(bad[0])
            raise ValueError(f"symmetry: {what} of joint {names[j]} ({v[j]:g}) is not the mirror image of "
                             f"{names[int(perm[j])]}'s ({v[int(perm[j])]:g})")

    check("the default angle (init_state.default_joint_angles)", env.default_dof_pos, True)
    check("the stiffness (control.stiffness)", env.p_gains, False)
    check("the damping (control.damping)", env.d_gains, False)
    scale = np.broadcast_to(f(env.cfg.control.action_scale), (D,)) if np.ndim(env.cfg.control.action_scale) == 0 \
        else f(env.cfg.control.action_scale)
    check("the action scale (control.action_scale)", scale, False)
    return perm, sign


def _scan_symmetry(cfg):
    """The scan's table: point (x_i, y_j) -> (x_i, -y_j), sign +1, found on the point list."""
    pts = scan_points(cfg)
    P = len(pts)
    perm = np.zeros(P, np.int32)
    for k in range(P):
        want = pts[k] * (1.0, -1.0, 1.0)
        hits = np.nonzero(np.abs(pts - want).max(axis=1) < 1e-9)[0]
        if len(hits) != 1:
            raise ValueError(f"symmetry: terrain.measured_points_y is not symmetric about 0 (the scan point "
                             f"({pts[k][0]:g}, {pts[k][1]:g}) has no mirror image)")
        perm[k] = hits[0]
    return perm, np.ones(P, np.float32)


def _cat(*tables):
    """Tables laid side by side: each block's permutation offset by the widths before it."""
    perm, sign, off = [], [], 0
    for p, s in tables:
        perm.append(np.asarray(p, np.int64) + off)
        sign.append(np.asarray(s, np.float32))
        off += len(p)
    return np.concatenate(perm).astype(np.int32), np.concatenate(sign).astype(np.float32)


def symmetry_tables(env):
    """The reflection across the robot's sagittal plane as signed permutations of the env's rows
    (DESIGN 3.19): ((perm, sign) of the policy row, of the critic row, of the action row), each
    perm int32 [K], sign float32 [K], mirror(x)[j] = sign[j] * x[perm[j]].  The critic row's table
    is the policy row's when the env has no privileged row.  Quadruped layout only: the frame is
    lin vel (+,-,+), ang vel (-,+,-), gravity (+,-,+), commands (+,-,-), then joint positions,
    velocities and previous actions through joint_symmetry; an observation history tiles it; the
    scan maps (x, y) -> (x, -y); the privileged row (3.17) is the clean frame, friction, added mass,
    the per-joint kp, kd and strength factors permuted by the pairing with sign +1, the delay, and
    the clean scan.  Refused: the handstand and the humanoid layouts, a task class with a Python
    compute_observations, and what joint_symmetry and the scan's table refuse."""
    if env.obs_layout == cabi.OBS_HANDSTAND:
        raise ValueError("symmetry: the handstand layout is not supported (its pose target and front-feet terms "
                         "are one-sided)")
    if env.obs_layout == cabi.OBS_HUMANOID:
        raise ValueError("symmetry: the humanoid layout is not supported yet (its registered tasks train "
                         "recurrent policies, which the augmentation refuses)")
    if env.obs_layout != cabi.OBS_QUADRUPED:
        raise ValueError("symmetry: unknown observation layout")
    if "compute_observations" in getattr(env, "_hooks", frozenset()):
        raise ValueError("symmetry: the task class overrides compute_observations in Python, so its rows are not "
                         "the layout's to describe")
    A = env.num_actions
    joints = joint_symmetry(env)
    if len(joints[0]) != A:
        raise ValueError("symmetry: num_actions must equal the number of DOFs")
    ident3 = np.arange(3)
    base = _cat((ident3, (1, -1, 1)), (ident3, (-1, 1, -1)), (ident3, (1, -1, 1)), (ident3, (1, -1, -1)))
    frame = _cat(base, joints, joints, joints)
    H = obs_history_params(env).frames if obs_history_params(env).enabled else 1
    P = check_scan_observations(env.cfg, env.obs_layout, A)
    scan = [_scan_symmetry(env.cfg)] if P else []
    policy = _cat(*([frame] * H + scan))
    if len(policy[0]) != env.num_obs:
        raise ValueError(f"symmetry: the policy row's table has {len(policy[0])} entries for {env.num_obs} observations")
    critic = policy
    if env.num_privileged_obs:
        R = priv_params(env)
        if not R.enabled:
            raise ValueError("symmetry: a privileged row without env.privileged_parameters is not the layout's "
                             "to describe")
        one = (np.zeros(1, np.int32), np.ones(1, np.float32))
        unsigned = (joints[0], np.ones(A, np.float32))
        tail = [one, one] + ([unsigned, unsigned, unsigned, one] if R.num_tail > 2 else [])
        critic = _cat(frame, *tail, *scan)
        if len(critic[0]) != env.num_privileged_obs:
            raise ValueError(f"symmetry: the critic row's table has {len(critic[0])} entries for "
                             f"{env.num_privileged_obs} privileged observations")
    return policy, critic, joints
