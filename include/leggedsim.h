/*
 * leggedsim.h — C ABI of the MI355X-native vectorised legged-robot simulator.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json
 * (`LeggedRobot.step()`: PD -> rigid-body dynamics + contact x decimation ->
 * obs / reward / done / reset).  It replaces two reference interfaces:
 *
 *  (1) the IsaacGym tensor API the env calls:
 *        gym.create_sim / prepare_sim          legged_robot.py:240, base_task.py:56
 *        acquire_*_tensor + wrap_tensor        legged_robot.py:83-92,104-120, h1_env.py:37
 *        refresh_*_tensor                      legged_robot.py:639,678-679, h1_env.py:49
 *        set_dof_actuation_force_tensor        legged_robot.py:629
 *        simulate / fetch_results              legged_robot.py:630,637-638
 *        set_actor_root_state_tensor_indexed   legged_robot.py:553-555,592-594
 *        set_dof_state_tensor_indexed          legged_robot.py:570-572
 *        per-env shape friction / base mass    legged_robot.py:412-440,472-483
 *  (2) the whole control step `LeggedRobot.step` (legged_robot.py:615-647) with
 *      `post_physics_step` (:673-709) fused into ONE launch (lgs_step), so the
 *      Python side keeps the VecEnv contract but issues no per-op kernels and
 *      no device->host syncs (the reference's nonzero() calls at :511,:545,:697
 *      become in-kernel masks).
 *
 * Conventions
 *  - All state / env buffers are DEVICE pointers, fp32, env-major, contiguous:
 *      root_states [N,13] = pos(3) quat xyzw(4) lin vel of the root COM(3) ang vel(3)
 *      dof_state   [N*D,2] = (q, qd)
 *      net_contact_forces [N*B,3]   (from the last substep, like PhysX)
 *      rigid_body_states  [N*B,13]  (origin pos, quat, COM lin vel, ang vel)
 *    The caller owns these buffers and binds them once (lgs_bind_state);
 *    the simulator reads and writes them in place, so refresh_* is a no-op
 *    and a torch tensor view is always current.
 *  - Booleans (reset, time_out, last_contacts) are 1 byte (torch.bool).
 *  - Host-side descriptors (model, params) are copied at call time.
 *  - Every call returns LGS_OK (0) or a negative status; lgs_last_error()
 *    gives a thread-local message.  No call aborts the process.
 *  - Work is enqueued on the stream set with lgs_set_stream (default stream 0);
 *    nothing synchronises the host except lgs_synchronize.  Launches are
 *    hipGraph-capturable (no allocation or sync inside lgs_step/lgs_simulate).
 *  - One host thread per lgs_sim.
 */
#ifndef LEGGEDSIM_H
#define LEGGEDSIM_H

#include <stdint.h>

#ifdef __cplusplus
#define LGS_EXTERN extern "C"
#else
#define LGS_EXTERN
#endif
#define LGS_API LGS_EXTERN __attribute__((visibility("default")))

#define LGS_OK 0
#define LGS_ERR_ARG (-1)
#define LGS_ERR_HIP (-2)
#define LGS_ERR_STATE (-3)

#define LGS_MAX_BODIES 32
#define LGS_MAX_DOFS 26
#define LGS_MAX_DEPTH 10
#define LGS_MAX_FEET 4
#define LGS_MAX_CONTACT_BODIES 16
#define LGS_MAX_OBS 128
#define LGS_MAX_REWARDS 24
#define LGS_MAX_SELF_PROXIES 64
#define LGS_MAX_SELF_PAIRS 192

/* ---- articulated model (host pointers; see leggedsim/model.py) ---------- */
typedef struct lgs_model_desc {
    int32_t num_bodies;       /* B (after fixed-joint collapse)          */
    int32_t num_dofs;         /* D (revolute joints, DFS order)          */
    int32_t num_points;       /* P contact candidate points              */
    const int32_t* parent;    /* [B]  -1 for the floating root            */
    const int32_t* dof;       /* [B]  dof of the joint to the parent or -1 */
    const int32_t* subtree_end; /* [B] subtree(b) = [b, subtree_end[b])    */
    const int32_t* depth;     /* [B]                                     */
    const int32_t* chain;     /* [B][LGS_MAX_DEPTH] root..b, -1 padded    */
    const float* joint_rot;   /* [B][9] parent frame -> joint frame (row-major) */
    const float* joint_pos;   /* [B][3]                                  */
    const float* axis;        /* [B][3] joint axis in the child frame     */
    const float* mass;        /* [B]                                     */
    const float* com;         /* [B][3] body frame                        */
    const float* inertia;     /* [B][6] Ixx Iyy Izz Ixy Ixz Iyz about com  */
    const int32_t* dof_body;  /* [D]                                     */
    const float* dof_lower;   /* [D] URDF limits                          */
    const float* dof_upper;
    const float* dof_effort;
    const float* dof_velocity;
    const int32_t* pt_body;   /* [P]                                     */
    const float* pt_pos;      /* [P][3] body frame                        */
    const float* pt_radius;   /* [P]                                     */
    /* names, copied at lgs_create_sim (get_asset_rigid_body_names / get_asset_dof_names,
     * legged_robot.py:342-343); either may be NULL (the queries then return NULL / -1) */
    const char* const* body_names; /* [B] */
    const char* const* dof_names;  /* [D] */
} lgs_model_desc;

/* ---- simulation parameters: cfg.sim + cfg.sim.physx + cfg.asset
 *      (legged_robot_config.py:131-143, 225-242)                         */
typedef struct lgs_sim_params {
    float dt;                        /* sim.dt (0.005; H1_2 0.0025)        */
    float gravity[3];                /* (0,0,-9.81), z up                  */
    int32_t solver_iterations;       /* contact/limit PGS sweeps per substep */
    float contact_offset;            /* physx.contact_offset  (0.01 m)     */
    float rest_offset;               /* physx.rest_offset     (0.0)        */
    float max_depenetration_velocity;/* physx (1.0 m/s)                    */
    float baumgarte;                 /* penetration fraction corrected per substep */
    float ground_friction;           /* plane static/dynamic friction (1.0), averaged with shape friction */
    float armature;                  /* asset.armature (H1_2: 1e-3)        */
    int32_t clamp_joint_velocity;    /* clamp |qd| to the URDF velocity limit */
    int32_t max_contacts;            /* contact slots per env               */
    int32_t max_rows;                /* constraint rows per env (<= compiled capacity);
                                        joint-limit rows: max_rows - 3*max_contacts, plus the
                                        rows of the contact slots a substep leaves unused */
} lgs_sim_params;
/* Contact slots per substep (PhysX reports every touching shape; a fixed-capacity solver has
 * to choose).  In this order, while slots last:
 *   1. every body touching the ground gets ONE slot, for its first touching candidate point
 *      (candidate order; bodies in the order of those candidates),
 *   2. self contacts (pair order), at most max_self_contacts,
 *   3. the remaining touching ground candidates, in candidate order.
 * So planted feet cannot take the slots of a knee, hip or pelvis on the ground (its contact
 * force, the collision penalty and contact terminations depend on them).  Joint limits take
 * the limit rows in DOF order, then the rows of unused contact slots.  Whatever still does not
 * fit is counted: lgs_get_contact_stats.
 * The solve visits the rows in this order: the ground contacts (1. then 3.), the self contacts, the
 * joint limits.  A ground contact's frame is n (the triangle's normal), t1 = normalise(e_x - n_x n),
 * t2 = n x t1, its friction 0.5 * (ground_friction + shape friction).  A contact's normal row aims at
 * -sep/dt over an open gap and at min(-baumgarte*sep/dt, max_depenetration_velocity) when it
 * penetrates.  A joint-limit row is taken when the predicted position q + dt*qd_free leaves
 * [lower, upper]; its target is -gap/dt, or -baumgarte*gap/dt when q is already beyond the limit
 * (gap < 0), and max_depenetration_velocity does not clamp it: that parameter is PhysX's for
 * contacts only.  Each sweep projects normal and limit impulses onto >= 0 and moves the two
 * friction rows of a contact together, each by its own diagonal of J M^-1 J^T (+ 1e-9), then scales
 * the pair back onto the disc of radius mu * lambda_n.  tests/phys_ref.py is these semantics in
 * fp64 from the textbook definitions; tests/test_gpu_phys_reference.py holds the kernel to it. */

/* ---- self-collision (IsaacGym create_actor collision filter, legged_robot.py:373-374:
 *      cfg.asset.self_collisions == 0 lets the links of one actor collide; see
 *      leggedsim/selfcollision.py).  Every collision shape group is a capsule proxy in its
 *      body frame; the listed proxy pairs (never a body with itself or its parent) are
 *      tested every substep: closest points of the two segments, signed distance minus both
 *      radii and rest_offset, active below contact_offset.  A touching pair is one contact
 *      (normal from the second body to the first, acting at the midpoint of the two surfaces; a
 *      friction pair t1 = normalise(e - (e.n) n), t2 = n x t1 with e = x, or e = y when |n_x| >=
 *      0.57735 so that t1 stays well defined for a normal near the x axis; the env's shape friction)
 *      in the slots after the ground contacts; up to max_self_contacts of them per substep,
 *      first in pair order, after one slot per touching ground body (the slot order above).
 *      The contact force joins both bodies' net contact force with opposite signs.      */
typedef struct lgs_self_collision_desc {
    int32_t num_proxies;          /* S <= LGS_MAX_SELF_PROXIES                          */
    const int32_t* proxy_body;    /* [S]                                                */
    const float* capsule;         /* [S][7] segment end points p0, p1 (body frame), radius */
    int32_t num_pairs;            /* Q <= LGS_MAX_SELF_PAIRS; 0 disables self-collision  */
    const int32_t* pair;          /* [Q][2] proxy indices                               */
    int32_t max_self_contacts;    /* contact slots self contacts may take per substep    */
} lgs_self_collision_desc;

/* ---- task (env) parameters: everything post_physics_step reads from cfg ---- */
enum lgs_obs_layout {
    LGS_OBS_QUADRUPED = 0,   /* legged_robot.py:800-807  [v*s, w*s, g, cmd*s, dq, qd*s, a]          */
    LGS_OBS_HUMANOID = 1,    /* h1_env.py:68-95 / g1_env.py:108-141  obs=[w,g,cmd,dq,qd,a,sin,cos], priv=[v, obs] */
    LGS_OBS_HANDSTAND = 2    /* go2_handstand_env.py:140-173  obs = priv = [w*s, g, dq*s, qd*s, a, front flags, hind flags] */
};

/* reward term ids; the task lists the active ones in alphabetical order
 * (class_to_dict uses dir(), legged_robot.py:822-836)                     */
enum lgs_reward_id {
    LGS_REW_ACTION_RATE = 0, LGS_REW_ALIVE, LGS_REW_ANG_VEL_XY, LGS_REW_BASE_HEIGHT,
    LGS_REW_COLLISION, LGS_REW_CONTACT, LGS_REW_CONTACT_NO_VEL, LGS_REW_DOF_ACC,
    LGS_REW_DOF_POS_LIMITS, LGS_REW_DOF_VEL, LGS_REW_DOF_VEL_LIMITS, LGS_REW_FEET_AIR_TIME,
    LGS_REW_FEET_CONTACT_FORCES, LGS_REW_FEET_STUMBLE, LGS_REW_FEET_SWING_HEIGHT,
    LGS_REW_HIP_POS, LGS_REW_LIN_VEL_Z, LGS_REW_ORIENTATION, LGS_REW_STAND_STILL,
    LGS_REW_TORQUE_LIMITS, LGS_REW_TORQUES, LGS_REW_TRACKING_ANG_VEL, LGS_REW_TRACKING_LIN_VEL,
    /* the Go2 handstand task (go2_handstand_env.py:224-383); its `orientation` and `base_height`
     * are its own formulas, so they have ids of their own (leggedsim/cabi.py, per-task aliases) */
    LGS_REW_HANDSTAND_ORIENTATION, LGS_REW_HANDSTAND_BASE_HEIGHT, LGS_REW_FRONT_FEET_CONTACT,
    LGS_REW_HIND_FEET_NO_CONTACT, LGS_REW_POSE, LGS_REW_STABILITY, LGS_REW_STAY_STILL, LGS_REW_LIN_VEL_XY,
    LGS_REW_ENERGY, LGS_REW_FRONT_HIP_NEUTRAL, LGS_REW_FRONT_FEET_TOGETHER,
    LGS_REW_COUNT
};

typedef struct lgs_task_params {
    int32_t obs_layout;            /* lgs_obs_layout                        */
    int32_t num_obs;               /* O                                     */
    int32_t num_privileged_obs;    /* P or 0                                */
    int32_t num_actions;           /* A (== D)                              */
    int32_t decimation;
    int32_t control_type;          /* 0 P, 1 V, 2 T (legged_robot.py:663-670) */
    float action_scale;
    float clip_actions, clip_observations;
    float control_dt;              /* decimation * sim.dt                   */
    float p_gains[LGS_MAX_DOFS], d_gains[LGS_MAX_DOFS];
    float default_dof_pos[LGS_MAX_DOFS];
    float torque_limits[LGS_MAX_DOFS];
    float soft_dof_pos_lower[LGS_MAX_DOFS], soft_dof_pos_upper[LGS_MAX_DOFS];
    float dof_vel_limits[LGS_MAX_DOFS];
    float obs_scale_lin_vel, obs_scale_ang_vel, obs_scale_dof_pos, obs_scale_dof_vel;
    float commands_scale[3];
    int32_t add_noise;
    float noise_vec[LGS_MAX_OBS];
    /* episode / commands / pushes */
    float max_episode_length;      /* ceil(episode_length_s / dt)            */
    float max_episode_length_s;
    int32_t resample_interval;     /* int(resampling_time / dt)              */
    int32_t heading_command;
    float cmd_lin_vel_x[2], cmd_lin_vel_y[2], cmd_ang_vel_yaw[2], cmd_heading[2];
    int32_t push_robots;
    int32_t push_interval;         /* int(ceil(push_interval_s / dt))        */
    float max_push_vel_xy;
    float base_init_state[13];
    /* bodies selected by name substring (legged_robot.py:346-407) */
    int32_t num_feet, feet_idx[LGS_MAX_FEET];
    int32_t num_penalised, penalised_idx[LGS_MAX_CONTACT_BODIES];
    int32_t num_termination, termination_idx[LGS_MAX_CONTACT_BODIES];
    int32_t num_hip, hip_dofs[8];
    /* rewards */
    int32_t num_rewards;
    int32_t reward_ids[LGS_MAX_REWARDS];
    float reward_scales[LGS_MAX_REWARDS];   /* already multiplied by dt      */
    int32_t has_termination_reward;
    float termination_scale;
    int32_t only_positive_rewards;
    float tracking_sigma, base_height_target, max_contact_force;
    float soft_dof_vel_limit, soft_torque_limit;
    /* humanoid gait phase (h1_env.py:55-65) */
    float phase_period, phase_offset, stance_threshold, swing_height_target;
    uint64_t seed;
    /* 1: refresh rigid_body_states [N,B,13] every control step (the humanoid envs
     * read it, h1_env.py:37,49); 0: leave it untouched (LeggedRobot never reads it) */
    int32_t write_body_states;
    /* 1: env origins are terrain tiles (legged_robot.py:582-585, custom_origins): reset_idx adds a
     * U[-1,1] xy offset to the root position (LGS_STREAM_RESET_ROOT draws 6, 7) */
    int32_t custom_origins;
    /* a task's reward terms written in Python (subclass _reward_* methods, legged_robot.py:817-840)
     * run between lgs_post_physics_rewards and lgs_post_physics_finish.  defer_reward_total = 1:
     * the kernel writes the raw sum of its own terms to rew (no only_positive_rewards clip, no
     * termination term; the caller adds its terms, clips and adds the termination term).
     * num_extra_sums: episode-sum rows after the native ones (and termination) that the caller
     * fills; they join the reset-time extras like the native sums. */
    int32_t defer_reward_total;
    int32_t num_extra_sums;
    /* with write_body_states: the bodies whose rigid_body_states rows each step refreshes (bit b =
     * body b; the humanoid tasks: their feet, the only rows h1_env.py:34-52 reads); 0 = every body.
     * lgs_forward_kinematics (refresh_rigid_body_state_tensor) always refreshes every body. */
    uint32_t body_state_mask;
    /* ---- task switches first used by the Go2 handstand task; all 0 = the behaviour above ---- */
    /* P control: the PD target action * action_scale + default_dof_pos[j] is clipped to
     * [pd_target_lower[j], pd_target_upper[j]] before the PD law, in every substep
     * (go2_handstand_env.py:326-350; -inf / +inf leave a DOF free) */
    int32_t clamp_pd_targets;
    float pd_target_lower[LGS_MAX_DOFS], pd_target_upper[LGS_MAX_DOFS];
    /* 1: env->torques, and what the torques / energy / torque_limits terms read, is the last
     * substep's PD torque BEFORE the effort clip (the reference's self.torques when a task's
     * _compute_torques does not clip, go2_handstand_env.py:349-350).  The joints are driven by the
     * clipped torque either way. */
    int32_t record_unclipped_torques;
    /* check_termination: 0 = contact on a termination body, |roll| > 0.8, |pitch| > 1.0, time-out
     * (legged_robot.py:711-721); 1 = contact, -fallen_band < projected_gravity.z < fallen_band,
     * time-out (go2_handstand_env.py:178-219) */
    int32_t termination_mode;
    float fallen_band;
    /* the `pose` term: (q - pose_target)^2 summed in DOF order over the DOFs of weight 1, then
     * over the others of non-zero weight; weight-1 sum + w * other sum (w: the others' weight) */
    float pose_target[LGS_MAX_DOFS], pose_weight[LGS_MAX_DOFS];
    /* feet_idx[0 .. num_front_feet) are the front feet, the rest the hind feet */
    int32_t num_front_feet;
    /* contact flags (the LGS_OBS_HANDSTAND observation, front_feet_contact, hind_feet_no_contact):
     * contact force z > contact_flag_threshold; with add_noise, observed flag j flips with
     * probability contact_flip_prob (LGS_STREAM_NOISE draw num_obs + j) */
    float contact_flag_threshold, contact_flip_prob;
    float feet_together_target;    /* front_feet_together: xy distance of the two front feet allowed */
    /* ---- rough-terrain switches; all 0 = the behaviour above ---- */
    /* 1: an env that resets in a control step or in lgs_reset_idx first moves its terrain level
     * (legged_gym's _update_terrain_curriculum; lgs_reset_all moves nothing), on its pre-reset root
     * xy and commands, all comparisons on squares (fp32, in this order):
     *   dx = x - ox; dy = y - oy; d2 = dx*dx + dy*dy            (ox, oy = env_origins[e])
     *   up   = d2 > terrain_half_length_sq
     *   h = 0.5f * max_episode_length_s
     *   down = !up && d2 < (cx*cx + cy*cy) * (h*h)               (cx, cy = commands[e][0:2])
     *   L = terrain_levels[e] + up - down
     *   L = L >= terrain_rows ? min((int)(u * terrain_rows), terrain_rows - 1) : max(L, 0)
     *   env_origins[e] = terrain_origins[L][terrain_types[e]]    (u: LGS_STREAM_TERRAIN draw 0)
     * The root placement of the same reset reads the new origin.  Needs the env buffers
     * terrain_levels, terrain_types and terrain_origins; terrain_level_sum is optional. */
    int32_t terrain_curriculum;
    int32_t terrain_rows, terrain_cols;   /* tile rows (levels) and columns (types) of terrain_origins */
    float terrain_half_length_sq;         /* (terrain_length / 2)^2 */
    /* 1: every control step fills env->measured_heights [N, P], P = num_height_x * num_height_y,
     * point k = ix * num_height_y + iy, from the post-physics, pre-reset root state (where
     * legged_gym's _post_physics_step_callback measures; legged_gym's _get_heights):
     *   (z', w') = (qz, qw) / sqrt(qz*qz + qw*qw); c = w'*w' - z'*z'; s = 2 * w' * z'   (yaw only)
     *   X = ((c*px - s*py) + x) + border_size;  Y = ((s*px + c*py) + y) + border_size
     *   i = clip((int)(X / horizontal_scale), 0, rows - 2); j likewise with cols
     *   height = min(H[i][j], H[i+1][j], H[i][j+1]) * vertical_scale        (0 on the plane) */
    int32_t measure_heights;
    int32_t num_height_x, num_height_y;   /* each <= LGS_MAX_HEIGHT_POINTS */
    float height_points_x[32], height_points_y[32];
    /* 1 (needs measure_heights): the height terms are relative to the ground.
     *   base_height       = (mean_k(root_z - measured_heights[k]) - base_height_target)^2; the mean's
     *                       order: partial j < 32 adds its points k = j, j + 32, ... in rising k
     *                       from 0, the partials are added j = 0..31 from 0, divided by P;
     *   feet_swing_height = ((foot_z - ground(foot_x, foot_y)) - swing_height_target)^2 off contact,
     *                       ground = the triangle interpolation documented at lgs_set_heightfield. */
    int32_t ground_relative_heights;
} lgs_task_params;
#define LGS_MAX_HEIGHT_POINTS 32

/* ---- the height scan in the observation row (lgs_set_height_observations) ----
 * enabled = 1 appends legged_gym's compute_observations tail to every observation row: with
 * P = num_height_x * num_height_y and `head` the layout's own width (LGS_OBS_QUADRUPED 12 + 3 A;
 * LGS_OBS_HUMANOID 11 + 3 A, privileged 14 + 3 A), the task's num_obs is head + P (and
 * num_privileged_obs, when the humanoid layout has that row, its head + P), and entry head + k is
 *   h    = clip((root_z - offset) - measured_heights[e][k], -clip, clip) * scale
 *   obs  = clip(h + (2u - 1) * noise_scale, -clip_observations, clip_observations)
 *   priv = clip(h, -clip_observations, clip_observations)            (humanoid layout only)
 * in fp32 without contraction; the noise only with add_noise, u = LGS_STREAM_NOISE draw head + k
 * (the head keeps its draws 0 .. head - 1, its arithmetic and its bits).  root_z is the root after
 * the step's reset; measured_heights is what the step measured before the reset (legged_gym's own
 * order: a reset env observes one row of heights from where its last episode ended).
 * Needs measure_heights and a layout other than LGS_OBS_HANDSTAND; head <= LGS_MAX_OBS and
 * P <= LGS_MAX_SCAN_OBS.  This call and lgs_set_task may come in either order: the pair is checked
 * by every step / reset entry point, which refuses an inconsistent one before any launch.
 * With an observation history (lgs_obs_history below) the scan follows the H frames of the head:
 * num_obs = H * head + P, entry H * head + k, and the draw stays head + k. */
#define LGS_MAX_SCAN_OBS 256
typedef struct lgs_height_obs {
    int32_t enabled;
    float offset;        /* legged_gym: 0.5 */
    float clip;          /* legged_gym: 1.0 */
    float scale;         /* normalization.obs_scales.height_measurements */
    float noise_scale;   /* noise_scales.height_measurements * noise_level * scale */
} lgs_height_obs;

/* ---- actuator randomisation and action latency (lgs_set_actuator_randomization) ----
 * enabled = 1 scales the PD gains of every env and DOF and delays the env's action by whole
 * physics substeps, inside the control step's decimation loop.  In fp32 without contraction and
 * in this order, for DOF j of env e (T = the task, D = the model's DOFs):
 *   kp = (T.p_gains[j] * kp_scale[e][j]) * strength[e][j]
 *   kd = (T.d_gains[j] * kd_scale[e][j]) * strength[e][j]          (both once per control step)
 *   a_used(it) = it < delay[e] ? a_prev : a        (substep it = 0 .. decimation - 1; a_prev =
 *                last_actions[e][j] as the step finds it, 0 in an episode's first step; a = this
 *                step's clipped action)
 *   as = a_used * T.action_scale
 *   control_type P:  t = kp * (target(as) - q) - kd * qd      (target: as + default_dof_pos[j],
 *                                                              clamped with clamp_pd_targets)
 *   control_type V:  t = kp * (as - qd) - kd * (qd - last_dof_vel) / dt
 *   control_type T:  t = as * strength[e][j]
 *   tau = clip(t, -T.torque_limits[j], T.torque_limits[j])    (record_unclipped_torques as without)
 * env->actions, the observations' action entries and the action_rate term keep a.  All factors 1
 * and delay 0 is, bit for bit, the step without the call.
 * The four buffers are the caller's device memory, read in place by every step (lgs_bind_state's
 * convention): editing them between steps is supported.  With resample_on_reset an env that
 * resets -- in a control step, in lgs_reset_idx (mask bytes 1 and 2) or in lgs_reset_all --
 * redraws its rows, u(k) = lgs_uniform(seed, e, step key, LGS_STREAM_ACTUATOR, k):
 *   kp_scale[e][j] = (kp_range[1] - kp_range[0]) * u(j) + kp_range[0]
 *   kd_scale[e][j] = likewise with kd_range and u(LGS_MAX_DOFS + j)
 *   strength[e][j] = likewise with strength_range and u(2 * LGS_MAX_DOFS + j)
 *   n = delay_range[1] - delay_range[0] + 1
 *   delay[e] = delay_range[0] + min((int)(u(3 * LGS_MAX_DOFS) * (float)n), n - 1)
 * The step in which an env resets ran on its old rows; the new ones act from the next step.
 * A range [1, 1] draws exactly 1.0f.  This call and lgs_set_task may come in either order: every
 * step / reset entry point checks the pair (non-NULL buffers, finite ranges with 0 <= lo <= hi,
 * 0 <= delay lo <= hi <= decimation) and refuses a bad one with LGS_ERR_ARG before any launch.
 * lgs_simulate (caller-supplied torques) is not affected. */
typedef struct lgs_actuator_rand {
    int32_t enabled;            /* 0: the step is what it is without this call */
    int32_t resample_on_reset;  /* 1: a resetting env redraws its rows; 0: the buffers are only read */
    float   kp_range[2], kd_range[2], strength_range[2];
    int32_t delay_range[2];     /* physics substeps, 0 <= lo <= hi <= decimation */
    float*   kp_scale;          /* device [N, D]  (D = the model's real DOFs, as env->torques) */
    float*   kd_scale;          /* device [N, D] */
    float*   strength;          /* device [N, D] */
    int32_t* delay;             /* device [N] */
} lgs_actuator_rand;

/* ---- observation history (lgs_set_observation_history) ----
 * Let F be the layout's own policy-row width, what lgs_set_task takes as num_obs without this
 * call (LGS_OBS_QUADRUPED 12 + 3 A; LGS_OBS_HUMANOID 11 + 3 A; LGS_OBS_HANDSTAND 6 + 3 A +
 * num_feet), and H = frames.  enabled = 1 makes the policy row of env e after a control step
 *   [frame(t-H+1) | ... | frame(t-1) | frame(t)]           (oldest first; num_obs = H * F)
 * where a frame is the F values the observation stage writes without the call: after the noise,
 * after the handstand's contact-flag flip and after clip_observations, so the history holds what
 * the policy was shown.  frame(t) uses noise_vec[0 .. F) and LGS_STREAM_NOISE draws 0 .. F)
 * (the handstand's flips F + j), exactly as without the call: no draw moves, none is added, and
 * older frames are copied, never re-noised.  The privileged row has no history in any layout
 * (the humanoid's P entries; the handstand's P = F noisy frame; the quadruped's one clean frame
 * under lgs_priv_params below, and no row without it: its critic then reads the history row).
 * Everything else the step writes -- rewards, termination,
 * resets, episode sums, commands, the last_* bookkeeping, the state -- is bit for bit what it
 * writes without the call.
 * Episode boundary: the first row an env writes after any reset of that env -- the reset inside
 * a control step, lgs_reset_idx (mask bytes 1 and 2), lgs_reset_all -- has all H slots equal to
 * that row's new frame: no zeros, and nothing of the ended episode.
 * State, the caller's device memory, read and written in place by every step (lgs_bind_state's
 * convention; editing them between steps is supported):
 *   history [N, (H-1) * F]  after a step the newest H - 1 frames of the row just written, oldest
 *                           first: row[F .. H * F).  The next step's older slots come from here,
 *                           never from an observation buffer (lgs_reset_idx and a caller that
 *                           does not double-buffer write env->obs in place).
 *   fill [N] int32          1: history[e] holds the env's running episode; 0: the env's next row
 *                           fills every slot with its frame (and sets the flag to 1).  A reset
 *                           writes 0, so zeroed buffers from the caller mean "fill on first write".
 * This call and lgs_set_task may come in either order: every step / reset entry point checks the
 * pair -- frames in 2 .. LGS_MAX_OBS_FRAMES, non-NULL buffers, num_obs == frames * F -- and
 * refuses a bad one with LGS_ERR_ARG before any launch.  With enabled = 0, num_obs is the
 * layout's own.
 * With the height observations (lgs_set_height_observations, P points, the three
 * setters in any order) the row is a history of the head alone, then one scan:
 *   [frame(t-H+1) | ... | frame(t) | scan(t)]                        (num_obs = H * F + P)
 * The frames follow every rule above with history and fill unchanged in shape and meaning; the
 * scan is lgs_height_obs's tail, current and never stored.  Scan point k keeps LGS_STREAM_NOISE
 * draw F + k, its index without a history, so the newest frame and the scan are bit for bit the
 * entries of the same env without this call.  The humanoid's privileged row stays its head + P.
 * The entry points accept the pair under the height observations' own rules (a task that measures
 * heights, P <= LGS_MAX_SCAN_OBS, the quadruped or humanoid layout) with num_obs == H * F + P;
 * both set on a task without a scan, or any other width, is refused ("observation history and
 * height observations do not combine", then what num_obs is and would have to be).
 * lgs_set_task itself takes num_obs up to LGS_MAX_OBS_FRAMES * LGS_MAX_OBS + LGS_MAX_SCAN_OBS. */
#define LGS_MAX_OBS_FRAMES 8
typedef struct lgs_obs_history {
    int32_t enabled;     /* 0: the rows are what they are without this call */
    int32_t frames;      /* H, 2 .. LGS_MAX_OBS_FRAMES */
    float*   history;    /* device [N, (H-1) * F] */
    int32_t* fill;       /* device [N] */
} lgs_obs_history;

/* ---- the randomised parameters in the privileged row (lgs_set_privileged_parameters) ----
 * The asymmetric critic's row: during training the critic may see the simulator's own truth,
 * the numbers that were randomised included.  With D the model's real DOFs, S the scan points in
 * the rows (0 without lgs_height_obs), F the quadruped layout's own frame width 12 + 3 A, and
 *   Wp = 2 + (3 D + 1)  with lgs_actuator_rand enabled,   Wp = 2  without,
 * enabled = 1 puts a parameter tail of Wp entries into the privileged row of env e, in this order:
 *   1   shape_friction[e] of lgs_set_env_properties (as the substep reads it)   group friction
 *   1   added_base_mass[e] (0 when never set)                                   group added_mass
 *   D   kp_scale[e][j]                                                          group kp
 *   D   kd_scale[e][j]                                                          group kd
 *   D   strength[e][j]                                                          group strength
 *   1   (float) delay[e]                                                        group delay
 * each  clip((v - offset) * scale, -clip_observations, clip_observations)  in fp32 without
 * contraction, {offset, scale} its group's.  No tail entry gets noise; no random draw is added
 * or moved.  The last four groups exist only with the actuator rows.
 *   LGS_OBS_QUADRUPED  num_privileged_obs = F + Wp + S, the row [clean frame | tail | clean scan]:
 *       the clean frame is the F values of the observation stage before the noise, clipped -- bit
 *       for bit what the same step writes to the newest frame of obs with add_noise = 0; the clean
 *       scan is clip(h, -clip_observations, clip_observations), the humanoid's rule.  With an
 *       observation history the privileged row still holds one frame.
 *   LGS_OBS_HUMANOID   num_privileged_obs = (14 + 3 A) + Wp + S, the row [head | tail | scan]: the
 *       head and the scan entries keep their bits, the scan only moves by Wp.
 *   LGS_OBS_HANDSTAND  refused: its privileged row is the reference's noisy frame by definition.
 * Limit: head + Wp <= LGS_MAX_OBS (a G1 with 23 DOFs and the actuator rows: 83 + 72 does not fit);
 * the row as a whole stays within what lgs_set_task accepts.
 * An env that resets shows the rows its NEXT control step acts on -- the redrawn ones
 * (lgs_actuator_rand's resample_on_reset), not those the ending step ran on: the privileged row
 * written after a reset is the first row of the new episode.  That holds for the reset inside a
 * control step (whose row is written by the same launch), and for lgs_reset_idx (mask bytes 1
 * and 2) and lgs_reset_all (whose rows the following step writes).
 * Everything else a step writes -- obs, rewards, termination, state, episode sums, the last_*
 * rows, the actuator rows, the history buffers, the extras -- is bit for bit what it writes
 * without the call; lgs_post_physics_finish and lgs_step_deferred write the same row as lgs_step.
 * This call, lgs_set_task and the other setters may come in any order: every step / reset entry
 * point checks them together -- the layout, finite offsets and scales, head + Wp <= LGS_MAX_OBS,
 * num_privileged_obs == head + Wp + S (the message names the width it would have to be), a
 * non-NULL env->priv_obs for a step -- and refuses with LGS_ERR_ARG before any launch. */
typedef struct lgs_priv_params {
    int32_t enabled;   /* 0: every row is what it is without this call */
    /* {offset, scale} per group: entry = (value - offset) * scale */
    float friction[2], added_mass[2], kp[2], kd[2], strength[2], delay[2];
} lgs_priv_params;

/* ---- per-env buffers of the VecEnv (device pointers; torch owns them) ---- */
typedef struct lgs_env_buffers {
    float* actions;          /* [N,A] in: raw policy actions; out: clipped env.actions (0 on reset) */
    float* last_actions;     /* [N,A] */
    float* last_dof_vel;     /* [N,D] */
    float* last_root_vel;    /* [N,6] */
    float* torques;          /* [N,D] last substep's torques */
    float* commands;         /* [N,4] */
    float* feet_air_time;    /* [N,F] */
    uint8_t* last_contacts;  /* [N,F] bool */
    int64_t* episode_length; /* [N] */
    float* obs;              /* [N,O] */
    float* priv_obs;         /* [N,P] or NULL */
    float* rew;              /* [N]   */
    uint8_t* reset;          /* [N] bool */
    uint8_t* time_out;       /* [N] bool */
    float* episode_sums;     /* [num_rewards(+1 termination), N] */
    float* episode_acc;      /* [num_sums + 1]: sums over envs reset this step, then the count */
    float* base_lin_vel;     /* [N,3] */
    float* base_ang_vel;     /* [N,3] */
    float* projected_gravity;/* [N,3] */
    float* rpy;              /* [N,3] */
    float* env_origins;      /* [N,3] */
    float* phase;            /* [N]   humanoid, else NULL */
    float* leg_phase;        /* [N,2] humanoid, else NULL */
    float* rew_terms;        /* [num_rewards, N] per-term reward of this step (diagnostics) or NULL */
    int64_t* step_counter;   /* [1] device copy of common_step_counter, or NULL.  When set, lgs_step and
                                lgs_reset_all read the Philox step key from it instead of the by-value
                                argument, and lgs_step advances it by one after the step: a captured
                                hipGraph of K steps then draws fresh noise/commands on every replay. */
    /* extras (legged_robot.py:742-768), refreshed by lgs_step after the step when >= 1 env reset;
       each may be NULL.  lgs_step also zeroes episode_acc for the next step.                      */
    float* ep_means;         /* [num_sums] carried extras["episode"] values (rew_* / max_episode_length_s) */
    float* ep_snapshot;      /* [num_sums] this step's copy of ep_means (the step's extras["episode"]) */
    uint8_t* time_outs_carry;/* [N] extras["time_outs"]: time_out of the last step with a reset */
    /* optional [N,A] policy actions read by lgs_step in place of `actions` (which still
       receives the clipped copy, legged_robot.py:623-624): the caller's tensor is read
       directly, with no separate copy launch; NULL: the actions are already in `actions`. */
    const float* actions_in;
    /* optional [num_sums + 1]: the accumulator the NEXT control step adds into, when the caller
       alternates two episode_acc slots (lgs_step_deferred); the extras zero it with episode_acc */
    float* episode_acc_next;
    /* ---- rough terrain (lgs_task_params terrain_curriculum / measure_heights); each may be NULL
     *      when its switch is off ---- */
    int64_t* terrain_levels;        /* [N] the env's level (tile row), live like episode_length */
    const int64_t* terrain_types;   /* [N] the env's tile column */
    const float* terrain_origins;   /* [terrain_rows, terrain_cols, 3] tile origins */
    /* [1] the sum of terrain_levels over all envs, kept exact: a reset env adds its integer level
     * change atomically.  When set (with ep_means), ep_means / ep_snapshot have one more trailing
     * slot [num_sums]: the extras write sum / N there when any env reset
     * (extras["episode"]["terrain_level"], the mean of terrain_levels as in legged_gym). */
    int64_t* terrain_level_sum;
    float* measured_heights;        /* [N, num_height_x * num_height_y] */
} lgs_env_buffers;

typedef struct lgs_sim lgs_sim;

LGS_API const char* lgs_last_error(void);
LGS_API int lgs_version(void);

/* gym.create_sim + load_asset + create_env/actor x N (legged_robot.py:240,328,364-381) */
LGS_API int lgs_create_sim(const lgs_model_desc* model, const lgs_sim_params* params,
                           int32_t num_envs, int32_t device_id, lgs_sim** out);
LGS_API int lgs_destroy_sim(lgs_sim* sim);
LGS_API int lgs_set_stream(lgs_sim* sim, void* hip_stream);
LGS_API int lgs_synchronize(lgs_sim* sim);

/* _process_rigid_shape_props / _process_rigid_body_props (legged_robot.py:412-440, 472-483):
 * per-env shape friction and added root-body mass (host arrays [N]; NULL = unchanged) */
LGS_API int lgs_set_env_properties(lgs_sim* sim, const float* shape_friction, const float* added_base_mass);

/* bind the caller-owned state tensors (acquire_* + wrap_tensor) */
LGS_API int lgs_bind_state(lgs_sim* sim, float* root_states, float* dof_state,
                           float* net_contact_forces, float* rigid_body_states);

/* refresh_* : no-ops kept for API parity (the bound views are written in place) */
LGS_API int lgs_refresh(lgs_sim* sim);

/* set_dof_actuation_force_tensor: torques [N*D] used by the next lgs_simulate */
LGS_API int lgs_set_dof_actuation_force(lgs_sim* sim, const float* torques);
/* gym.simulate: ONE physics substep of every env (dynamics + contact + integrate) */
LGS_API int lgs_simulate(lgs_sim* sim);
/* forward kinematics only: rigid_body_states from root/dof state */
LGS_API int lgs_forward_kinematics(lgs_sim* sim);

/* set_*_tensor_indexed: copy rows `ids` (int32, device) from src into the bound state.
 * When src is the bound buffer itself this is a no-op. */
LGS_API int lgs_set_actor_root_state_indexed(lgs_sim* sim, const float* root_src, const int32_t* ids, int32_t n);
LGS_API int lgs_set_dof_state_indexed(lgs_sim* sim, const float* dof_src, const int32_t* ids, int32_t n);

/* task setup + the fused control step (LeggedRobot.step + post_physics_step) */
LGS_API int lgs_set_task(lgs_sim* sim, const lgs_task_params* task);
LGS_API int lgs_step(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* The two halves of lgs_step, for callers that act between them (a task's Python reward
 * terms) and for parity tests that check each half on its own.  lgs_step is bit-for-bit
 * lgs_step_physics followed by lgs_post_physics with the same step_counter.
 *  - lgs_step_physics: clip actions (legged_robot.py:623-624), decimation x (_compute_torques
 *    :649-671 + one substep :628-639), torques of the last substep, rigid_body_states for tasks
 *    that read them (h1_env.py:49).  No post-physics, no extras, no step-counter advance.
 *  - lgs_post_physics: post_physics_step (:673-709) + extras on the bound state, reading the
 *    clipped actions from env->actions, the last substep's torques from env->torques and the
 *    contact forces from the bound net_contact_forces; advances env->step_counter like lgs_step. */
LGS_API int lgs_step_physics(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
LGS_API int lgs_post_physics(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* lgs_post_physics in two parts around a caller's reward terms (compute_reward, :770-787):
 *  - _rewards: episode length, base-frame state, commands (:681-698), check_termination (:711-721)
 *    and the native reward terms (rew, per-term episode sums, reset/time_out); nothing is reset;
 *  - _finish: reset_idx of the envs whose reset byte is set, push, observations, bookkeeping,
 *    extras (:697-709), reading the base-frame state and commands the first part wrote.
 * lgs_post_physics == _rewards then _finish (without deferred rewards).                        */
LGS_API int lgs_post_physics_rewards(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
LGS_API int lgs_post_physics_finish(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* lgs_post_physics_rewards in two parts around a task's Python _post_physics_step_callback
 * (legged_robot.py:692; the reference's H1Robot / G1Robot override it, h1_env.py:55-65,
 * g1_env.py:56-105):
 *  - _prepare: episode length + 1, base-frame state (:681-690 into env->base_lin_vel,
 *    base_ang_vel, projected_gravity, rpy), the native callback (:488-517: command resampling,
 *    heading; the humanoid gait phase into env->phase / leg_phase);
 *  - _term_rewards: check_termination (:711-721) and the native reward terms on what the env
 *    buffers hold now (commands, phase, leg_phase, base-frame state, episode length).
 * _prepare then _term_rewards == _rewards, bit for bit, when the caller changes nothing.       */
LGS_API int lgs_post_physics_prepare(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
LGS_API int lgs_post_physics_term_rewards(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* reset_idx(all) as used by BaseTask.reset (base_task.py:82-86) */
LGS_API int lgs_reset_all(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* reset_idx(env_ids) (legged_robot.py:723-768) for an arbitrary subset: env_mask is a DEVICE
 * byte per env (nonzero = reset).  Resets dofs/root/commands/buffers of those envs, sets their
 * reset byte, and fills the extras like lgs_step (episode means over the reset envs, carried
 * time-outs); the step counter is not advanced.  With lgs_task_params.terrain_curriculum the
 * reset envs first move their terrain level, as in a control step; a mask byte of 2 resets the
 * env and holds its level (BaseTask.reset: the reset of every env at a runner's construction is
 * no episode end and must not demote the population; lgs_reset_all moves no level either). */
LGS_API int lgs_reset_idx(lgs_sim* sim, const lgs_env_buffers* env, const uint8_t* env_mask, int64_t step_counter);

/* lgs_step with its extras left to the step's consumer: the rollout's next policy launch
 * (include/ppo_mlp.h, pmlp_env_extras: pmlp_rollout_forward / pmlp_store_step_env), which does
 * k_step_extras' work on its own rows and once.  Until the consumer (or lgs_step_extras) has run,
 * env->ep_means / ep_snapshot / time_outs_carry hold the previous step's extras, episode_acc
 * holds this step's sums, last_root_vel[:, 0:2] every env's push draw, and the step counter is
 * not advanced.  The consumer zeroes episode_acc_next, not episode_acc (its other workgroups
 * still read that), so the caller alternates two slots: the next step's episode_acc is this
 * step's episode_acc_next.  lgs_step == lgs_step_deferred then lgs_step_extras, bit for bit.  */
LGS_API int lgs_step_deferred(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
LGS_API int lgs_step_extras(lgs_sim* sim, const lgs_env_buffers* env, int64_t step_counter);
/* the push bookkeeping a deferred step's consumer reads (device pointers owned by the sim):
 * vsim [N, 2] (the simulated xy base velocity before the all-env push draw) and pushed [3]
 * (the push flags of the two step-key parities, then the key of the last control step)      */
LGS_API int lgs_get_push_state(lgs_sim* sim, float** vsim, uint32_t** pushed);

/* gym.add_heightfield -- the rough-terrain ground of legged_gym (utils/terrain.py builds
 * height_field_raw; the reference's create_sim only ever adds the plane, legged_robot.py:240-257).
 * heights: HOST int16 [rows][cols]; sample (i, j) sits at world x = i*horizontal_scale - border_size,
 * y = j*horizontal_scale - border_size, z = heights[i][j]*vertical_scale.  Cell (i, j) is split into
 * two triangles along its (i,j)-(i+1,j+1) diagonal (terrain_utils.convert_heightfield_to_trimesh);
 * contact points are tested against the triangle under them (outside the map: its edge samples).
 * Replaces the z = 0 plane for every env; heights = NULL (or rows = 0) restores the plane. */
LGS_API int lgs_set_heightfield(lgs_sim* sim, const int16_t* heights, int32_t rows, int32_t cols,
                                float horizontal_scale, float vertical_scale, float border_size);

/* the height scan as the tail of the observation rows (lgs_height_obs above); desc = NULL or
 * enabled = 0: the rows are the layout's own (the default) */
LGS_API int lgs_set_height_observations(lgs_sim* sim, const lgs_height_obs* desc);

/* per-env, per-DOF PD gain / motor strength factors and a per-env action delay in the control
 * step (lgs_actuator_rand above).  desc->enabled = 0 turns it off; a NULL sim or desc is an error. */
LGS_API int lgs_set_actuator_randomization(lgs_sim* sim, const lgs_actuator_rand* desc);

/* the last `frames` observation frames as the policy row (lgs_obs_history above).
 * desc->enabled = 0 turns it off; a NULL sim or desc is an error. */
LGS_API int lgs_set_observation_history(lgs_sim* sim, const lgs_obs_history* desc);

/* the randomised parameters as a tail of the privileged row (lgs_priv_params above).
 * desc->enabled = 0 turns it off; a NULL sim or desc is an error. */
LGS_API int lgs_set_privileged_parameters(lgs_sim* sim, const lgs_priv_params* desc);

/* create_actor(..., self_collisions, 0) (legged_robot.py:373-374): the self-collision
 * proxies and pairs of every env (host descriptor, copied; NULL or num_pairs = 0: off) */
LGS_API int lgs_set_self_collision(lgs_sim* sim, const lgs_self_collision_desc* desc);

/* name/index queries (legged_robot.py:332-343, 388-407):
 *  lgs_get_counts     <- get_asset_dof_count / get_asset_rigid_body_count (:332-333)
 *  lgs_get_body_name  <- get_asset_rigid_body_names()[i] (:342); NULL when out of range or unnamed
 *  lgs_get_dof_name   <- get_asset_dof_names()[i] (:343); NULL likewise.  The strings are owned by
 *                        the sim and live until lgs_destroy_sim.
 *  lgs_find_body      <- find_actor_rigid_body_handle(env, actor, name) (:388-407): the body index
 *                        (bodies are env-major, so the index is the same in every env), -1 if absent
 *  lgs_find_dof       <- find_actor_dof_handle: the DOF index, -1 if absent                         */
LGS_API int lgs_get_counts(lgs_sim* sim, int32_t* num_envs, int32_t* num_bodies, int32_t* num_dofs);
LGS_API const char* lgs_get_body_name(lgs_sim* sim, int32_t index);
LGS_API const char* lgs_get_dof_name(lgs_sim* sim, int32_t index);
LGS_API int32_t lgs_find_body(lgs_sim* sim, const char* name);
LGS_API int32_t lgs_find_dof(lgs_sim* sim, const char* name);

/* capacity diagnostics (see the slot order above lgs_self_collision_desc): counts summed
 * over every env and substep of lgs_step / lgs_step_physics / lgs_simulate since the sim was
 * created or last reset:
 *   out[0] touching bodies that got no contact slot
 *   out[1] touching self-collision pairs without a slot
 *   out[2] violated joint limits without a constraint row
 * Synchronises the sim's stream; reset != 0 zeroes the counters afterwards. */
#define LGS_NUM_CONTACT_STATS 3
LGS_API int lgs_get_contact_stats(lgs_sim* sim, uint64_t* out, int32_t reset);

/* the compiled kernel shape the sim runs on: *dofs >= the model's DOFs, *bodies >= its bodies
 * (a robot without an instantiation of its own is padded to the smallest generic one that
 * fits -- inert DOFs and bodies, results bit-identical to the unpadded model), *rows the
 * constraint-row capacity.  Any pointer may be NULL. */
LGS_API int lgs_get_instantiation(lgs_sim* sim, int32_t* dofs, int32_t* bodies, int32_t* rows);

/* the factorisation order of that instantiation: 0 = the joint-space Cholesky eliminates
 * pivots in index order; CH > 0 = the model is D/CH equal chains of CH DOFs on the base and
 * the chain-structured kernel eliminates the chains' pivots level by level (every base-row
 * sum over the joint columns in level order; the CPU oracle takes it via
 * orc_set_factor_chain to reproduce the step bit for bit). */
LGS_API int lgs_get_factor_chain(lgs_sim* sim, int32_t* chain);

/* diagnostics: per-phase s_memtime cycle sums [N][24] of the last lgs_step
 * (only in a library built with -DLGS_PHASE_STAMPS; otherwise LGS_ERR_STATE) */
LGS_API int lgs_debug_set_phase_buffer(void* dev_ptr);

/* counter-based RNG used by every random draw of the step (Philox4x32-10);
 * exposed so tests and the oracle can reproduce the draws bit-exactly. */
LGS_API float lgs_uniform(uint64_t seed, uint32_t env, uint32_t step, uint32_t stream, uint32_t index);

/* random draw streams */
#define LGS_STREAM_NOISE 0u
#define LGS_STREAM_CMD 1u
#define LGS_STREAM_RESET_DOF 2u
#define LGS_STREAM_RESET_ROOT 3u
#define LGS_STREAM_RESET_CMD 4u
#define LGS_STREAM_PUSH 5u
#define LGS_STREAM_TERRAIN 6u
#define LGS_STREAM_ACTUATOR 7u

#endif /* LEGGEDSIM_H */
