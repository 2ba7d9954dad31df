"""Default env / PPO configuration (values of the reference's
envs/base/legged_robot_config.py:51-286; attribute names are API)."""
from .base_config import BaseConfig


class LeggedRobotCfg(BaseConfig):
    class env:
        num_envs = 4096
        num_observations = 48
        num_privileged_obs = None  # not None -> step() also returns critic observations
        # history_length H > 1: the policy row is the env's last H observation frames,
        # oldest first, built inside the native step (an episode's first row repeats its frame);
        # num_observations is then H x the layout's own width.  1: off.
        history_length = 1
        # privileged_parameters: the privileged (critic) row carries the randomised
        # parameters -- shape friction, added base mass and, with the actuator randomisation on, the
        # per-DOF kp / kd / strength factors and the action delay -- each mapped to [-1, 1] over its
        # range.  num_privileged_obs is then the layout's privileged head (the quadruped's clean
        # frame, 12 + 3 A; the humanoid's 14 + 3 A) + the tail + the scan's points.  False: off.
        privileged_parameters = False
        # privileged_as_observations (envs/base/privileged_actor.py): the env presents
        # its privileged row as THE observation and no privileged row (a teacher task: actor and
        # critic share the clean row).  False: off.
        privileged_as_observations = False
        num_actions = 12
        env_spacing = 3.0          # plane grid spacing [m]
        send_timeouts = True       # extras["time_outs"] for value bootstrapping
        episode_length_s = 20
        test = False

    class terrain:
        mesh_type = "plane"  # the reference env always builds a plane (legged_robot.py:240-242)
        horizontal_scale = 0.1
        vertical_scale = 0.005
        border_size = 25
        curriculum = True
        static_friction = 1.0
        dynamic_friction = 1.0
        restitution = 0.0
        measure_heights = True
        measured_points_x = [-0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
        measured_points_y = [-0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
        selected = False
        terrain_kwargs = None
        max_init_terrain_level = 5
        terrain_length = 8.0
        terrain_width = 8.0
        num_rows = 10
        num_cols = 20
        terrain_proportions = [0.1, 0.1, 0.35, 0.25, 0.2]
        slope_treshold = 0.75
        # rough-terrain switches of the fused step, off by default; none works on a plane
        # level_curriculum: a resetting env moves up / down a tile row (legged_gym's
        # _update_terrain_curriculum).  `curriculum` above only lays the map out in difficulty rows.
        level_curriculum = False
        # scan_heights: env.measured_heights [N, len(x) * len(y)] of measured_points_x / _y every step
        scan_heights = False
        # scan_in_observations (needs scan_heights): the scan is the tail of the observation
        # rows, legged_gym's clip(root_z - 0.5 - measured_heights, -1, 1) * obs_scales.height_measurements;
        # env.num_observations (and num_privileged_obs of the humanoid layout) then count the
        # len(x) * len(y) points after the layout's own entries.  (measure_heights above is inert.)
        scan_in_observations = False

    class commands:
        curriculum = False
        max_curriculum = 1.0
        num_commands = 4        # lin_vel_x, lin_vel_y, ang_vel_yaw, heading
        resampling_time = 10.0  # [s]
        heading_command = True  # yaw rate derived from the heading error

        class ranges:
            lin_vel_x = [-1.0, 1.0]
            lin_vel_y = [-1.0, 1.0]
            ang_vel_yaw = [-1, 1]
            heading = [-3.14, 3.14]

    class init_state:
        pos = [0.0, 0.0, 1.0]
        rot = [0.0, 0.0, 0.0, 1.0]  # x, y, z, w
        lin_vel = [0.0, 0.0, 0.0]
        ang_vel = [0.0, 0.0, 0.0]
        default_joint_angles = {"joint_a": 0.0, "joint_b": 0.0}

    class control:
        control_type = "P"  # P position, V velocity, T torque
        stiffness = {"joint_a": 10.0, "joint_b": 15.0}
        damping = {"joint_a": 1.0, "joint_b": 1.5}
        action_scale = 0.5
        decimation = 4

    class asset:
        file = ""
        name = "legged_robot"
        foot_name = "None"
        penalize_contacts_on = []
        terminate_after_contacts_on = []
        disable_gravity = False
        collapse_fixed_joints = True
        fix_base_link = False
        default_dof_drive_mode = 3
        self_collisions = 0
        replace_cylinder_with_capsule = True
        flip_visual_attachments = True
        density = 0.001
        angular_damping = 0.0
        linear_damping = 0.0
        max_angular_velocity = 1000.0
        max_linear_velocity = 1000.0
        armature = 0.0
        thickness = 0.01

    class domain_rand:
        randomize_friction = True
        friction_range = [0.5, 1.25]
        randomize_base_mass = False
        added_mass_range = [-1.0, 1.0]
        push_robots = True
        push_interval_s = 15
        max_push_vel_xy = 1.0
        # actuator randomisation inside the native step, all off by default: a factor
        # per env and joint on the PD gains and on the motor strength, and a per-env delay of the
        # action in physics substeps (0 .. control.decimation); an env redraws its rows when it
        # resets unless actuator_resample_on_reset is False (the tensors are then only read)
        randomize_kp = False
        kp_range = [0.9, 1.1]
        randomize_kd = False
        kd_range = [0.9, 1.1]
        randomize_motor_strength = False
        motor_strength_range = [0.9, 1.1]
        randomize_action_delay = False
        action_delay_range = [0, 2]
        actuator_resample_on_reset = True

    class rewards:
        class scales:
            termination = -0.0
            tracking_lin_vel = 1.0
            tracking_ang_vel = 0.5
            lin_vel_z = -2.0
            ang_vel_xy = -0.05
            orientation = -0.0
            torques = -0.00001
            dof_vel = -0.0
            dof_acc = -2.5e-7
            base_height = -0.0
            feet_air_time = 1.0
            collision = -1.0
            feet_stumble = -0.0
            action_rate = -0.01
            stand_still = -0.0

        only_positive_rewards = True
        tracking_sigma = 0.25
        soft_dof_pos_limit = 1.0
        soft_dof_vel_limit = 1.0
        soft_torque_limit = 1.0
        base_height_target = 1.0
        max_contact_force = 100.0
        # base_height and feet_swing_height measure from the ground under the robot, not from
        # world z = 0 (needs terrain.scan_heights)
        ground_relative_heights = False

    class normalization:
        class obs_scales:
            lin_vel = 2.0
            ang_vel = 0.25
            dof_pos = 1.0
            dof_vel = 0.05
            height_measurements = 5.0

        clip_observations = 100.0
        clip_actions = 100.0

    class noise:
        add_noise = True
        noise_level = 1.0

        class noise_scales:
            dof_pos = 0.01
            dof_vel = 1.5
            lin_vel = 0.1
            ang_vel = 0.2
            gravity = 0.05
            height_measurements = 0.1

    class viewer:
        ref_env = 0
        pos = [10, 0, 6]
        lookat = [11.0, 5, 3.0]

    class sim:
        dt = 0.005
        substeps = 1
        gravity = [0.0, 0.0, -9.81]
        up_axis = 1  # 1 = z

        class physx:
            num_threads = 10
            solver_type = 1
            num_position_iterations = 4
            num_velocity_iterations = 0
            contact_offset = 0.01
            rest_offset = 0.0
            bounce_threshold_velocity = 0.5
            max_depenetration_velocity = 1.0
            max_gpu_contact_pairs = 2 ** 23
            default_buffer_size_multiplier = 5
            contact_collection = 2
            # (this build) Gauss-Seidel sweeps of the contact solve per substep; None: the budget
            # 2 x num_position_iterations + num_velocity_iterations.  A task sets the fewest sweeps
            # that meet the convergence bar on its own contacts (tools/pgs_sweeps)
            pgs_sweeps = None


class LeggedRobotCfgPPO(BaseConfig):
    seed = 1
    runner_class_name = "OnPolicyRunner"

    class policy:
        init_noise_std = 1.0
        actor_hidden_dims = [512, 256, 128]
        critic_hidden_dims = [512, 256, 128]
        activation = "elu"

    class algorithm:
        value_loss_coef = 1.0
        use_clipped_value_loss = True
        clip_param = 0.2
        entropy_coef = 0.01
        num_learning_epochs = 5
        num_mini_batches = 4
        learning_rate = 1.0e-3
        schedule = "adaptive"
        gamma = 0.99
        lam = 0.95
        desired_kl = 0.01
        max_grad_norm = 1.0

        # left-right symmetry (rsl_rl 2.x's names).  use_data_augmentation: every
        # mini-batch is trained together with its mirror image, built from the env's
        # symmetry_tables().  use_mirror_loss is refused (not built yet).
        class symmetry_cfg:
            use_data_augmentation = False
            use_mirror_loss = False
            mirror_loss_coeff = 0.0

        # random network distillation (rsl_rl 2.x's names): an exploration bonus
        # weight * ||target(s) - predictor(s)||_2 added to the rewards of every rollout.  weight 0
        # with no schedule: off.  state: the stored row the nets read, "critic" (the privileged
        # row where there is one) or "policy".  The two normalisers are refused (not built yet).
        class rnd_cfg:
            weight = 0.0
            weight_schedule = None
            learning_rate = 1.0e-3
            num_outputs = 16
            predictor_hidden_dims = [256, 128, 64]
            target_hidden_dims = [256, 128, 64]
            reward_normalization = False
            state_normalization = False
            state = "critic"

    class runner:
        policy_class_name = "ActorCritic"
        algorithm_class_name = "PPO"
        num_steps_per_env = 24
        max_iterations = 1500
        save_interval = 50
        # running mean / variance of the observation rows, applied before the policy and the
        # critic see them (rsl_rl's EmpiricalNormalization); `_until`: rows after which the
        # statistics freeze (None: never)
        empirical_normalization = False
        empirical_normalization_until = None
        experiment_name = "test"
        run_name = ""
        resume = False
        load_run = -1
        checkpoint = -1
        resume_path = None
