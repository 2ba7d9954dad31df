"""G1 12-DOF humanoid task (reference envs/g1/g1_config.py:3-108)."""
from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO


class G1RoughCfg(LeggedRobotCfg):
    class init_state(LeggedRobotCfg.init_state):
        pos = [0.0, 0.0, 0.8]
        default_joint_angles = {
            "left_hip_yaw_joint": 0.0, "left_hip_roll_joint": 0, "left_hip_pitch_joint": -0.1,
            "left_knee_joint": 0.3, "left_ankle_pitch_joint": -0.2, "left_ankle_roll_joint": 0,
            "right_hip_yaw_joint": 0.0, "right_hip_roll_joint": 0, "right_hip_pitch_joint": -0.1,
            "right_knee_joint": 0.3, "right_ankle_pitch_joint": -0.2, "right_ankle_roll_joint": 0,
            "torso_joint": 0.0,
        }

    class env(LeggedRobotCfg.env):
        num_observations = 47
        num_privileged_obs = 50
        num_actions = 12

    class domain_rand(LeggedRobotCfg.domain_rand):
        randomize_friction = True
        friction_range = [0.1, 1.25]
        randomize_base_mass = True
        added_mass_range = [-1.0, 3.0]
        push_robots = True
        push_interval_s = 5
        max_push_vel_xy = 1.5

    class control(LeggedRobotCfg.control):
        control_type = "P"
        stiffness = {"hip_yaw": 100, "hip_roll": 100, "hip_pitch": 100, "knee": 150, "ankle": 40}
        damping = {"hip_yaw": 2, "hip_roll": 2, "hip_pitch": 2, "knee": 4, "ankle": 2}
        action_scale = 0.25
        decimation = 4

    class asset(LeggedRobotCfg.asset):
        file = "{LEGGED_GYM_ROOT_DIR}/resources/robots/g1_description/g1_12dof.urdf"
        name = "g1"
        foot_name = "ankle_roll"
        penalize_contacts_on = ["hip", "knee"]
        terminate_after_contacts_on = ["pelvis"]
        self_collisions = 0
        flip_visual_attachments = False

    class rewards(LeggedRobotCfg.rewards):
        soft_dof_pos_limit = 0.9
        base_height_target = 0.78

        class scales(LeggedRobotCfg.rewards.scales):
            tracking_lin_vel = 1.0
            tracking_ang_vel = 0.5
            lin_vel_z = -2.0
            ang_vel_xy = -0.05
            orientation = -1.0
            base_height = -10.0
            dof_acc = -2.5e-7
            dof_vel = -1e-3
            feet_air_time = 0.0
            collision = 0.0
            action_rate = -0.01
            dof_pos_limits = -5.0
            alive = 0.15
            hip_pos = -1.0
            contact_no_vel = -0.2
            feet_swing_height = -20.0
            contact = 0.18


class G1RoughCfgPPO(LeggedRobotCfgPPO):
    class policy:
        init_noise_std = 0.8
        actor_hidden_dims = [32]
        critic_hidden_dims = [32]
        activation = "elu"
        rnn_type = "lstm"
        rnn_hidden_size = 64
        rnn_num_layers = 1

    class algorithm(LeggedRobotCfgPPO.algorithm):
        entropy_coef = 0.01

    class runner(LeggedRobotCfgPPO.runner):
        policy_class_name = "ActorCriticRecurrent"
        max_iterations = 10000
        run_name = ""
        experiment_name = "g1"


class G1GruCfgPPO(G1RoughCfgPPO):
    """g1 with a GRU memory (rsl_rl's rnn_type="gru"): three quarters of the LSTM's gate columns
    and no cell state, on the GRU sequence kernels (rsl_rl/modules/gru_seq.py)."""
    class policy(G1RoughCfgPPO.policy):
        rnn_type = "gru"

    class runner(G1RoughCfgPPO.runner):
        experiment_name = "g1_gru"


class G1HeightfieldCfg(G1RoughCfg):
    """BASELINE configs[2]: G1 on the rough-terrain heightfield (utils/terrain.py's
    curriculum map: 10 x 20 tiles of slopes, stairs and obstacles).  The reference
    registers no such task (its create_sim only adds a plane); everything else is
    G1RoughCfg."""

    class terrain(G1RoughCfg.terrain):
        mesh_type = "heightfield"


class G1TerrainCfg(G1HeightfieldCfg):
    """g1_terrain: G1HeightfieldCfg with the rough-terrain path of the fused step on:
    the level curriculum at reset, the height scan, and base_height / feet_swing_height measured
    from the ground instead of world z."""

    class terrain(G1HeightfieldCfg.terrain):
        level_curriculum = True
        scan_heights = True

    class rewards(G1HeightfieldCfg.rewards):
        ground_relative_heights = True


class G1TerrainScanCfg(G1TerrainCfg):
    """g1_terrain_scan: g1_terrain with the 17 x 11 height scan as the tail of the observation
    rows (47 / 50 + 187 = 234 / 237 inputs of the recurrent policy's memories: the wide LSTM
    kernels)."""

    class env(G1TerrainCfg.env):
        num_observations = 234
        num_privileged_obs = 237

    class terrain(G1TerrainCfg.terrain):
        scan_in_observations = True


class G1TerrainScanCfgPPO(G1RoughCfgPPO):
    class runner(G1RoughCfgPPO.runner):
        experiment_name = "g1_terrain_scan"
