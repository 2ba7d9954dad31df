"""Go2 handstand task (reference envs/go2/go2_handstand_config.py:4-207): the front feet carry
the robot, the hind feet stay off the ground, the trunk balances upside down."""
from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO


class GO2HandstandCfg(LeggedRobotCfg):
    class env(LeggedRobotCfg.env):
        num_observations = 46
        num_privileged_obs = 46
        num_actions = 12

    class init_state(LeggedRobotCfg.init_state):
        pos = [0.0, 0.0, 0.28]
        default_joint_angles = {
            "FL_hip_joint": 0.3, "FR_hip_joint": -0.3, "FL_thigh_joint": 1.2, "FR_thigh_joint": 1.2,
            "FL_calf_joint": -2.0, "FR_calf_joint": -2.0,
            "RL_hip_joint": 0.1, "RR_hip_joint": -0.1, "RL_thigh_joint": 0.3, "RR_thigh_joint": 0.3,
            "RL_calf_joint": -1.4, "RR_calf_joint": -1.4,
        }

    class control(LeggedRobotCfg.control):
        control_type = "P"
        stiffness = {"joint": 35.0}
        damping = {"joint": 0.5}
        action_scale = 0.3
        decimation = 5

    class asset(LeggedRobotCfg.asset):
        file = "{LEGGED_GYM_ROOT_DIR}/resources/robots/go2/urdf/go2.urdf"
        name = "go2"
        foot_name = "foot"
        penalize_contacts_on = ["thigh", "calf", "hip"]
        terminate_after_contacts_on = ["base", "thigh", "calf", "hip", "Head_lower", "Head_upper"]
        self_collisions = 1

    class noise(LeggedRobotCfg.noise):
        add_noise = True
        noise_level = 1.0

        class noise_scales(LeggedRobotCfg.noise.noise_scales):
            gyro = 0.2
            gravity = 0.05
            dof_pos = 0.01
            dof_vel = 1.5
            lin_vel = 0.1
            actions = 0.0

    class rewards(LeggedRobotCfg.rewards):
        only_positive_rewards = False
        base_height_target = 0.65
        soft_dof_pos_limit = 0.9

        class scales(LeggedRobotCfg.rewards.scales):
            # the handstand itself
            orientation = 5.0
            base_height = 2.0
            front_feet_contact = 3.0
            hind_feet_no_contact = 3.0
            pose = 10.0
            stability = 1.0
            stay_still = 2.0
            lin_vel_xy = -3
            front_hip_neutral = 2.0
            front_feet_together = 1.5
            # regularisation
            lin_vel_z = -0.001
            ang_vel_xy = -0.005
            torques = -2e-4
            dof_vel = -1e-5
            dof_acc = 0.0
            action_rate = -0.006
            dof_pos_limits = -1.0
            dof_vel_limits = 0.0
            torque_limits = 0.0
            collision = -2.0
            feet_contact_forces = 0.0
            energy = 0.0
            termination = -5.0
            # the walking terms are off
            tracking_lin_vel = 0.0
            tracking_ang_vel = 0.0
            feet_air_time = 0.0
            stumble = 0.0

    class handstand_pose:
        joint_angles = {
            "FL_hip_joint": 0.0, "FL_thigh_joint": -0.89, "FL_calf_joint": -1.5,
            "FR_hip_joint": 0.0, "FR_thigh_joint": -0.89, "FR_calf_joint": -1.5,
            "RL_hip_joint": 0.0, "RL_thigh_joint": 1.7, "RL_calf_joint": -1.853,
            "RR_hip_joint": 0.0, "RR_thigh_joint": 1.7, "RR_calf_joint": -1.853,
        }

    # (carried for a footstand task; nothing reads it)
    class footstand_pose:
        joint_angles = {
            "FL_hip_joint": 0.0, "FL_thigh_joint": 0.82, "FL_calf_joint": -1.6,
            "FR_hip_joint": 0.0, "FR_thigh_joint": 0.82, "FR_calf_joint": -1.68,
            "RL_hip_joint": 0.0, "RL_thigh_joint": 1.82, "RL_calf_joint": -1.16,
            "RR_hip_joint": 0.0, "RR_thigh_joint": 1.82, "RR_calf_joint": -1.16,
        }


class GO2HandstandCfgPPO(LeggedRobotCfgPPO):
    class algorithm(LeggedRobotCfgPPO.algorithm):
        entropy_coef = 0.01

    class runner(LeggedRobotCfgPPO.runner):
        run_name = ""
        experiment_name = "go2_handstand"
