"""Go2 flat-terrain task (reference envs/go2/go2_config.py:3-53)."""
from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO


class GO2RoughCfg(LeggedRobotCfg):
    class init_state(LeggedRobotCfg.init_state):
        pos = [0.0, 0.0, 0.42]
        default_joint_angles = {
            "FL_hip_joint": 0.1, "RL_hip_joint": 0.1, "FR_hip_joint": -0.1, "RR_hip_joint": -0.1,
            "FL_thigh_joint": 0.8, "RL_thigh_joint": 1.0, "FR_thigh_joint": 0.8, "RR_thigh_joint": 1.0,
            "FL_calf_joint": -1.5, "RL_calf_joint": -1.5, "FR_calf_joint": -1.5, "RR_calf_joint": -1.5,
        }

    class control(LeggedRobotCfg.control):
        control_type = "P"
        stiffness = {"joint": 20.0}
        damping = {"joint": 0.5}
        action_scale = 0.25
        decimation = 4

    class asset(LeggedRobotCfg.asset):
        file = "{LEGGED_GYM_ROOT_DIR}/resources/robots/go2/urdf/go2.urdf"
        name = "go2"
        foot_name = "foot"
        penalize_contacts_on = ["thigh", "calf"]
        terminate_after_contacts_on = ["base"]
        self_collisions = 1

    class rewards(LeggedRobotCfg.rewards):
        soft_dof_pos_limit = 0.9
        base_height_target = 0.25

        class scales(LeggedRobotCfg.rewards.scales):
            torques = -0.0002
            dof_pos_limits = -10.0


    class sim(LeggedRobotCfg.sim):
        class physx(LeggedRobotCfg.sim.physx):
            # 5 contact sweeps: the fewest whose solve is within 1 % of the converged one (mean
            # relative error of its velocity change, kinetic-energy norm) on Go2's contacts, open
            # and closed loop (profiles/round6/pgs_sweeps: 0.56 % / 0.83 % at 5, 1.24 % closed at 4)
            pgs_sweeps = 5


class GO2TerrainCfg(GO2RoughCfg):
    """go2_terrain: legged_gym's rough-terrain task on the fused step: the
    curriculum heightfield, the level curriculum at reset, the 17 x 11 height scan as the tail of
    the observation row (48 + 187 = 235 policy inputs) and base_height measured from the ground."""

    class env(GO2RoughCfg.env):
        num_observations = 235

    class terrain(GO2RoughCfg.terrain):
        mesh_type = "heightfield"
        level_curriculum = True
        scan_heights = True
        scan_in_observations = True

    class rewards(GO2RoughCfg.rewards):
        ground_relative_heights = True


class GO2RobustCfg(GO2RoughCfg):
    """go2_robust: the flat-terrain Go2 task with the actuator randomisation of DESIGN 3.11 on:
    per-joint PD gains and motor strength within +-10 %, and 0 to 2 physics substeps (0 to 10 ms)
    of action latency, redrawn for an env at each of its resets."""

    class domain_rand(GO2RoughCfg.domain_rand):
        randomize_kp = True
        randomize_kd = True
        randomize_motor_strength = True
        randomize_action_delay = True


class GO2RobustHistoryCfg(GO2RobustCfg):
    """go2_robust_history: go2_robust with the last 5 observation frames as the policy row
    (5 x 48 = 240 inputs, oldest frame first), so a feed-forward policy can see the
    actuator it is driving."""

    class env(GO2RobustCfg.env):
        history_length = 5
        num_observations = 240


class GO2TerrainRobustCfg(GO2TerrainCfg):
    """go2_terrain_robust: the usual sim-to-real recipe in one task: go2_terrain's
    rough terrain and height scan, go2_robust's actuator randomisation and action latency, and
    the last 5 proprioceptive frames in front of the one current scan (5 x 48 + 187 = 427 policy
    inputs: a history of the head alone, the scan never stored)."""

    class env(GO2TerrainCfg.env):
        history_length = 5
        num_observations = 427

    class domain_rand(GO2TerrainCfg.domain_rand):
        randomize_kp = True
        randomize_kd = True
        randomize_motor_strength = True
        randomize_action_delay = True


class GO2RobustAsymCfg(GO2RobustHistoryCfg):
    """go2_robust_asym: go2_robust_history with an asymmetric critic.  The actor keeps
    its 240 noisy inputs; the critic reads the privileged row: one clean frame (48), the shape
    friction and added base mass (2) and the randomised actuator rows (3 x 12 + 1 = 37), 87 in all."""

    class env(GO2RobustHistoryCfg.env):
        privileged_parameters = True
        num_privileged_obs = 87


class GO2TerrainRobustAsymCfg(GO2TerrainRobustCfg):
    """go2_terrain_robust_asym: go2_terrain_robust with the asymmetric critic: the 427-input actor,
    and a critic on the clean frame, the parameter tail and the clean scan (87 + 187 = 274)."""

    class env(GO2TerrainRobustCfg.env):
        privileged_parameters = True
        num_privileged_obs = 274


class GO2RobustTeacherCfg(GO2RobustAsymCfg):
    """go2_robust_teacher: go2_robust_asym's env presenting its privileged row (87) as the one
    observation row: the teacher of go2_robust_distill."""

    class env(GO2RobustAsymCfg.env):
        privileged_as_observations = True


class GO2TerrainRobustTeacherCfg(GO2TerrainRobustAsymCfg):
    """go2_terrain_robust_teacher: likewise on the terrain task (274 inputs)."""

    class env(GO2TerrainRobustAsymCfg.env):
        privileged_as_observations = True


class GO2RoughCfgPPO(LeggedRobotCfgPPO):
    class algorithm(LeggedRobotCfgPPO.algorithm):
        entropy_coef = 0.01

    class runner(LeggedRobotCfgPPO.runner):
        run_name = ""
        experiment_name = "rough_go2"


class GO2TerrainCfgPPO(GO2RoughCfgPPO):
    class runner(GO2RoughCfgPPO.runner):
        experiment_name = "go2_terrain"


class GO2RobustCfgPPO(GO2RoughCfgPPO):
    class runner(GO2RoughCfgPPO.runner):
        experiment_name = "go2_robust"


class GO2RobustHistoryCfgPPO(GO2RobustCfgPPO):
    class runner(GO2RobustCfgPPO.runner):
        experiment_name = "go2_robust_history"


class GO2TerrainRobustCfgPPO(GO2TerrainCfgPPO):
    class runner(GO2TerrainCfgPPO.runner):
        experiment_name = "go2_terrain_robust"


class GO2RobustAsymCfgPPO(GO2RobustHistoryCfgPPO):
    class runner(GO2RobustHistoryCfgPPO.runner):
        experiment_name = "go2_robust_asym"


class GO2TerrainRobustAsymCfgPPO(GO2TerrainRobustCfgPPO):
    class runner(GO2TerrainRobustCfgPPO.runner):
        experiment_name = "go2_terrain_robust_asym"


class GO2RobustSymCfgPPO(GO2RobustAsymCfgPPO):
    """go2_robust_sym: go2_robust_asym trained with symmetry augmentation: every
    mini-batch together with its left-right mirror image."""

    class algorithm(GO2RobustAsymCfgPPO.algorithm):
        class symmetry_cfg(GO2RobustAsymCfgPPO.algorithm.symmetry_cfg):
            use_data_augmentation = True

    class runner(GO2RobustAsymCfgPPO.runner):
        experiment_name = "go2_robust_sym"


class GO2TerrainRobustSymCfgPPO(GO2TerrainRobustAsymCfgPPO):
    """go2_terrain_robust_sym: go2_terrain_robust_asym with symmetry augmentation."""

    class algorithm(GO2TerrainRobustAsymCfgPPO.algorithm):
        class symmetry_cfg(GO2TerrainRobustAsymCfgPPO.algorithm.symmetry_cfg):
            use_data_augmentation = True

    class runner(GO2TerrainRobustAsymCfgPPO.runner):
        experiment_name = "go2_terrain_robust_sym"


class GO2RobustRndCfgPPO(GO2RobustAsymCfgPPO):
    """go2_robust_rnd: go2_robust_asym with random network distillation on the
    privileged row (87).  The weight is a starting point, not a tuned value: see DESIGN 3.21 for
    the measurement it comes from.  It decays linearly to 0 over the first half of the run (the
    schedule counts env steps: max_iterations / 2 x num_steps_per_env)."""

    class algorithm(GO2RobustAsymCfgPPO.algorithm):
        class rnd_cfg(GO2RobustAsymCfgPPO.algorithm.rnd_cfg):
            weight = 1.4e-5
            weight_schedule = {"mode": "linear", "initial_step": 0, "final_step": 750 * 24, "final_value": 0.0}
            state = "critic"

    class runner(GO2RobustAsymCfgPPO.runner):
        experiment_name = "go2_robust_rnd"


class GO2TerrainRobustRndCfgPPO(GO2TerrainRobustAsymCfgPPO):
    """go2_terrain_robust_rnd: go2_terrain_robust_asym with random network distillation on the
    privileged row (274)."""

    class algorithm(GO2TerrainRobustAsymCfgPPO.algorithm):
        class rnd_cfg(GO2TerrainRobustAsymCfgPPO.algorithm.rnd_cfg):
            weight = 1.5e-5
            weight_schedule = {"mode": "linear", "initial_step": 0, "final_step": 750 * 24, "final_value": 0.0}
            state = "critic"

    class runner(GO2TerrainRobustAsymCfgPPO.runner):
        experiment_name = "go2_terrain_robust_rnd"


class GO2RobustTeacherCfgPPO(GO2RobustAsymCfgPPO):
    """go2_robust_teacher: PPO as go2_robust_asym's, on the privileged row."""

    class runner(GO2RobustAsymCfgPPO.runner):
        experiment_name = "go2_robust_teacher"


class GO2TerrainRobustTeacherCfgPPO(GO2TerrainRobustAsymCfgPPO):
    class runner(GO2TerrainRobustAsymCfgPPO.runner):
        experiment_name = "go2_terrain_robust_teacher"


class GO2RobustDistillCfgPPO(LeggedRobotCfgPPO):
    """go2_robust_distill: the student of go2_robust_teacher on go2_robust_asym's
    env: the student reads the 240 noisy inputs, the frozen teacher the privileged row (87).  One
    optimizer step is 6 x 4096 = 24,576 rows, the mini-batch the GEMM tiles were tuned at."""

    class policy:
        init_noise_std = 0.1
        student_hidden_dims = [512, 256, 128]
        teacher_hidden_dims = [512, 256, 128]
        activation = "elu"

    class algorithm:
        num_learning_epochs = 1
        gradient_length = 6
        learning_rate = 1.0e-3
        max_grad_norm = None
        loss_type = "mse"

        # (every train cfg carries the key; Distillation refuses it switched on)
        class symmetry_cfg(LeggedRobotCfgPPO.algorithm.symmetry_cfg):
            pass

    class runner(LeggedRobotCfgPPO.runner):
        policy_class_name = "StudentTeacher"
        algorithm_class_name = "Distillation"
        experiment_name = "go2_robust_distill"
        # the distillation rollout consumes no deferred env extras: the env keeps its own launch
        defer_env_extras = False
        # the teacher's checkpoint: logs/<teacher_experiment_name>/<teacher_load_run>/model_<n>.pt
        # (-1: the last run / the last checkpoint, as load_run / checkpoint)
        teacher_experiment_name = "go2_robust_teacher"
        teacher_load_run = -1
        teacher_checkpoint = -1


class GO2TerrainRobustDistillCfgPPO(GO2RobustDistillCfgPPO):
    """go2_terrain_robust_distill: 427 student inputs, 274 teacher inputs."""

    class runner(GO2RobustDistillCfgPPO.runner):
        experiment_name = "go2_terrain_robust_distill"
        teacher_experiment_name = "go2_terrain_robust_teacher"
