"""Go2 handstand (reference envs/go2/go2_handstand_env.py:6-423), inside the native step.

The reference class replaces observations, termination, eleven reward terms and the PD law
(a clamp on the rear legs' targets).  Here all of that runs in the fused control step: the
class defines no per-step Python method, only the constants the kernel needs
(`extend_spec`, on the host) and the attributes the reference class exposes.

  observations   LGS_OBS_HANDSTAND: 46 entries, contact flags last (:140-173)
  termination    termination_mode 1: contact, fallen band, time-out (:178-219)
  rewards        the handstand_* / front_* / hind_* / pose / ... ids (:224-383)
  PD clamp       _pd_target_limits: rear_center +- rear_limit on the rear DOFs (:326-350)
  torques        record_unclipped_torques: self.torques is the raw PD torque (:349-350); the
                 joints are driven with the torque clipped to the URDF effort limit (DESIGN)
"""
from types import SimpleNamespace

import numpy as np
import torch

from leggedsim import cabi
from legged_gym.envs.base.humanoid import FeetStateViews
from legged_gym.envs.base.legged_robot import LeggedRobot

FRONT_JOINTS = ("FL_hip_joint", "FL_thigh_joint", "FL_calf_joint", "FR_hip_joint", "FR_thigh_joint", "FR_calf_joint")
REAR_JOINTS = ("RL_hip_joint", "RL_thigh_joint", "RL_calf_joint", "RR_hip_joint", "RR_thigh_joint", "RR_calf_joint")


class GO2HandstandEnv(FeetStateViews, LeggedRobot):
    obs_layout = cabi.OBS_HANDSTAND
    reward_aliases = cabi.HANDSTAND_REWARD_ALIASES
    record_unclipped_torques = True
    uses_rigid_body_states = True      # front_feet_together reads the front feet's rows
    rigid_body_state_bodies = "feet"
    rear_limit = 0.15                  # rad the rear legs' PD targets may leave the handstand pose (:46)
    fallen_band = 0.2                  # |projected_gravity.z| below it: lying on a side (:211-212)
    contact_flag_threshold = 5.0       # N (:146-147, :254, :263)
    contact_flip_prob = 0.01           # observed contact flags, with add_noise (:162)
    feet_together_target = 0.12        # m (:370)
    hind_pose_weight = 0.3             # (:304)

    @classmethod
    def extend_spec(cls, s):
        """The task's constants on the host (derive_env_spec): pose table, rear DOFs and their PD
        target bounds, front / hind feet, front hip DOFs."""
        names = s.dof_names
        idx = {n: i for i, n in enumerate(names)}
        if len(s.feet_indices) < 4:
            raise ValueError("Expected at least 4 feet for Go2.")
        pose = np.asarray(s.default_dof_pos, dtype=np.float32).reshape(-1).copy()
        for name, angle in s.cfg.handstand_pose.joint_angles.items():
            if name in idx:
                pose[idx[name]] = angle
        rear = [idx[n] for n in REAR_JOINTS if n in idx]
        front = [idx[n] for n in FRONT_JOINTS if n in idx]
        lo = np.full(len(names), -np.inf, dtype=np.float32)
        hi = np.full(len(names), np.inf, dtype=np.float32)
        lo[rear] = pose[rear] - np.float32(cls.rear_limit)
        hi[rear] = pose[rear] + np.float32(cls.rear_limit)
        weight = np.zeros(len(names), dtype=np.float32)
        weight[front] = 1.0
        weight[rear] = cls.hind_pose_weight
        s.dof_name_to_idx = idx
        s.rear_dof_idx = rear
        s.pd_target_limits = (lo, hi)
        s.uses_rigid_body_states, s.rigid_body_state_bodies = cls.uses_rigid_body_states, cls.rigid_body_state_bodies
        s.hip_dof_indices = tuple(idx[n] for n in ("FL_hip_joint", "FR_hip_joint"))  # front_hip_neutral
        s.handstand = SimpleNamespace(
            pose_target=pose, pose_weight=weight, num_front_feet=2, fallen_band=cls.fallen_band,
            contact_flag_threshold=cls.contact_flag_threshold, contact_flip_prob=cls.contact_flip_prob,
            feet_together_target=cls.feet_together_target)

    def _init_buffers(self):
        super()._init_buffers()
        hs, dev = self.spec.handstand, self.device
        self.handstand = hs
        self.front_feet_indices = self.feet_indices[[0, 1]]
        self.hind_feet_indices = self.feet_indices[[2, 3]]
        self.dof_name_to_idx = dict(self.spec.dof_name_to_idx)
        self.pose_targets = torch.tensor(hs.pose_target, device=dev).unsqueeze(0).repeat(self.num_envs, 1)
        self.rear_dof_idx = torch.tensor(self.spec.rear_dof_idx, dtype=torch.long, device=dev)
        self.rear_center = self.pose_targets[0, self.rear_dof_idx].clone()

    def _pd_target_limits(self):
        lo = torch.full((self.num_dof,), -float("inf"), device=self.device)
        hi = torch.full((self.num_dof,), float("inf"), device=self.device)
        lo[self.rear_dof_idx] = self.rear_center - self.rear_limit
        hi[self.rear_dof_idx] = self.rear_center + self.rear_limit
        return lo, hi
