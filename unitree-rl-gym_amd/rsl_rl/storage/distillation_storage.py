import torch


class DistillationStorage:
    """The rollout of teacher-student distillation (rsl_rl 2.x's distillation storage, feed-forward):
    per step the student's observation row and the teacher's action on the privileged row.  The
    update walks the steps in time order, so an optimizer step reads a contiguous block of rows."""

    class Transition:
        def __init__(self):
            self.observations = None
            self.privileged_actions = None
            self.dones = None

        def clear(self):
            self.__init__()

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, actions_shape, device="cpu"):
        self.device = device
        self.obs_shape = obs_shape
        self.actions_shape = actions_shape
        T, N = num_transitions_per_env, num_envs
        self.observations = torch.zeros(T, N, *obs_shape, device=device)
        self.privileged_actions = torch.zeros(T, N, *actions_shape, device=device)
        self.dones = torch.zeros(T, N, 1, device=device).byte()
        self.num_transitions_per_env = T
        self.num_envs = N
        self.step = 0

    def add_transitions(self, transition):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        self.observations[self.step].copy_(transition.observations)
        self.privileged_actions[self.step].copy_(transition.privileged_actions)
        if transition.dones is not None:
            self.dones[self.step].copy_(transition.dones.view(-1, 1))
        self.step += 1

    def clear(self):
        self.step = 0
