"""StudentTeacher: the policy of teacher-student distillation (rsl_rl 2.x StudentTeacher,
feed-forward).  Two Linear/ELU MLPs: a `student` that reads the policy row and is
trained, and a frozen `teacher` that reads the privileged row and only labels the rollout."""
import torch
import torch.nn as nn
from torch.distributions import Normal

from . import mfma_mlp
from .actor_critic import get_activation, mlp


class StudentTeacher(nn.Module):
    is_recurrent = False

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_hidden_dims=[256, 256, 256],
                 teacher_hidden_dims=[256, 256, 256], activation="elu", init_noise_std=0.1, mixed_precision=True,
                 **kwargs):
        if kwargs:
            print("StudentTeacher.__init__ got unexpected arguments, which will be ignored: " +
                  str([k for k in kwargs]))
        super().__init__()
        act = get_activation(activation)
        self.student = mlp(num_student_obs, student_hidden_dims, num_actions, act)
        self.teacher = mlp(num_teacher_obs, teacher_hidden_dims, num_actions, act)
        # the teacher is a label source: never trained, never in an optimizer
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.teacher.eval()
        print(f"Student MLP: {self.student}")
        print(f"Teacher MLP: {self.teacher}")
        self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        self.distribution = None
        self.mixed_precision = mixed_precision
        self.loaded_teacher = False  # set by load_state_dict; Distillation.update refuses without it

    # `actor` is the student: helpers.export_policy_as_jit and play.py export it as policy_1.pt
    @property
    def actor(self):
        return self.student

    def _run(self, net, x):
        if self.mixed_precision and mfma_mlp.usable(net, x):
            return mfma_mlp.mlp_apply(net, x)  # hand-written bf16 MFMA forward/backward
        return net(x)

    def reset(self, dones=None):
        pass

    def forward(self):
        raise NotImplementedError

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def update_distribution(self, observations):
        mean = self._run(self.student, observations)
        self.distribution = Normal(mean, mean * 0.0 + self.std, validate_args=False)

    def act(self, observations, **kwargs):
        self.update_distribution(observations)
        d = self.distribution  # (= distribution.sample(), capturable: see ActorCritic.act)
        with torch.no_grad():
            return d.mean + d.stddev * torch.randn_like(d.mean)

    def act_inference(self, observations):
        return self._run(self.student, observations)

    def evaluate(self, teacher_observations, **kwargs):
        with torch.no_grad():
            return self._run(self.teacher, teacher_observations)

    def train(self, mode=True):
        super().train(mode)
        self.teacher.eval()  # the teacher stays in evaluation mode (rsl_rl)
        return self

    def load_state_dict(self, state_dict, strict=True):
        """rsl_rl's rule.  A PPO checkpoint (keys `actor.*`): the teacher takes the actor's
        parameters, nothing else is touched, and the run does not resume (returns False).  A
        distillation checkpoint (keys `student.*`): everything is loaded and the run resumes
        (returns True).  Either way loaded_teacher is set."""
        if any(k.startswith("actor.") for k in state_dict):
            teacher = {k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
            self.teacher.load_state_dict(teacher, strict=strict)
            self.loaded_teacher = True
            self.teacher.eval()
            return False
        if any(k.startswith("student.") for k in state_dict):
            super().load_state_dict(state_dict, strict=strict)
            self.loaded_teacher = True
            self.teacher.eval()
            return True
        raise ValueError("StudentTeacher.load_state_dict: neither a PPO checkpoint (actor.*) nor a distillation "
                         "checkpoint (student.*)")
