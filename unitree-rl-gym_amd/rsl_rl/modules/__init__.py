from .actor_critic import ActorCritic
from .actor_critic_recurrent import ActorCriticRecurrent
from .student_teacher import StudentTeacher
from .rnd import RandomNetworkDistillation
