from .ppo import PPO
from .distillation import Distillation
