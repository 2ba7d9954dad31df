from .rollout_storage import RolloutStorage
from .distillation_storage import DistillationStorage
