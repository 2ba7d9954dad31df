"""Task registration (reference envs/__init__.py:1-27): the plugin API."""
from legged_gym import LEGGED_GYM_ROOT_DIR, LEGGED_GYM_ENVS_DIR  # noqa: F401

from legged_gym.envs.go2.go2_config import GO2RobustRndCfgPPO, GO2TerrainRobustRndCfgPPO
from legged_gym.envs.go2.go2_config import (GO2RobustDistillCfgPPO, GO2RobustTeacherCfg, GO2RobustTeacherCfgPPO,
                                            GO2TerrainRobustDistillCfgPPO, GO2TerrainRobustTeacherCfg,
                                            GO2TerrainRobustTeacherCfgPPO)
from legged_gym.envs.go2.go2_config import (GO2RobustAsymCfg, GO2RobustAsymCfgPPO, GO2RobustCfg, GO2RobustCfgPPO,
                                            GO2RobustHistoryCfg, GO2RobustHistoryCfgPPO, GO2RobustSymCfgPPO,
                                            GO2RoughCfg, GO2RoughCfgPPO, GO2TerrainCfg, GO2TerrainCfgPPO,
                                            GO2TerrainRobustAsymCfg, GO2TerrainRobustAsymCfgPPO, GO2TerrainRobustCfg,
                                            GO2TerrainRobustCfgPPO, GO2TerrainRobustSymCfgPPO)
from legged_gym.envs.go2.go2_handstand_config import GO2HandstandCfg, GO2HandstandCfgPPO
from legged_gym.envs.go2.go2_handstand_env import GO2HandstandEnv
from legged_gym.envs.h1.h1_config import H1RoughCfg, H1RoughCfgPPO
from legged_gym.envs.h1.h1_env import H1Robot
from legged_gym.envs.h1_2.h1_2_config import H1_2RoughCfg, H1_2RoughCfgPPO
from legged_gym.envs.h1_2.h1_2_env import H1_2Robot
from legged_gym.envs.g1.g1_config import (G1GruCfgPPO, G1HeightfieldCfg, G1RoughCfg, G1RoughCfgPPO, G1TerrainCfg,
                                          G1TerrainScanCfg, G1TerrainScanCfgPPO)
from legged_gym.envs.g1.g1_env import G1Robot
from .base.legged_robot import LeggedRobot
from .base.privileged_actor import PrivilegedActorRobot

from legged_gym.utils.task_registry import task_registry

task_registry.register("go2", LeggedRobot, GO2RoughCfg(), GO2RoughCfgPPO())
task_registry.register("go2_terrain", LeggedRobot, GO2TerrainCfg(), GO2TerrainCfgPPO())
task_registry.register("go2_robust", LeggedRobot, GO2RobustCfg(), GO2RobustCfgPPO())
task_registry.register("go2_robust_history", LeggedRobot, GO2RobustHistoryCfg(), GO2RobustHistoryCfgPPO())
task_registry.register("go2_terrain_robust", LeggedRobot, GO2TerrainRobustCfg(), GO2TerrainRobustCfgPPO())
task_registry.register("go2_robust_asym", LeggedRobot, GO2RobustAsymCfg(), GO2RobustAsymCfgPPO())
task_registry.register("go2_terrain_robust_asym", LeggedRobot, GO2TerrainRobustAsymCfg(), GO2TerrainRobustAsymCfgPPO())
task_registry.register("go2_robust_sym", LeggedRobot, GO2RobustAsymCfg(), GO2RobustSymCfgPPO())
task_registry.register("go2_terrain_robust_sym", LeggedRobot, GO2TerrainRobustAsymCfg(), GO2TerrainRobustSymCfgPPO())
task_registry.register("go2_robust_rnd", LeggedRobot, GO2RobustAsymCfg(), GO2RobustRndCfgPPO())
task_registry.register("go2_terrain_robust_rnd", LeggedRobot, GO2TerrainRobustAsymCfg(), GO2TerrainRobustRndCfgPPO())
task_registry.register("go2_robust_teacher", PrivilegedActorRobot, GO2RobustTeacherCfg(), GO2RobustTeacherCfgPPO())
task_registry.register("go2_terrain_robust_teacher", PrivilegedActorRobot, GO2TerrainRobustTeacherCfg(),
                       GO2TerrainRobustTeacherCfgPPO())
task_registry.register("go2_robust_distill", LeggedRobot, GO2RobustAsymCfg(), GO2RobustDistillCfgPPO())
task_registry.register("go2_terrain_robust_distill", LeggedRobot, GO2TerrainRobustAsymCfg(),
                       GO2TerrainRobustDistillCfgPPO())
task_registry.register("go2_handstand", GO2HandstandEnv, GO2HandstandCfg(), GO2HandstandCfgPPO())
task_registry.register("h1", H1Robot,H1RoughCfg(), H1RoughCfgPPO())
task_registry.register("h1_2", H1_2Robot, H1_2RoughCfg(), H1_2RoughCfgPPO())
task_registry.register("g1", G1Robot, G1RoughCfg(), G1RoughCfgPPO())
task_registry.register("g1_gru", G1Robot, G1RoughCfg(), G1GruCfgPPO())
task_registry.register("g1_rough", G1Robot, G1HeightfieldCfg(), G1RoughCfgPPO())
task_registry.register("g1_terrain", G1Robot, G1TerrainCfg(), G1RoughCfgPPO())
task_registry.register("g1_terrain_scan", G1Robot, G1TerrainScanCfg(), G1TerrainScanCfgPPO())
