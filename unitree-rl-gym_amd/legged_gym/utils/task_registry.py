"""Task plugin registry (reference utils/task_registry.py:15-130).

``register(name, task_class, env_cfg, train_cfg)`` is the plugin API new tasks
hook into; ``make_env`` / ``make_alg_runner`` keep their signatures, return
values and ValueError behaviour.  Under ``torch.distributed.run`` both first bind
the rank to its device and join the process group (``distributed.init_from_env``),
so the unmodified ``train.py`` trains data-parallel.
"""
import os
from datetime import datetime
from typing import Tuple

from rsl_rl.env import VecEnv
from rsl_rl.runners import OnPolicyRunner

from legged_gym import LEGGED_GYM_ROOT_DIR
from legged_gym.envs.base.legged_robot_config import LeggedRobotCfg, LeggedRobotCfgPPO

from .distributed import init_from_env
from .helpers import class_to_dict, get_args, get_load_path, parse_sim_params, set_seed, update_cfg_from_args


class TaskRegistry:
    def __init__(self):
        self.task_classes = {}
        self.env_cfgs = {}
        self.train_cfgs = {}

    def register(self, name: str, task_class: VecEnv, env_cfg: LeggedRobotCfg, train_cfg: LeggedRobotCfgPPO):
        self.task_classes[name] = task_class
        self.env_cfgs[name] = env_cfg
        self.train_cfgs[name] = train_cfg

    def get_task_class(self, name: str) -> VecEnv:
        return self.task_classes[name]

    def get_cfgs(self, name) -> Tuple[LeggedRobotCfg, LeggedRobotCfgPPO]:
        env_cfg, train_cfg = self.env_cfgs[name], self.train_cfgs[name]
        env_cfg.seed = train_cfg.seed
        return env_cfg, train_cfg

    def make_env(self, name, args=None, env_cfg=None) -> Tuple[VecEnv, LeggedRobotCfg]:
        if args is None:
            args = get_args()
        if name not in self.task_classes:
            raise ValueError(f"Task with name: {name} was not registered")
        init_from_env(args)  # WORLD_SIZE > 1: this rank's device into args, process group
        task_class = self.get_task_class(name)
        if env_cfg is None:
            env_cfg, _ = self.get_cfgs(name)
        env_cfg, _ = update_cfg_from_args(env_cfg, None, args)
        set_seed(env_cfg.seed)
        sim_params = parse_sim_params(args, {"sim": class_to_dict(env_cfg.sim)})
        env = task_class(cfg=env_cfg, sim_params=sim_params, physics_engine=args.physics_engine,
                         sim_device=args.sim_device, headless=args.headless)
        return env, env_cfg

    def make_alg_runner(self, env, name=None, args=None, train_cfg=None,
                        log_root="default") -> Tuple[OnPolicyRunner, LeggedRobotCfgPPO]:
        if args is None:
            args = get_args()
        if train_cfg is None:
            if name is None:
                raise ValueError("Either 'name' or 'train_cfg' must be not None")
            _, train_cfg = self.get_cfgs(name)
        elif name is not None:
            print(f"'train_cfg' provided -> Ignoring 'name={name}'")
        _, train_cfg = update_cfg_from_args(None, train_cfg, args)
        init_from_env(args)
        stamp = datetime.now().strftime("%b%d_%H-%M-%S") + "_" + train_cfg.runner.run_name
        if log_root == "default":
            log_root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", train_cfg.runner.experiment_name)
            log_dir = os.path.join(log_root, stamp)
        elif log_root is None:
            log_dir = None
        else:
            log_dir = os.path.join(log_root, stamp)
        runner = OnPolicyRunner(env, class_to_dict(train_cfg), log_dir, device=args.rl_device)
        teacher_name = getattr(train_cfg.runner, "teacher_experiment_name", None)
        if teacher_name and train_cfg.runner.algorithm_class_name == "Distillation" and not train_cfg.runner.resume:
            # distillation: the frozen teacher comes from the teacher task's run (a
            # resumed run, play.py included, takes it from its own checkpoint's teacher.*)
            teacher_root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", teacher_name)
            teacher_path = get_load_path(teacher_root, load_run=getattr(train_cfg.runner, "teacher_load_run", -1),
                                         checkpoint=getattr(train_cfg.runner, "teacher_checkpoint", -1))
            print(f"Loading teacher from: {teacher_path}")
            runner.load_teacher(teacher_path)
        if train_cfg.runner.resume:
            resume_path = get_load_path(log_root, load_run=train_cfg.runner.load_run,
                                        checkpoint=train_cfg.runner.checkpoint)
            print(f"Loading model from: {resume_path}")
            runner.load(resume_path)
        return runner, train_cfg


task_registry = TaskRegistry()
