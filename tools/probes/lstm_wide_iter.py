"""PPO iteration time of the recurrent G1 policy on narrow or wide observation rows:
g1_terrain as registered (47 / 50), or with the height scan in its rows (234 / 237: the cfg edit
g1_terrain_scan registers, spelled out here so that a tree without that task runs it too).
usage: python tools/probes/lstm_wide_iter.py {narrow|scan} num_envs iterations [root]
root: the tree whose package is imported (default: this file's)."""
import copy
import os
import statistics
import sys

ROOT = sys.argv[4] if len(sys.argv) > 4 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "unitree-rl-gym_amd"))

import torch  # noqa: E402
import isaacgym  # noqa: F401,E402
from legged_gym.envs import task_registry  # noqa: E402
from legged_gym.utils import get_args  # noqa: E402
from legged_gym.utils.helpers import class_to_dict  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402

mode, n, iters = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
args = get_args(["--task", "g1_terrain", "--num_envs", str(n), "--headless"])
env_cfg, train_cfg = task_registry.get_cfgs("g1_terrain")
cfg = copy.deepcopy(env_cfg)
if mode == "scan":
    cfg.terrain.scan_in_observations = True
    cfg.env.num_observations, cfg.env.num_privileged_obs = 234, 237
env, _ = task_registry.make_env(name="g1_terrain", args=args, env_cfg=cfg)
runner = OnPolicyRunner(env, class_to_dict(train_cfg), log_dir=None, device="cuda:0")
runner.sync_phase_times = True
rows = []


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def log(locs, width=80, pad=35):
    rows.append((1e3 * locs["collection_time"], 1e3 * locs["learn_time"]))


runner.log, runner.save, runner.writer, runner.log_dir = log, (lambda *a, **k: None), _Writer(), "unused"
runner.learn(iters, init_at_random_ep_len=True)
torch.cuda.synchronize()
alg = runner.alg
rf = alg._rfused
tail = rows[-20:]
col, learn = statistics.median(r[0] for r in tail), statistics.median(r[1] for r in tail)
print(f"{os.path.basename(ROOT) or ROOT} g1_terrain {mode} n={n} obs {env.num_obs}/{env.num_privileged_obs}: "
      f"rfused {rf is not None} mfma {getattr(rf, 'mfma', None)} mfma_step {getattr(alg._rollout, 'mfma_step', None)} "
      f"rollout_graph {runner._rollout_graph is not None}; last {len(tail)} of {iters} iterations: "
      f"iteration {col + learn:.3f} ms, collection+GAE {col:.3f} ms, update {learn:.3f} ms")
