"""PPO iteration time of the recurrent G1 policy with an LSTM or a GRU memory.
usage: python tools/probes/gru_iter.py {lstm|gru} num_envs iterations [root]
The g1 task with policy.rnn_type set here, so that a tree without the g1_gru task runs the GRU
too (there: torch's nn.GRU per step, the padded generator and the eager update).
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

kind, n, iters = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
args = get_args(["--task", "g1", "--num_envs", str(n), "--headless"])
env_cfg, train_cfg = task_registry.get_cfgs("g1")
env, _ = task_registry.make_env(name="g1", args=args, env_cfg=copy.deepcopy(env_cfg))
cfg = class_to_dict(train_cfg)
cfg["policy"]["rnn_type"] = kind
runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
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
tail = rows[-(2 * iters // 3):]
col, learn = statistics.median(r[0] for r in tail), statistics.median(r[1] for r in tail)
graph = alg._graph is not None or getattr(alg, "_rgraph", None) is not None
print(f"{os.path.basename(ROOT) or ROOT} g1 {kind} n={n}: dense {alg._dense_recurrent} rfused {alg._rfused is not None} "
      f"update_graph {graph} rollout_graph {runner._rollout_graph is not None}; "
      f"last {len(tail)} of {iters} iterations: iteration {col + learn:.3f} ms, collection+GAE {col:.3f} ms, "
      f"update {learn:.3f} ms")
