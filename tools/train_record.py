"""Training record: N PPO iterations of a task, one CSV row per iteration with the mean over the
iteration's steps of the extras["episode"] keys in KEYS and the mean reward / episode length of the
finished episodes (the runner's 100-episode buffers); a key the task does not log stays empty.
usage: python tools/train_record.py task iterations num_envs out.csv"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unitree-rl-gym_amd"))

import torch  # noqa: E402
import isaacgym  # noqa: F401,E402
from legged_gym.envs import task_registry  # noqa: E402
from legged_gym.utils import get_args  # noqa: E402
from legged_gym.utils.helpers import class_to_dict  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402

task, iters, n, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
env, _ = task_registry.make_env(name=task, args=args)
_, train_cfg = task_registry.get_cfgs(task)
runner = OnPolicyRunner(env, class_to_dict(train_cfg), log_dir=None, device="cuda:0")
runner.sync_phase_times = True
KEYS = ["terrain_level", "rew_base_height", "rew_feet_swing_height", "mean_reward", "mean_episode_length"]
rows = []


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def log(locs, width=80, pad=35):
    row = {"it": locs["it"], "collection_ms": 1e3 * locs["collection_time"], "learn_ms": 1e3 * locs["learn_time"]}
    if locs["ep_infos"]:
        for key in locs["ep_infos"][0]:
            row[key] = float(torch.stack([torch.as_tensor(e[key]).float().reshape(()) for e in locs["ep_infos"]]).mean())
    if len(locs["rewbuffer"]) > 0:
        row["mean_reward"] = statistics.mean(locs["rewbuffer"])
        row["mean_episode_length"] = statistics.mean(locs["lenbuffer"])
    rows.append(row)


runner.log, runner.save, runner.writer, runner.log_dir = log, (lambda *a, **k: None), _Writer(), "unused"
runner.learn(iters, init_at_random_ep_len=True)
torch.cuda.synchronize()
keys = KEYS
with open(out, "w") as f:
    f.write(",".join(["it"] + keys) + "\n")
    for r in rows:
        f.write(",".join([str(r["it"])] + ["%.6g" % r[k] if k in r else "" for k in keys]) + "\n")
for r in (rows[0], rows[len(rows) // 2], rows[-1]):
    print(task, "it", r["it"], {k: round(r[k], 5) for k in keys if k in r})
tail = rows[-20:]
print(task, "last 20 iterations: collection %.2f ms, learn %.2f ms" % (
    statistics.median(r["collection_ms"] for r in tail), statistics.median(r["learn_ms"] for r in tail)))
if hasattr(env, "terrain_levels") and "terrain_level" in rows[-1]:
    print(task, "levels histogram", torch.bincount(env.terrain_levels, minlength=10).tolist())
