"""The learning record of teacher-student distillation: train a teacher task with
PPO, then its student task from the teacher's checkpoint, printing per iteration the behaviour
loss, the mean episode length and the tracking rewards of the episodes that ended; then the
device-synchronised iteration times of the student task next to a PPO task's.
usage: python tools/distill_record.py teacher_task teacher_iters student_task student_iters envs [ppo_task]"""
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "unitree-rl-gym_amd"))

import torch  # noqa: E402

import isaacgym  # noqa: F401,E402
from legged_gym.envs import task_registry  # noqa: E402
from legged_gym.utils import get_args  # noqa: E402
from legged_gym.utils.helpers import class_to_dict  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402

TRACK = ("rew_tracking_lin_vel", "rew_tracking_ang_vel")


def build(task, n):
    args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
    env, _ = task_registry.make_env(name=task, args=args)
    runner = OnPolicyRunner(env, class_to_dict(task_registry.get_cfgs(task)[1]), log_dir=None, device="cuda:0")
    return env, runner


def train(task, env, runner, iters, losses=None):
    print(f"{task} x{env.num_envs}: {iters} iterations", flush=True)
    for it in range(iters):
        runner.learn(1)
        ep = float(env._episode_length.float().mean())
        track = " ".join(f"{k[4:]} {float(env.extras['episode'][k]):+.4f}" for k in TRACK if k in env.extras["episode"])
        if it % 10 == 0 or it == iters - 1:
            loss = "" if losses is None else f"behaviour loss {losses[-1]:.6f}  "
            print(f"it {it:4d} {loss}mean episode length {ep:7.1f}  {track}", flush=True)


def timing(task, env, runner, warm=5, count=20):
    runner.sync_phase_times = True
    runner.learn(warm)
    col, upd = [], []
    for _ in range(count):
        runner.learn(1)
        c, u = runner.last_iteration_times
        col.append(1e3 * c)
        upd.append(1e3 * u)
    tot = [a + b for a, b in zip(col, upd)]
    print(f"{task} x{env.num_envs}: median of {count} iterations after {warm}: iteration {statistics.median(tot):.3f} ms, "
          f"collection {statistics.median(col):.3f} ms, update {statistics.median(upd):.3f} ms", flush=True)


def kernel_times(n, A=12, O=240, G=6, reps=200):
    """The two kernels of csrc/distill.hip alone, at the student task's shapes (device events)."""
    from rsl_rl.modules import mfma_mlp as mm
    dev, M = "cuda", G * n
    mu, tg = torch.randn(M, A, device=dev), torch.randn(M, A, device=dev)
    part = torch.empty(mm.load().pmlp_distill_loss_parts(M), device=dev)
    stats, dz = torch.empty(4, device=dev), torch.empty(M, 16, dtype=torch.bfloat16, device=dev)
    obs, std = torch.randn(n, O, device=dev), torch.full((A,), 0.1, device=dev)
    act, so, stt = torch.empty(n, A, device=dev), torch.empty(n, O, device=dev), torch.empty(n, A, device=dev)
    draw = torch.zeros(2, dtype=torch.int64, device=dev)
    jobs = (("pmlp_distill_loss_step (rows + finish)", f"{M} x {A}",
             lambda k: mm.distill_loss_step(mu, tg, "mse", 1.0 / (n * A), part, stats, dz)),
            ("pmlp_distill_act", f"{n} x {A}, O = {O}",
             lambda k: mm.distill_act(mu[:n], tg[:n], std, obs, draw, k % 2, 1, act, so, stt)))
    for name, shape, fn in jobs:
        for k in range(10):
            fn(k)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(reps):
            fn(k)
        t1.record()
        torch.cuda.synchronize()
        print(f"{name} at {shape}: {1e3 * t0.elapsed_time(t1) / reps:.2f} us per call "
              f"({reps} back-to-back calls, launch overhead included)", flush=True)


def main(teacher_task, teacher_iters, student_task, student_iters, n, ppo_task=None):
    env, runner = build(teacher_task, n)
    train(teacher_task, env, runner, teacher_iters)
    path = os.path.join(tempfile.mkdtemp(), f"model_{teacher_iters}.pt")
    runner.save(path)
    env.close()
    env, runner = build(student_task, n)
    runner.load_teacher(path)
    losses, update = [], runner.alg.update

    def recorded(host_means=True):
        losses.append(update(host_means=True))
        return losses[-1]
    runner.alg.update = recorded
    train(student_task, env, runner, student_iters, losses)
    print("behaviour loss per iteration: " + " ".join(f"{v:.5f}" for v in losses), flush=True)
    runner.alg.update = update
    timing(student_task, env, runner)
    env.close()
    if ppo_task:
        env, runner = build(ppo_task, n)
        timing(ppo_task, env, runner)
        env.close()
    kernel_times(n)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]),
         sys.argv[6] if len(sys.argv) > 6 else None)
