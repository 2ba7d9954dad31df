"""The record of random network distillation.

  measure  task envs        one iteration of an RND task at weight 1: the mean unweighted error of
                            the fresh nets and the mean absolute step reward without the bonus
                            (what the task's weight is chosen from)
  learn    task base iters envs   train the RND task and its parent task, printing per iteration the
                            mean episode length, the tracking rewards of the episodes that ended,
                            and for the RND task the mean bonus and Loss/rnd
  time     task base envs   device-synchronised iteration times of both tasks in one process, then
                            the two kernels of csrc/rnd.hip alone
usage: python tools/rnd_record.py measure|learn|time ..."""
import copy
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

TRACK = ("rew_tracking_lin_vel", "rew_tracking_ang_vel")


def build(task, n, rnd=None):
    args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
    env, _ = task_registry.make_env(name=task, args=args)
    cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(task)[1]))
    if rnd:
        cfg["algorithm"]["rnd_cfg"].update(rnd)
    torch.manual_seed(cfg["seed"])
    torch.cuda.manual_seed(cfg["seed"])
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    return env, runner


def measure(task, n):
    env, runner = build(task, n, dict(weight=1.0, weight_schedule=None))
    alg = runner.alg
    assert alg._rnd_pass is not None, "the fused RND pieces are not active"
    T = runner.num_steps_per_env
    alg._rnd_pass.intrinsic = torch.zeros(T * n, device="cuda:0")
    seen = {}
    gae = alg.compute_returns

    def spy(last):
        gae(last)
        rew = alg.storage.rewards.flatten()
        seen["abs"] = float((rew - alg._rnd_pass.intrinsic).abs().mean())
        seen["err"], seen["bonus"] = float(alg._rnd_stats[1]), float(alg._rnd_stats[0])
    alg.compute_returns = spy
    runner.learn(1)
    print(f"{task} x{n}, iteration 0, weight 1: mean unweighted error {seen['err']:.6f} (mean bonus "
          f"{seen['bonus']:.6f}); mean |step reward| without the bonus {seen['abs']:.6f}; a tenth of it over the "
          f"error: weight {0.1 * seen['abs'] / seen['err']:.6f}", flush=True)
    env.close()


def train(task, env, runner, iters):
    print(f"{task} x{env.num_envs}: {iters} iterations", flush=True)
    alg = runner.alg
    rnd = getattr(alg, "rnd", None) is not None
    for it in range(iters):
        runner.learn(1)
        if it % 10 == 0 or it == iters - 1:
            ep = float(env._episode_length.float().mean())
            track = " ".join(f"{k[4:]} {float(env.extras['episode'][k]):+.4f}" for k in TRACK
                             if k in env.extras["episode"])
            extra = ""
            if rnd:
                extra = (f"  mean bonus {float(alg._rnd_stats[0]):.3e} (weight {alg.rnd.weight:.3e}, error "
                         f"{float(alg._rnd_stats[1]):.5f})  Loss/rnd {float(alg.rnd_loss_mean):.3e}")
            print(f"it {it:4d} mean episode length {ep:7.1f}  {track}{extra}", flush=True)


def learn(task, base, iters, n):
    for name in (task, base):
        env, runner = build(name, n)
        train(name, env, runner, iters)
        env.close()


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
          f"collection {statistics.median(col):.3f} ms, returns + update {statistics.median(upd):.3f} ms", flush=True)


def kernel_times(n, T=24, E=16, mbs=4, reps=200):
    """The two kernels of csrc/rnd.hip alone, at the task's shapes (device events)."""
    from rsl_rl.modules import mfma_mlp as mm
    dev, R = "cuda", T * n
    M = R // mbs
    pred, tgt = torch.randn(R, E, device=dev), torch.randn(R, E, device=dev)
    w, rew = torch.full((T,), 0.01, device=dev), torch.zeros(R, device=dev)
    part, stats = torch.empty(2 * mm.load().pmlp_rnd_parts(R), device=dev), torch.empty(4, device=dev)
    idx = torch.randperm(R, device=dev)[:M].contiguous()
    mu, dz = torch.randn(M, E, device=dev), torch.empty(M, 16, dtype=torch.bfloat16, device=dev)
    lpart = torch.empty(mm.load().pmlp_rnd_parts(M), device=dev)
    jobs = (("pmlp_rnd_reward (rows + finish)", f"{R} x {E}",
             lambda: mm.rnd_reward(pred, tgt, w, T, n, rew, None, part, stats)),
            ("pmlp_rnd_loss_step (rows + finish)", f"{M} x {E} gathered from {R}",
             lambda: mm.rnd_loss_step(mu, tgt, idx, 1.0 / (M * E), lpart, stats, dz)))
    for name, shape, fn in jobs:
        for _ in range(10):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        print(f"{name} at {shape}: {1e3 * t0.elapsed_time(t1) / reps:.2f} us per call "
              f"({reps} back-to-back calls, launch overhead included)", flush=True)


def time_tasks(task, base, n):
    for name in (task, base):
        env, runner = build(name, n)
        timing(name, env, runner)
        env.close()
    kernel_times(n)


if __name__ == "__main__":
    mode, a = sys.argv[1], sys.argv[2:]
    if mode == "measure":
        measure(a[0], int(a[1]))
    elif mode == "learn":
        learn(a[0], a[1], int(a[2]), int(a[3]))
    elif mode == "time":
        time_tasks(a[0], a[1], int(a[2]))
    else:
        raise SystemExit(__doc__)
