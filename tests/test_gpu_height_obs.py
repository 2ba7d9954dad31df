"""The height scan as the tail of the observation rows on the GPU (DESIGN 3.9;
csrc/leggedsim.hip, lgs_set_height_observations).

The CPU oracle has no such tail, so the reference is the numpy fp32 restatement of the formula
in include/leggedsim.h (lgs_height_obs) on the buffers the step leaves: the post-reset root and
the scan measured before the reset (test_gpu_terrain_curriculum checks the scan itself).  The
build has FP contraction off, so the same operations in the same order give the same bits.  The
head of the rows, the rewards and the resets are compared bit for bit with the same env built
with the switch off on the same seed, actions and interventions.

Maps: 3 rows x 2 cols of 8 m tiles, 5 m border.  Go2 5 envs (one per wave) and 8 (two per wave);
G1 3 and 8 through a cfg edit (humanoid layout, 234 / 237 rows).  Resets: forced time-outs
(episode_length_s = 3), terminations (a robot rolled past the limit), reset_idx(env_ids), reset().
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from test_gpu_parity import fused_vs_oracle, make, restore, save  # noqa: E402
from test_gpu_terrain_curriculum import MAP, SHORT, begin_step, end_step, t2n  # noqa: E402

F = np.float32
TERRAIN_STATE = ("terrain_levels", "env_origins", "_terrain_level_sum")
ROBOTS = [("go2", 5), ("go2", 8), ("g1", 3), ("g1", 8)]
P = 187


def build(robot, n, scan_obs, noise):
    kw = dict(MAP, **SHORT, noise__add_noise=noise)
    if robot == "go2":
        kw.update(terrain__level_curriculum=True, terrain__scan_heights=True)
        if scan_obs:
            kw.update(terrain__scan_in_observations=True, env__num_observations=48 + P)
        return make("go2", n, **kw)
    if scan_obs:
        kw.update(terrain__scan_in_observations=True, env__num_observations=47 + P, env__num_privileged_obs=50 + P)
    return make("g1_terrain", n, **kw)


def restate_tail(env):
    """(h, clipped h) of include/leggedsim.h (lgs_height_obs) from the buffers a step left; no case
    within 1e-4 of a clip bound."""
    rz, mh = t2n(env.root_states)[:, 2:3], t2n(env.measured_heights)
    d = (rz - F(0.5)) - mh
    assert d.dtype == F and (np.abs(np.abs(d) - F(1.0)) > 1e-4).all(), "a case sits on the clip bound"
    h = np.clip(d, F(-1.0), F(1.0)) * F(env.obs_scales.height_measurements)
    c = F(env.cfg.normalization.clip_observations)
    assert h.dtype == F and (np.abs(np.abs(h) - c) > 1e-4).all()
    return h, np.clip(h, -c, c)


def script(n):
    """Per step: envs to time out, envs to roll over (termination), envs to reset_idx before it."""
    return [dict(), dict(timeout=[0]), dict(flip=[1]), dict(), dict(ids=[n - 1, 0]), dict(timeout=[1], flip=[n - 1]),
            dict()]


def intervene(env, what):
    if what.get("ids"):
        env.reset_idx(torch.tensor(what["ids"], device=env.device))
    for e in what.get("timeout", []):
        env.episode_length_buf[e] = int(env.max_episode_length)
    for e in what.get("flip", []):  # roll 1.5 rad (> 0.8), lifted clear of the ground
        env.root_states[e, 3:7] = torch.tensor([np.sin(0.75), 0.0, 0.0, np.cos(0.75)], dtype=torch.float,
                                               device=env.device)
        env.root_states[e, 2] += 0.3


def drive(envs, n, each_step):
    """The same reset(), warm-up, interventions and actions for every env of `envs`."""
    g = torch.Generator(device="cuda").manual_seed(n)
    for env in envs:
        env.reset()
    acts = [0.3 * torch.randn(n, envs[0].num_actions, device="cuda", generator=g) for _ in range(3 + len(script(n)))]
    for a in acts[:3]:
        for env in envs:
            env.step(a.clone())
    for what, a in zip(script(n), acts[3:]):
        for env in envs:
            intervene(env, what)
            env.step(a.clone())
        torch.cuda.synchronize()
        each_step(what)
    for env in envs:  # BaseTask.reset: reset_idx of every env, then a zero-action step
        env.reset()
    torch.cuda.synchronize()
    each_step(dict(all=True))


def rows(env):
    head = env.num_obs - P
    obs = t2n(env.obs_buf)
    priv = None if env.privileged_obs_buf is None else t2n(env.privileged_obs_buf)
    return head, obs, priv


def same_head_and_outcomes(on, off, what):
    head, obs, priv = rows(on)
    assert off.num_obs == head
    np.testing.assert_array_equal(obs[:, :head], t2n(off.obs_buf), err_msg=f"head {what}")
    if priv is not None:
        np.testing.assert_array_equal(priv[:, :priv.shape[1] - P], t2n(off.privileged_obs_buf), err_msg=f"priv {what}")
    for name in ("rew_buf", "reset_buf", "time_out_buf", "_episode_sums", "root_states", "measured_heights",
                 "terrain_levels"):
        np.testing.assert_array_equal(t2n(getattr(on, name)), t2n(getattr(off, name)), err_msg=f"{name} {what}")


@pytest.mark.parametrize("robot,n", ROBOTS)
def test_noiseless_tail_is_the_restatement_and_the_head_is_the_switch_off_row(robot, n):
    on, off = build(robot, n, True, False), build(robot, n, False, False)
    assert on.height_obs.enabled == 1 and off.height_obs.enabled == 0
    assert (on.num_obs, on.num_privileged_obs or 0) == ((235, 0) if robot == "go2" else (234, 237))
    seen = dict(timeout=0, term=0, stale=0)

    def check(what):
        head, obs, priv = rows(on)
        h, hc = restate_tail(on)
        np.testing.assert_array_equal(obs[:, head:], hc, err_msg=str(what))
        if robot == "g1":
            np.testing.assert_array_equal(priv[:, 50:], hc, err_msg=str(what))
        same_head_and_outcomes(on, off, what)
        reset, tout = t2n(on.reset_buf).astype(bool), t2n(on.time_out_buf).astype(bool)
        for e in what.get("timeout", []):
            assert reset[e] and tout[e]
            seen["timeout"] += 1
        for e in what.get("flip", []):
            assert reset[e] and not tout[e]
            seen["term"] += 1
        if reset.any() and not what.get("all"):
            # a reset env's row: the root it was placed at, the heights from where its episode ended
            assert np.isfinite(obs[reset]).all()
            seen["stale"] += int(reset.sum())

    drive([on, off], n, check)
    assert seen["timeout"] >= 2 and seen["term"] >= 2 and seen["stale"] >= 4
    assert np.abs(t2n(on.measured_heights)).max() > 0  # (not a flat map)


@pytest.mark.parametrize("robot,n", ROBOTS)
def test_noisy_tail_stays_within_its_scale_and_the_head_keeps_its_draws(robot, n):
    on, off = build(robot, n, True, True), build(robot, n, False, True)
    assert on.add_noise and on.task_params.add_noise == 1
    ns = F(on.height_obs.noise_scale)
    assert ns == F(on.cfg.noise.noise_scales.height_measurements * on.cfg.noise.noise_level *
                   on.obs_scales.height_measurements) and ns > 0
    noise = []

    def check(what):
        head, obs, priv = rows(on)
        h, hc = restate_tail(on)
        same_head_and_outcomes(on, off, what)  # the head's draws did not move
        # |(2u - 1) * ns| <= ns; the sum's rounding is at most half a spacing of its magnitude
        # (clip_observations = 100 is far from these values: restate_tail)
        d = obs[:, head:] - h
        assert (np.abs(d) <= ns + np.spacing(np.abs(h) + ns)).all(), float(np.abs(d).max())
        assert np.abs(d).max() > 0.5 * ns and len(np.unique(d)) > 0.9 * d.size  # (noise, not a constant)
        noise.append(d)
        if robot == "g1":  # the privileged tail carries none
            np.testing.assert_array_equal(priv[:, 50:], hc, err_msg=str(what))

    drive([on, off], n, check)
    for a, b in zip(noise, noise[1:]):  # fresh draws every step
        assert (a != b).mean() > 0.9


@pytest.mark.parametrize("robot,n", ROBOTS)
def test_one_launch_step_and_split_launches_give_the_same_rows(robot, n):
    """lgs_step against lgs_step_physics / _post_physics_prepare / _term_rewards / _finish (what a task
    with a no-op _post_physics_step_callback takes), noise on, with a time-out and a termination."""
    env = build(robot, n, True, True)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(3):
        env.step(0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    intervene(env, dict(timeout=[0], flip=[1]))
    a = 0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g)
    torch.cuda.synchronize()
    st = save(env)
    terrain = {k: getattr(env, k).clone() for k in TERRAIN_STATE}  # (a reset moves its env's level)
    env.step(a.clone())
    torch.cuda.synchronize()
    names = ("rew_buf", "reset_buf", "time_out_buf", "root_states", "measured_heights", "_episode_sums") + TERRAIN_STATE
    fused = (rows(env), {k: t2n(getattr(env, k)) for k in names})
    restore(env, st)
    for name, v in terrain.items():
        getattr(env, name).copy_(v)
    E, k = begin_step(env, a)
    env.sim.step_physics(E, k)
    env.sim.post_physics_prepare(E, k)
    env.sim.post_physics_term_rewards(E, k)
    env.sim.post_physics_finish(E, k)
    end_step(env)
    torch.cuda.synchronize()
    (head, obs, priv), (_, obs1, priv1) = fused[0], rows(env)
    reset = fused[1]["reset_buf"].astype(bool)
    assert reset[0] and reset[1] and not reset.all()
    np.testing.assert_array_equal(obs1, obs)
    if priv is not None:
        np.testing.assert_array_equal(priv1, priv)
    for name in names:
        np.testing.assert_array_equal(t2n(getattr(env, name)), fused[1][name], err_msg=name)
    assert np.abs(obs[:, head:]).max() > 0


@pytest.mark.parametrize("task,n", [("go2", 8), ("go2", 5), ("g1_rough", 3), ("g1_rough", 8)])
def test_switches_off_step_is_still_the_oracle_bitwise(task, n):
    env = make(task, n, **MAP)
    assert env.height_obs.enabled == 0 and env.num_scan_obs == 0
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(5):
        env.step(0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    try:
        fused_vs_oracle(env, g, 3, f"{task} x{n} height observations off")
    finally:
        bridge.set_ground(bridge.ensure_built())


def test_an_inconsistent_num_obs_is_refused_before_any_launch():
    """lgs_set_task and lgs_set_height_observations may come in either order; the step entry points
    check the pair: a status and an error text, and nothing ran (state, rows and the device step
    counter are untouched)."""
    n = 5
    env = build("go2", n, True, False)
    env.reset()
    a = torch.zeros(n, env.num_actions, device="cuda")
    env.step(a)
    torch.cuda.synchronize()
    lib, tp = env.sim.lib, env.task_params
    E = env._env_structs[env._buf_idx]
    mask = torch.ones(n, dtype=torch.uint8, device="cuda")
    keep = ("root_states", "dof_state", "obs_buf", "_episode_length", "_d_step_counter", "measured_heights")

    def refused(match):
        before = {k: t2n(getattr(env, k)) for k in keep}
        for call in (lambda: lib.lgs_step(env.sim.handle, C.byref(E), env.common_step_counter),
                     lambda: lib.lgs_post_physics_finish(env.sim.handle, C.byref(E), env.common_step_counter),
                     lambda: lib.lgs_reset_idx(env.sim.handle, C.byref(E), mask.data_ptr(), env.common_step_counter),
                     lambda: lib.lgs_reset_all(env.sim.handle, C.byref(E), env.common_step_counter)):
            assert call() == -1  # LGS_ERR_ARG
            assert match in lib.lgs_last_error().decode()
        torch.cuda.synchronize()
        for k in keep:
            np.testing.assert_array_equal(t2n(getattr(env, k)), before[k], err_msg=k)

    try:
        tp.num_obs = 234  # head + P - 1
        env.sim.set_task(tp)
        refused("do not match the layout's head (48) + 187 scan points")
        tp.num_obs = 235
        env.sim.set_task(tp)
        env.sim.set_height_observations(None)  # 235 entries without the tail: past LGS_MAX_OBS
        refused("exceed LGS_MAX_OBS")
    finally:
        tp.num_obs = 235
        env.sim.set_task(tp)
        env.sim.set_height_observations(env.height_obs)
    env.step(a)  # consistent again: the step runs
    torch.cuda.synchronize()
    head, obs, _ = rows(env)
    np.testing.assert_array_equal(obs[:, head:], restate_tail(env)[1])
