"""The branches of the control step's post-physics half that a short warm rollout hardly
reaches: time-out and termination resets, command resampling, pushes, a wave whose two envs
take different branches, host writes between steps, and the split entry points on such steps.

The kernel evaluates this half lane-parallel (base-frame vectors, Euler angles, heading,
commands, gait phase and termination each on a lane; reward terms staged per element, then
added in index order; observations entry per lane) from inputs it fetches with the state at the
start of the launch.  None of that may change a bit: every buffer is compared with the CPU
oracle's (exact), on the snapshot taken right before the step.

Short episodes (0.4 s), resampling (0.2 s) and pushes (0.3 s) bring every branch up within
~45 control steps; one env's root is tilted past the roll limit so that it terminates, which
also staggers the envs' episode counters (a wave with one env resetting and one not).  The
conditions are counted from the oracle's outputs alone, and a run that misses one fails.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from leggedsim import cabi  # noqa: E402
from test_gpu_parity import (POST, STATE, assert_exact, env_arrays, fused_vs_oracle, restore, save, warm,  # noqa: E402
                             writes_body_states)

EDITS = dict(env__episode_length_s=0.4, commands__resampling_time=0.2, domain_rand__push_interval_s=0.3)
STEPS = 48
TILT_AT = 3     # the step before which the last env's root is rolled past the limit
WRITE_AT = 30   # the step before which the host overwrites commands / air time / episode length


def tilt(env, i, roll=1.0):
    """Roll env i's base by `roll` rad (limit 0.8) through the sim's root-state setter."""
    env._sync_stream()
    env.root_states[i, 3:7] = torch.tensor([math.sin(roll / 2), 0.0, 0.0, math.cos(roll / 2)], device=env.device)
    ids = torch.tensor([i], dtype=torch.int32, device=env.device)
    env.sim.set_root_indexed(env.root_states, ids, 1)


def host_writes(env):
    n = env.num_envs
    env._sync_stream()
    env.commands[:] = torch.tensor([0.7, -0.3, 0.2, 1.1], device=env.device)
    env.feet_air_time[:] = 0.37
    env.episode_length_buf = torch.arange(5, 5 + n, device=env.device)


def split_step(env, a, three):
    """The step as lgs_step_physics + the post half (one launch, or prepare / term_rewards /
    finish), on the env's buffers like LeggedRobot.step."""
    env._sync_stream()
    env._buf_idx ^= 1
    E = env._env_structs[env._buf_idx]
    env.actions.copy_(a)
    E.actions_in = None
    E.ep_snapshot = None
    k = env.common_step_counter
    env.sim.step_physics(E, k)
    if three:
        env.sim.post_physics_prepare(E, k)
        env.sim.post_physics_term_rewards(E, k)
        env.sim.post_physics_finish(E, k)
    else:
        env.sim.post_physics(E, k)
    env._step_mirror += 1
    env.obs_buf, env.privileged_obs_buf = env._obs_bufs[env._buf_idx], env._priv_bufs[env._buf_idx]
    env.reset_buf, env.time_out_buf = env._reset_bufs[env._buf_idx], env._timeout_bufs[env._buf_idx]
    return env_arrays(env)


def events(env, snap, ref):
    """What this step did, from the oracle's inputs and outputs."""
    T = env.task_params
    reset, tout = ref["reset"].astype(bool).ravel(), ref["time_out"].astype(bool).ravel()
    cols = [0, 1, 3] if T.heading_command else [0, 1, 2]
    resampled = ~reset & (ref["commands"][:, cols] != snap["commands"][:, cols]).any(axis=1)
    pushed = ~reset & bool(T.push_robots) & (ref["episode_length"].ravel() % T.push_interval == 0)
    return {"time-out reset": bool(tout.any()), "termination reset": bool((reset & ~tout).any()),
            "command resample": bool(resampled.any()), "push step": bool(pushed.any()),
            "one env of the wave resets": env.num_envs == 2 and int(reset.sum()) == 1}


def scenario(task, n, split):
    env, g = warm(task, n, steps=0, seed=n, **EDITS)
    skip_rbs = not writes_body_states(env)
    seen = {}
    split_on_mixed = 0
    for it in range(STEPS):
        if it == TILT_AT:
            tilt(env, n - 1)
        if it == WRITE_AT:
            host_writes(env)
        snap = bridge.snapshot(env)
        a = 0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        ref = bridge.step(env, snap, a.cpu().numpy(), env.common_step_counter)
        st = save(env) if split else None
        env.step(a)
        got = env_arrays(env)
        assert_exact(got, ref, STATE + POST, n, f"{task} x{n} step {it}", skip_body_states=skip_rbs)
        ev = events(env, snap, ref)
        for k, v in ev.items():
            seen[k] = seen.get(k, 0) + int(v)
        if split:
            for three in (False, True):
                restore(env, st)
                parts = split_step(env, a, three)
                assert_exact(parts, got, STATE + POST, n,
                             f"{task} x{n} step {it}: {'prepare/term_rewards/finish' if three else 'physics + post'}")
            split_on_mixed += int(ev["one env of the wave resets"])
    need = ["time-out reset", "termination reset", "command resample", "push step"]
    if n == 2:
        need.append("one env of the wave resets")
    missing = [k for k in need if not seen.get(k)]
    assert not missing, f"{task} x{n}: the run never reached: {missing} (seen {seen})"
    if split and n == 2:
        assert split_on_mixed > 0
    env.close()


@pytest.mark.parametrize("task,n,split", [("go2", 2, True), ("go2", 1, False), ("go2", 6, False),
                                          ("h1", 2, True), ("h1_2", 3, False)])
def test_every_post_physics_branch_matches_oracle_bitwise(task, n, split):
    """One wave with an env per half, one env per wave (64-lane strides), several waves, the
    humanoid layout (gait phase, body-state rewards), an odd count.  With `split`, every step
    is also taken as lgs_step_physics + lgs_post_physics and as physics + prepare /
    term_rewards / finish from the same state: bitwise the fused step, the steps where one
    half of the wave resets included."""
    scenario(task, n, split)


@pytest.mark.parametrize("ground", ["plane", "heightfield"])
def test_contact_forces_of_step_and_simulate_match_oracle_bitwise(ground):
    """A control step computes the contact forces of its last substep only, lgs_simulate those
    of its one substep: both the oracle's, on the plane and on a 5 x 8-tile heightfield."""
    edits = {} if ground == "plane" else dict(terrain__mesh_type="heightfield", terrain__num_rows=5,
                                              terrain__num_cols=8)
    env, g = warm("go2", 2, steps=12, seed=5, **edits)
    try:
        fused_vs_oracle(env, g, 3, f"go2 x2 {ground}")  # (STATE holds cforce)
        assert np.abs(env_arrays(env)["cforce"]).max() > 0
        tau = (5.0 * torch.randn(2, env.num_actions, device="cuda", generator=g)).contiguous()
        snap = bridge.snapshot(env)
        env.sim.simulate(tau)
        torch.cuda.synchronize()
        lib = bridge.ensure_built()
        bridge.set_env(lib, env)
        mh = cabi.ModelHandle(env.model)
        root, dofs = snap["root"].copy(), snap["dofs"].copy()
        cf, rbs = snap["cforce"].copy(), snap["rbs"].copy()
        t = tau.cpu().numpy()
        p = lambda a: a.ctypes.data  # noqa: E731
        lib.orc_simulate(C.byref(mh.desc), C.byref(env._lgs_params), 2, p(root), p(dofs), p(t), p(cf), p(rbs),
                         p(snap["added_mass"]), p(snap["friction"]))
        np.testing.assert_array_equal(env.root_states.cpu().numpy(), root)
        np.testing.assert_array_equal(env.dof_state.cpu().numpy(), dofs)
        np.testing.assert_array_equal(env._contact_forces.cpu().numpy().reshape(cf.shape), cf)
    finally:
        bridge.set_ground(bridge.ensure_built())
