"""Actuator randomisation and action latency inside the fused env step, on the GPU.

The CPU oracle does not know the feature, but its control step is compute_torques + one physics
substep in a loop, and that substep (orc_simulate) is bitwise the kernel's.  So the reference for
the new PD law is its numpy fp32 restatement (tests/test_actuator_rand_host.py, checked there
against hand-computed values) feeding orc_simulate, `decimation` times; orc_post_physics on that
result is the reference for the rest of the step.  Every comparison is exact.

Shapes: Go2 x 2 (two envs in one wave, different rows per half), Go2 x 3 (odd: one env per wave),
H1 x 2 (10 DOFs, lanes beyond D, humanoid layout), G1 23-DOF with the wrists locked x 2 (padded
instantiation: the kernel's DOF count is not the model's).  Episodes are 8 control steps and the
envs' episode counters are staggered, so resets fall inside the 6 checked steps, one env at a time.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
import legged_gym.envs.base.legged_robot as lr  # noqa: E402
from legged_gym.envs import task_registry  # noqa: E402
from leggedsim import cabi, native  # noqa: E402
from test_actuator_rand_host import actuator_draws, actuator_gains, actuator_torques  # noqa: E402
from test_gpu_padded import lock_dofs  # noqa: E402
from test_gpu_parity import (POST, STATE, _register_g1_23dof, assert_exact, env_arrays, make, restore, save,  # noqa: E402
                             writes_body_states)
from test_gpu_post_physics_branches import split_step  # noqa: E402

F = np.float32
SHAPES = [("go2", 2), ("go2", 3), ("h1", 2), ("g1_23dof_locked", 2)]
ON = dict(domain_rand__randomize_kp=True, domain_rand__randomize_kd=True,
          domain_rand__randomize_motor_strength=True, domain_rand__randomize_action_delay=True)
NEUTRAL = dict(domain_rand__kp_range=[1.0, 1.0], domain_rand__kd_range=[1.0, 1.0],
               domain_rand__motor_strength_range=[1.0, 1.0], domain_rand__action_delay_range=[0, 0])
EPISODE = 8   # control steps per episode of the runs with resets
STEPS = 6
ROWS = ("kp_factors", "kd_factors", "motor_strengths", "action_delay_substeps")


@pytest.fixture
def build(monkeypatch):
    """build(shape, n, reset=True, short=False, **edits): the env of a shape, the feature's switches
    in `edits`; `short`: episodes of EPISODE control steps."""
    envs = []

    def _build(shape, n, reset=True, short=False, **edits):
        task = shape
        if shape == "g1_23dof_locked":
            _register_g1_23dof()
            real = lr.load_model
            monkeypatch.setattr(lr, "load_model", lambda *a, **k: lock_dofs(
                real(*a, **k), ["left_wrist_roll_joint", "right_wrist_roll_joint"]))
            task, D = "g1_23dof", 21
            edits.update(env__num_actions=D, env__num_observations=9 + 3 * D + 2, env__num_privileged_obs=12 + 3 * D + 2)
        if short:
            c = task_registry.get_cfgs(task)[0]
            edits["env__episode_length_s"] = (EPISODE - 0.5) * c.control.decimation * c.sim.dt
        env = make(task, n, **edits)
        envs.append(env)
        if shape == "g1_23dof_locked":
            assert env.num_dof == 21 and env.sim.padded_shape() == (26, 32)
        if short:
            assert int(env.max_episode_length) == EPISODE
        if reset:
            env.reset()
        return env
    yield _build
    for env in envs:
        env.close()
    bridge.set_ground(bridge.ensure_built())


def rows(env):
    torch.cuda.synchronize()
    return {k: getattr(env, k).detach().cpu().numpy().copy() for k in ROWS}


def assert_rows_equal(got, want, what):
    for k in ROWS:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {k}"


def stagger(env):
    """Env e's time-out falls about 2 + e steps ahead: one env resets at a time."""
    env._sync_stream()
    n = env.num_envs
    env.episode_length_buf = torch.tensor([EPISODE - 2 - e for e in range(n)], device=env.device)


def actions(env, g, scale=0.3):
    return scale * torch.randn(env.num_envs, env.num_actions, device="cuda", generator=g)


def restate_physics(env, snap, a):
    """The physics half of a control step from `snap` on the env's present factor rows:
    decimation x { the PD law's restatement -> orc_simulate }.  Returns the state after it
    (root, dofs, cforce, last substep's torques, body states, clipped actions) and whether a
    torque reached its effort clip."""
    lib = bridge.ensure_built()
    bridge.set_env(lib, env)
    T, n, D = env.task_params, env.num_envs, env.num_dof
    r = rows(env)
    kp, kd = actuator_gains(T, D, r["kp_factors"], r["kd_factors"], r["motor_strengths"])
    ac = np.clip(np.asarray(a, F), -F(T.clip_actions), F(T.clip_actions)).astype(F)
    root, dofs, cf, rbs = (np.ascontiguousarray(snap[k]).copy() for k in ("root", "dofs", "cforce", "rbs"))
    mh = cabi.ModelHandle(env.model)
    p = lambda x: x.ctypes.data  # noqa: E731
    clipped = False
    tau = None
    for it in range(T.decimation):
        qv = dofs.reshape(n, D, 2)
        tau, raw = actuator_torques(T, D, kp, kd, r["motor_strengths"], r["action_delay_substeps"], it,
                                    snap["last_actions"], ac, qv[..., 0], qv[..., 1], snap["last_dof_vel"],
                                    env._lgs_params.dt)
        clipped |= bool((tau != raw).any())
        tau = np.ascontiguousarray(tau, F)
        lib.orc_simulate(C.byref(mh.desc), C.byref(env._lgs_params), n, p(root), p(dofs), p(tau), p(cf),
                         p(rbs) if it == T.decimation - 1 else None, p(snap["added_mass"]), p(snap["friction"]))
    # the step refreshes the rigid_body_states rows of the task's mask alone (0: every body)
    out = np.ascontiguousarray(snap["rbs"]).copy()
    if T.write_body_states:
        B, mask = env.num_bodies, int(T.body_state_mask)
        sel = [k for k in range(B) if not mask or (mask >> k) & 1]
        out.reshape(n, B, 13)[:, sel] = rbs.reshape(n, B, 13)[:, sel]
    return dict(root=root, dofs=dofs, cforce=cf, torques=tau, rbs=out, actions=ac), clipped


def restate_step(env, snap, phys, step):
    """orc_post_physics on the restated physics result: the whole step's buffers."""
    lib = bridge.ensure_built()
    b = {k: (None if v is None else np.ascontiguousarray(v).copy()) for k, v in snap.items()}
    b.update({k: v.copy() for k, v in phys.items()})
    b["episode_acc"][:] = 0
    mh = cabi.ModelHandle(env.model)
    E = bridge._env_struct(b)
    p = lambda x: x.ctypes.data  # noqa: E731
    lib.orc_post_physics(C.byref(mh.desc), C.byref(env.task_params), env.num_envs, p(b["root"]), p(b["dofs"]),
                         p(b["cforce"]), p(b["rbs"]) if writes_body_states(env) else None, C.byref(E), int(step))
    return b


def physics_half(env, a):
    """lgs_step_physics on the env's buffers; the state it left."""
    env._sync_stream()
    env._buf_idx ^= 1
    E = env._env_structs[env._buf_idx]
    env.actions.copy_(a)
    E.actions_in = None
    E.ep_snapshot = None
    env.sim.step_physics(E, env.common_step_counter)
    torch.cuda.synchronize()
    t = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    return dict(root=t(env.root_states), dofs=t(env.dof_state), cforce=t(env._contact_forces), torques=t(env.torques),
                actions=t(env.actions))


# ------------------------------------------------------------- 1. neutral ---
@pytest.mark.parametrize("shape,n", SHAPES)
def test_neutral_rows_are_the_step_without_the_feature_bitwise(build, shape, n):
    """Enabled, every range [1, 1] and the delay [0, 0], resampling on: the fused step is the
    oracle's (which has no such feature), resets and their redraws of 1.0f / 0 included."""
    env = build(shape, n, short=True, **ON, **NEUTRAL)
    R = env.actuator_rand
    assert (R.enabled, R.resample_on_reset) == (1, 1) and env.kp_factors.shape == (n, env.num_dof)
    assert env.action_delay_substeps.dtype == torch.int32 and env.action_delay_substeps.shape == (n,)
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(3):
        env.step(actions(env, g, 0.5))
    stagger(env)
    resets = []
    for it in range(STEPS):
        snap = bridge.snapshot(env)
        a = actions(env, g, 0.5)
        ref = bridge.step(env, snap, a.cpu().numpy(), env.common_step_counter)
        env.step(a)
        assert_exact(env_arrays(env), ref, STATE + POST, n, f"{shape} x{n} neutral step {it}",
                     skip_body_states=not writes_body_states(env))
        resets.append(ref["reset"].astype(bool).ravel())
    resets = np.array(resets)
    assert resets.any(axis=0).all(), "every env resets inside the run"
    assert (resets[:, :2].sum(axis=1) == 1).any(), "a step in which one env of the first wave resets alone"
    r = rows(env)
    assert all((r[k] == 1.0).all() for k in ROWS[:3]) and not r["action_delay_substeps"].any()


# ------------------------------------------------- 2. the PD law, bitwise ---
def fill_rows(env, it):
    """Distinct factors per env and DOF; the envs' delays walk over 0, an interior value and
    the whole decimation loop."""
    env._sync_stream()
    n, D, dec = env.num_envs, env.num_dof, env.cfg.control.decimation
    e = torch.arange(n, device=env.device, dtype=torch.float).view(n, 1)
    j = torch.arange(D, device=env.device, dtype=torch.float).view(1, D)
    env.kp_factors.copy_(0.7 + 0.11 * e + 0.02 * j + 0.01 * it)
    env.kd_factors.copy_(1.3 - 0.07 * e - 0.015 * j)
    env.motor_strengths.copy_(0.85 + 0.09 * e + 0.005 * j)
    choices = [0, dec // 2, dec]
    assert 0 < dec // 2 < dec
    d = [choices[(k + it) % 3] for k in range(n)]
    env.action_delay_substeps.copy_(torch.tensor(d, dtype=torch.int32, device=env.device))
    return d


@pytest.mark.parametrize("shape,n,control,steps", [(s, n, "P", STEPS) for s, n in SHAPES] +
                         [("go2", 2, "V", 3), ("go2", 2, "T", 3)])
def test_pd_law_and_latency_match_the_restatement_bitwise(build, shape, n, control, steps):
    """Hand-filled rows, no resampling.  From the snapshot before the step, decimation rounds of
    { restated PD law -> orc_simulate } give lgs_step_physics' root_states, dof_state, torques and
    contact forces; orc_post_physics on that gives the fused lgs_step's observations, rewards,
    reset flags and every other buffer.  No step ends an episode.  (The velocity and torque
    control modes: Go2 x 2, three steps from the reset pose.)"""
    # (torque control: a scale at which the clipped action, times the smallest strength, passes the effort limit)
    more = dict(control__action_scale=0.5) if control == "T" else {}
    env = build(shape, n, **ON, domain_rand__actuator_resample_on_reset=False, control__control_type=control, **more)
    assert (env.actuator_rand.enabled, env.actuator_rand.resample_on_reset) == (1, 0)
    env.sim.set_task(env.task_params)  # (the two setters in the other order)
    g = torch.Generator(device="cuda").manual_seed(10 + n)
    if control == "P":
        for _ in range(3):
            env.step(actions(env, g))
    r = rows(env)
    assert all((r[k] == 1.0).all() for k in ROWS[:3]) and not r["action_delay_substeps"].any()  # never drawn
    skip_rbs = not writes_body_states(env)
    any_clip, delays = False, set()
    for it in range(steps):
        delays.update(fill_rows(env, it))
        a = actions(env, g)
        if it == steps - 1:  # a target far outside the joint's range: the effort clip, in the last step
            a[0, 1], a[n - 1, env.num_actions - 1] = 100.0, -100.0
        st = save(env)
        snap = bridge.snapshot(env)
        assert np.abs(snap["last_actions"]).max() > 0 or it == 0
        want, clipped = restate_physics(env, snap, a.cpu().numpy())
        any_clip |= clipped
        got = physics_half(env, a)
        assert_exact(got, want, ["root", "dofs", "torques", "cforce", "actions"], n,
                     f"{shape} x{n} {control} step {it}: lgs_step_physics vs the restatement")
        restore(env, st)
        k = env.common_step_counter
        env.step(a)
        fused = env_arrays(env)
        ref = restate_step(env, snap, want, k)
        assert_exact(fused, ref, STATE + POST, n, f"{shape} x{n} {control} step {it}: lgs_step vs the restatement",
                     skip_body_states=skip_rbs)
        assert not fused["reset"].any(), "the step must not end an episode"
    assert any_clip, "no torque reached its effort clip"
    assert delays == {0, env.cfg.control.decimation // 2, env.cfg.control.decimation}


# ---------------------------------------------------------- 3. resampling ---
def expected_rows(env, before, reset, step):
    """The rows after a launch with step key `step` in which the envs of `reset` reset."""
    seed = int(env.task_params.seed)

    def uniform(e, s, stream, index):
        return F(env.sim.lib.lgs_uniform(seed, int(e), int(s) & 0xFFFFFFFF, stream, index))

    want = {k: v.copy() for k, v in before.items()}
    for e in np.nonzero(reset)[0]:
        kp, kd, st, d = actuator_draws(uniform, env.actuator_rand, env.num_dof, int(e), step)
        want["kp_factors"][e], want["kd_factors"][e], want["motor_strengths"][e] = kp, kd, st
        want["action_delay_substeps"][e] = d
    return want


@pytest.mark.parametrize("shape,n", SHAPES)
def test_resetting_envs_redraw_their_rows_on_all_three_routes(build, shape, n):
    """reset(), reset_idx(ids) and the control step's reset branch: the rows of the envs that reset
    are the header's formulas on the host lgs_uniform with the launch's step key, exactly; every
    other row keeps its bits; and the step in which an env resets still ran on its old row (its
    torques are the restatement's on the rows before the step)."""
    env = build(shape, n, reset=False, short=True, **ON)
    R = env.actuator_rand
    assert (R.enabled, R.resample_on_reset) == (1, 1) and list(R.delay_range) == [0, 2]
    r0 = rows(env)
    assert all((r0[k] == 1.0).all() for k in ROWS[:3]) and not r0["action_delay_substeps"].any()  # neutral until a reset
    every = np.ones(n, bool)
    # BaseTask.reset(): reset_idx of every env, then a zero-action step in which nobody resets
    k = env.common_step_counter
    env.reset()
    r1 = rows(env)
    assert_rows_equal(r1, expected_rows(env, r0, every, k), "reset()")
    lo, hi = F(0.9), F(1.1)
    assert all(((r1[key] >= lo) & (r1[key] <= hi)).all() and len(np.unique(r1[key])) > n for key in ROWS[:3])
    assert ((r1["action_delay_substeps"] >= 0) & (r1["action_delay_substeps"] <= 2)).all()
    g = torch.Generator(device="cuda").manual_seed(20 + n)
    for _ in range(2):
        env.step(actions(env, g))
    assert_rows_equal(rows(env), r1, "steps without a reset")
    # reset_idx(ids)
    k = env.common_step_counter
    env.reset_idx(torch.tensor([n - 1], device=env.device))
    only = np.zeros(n, bool)
    only[n - 1] = True
    r2 = rows(env)
    assert_rows_equal(r2, expected_rows(env, r1, only, k), "reset_idx")
    assert (r2["kp_factors"][n - 1] != r1["kp_factors"][n - 1]).any()
    # lgs_reset_all (the C entry point BaseTask.reset does not go through)
    k = env.common_step_counter
    env._sync_stream()
    env.sim.reset_all(env._env_structs[env._buf_idx], k)
    r3 = rows(env)
    assert_rows_equal(r3, expected_rows(env, r2, every, k), "lgs_reset_all")
    # the control step's reset branch
    stagger(env)
    seen = []
    for it in range(STEPS):
        before = rows(env)
        snap = bridge.snapshot(env)
        a = actions(env, g)
        k = env.common_step_counter
        phys, _ = restate_physics(env, snap, a.cpu().numpy())
        env.step(a)
        torch.cuda.synchronize()
        reset = env.reset_buf.cpu().numpy().astype(bool).ravel()
        after = rows(env)
        assert_rows_equal(after, expected_rows(env, before, reset, k), f"control step {it}")
        np.testing.assert_array_equal(env.torques.cpu().numpy(), phys["torques"],
                                      err_msg=f"step {it}: the step's physics ran on the rows before it")
        for e in np.nonzero(reset)[0]:
            assert (after["kp_factors"][e] != before["kp_factors"][e]).any()
        seen.append(reset)
    seen = np.array(seen)
    assert seen.any(axis=0).all(), "every env resets inside the run"
    assert (seen[:, :2].sum(axis=1) == 1).any(), "a step in which one env of the first wave resets alone"


def test_resample_off_only_reads_the_rows(build):
    env = build("go2", 2, reset=False, short=True, **ON, domain_rand__actuator_resample_on_reset=False)
    fill_rows(env, 0)
    r0 = rows(env)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    for _ in range(EPISODE + 2):
        env.step(actions(env, g))
    assert_rows_equal(rows(env), r0, "resample_on_reset = 0")


# ------------------------------------------------------ 4. the split path ---
@pytest.mark.parametrize("shape,n", SHAPES)
def test_split_path_is_the_fused_step_bitwise_with_the_feature_on(build, shape, n):
    """lgs_step_physics + lgs_post_physics, and physics + prepare / term_rewards / finish, from
    the same state and rows: the fused lgs_step's buffers and redrawn rows, resets included."""
    env = build(shape, n, short=True, **ON)
    g = torch.Generator(device="cuda").manual_seed(30 + n)
    for _ in range(2):
        env.step(actions(env, g, 0.5))
    stagger(env)
    resets = 0
    for it in range(STEPS):
        a = actions(env, g, 0.5)
        st, r0 = save(env), {k: getattr(env, k).clone() for k in ROWS}
        env.step(a)
        fused, rf = env_arrays(env), rows(env)
        resets += int(fused["reset"].sum())
        for three in (False, True):
            restore(env, st)
            for k in ROWS:
                getattr(env, k).copy_(r0[k])
            parts = split_step(env, a, three)
            what = f"{shape} x{n} step {it}: {'prepare/term_rewards/finish' if three else 'physics + post'}"
            assert_exact(parts, fused, STATE + POST, n, what)
            assert_rows_equal(rows(env), rf, what)
    assert resets >= n


# ------------------------------------------------------------ the C ABI -----
def test_entry_points_refuse_a_bad_descriptor_before_any_launch(build):
    env = build("go2", 2, **ON)
    lib, h = env.sim.lib, env.sim.handle
    assert lib.lgs_set_actuator_randomization(h, None) == -1 and b"null" in lib.lgs_last_error()
    good = cabi.ActuatorRand.from_buffer_copy(env.actuator_rand)
    E = env._env_structs[env._buf_idx]
    k = env.common_step_counter
    mask = torch.ones(2, dtype=torch.uint8, device=env.device)
    before = save(env)

    def refused(edit, match):
        bad = cabi.ActuatorRand.from_buffer_copy(good)
        edit(bad)
        env.sim.set_actuator_randomization(bad, env.sim._act_buffers)
        for call in (lambda: env.sim.step(E, k), lambda: env.sim.step_physics(E, k), lambda: env.sim.reset_all(E, k),
                     lambda: env.sim.reset_idx(E, mask, k)):
            with pytest.raises(native.LeggedSimError, match=match):
                call()

    def set_delay(lo, hi):
        def edit(R):
            R.delay_range[:] = (lo, hi)
        return edit

    def set_range(name, lo, hi):
        def edit(R):
            getattr(R, name)[:] = (lo, hi)
        return edit

    refused(set_delay(0, 5), "decimation")       # go2: decimation 4
    refused(set_delay(-1, 2), "decimation")
    refused(set_delay(3, 2), "decimation")
    refused(set_range("kp_range", 1.1, 0.9), "ranges")
    refused(set_range("kd_range", -0.5, 1.0), "ranges")
    refused(set_range("strength_range", 0.9, float("inf")), "ranges")
    refused(set_range("kp_range", float("nan"), 1.0), "ranges")
    for name in ("kp_scale", "kd_scale", "strength", "delay"):
        refused(lambda R, name=name: setattr(R, name, None), "needs kp_scale")
    torch.cuda.synchronize()
    for key in ("root_states", "dof_state", "actions", "_episode_length"):  # nothing was launched
        assert torch.equal(getattr(env, key), before[key]), key
    # disabled: nothing is checked, and the step is the plain one; the good descriptor steps again
    off = cabi.ActuatorRand()
    env.sim.set_actuator_randomization(off)
    env.step(torch.zeros(2, env.num_actions, device="cuda"))
    env.sim.set_actuator_randomization(good, env.sim._act_buffers)
    env.step(torch.zeros(2, env.num_actions, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs_buf).all()


# ------------------------------------------------- 5. the captured rollout ---
def test_runner_collects_go2_robust_through_the_captured_graph():
    """OnPolicyRunner.learn(2) on go2_robust, 64 envs, episodes shorter than a rollout: the second
    iteration's collection replays the captured graph (not the eager fallback), and its storage,
    the policy and the redrawn rows equal an eager-collecting twin's, bitwise."""
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (True, False):
        env = make("go2_robust", 64, env__episode_length_s=0.3)
        assert env.actuator_rand.enabled == 1 and env.kp_factors is not None
        _, train_cfg = task_registry.get_cfgs("go2_robust")
        cfg = copy.deepcopy(class_to_dict(train_cfg))
        assert cfg["runner"]["experiment_name"] == "go2_robust"
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        assert runner.alg._fused is not None and runner.alg._rollout is not None, "native PPO path not active"
        assert not env._split_step
        runner.learn(2)
        env.flush_extras()
        torch.cuda.synchronize()
        if graph:
            assert runner._rollout_graph is not None and not getattr(runner, "_rollout_graph_failed", False)
        else:
            assert runner._rollout_graph is None
        st = runner.alg.storage
        out[graph] = dict(storage=[t.clone() for t in (st.observations, st.actions, st.actions_log_prob, st.mu, st.sigma,
                                                       st.values, st.rewards, st.dones, st.returns, st.advantages)],
                          params=[p.detach().clone() for p in runner.alg.actor_critic.parameters()],
                          rows=[getattr(env, k).clone() for k in ROWS], obs=env.obs_buf.clone())
        assert st.dones.any(), "episodes end inside the rollout"
        assert all(torch.isfinite(t.float()).all() for t in out[graph]["storage"])
        r = out[graph]["rows"]
        assert (r[0] != 1.0).any() and (r[3] > 0).any()  # drawn rows, latency on
        env.close()
    for key in ("storage", "params", "rows"):
        for a, b in zip(out[True][key], out[False][key]):
            assert torch.equal(a, b), key
    assert torch.equal(out[True]["obs"], out[False]["obs"])
