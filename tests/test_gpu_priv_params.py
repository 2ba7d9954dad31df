"""The asymmetric critic's privileged row inside the fused env step, on the GPU.

The statement (include/leggedsim.h, lgs_priv_params) is elementwise fp32, so every comparison is
bitwise.  References: a twin env -- same task, seed and actions -- with the switch off (everything
but the privileged row, and the humanoid's head and scan), a twin without noise (the quadruped's
clean frame and clean scan), and the numpy fp32 restatement of the tail
(tests/test_priv_params_host.py, checked there against hand-computed values) on the env's own rows.

Shapes: Go2 x 2 (two envs share a wave) and Go2 x 3 (a half-filled one), with the actuator rows
(87 columns) and without (50); go2_robust_history x 2 (the history buffers); H1 x 2 (humanoid
layout, 10 DOFs) with and without the actuator rows; go2_terrain x 2 and g1_terrain x 2 with the
scan in the rows; go2_terrain_robust x 2 (history, actuator rows and scan together: 274 columns).  Episodes are 8 control steps and staggered, so resets fall inside the 6 checked
steps, one env at a time.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from legged_gym.envs import task_registry  # noqa: E402
from leggedsim import cabi, native  # noqa: E402
from test_gpu_actuator_rand import EPISODE, ON, ROWS, STEPS, actions, rows, stagger  # noqa: E402
from test_gpu_parity import POST, STATE, _register_g1_23dof, assert_exact, env_arrays, make  # noqa: E402
from test_gpu_post_physics_branches import split_step  # noqa: E402
from test_gpu_terrain_curriculum import MAP  # noqa: E402
from test_priv_params_host import priv_tail  # noqa: E402

F = np.float32
SCAN = 187
REST = [k for k in STATE + POST if k != "priv_obs"]
# case -> (task, edits, privileged head, A, actuator rows, scan points in the rows, history frames)
CASES = {
    "go2": ("go2", {}, 48, 12, False, 0, 1),
    "go2_robust": ("go2_robust", {}, 48, 12, True, 0, 1),
    "go2_robust_history": ("go2_robust_history", {}, 48, 12, True, 0, 5),
    "h1": ("h1", {}, 44, 10, False, 0, 1),
    "h1_act": ("h1", ON, 44, 10, True, 0, 1),
    "go2_terrain": ("go2_terrain", MAP, 48, 12, False, SCAN, 1),
    "go2_terrain_robust": ("go2_terrain_robust", MAP, 48, 12, True, SCAN, 5),
    "g1_terrain": ("g1_terrain", dict(MAP, terrain__scan_in_observations=True, env__num_observations=47 + SCAN,
                                      env__num_privileged_obs=50 + SCAN), 50, 12, False, SCAN, 1),
}


def widths(case):
    _, _, head, A, act, S, _ = CASES[case]
    Wp = 2 + (3 * A + 1 if act else 0)
    return head, Wp, S, head + Wp + S


@pytest.fixture
def build():
    """build(case, n, on, noise=True, short=True, **edits): the env of a case, the switch on or off;
    `short`: episodes of EPISODE control steps.  Reset before it is returned."""
    envs = []

    def _build(case, n, on, noise=True, short=True, **edits):
        task, base, head, A, act, S, H = CASES[case]
        kw = dict(base, noise__add_noise=noise, **edits)
        if short:
            c = task_registry.get_cfgs(task)[0]
            kw["env__episode_length_s"] = (EPISODE - 0.5) * c.control.decimation * c.sim.dt
        if on:
            kw.update(env__privileged_parameters=True, env__num_privileged_obs=widths(case)[3])
        env = make(task, n, **kw)
        envs.append(env)
        assert bool(env.priv_params.enabled) == on and env.num_priv_tail == (widths(case)[1] if on else 0)
        assert bool(env.actuator_rand.enabled) == act and not env._split_step
        if on:
            assert env.privileged_obs_buf.shape == (n, widths(case)[3])
        env.reset()
        return env
    yield _build
    for env in envs:
        env.close()
    bridge.set_ground(bridge.ensure_built())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def t2n(t):
    return t.detach().cpu().numpy().copy()


def state_rows(env):
    """The env's own state next to the step's buffers: the actuator rows, the history buffers."""
    out = rows(env) if env.actuator_rand.enabled else {}
    if env.obs_history is not None:
        out.update(obs_history=t2n(env.obs_history), fill=t2n(env._obs_history_fill))
    return out


def assert_state_rows_equal(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k}"


def expected_tail(env, r=None):
    """The restated tail on the env's friction, added mass and (present, or given) actuator rows."""
    clip = env.cfg.normalization.clip_observations
    fr, ms = np.asarray(env.shape_friction, F), np.asarray(env.added_base_mass, F)
    if not env.actuator_rand.enabled:
        return priv_tail(env.priv_params, clip, fr, ms)
    r = rows(env) if r is None else r
    return priv_tail(env.priv_params, clip, fr, ms, r["kp_factors"], r["kd_factors"], r["motor_strengths"],
                     r["action_delay_substeps"])


# ----------------------------------- 1. nothing else moves; in-step resets ---
@pytest.mark.parametrize("case,n", [("go2_robust", 2), ("go2_robust", 3), ("go2", 3), ("go2_robust_history", 2),
                                    ("h1", 2), ("h1_act", 2), ("g1_terrain", 2), ("go2_terrain_robust", 2)])
def test_nothing_else_moves_and_the_tail_shows_the_rows_of_the_next_step(build, case, n):
    """Switch on against a twin with it off, 6 steps with staggered time-outs: every buffer but the
    privileged row is the twin's, the actuator rows and the history buffers included; the
    humanoid's head and scan keep their bits (the scan Wp columns later); the tail is the
    restatement on the rows as the step left them -- for an env the step reset, the redrawn ones."""
    on, off = build(case, n, True), build(case, n, False)
    head, Wp, S, P = widths(case)
    hum = on.obs_layout == cabi.OBS_HUMANOID
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(2):
        a = actions(on, g, 0.5)
        on.step(a)
        off.step(a)
    stagger(on)
    stagger(off)
    resets, redrawn = np.zeros(n, bool), 0
    for it in range(STEPS):
        what = f"{case} x{n} step {it}"
        a = actions(on, g, 0.5)
        before = state_rows(on)
        on.step(a)
        off.step(a)
        got, ref = env_arrays(on), env_arrays(off)
        assert_exact(got, ref, REST, n, what + ": everything but the privileged row vs the twin")
        assert_state_rows_equal(state_rows(on), state_rows(off), what)
        priv = got["priv_obs"]
        assert priv.shape == (n, P) and np.isfinite(priv).all()
        if hum:
            assert ref["priv_obs"].shape == (n, head + S)
            assert same(priv[:, :head], ref["priv_obs"][:, :head]), what + ": the humanoid's head"
            assert same(priv[:, head + Wp:], ref["priv_obs"][:, head:]), what + ": the scan, Wp columns later"
        assert same(priv[:, head:head + Wp], expected_tail(on)), what + ": the tail vs the restatement"
        reset = got["reset"].astype(bool).ravel()
        resets |= reset
        if on.actuator_rand.enabled and reset.any():
            now = state_rows(on)
            for e in np.nonzero(reset)[0]:  # the ending step ran on other rows than the ones shown
                assert not np.array_equal(now["kp_factors"][e], before["kp_factors"][e]), what
                redrawn += 1
    assert resets.all(), "every env resets inside the run"
    assert redrawn >= n or not on.actuator_rand.enabled


# ------------------------------------------- 2 + 5. clean frame, clean scan ---
@pytest.mark.parametrize("case,n", [("go2_robust", 3), ("go2_robust_history", 2), ("go2_terrain", 2),
                                    ("go2_terrain_robust", 2)])
def test_quadruped_head_and_scan_are_the_rows_of_a_twin_without_noise(build, case, n):
    """priv[:, :F] is the newest frame of obs of a twin stepped with noise.add_noise = False (the
    last slot of its history row), priv[:, F + Wp:] its scan entries."""
    on, twin = build(case, n, True, noise=True), build(case, n, False, noise=False)
    head, Wp, S, P = widths(case)
    H = CASES[case][6]
    assert on.task_params.add_noise == 1 and twin.task_params.add_noise == 0
    g = torch.Generator(device="cuda").manual_seed(7 + n)
    stagger(on)
    stagger(twin)
    noisy, resets = False, np.zeros(n, bool)
    for it in range(STEPS):
        what = f"{case} x{n} step {it}"
        a = actions(on, g, 0.5)
        on.step(a)
        twin.step(a)
        got, ref = env_arrays(on), env_arrays(twin)
        assert_exact(got, ref, STATE + ["rew", "reset"], n, what + ": the twin is in lockstep")
        priv, clean = got["priv_obs"], ref["obs"]
        assert clean.shape == (n, H * head + S)
        assert same(priv[:, :head], clean[:, (H - 1) * head:H * head]), what + ": the clean frame"
        if S:
            assert same(priv[:, head + Wp:], clean[:, H * head:]), what + ": the clean scan"
        noisy |= not same(got["obs"][:, (H - 1) * head:H * head], priv[:, :head])
        resets |= got["reset"].astype(bool).ravel()
    assert noisy and resets.all()


# ------------------------------------------- 3. the tail, entry by entry ---
@pytest.mark.parametrize("case", ["go2_robust", "go2"])
def test_tail_of_distinct_rows_is_the_restatement_clip_included(build, case):
    """Distinct values per env and DOF in the four actuator rows, per-env friction and mass through
    set_env_properties, clip_observations = 0.9 so the clip catches some entries: 87 columns with
    the actuator group, 50 without."""
    n = 3
    env = build(case, n, True, short=False, normalization__clip_observations=0.9,
                domain_rand__randomize_friction=True, domain_rand__friction_range=[0.1, 1.25],
                domain_rand__randomize_base_mass=True, domain_rand__added_mass_range=[-1.0, 3.0])
    head, Wp, S, P = widths(case)
    assert P == (87 if case == "go2_robust" else 50)
    R = env.priv_params
    assert list(R.friction) == [F((0.1 + 1.25) / 2), F(2 / (1.25 - 0.1))] and list(R.added_mass) == [1.0, 0.5]
    env._sync_stream()
    fr, ms = np.array([0.1, 0.7, 2.5], F), np.array([-1.0, 1.25, 2.5], F)
    env.sim.set_env_properties(fr, ms)
    env.shape_friction, env.added_base_mass = fr, ms
    if env.actuator_rand.enabled:
        D = env.num_dof
        e = torch.arange(n, device=env.device, dtype=torch.float).view(n, 1)
        j = torch.arange(D, device=env.device, dtype=torch.float).view(1, D)
        env.kp_factors.copy_(0.93 + 0.04 * e + 0.005 * j)      # 0.93 .. 1.065, and past the range's end
        env.kd_factors.copy_(1.2 - 0.1 * e - 0.01 * j)         # below 0.91: the clip
        env.motor_strengths.copy_(0.95 + 0.03 * e + 0.004 * j)
        env.action_delay_substeps.copy_(torch.tensor([0, 1, 4], dtype=torch.int32, device=env.device))
    left = state_rows(env)
    g = torch.Generator(device="cuda").manual_seed(3)
    env.step(actions(env, g, 0.3))
    got = env_arrays(env)
    assert not got["reset"].any()
    assert_state_rows_equal(state_rows(env), left, "no env reset: the rows are the ones written")
    tail, want = got["priv_obs"][:, head:head + Wp], expected_tail(env)
    assert want.shape == (n, Wp)
    assert same(tail, want)
    assert (np.abs(want) == F(0.9)).any() and (np.abs(want) < F(0.9)).any(), "clipped and unclipped entries"
    assert len(np.unique(want[:, :2])) == 6 - 1   # (2.5 on both groups clips to 0.9)
    if env.actuator_rand.enabled:
        inner = want[:, 2:][np.abs(want[:, 2:]) < F(0.9)]
        assert len(np.unique(inner)) > 3 * env.num_dof, "distinct values per env and DOF: an index mix-up shows"
    # the clean frame is clipped like the observations
    assert (np.abs(got["priv_obs"]) <= F(0.9)).all()


# --------------------------------------------- 4. lgs_reset_idx, lgs_reset_all ---
def test_first_row_after_reset_idx_and_reset_all_carries_the_rows_the_call_left(build):
    n = 3
    env = build("go2_robust", n, True, short=False)
    head, Wp, S, P = widths("go2_robust")
    g = torch.Generator(device="cuda").manual_seed(11)
    for _ in range(2):
        env.step(actions(env, g, 0.3))
    snap = torch.empty(env._ep_means.numel(), dtype=torch.float, device=env.device)
    for route, byte, hit in (("reset_idx byte 1", 1, [0, 2]), ("reset_idx byte 2", 2, [1]), ("reset_all", 0, [0, 1, 2])):
        env._sync_stream()
        env.flush_extras()
        before, priv_before = state_rows(env), [b.clone() for b in env._priv_bufs]
        E, k = env._env_structs[env._buf_idx], env.common_step_counter
        E.ep_snapshot = snap.data_ptr()
        if byte:
            mask = torch.zeros(n, dtype=torch.uint8, device=env.device)
            mask[hit] = byte
            env.sim.reset_idx(E, mask, k)
        else:
            env.sim.reset_all(E, k)
        left = state_rows(env)
        for e in range(n):
            changed = not all(np.array_equal(left[r][e], before[r][e]) for r in ROWS)
            assert changed == (e in hit), f"{route}: env {e}"
        for b, pb in zip(env._priv_bufs, priv_before):  # a reset call writes no row, of any env
            assert torch.equal(b, pb), route
        env.step(actions(env, g, 0.3))
        got = env_arrays(env)
        assert_state_rows_equal(state_rows(env), left, route + ": the step after the call resets no env")
        assert same(got["priv_obs"][:, head:head + Wp], expected_tail(env, left)), route


# ------------------------------------------------------ 6. the split path ---
@pytest.mark.parametrize("case,n", [("go2_robust_history", 2), ("h1_act", 2)])
def test_split_path_writes_the_row_of_the_fused_step(build, case, n):
    """lgs_step_physics, _prepare, _term_rewards, _finish against lgs_step with the switch on,
    through staggered resets: every buffer, the privileged row included."""
    fused, split = build(case, n, True), build(case, n, True)
    g = torch.Generator(device="cuda").manual_seed(5)
    stagger(fused)
    stagger(split)
    resets = np.zeros(n, bool)
    for it in range(STEPS):
        a = actions(fused, g, 0.5)
        fused.step(a)
        ref = env_arrays(fused)
        got = split_step(split, a, True)
        assert_exact(got, ref, STATE + POST, n, f"{case} step {it}: split vs fused")
        assert_state_rows_equal(state_rows(split), state_rows(fused), f"{case} step {it}")
        resets |= ref["reset"].astype(bool).ravel()
    assert resets.all()


# ------------------------------------------------------------ 7. refusals ---
def _entry_points(env):
    E, k = env._env_structs[env._buf_idx], env.common_step_counter
    mask = torch.ones(env.num_envs, dtype=torch.uint8, device=env.device)
    return (lambda: env.sim.step(E, k), lambda: env.sim.step_physics(E, k), lambda: env.sim.reset_all(E, k),
            lambda: env.sim.reset_idx(E, mask, k), lambda: env.sim.post_physics_finish(E, k),
            lambda: env.sim.step_deferred(E, k))


def _refused(env, match):
    for call in _entry_points(env):
        with pytest.raises(native.LeggedSimError, match=match):
            call()


def _untouched(env, before):
    torch.cuda.synchronize()
    for key in ("root_states", "dof_state", "actions", "_episode_length"):  # nothing was launched
        assert torch.equal(getattr(env, key), before[key]), key


def test_entry_points_refuse_a_bad_descriptor_before_any_launch(build):
    env = build("go2_robust", 2, True)
    lib, h = env.sim.lib, env.sim.handle
    assert lib.lgs_set_privileged_parameters(h, None) == -1 and b"null" in lib.lgs_last_error()
    good = cabi.PrivParams.from_buffer_copy(env.priv_params)
    env._sync_stream()
    env.flush_extras()
    before = {k: getattr(env, k).clone() for k in ("root_states", "dof_state", "actions", "_episode_length")}
    priv_before = [b.clone() for b in env._priv_bufs]
    # a non-finite offset or scale, in any group
    for group, i, v in (("friction", 0, float("nan")), ("kp", 1, float("inf")), ("delay", 0, float("-inf")),
                        ("added_mass", 1, float("nan"))):
        bad = cabi.PrivParams.from_buffer_copy(good)
        getattr(bad, group)[i] = v
        env.sim.set_privileged_parameters(bad)
        _refused(env, "finite offset and scale")
    env.sim.set_privileged_parameters(good)
    # a num_privileged_obs other than the row's: the message names the width it would have to be
    T = copy.deepcopy(env.task_params)
    for P in (86, 88, 48, 0):
        T.num_privileged_obs = P
        env.sim.set_task(T)
        _refused(env, rf"num_privileged_obs is {P}, the row is the head \(48\) \+ the parameter tail \(39\) \+ 0 scan points = 87")
    # the quadruped's own bound gives way with the descriptor on, and only then
    T.num_privileged_obs = 129
    env.sim.set_task(T)
    _refused(env, "= 87")
    env.sim.set_privileged_parameters(cabi.PrivParams())
    _refused(env, "exceed LGS_MAX_OBS")
    env.sim.set_task(env.task_params)
    _untouched(env, before)
    for b, pb in zip(env._priv_bufs, priv_before):
        assert torch.equal(b, pb)
    # off: the 87-wide buffer is one no kernel writes; the good descriptor steps again
    env.step(torch.zeros(2, env.num_actions, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(env.privileged_obs_buf, priv_before[env._buf_idx])
    env.sim.set_privileged_parameters(good)
    env.step(torch.zeros(2, env.num_actions, device="cuda"))
    assert same(env_arrays(env)["priv_obs"][:, 48:], expected_tail(env))


def test_the_handstand_layout_and_an_oversize_head_are_refused(build):
    on = cabi.PrivParams()
    on.enabled = 1
    for g in cabi.PRIV_GROUPS:
        getattr(on, g)[:] = (0.0, 1.0)
    env = make("go2_handstand", 2)
    try:
        env.reset()
        env._sync_stream()
        env.flush_extras()
        before = {k: getattr(env, k).clone() for k in ("root_states", "dof_state", "actions", "_episode_length")}
        env.sim.set_privileged_parameters(on)
        _refused(env, "handstand layout's privileged row is its noisy frame")
        _untouched(env, before)
        env.sim.set_privileged_parameters(cabi.PrivParams())
        env.step(torch.zeros(2, env.num_actions, device="cuda"))
    finally:
        env.close()
    # a G1 with 23 DOFs and the actuator group: 83 + 72 does not fit, and the message has the numbers
    _register_g1_23dof()
    env = make("g1_23dof", 2, **ON)
    try:
        env.reset()
        env._sync_stream()
        env.flush_extras()
        before = {k: getattr(env, k).clone() for k in ("root_states", "dof_state", "actions", "_episode_length")}
        env.sim.set_privileged_parameters(on)
        _refused(env, r"the head \(83\) \+ the parameter tail \(72\) = 155 exceed LGS_MAX_OBS \(128\)")
        _untouched(env, before)
        env.sim.set_privileged_parameters(cabi.PrivParams())
        env.step(torch.zeros(2, env.num_actions, device="cuda"))
    finally:
        env.close()
        bridge.set_ground(bridge.ensure_built())


# -------------------------------------------------------------- 8. runner ---
def test_runner_trains_go2_robust_asym_on_the_fused_step_and_the_captured_rollout():
    """OnPolicyRunner.learn(3) on go2_robust_asym, 64 envs, episodes shorter than a rollout: the
    one-launch forward and the one-launch rollout step are taken with a 240-input actor and an
    87-input critic (padded 240 / 96), the stored critic rows are the env's, and collecting
    through the captured graph equals collecting eagerly, bitwise, in storage and parameters (after
    three iterations, so after two as well: the chain is deterministic)."""
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (True, False):
        env = make("go2_robust_asym", 64, env__episode_length_s=0.3)
        assert env.priv_params.enabled == 1 and (env.num_obs, env.num_privileged_obs) == (240, 87)
        _, train_cfg = task_registry.get_cfgs("go2_robust_asym")
        cfg = copy.deepcopy(class_to_dict(train_cfg))
        assert cfg["runner"]["experiment_name"] == "go2_robust_asym"
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        alg = runner.alg
        assert alg._fused is not None and alg._rollout is not None, "native PPO path not active"
        # (the loss joins the forward's launch from mini-batches of 96 * 192 rows up, whatever the
        # widths: at 64 envs it cannot; test_fused_update_with_an_87_input_critic... runs that size)
        assert alg._fused.fused_fwd and alg._fused.wf is not None and alg._fused.k0p == [240, 96]
        assert alg.actor_critic.critic[0].in_features == 87 and alg.actor_critic.actor[0].in_features == 240
        st = alg.storage
        assert alg._rollout.usable(env.get_observations(), env.get_privileged_observations(), st)
        runner.learn(3)
        env.flush_extras()
        torch.cuda.synchronize()
        if graph:
            assert runner._rollout_graph is not None and not getattr(runner, "_rollout_graph_failed", False)
        else:
            assert runner._rollout_graph is None
        assert st.privileged_observations.shape[-1] == 87 and st.observations.shape[-1] == 240
        pv, d = st.privileged_observations, st.dones.reshape(st.dones.shape[0], -1).bool()
        assert d.any() and torch.isfinite(pv).all()
        # the stored critic rows are the env's: the last one was written by the step before the last,
        # and an env the last step did not reset still has the rows that one showed
        keep = (~d[-1]).cpu().numpy()
        want = expected_tail(env)
        assert keep.any() and same(t2n(pv[-1])[keep, 48:], want[keep])
        assert same(t2n(env.privileged_obs_buf)[:, 48:], want)
        # a clean frame: where the policy row's newest frame is the noisy one
        assert not torch.equal(pv[:, :, :48], st.observations[:, :, 192:])
        out[graph] = dict(storage=[t.clone() for t in (st.observations, pv, st.actions, st.values, st.rewards,
                                                       st.dones, st.returns, st.advantages)],
                          params=[p.detach().clone() for p in alg.actor_critic.parameters()],
                          priv=env.privileged_obs_buf.clone())
        env.close()
    for key in ("storage", "params"):
        for a, b in zip(out[True][key], out[False][key]):
            assert torch.equal(a, b), key
    assert torch.equal(out[True]["priv"], out[False]["priv"])


def _fill_asym(alg, T, N, O, CO, A, seed):
    """tests/test_gpu_fused_ppo.py's _fill_storage with critic rows of their own width."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ro, alg._rollout = alg._rollout, None  # the reference act()/process_env_step path (custom actions)
    with torch.inference_mode():
        for _ in range(T):
            obs, cobs = torch.randn(N, O, device="cuda", generator=g), torch.randn(N, CO, device="cuda", generator=g)
            alg.act(obs, cobs)
            alg.transition.actions = alg.transition.action_mean + 0.3 * torch.randn(N, A, device="cuda", generator=g)
            alg.transition.actions_log_prob = alg.actor_critic.get_actions_log_prob(alg.transition.actions).detach()
            rew = 0.2 * torch.randn(N, device="cuda", generator=g)
            done = torch.rand(N, device="cuda", generator=g) < 0.05
            alg.process_env_step(rew, done, {"time_outs": done & (torch.rand(N, device="cuda", generator=g) < 0.5)})
        alg.compute_returns(torch.randn(N, CO, device="cuda", generator=g))
    alg._rollout = ro
    return {k: v.clone() for k, v in alg.storage.__dict__.items() if torch.is_tensor(v) and not k.startswith("_")}


def test_fused_update_with_an_87_input_critic_matches_the_fp32_autograd_update():
    """tests/test_gpu_wide_mlp.py's test_fused_update_at_235_inputs_matches_the_fp32_autograd_update
    with go2_robust_asym's widths -- a 240-input actor beside an 87-input critic padded to 96 -- at
    mini-batches of 18,432 rows: the forward of both nets and the loss in one launch, the critic's
    96-wide first-layer weight gradient, the staged copy (87 != 96) and the fragment mirror.  The
    bars are that test's.  go2_terrain_robust_asym's widths take the same path at 448 / 320."""
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCritic, mfma_mlp
    from test_gpu_wide_mlp import A, HID
    O, CO, N, T = 240, 87, 2048, 18
    torch.manual_seed(0)
    ac32 = ActorCritic(O, CO, A, HID, HID, mixed_precision=False).cuda()
    acbf = copy.deepcopy(ac32)
    acbf.mixed_precision = True
    kw = dict(learning_rate=1e-3, device="cuda", num_learning_epochs=1, num_mini_batches=2, schedule="adaptive")
    ref = PPO(ac32, fused_loss=False, **kw)
    ref.use_graph = False
    fus = PPO(acbf, **kw)
    for alg in (ref, fus):
        alg.init_storage(N, T, [O], [CO], [A])
    f = fus._fused
    assert f is not None and ref._fused is None and f.fused_fwd and f.fused_loss and f.M == 18432
    assert f.k0p == [240, 96] and f.dw_stage[0][0] is None and f.dw_stage[0][1] is not None
    data = _fill_asym(ref, T, N, O, CO, A, seed=1)
    for k, v in data.items():
        getattr(fus.storage, k).copy_(v)
    fus.storage.step = T
    p0 = [p.detach().clone() for p in ref.actor_critic.parameters()]
    torch.manual_seed(7)
    l_ref = ref.update()
    torch.manual_seed(7)
    l_fus = fus.update()
    print("losses fused / fp32:", l_fus, l_ref)
    np.testing.assert_allclose(l_fus, l_ref, rtol=2e-2, atol=2e-3)
    assert fus.learning_rate == pytest.approx(ref.learning_rate, rel=1e-6)
    lr = 1e-3
    for a, b, c in zip(ref.actor_critic.parameters(), fus.actor_critic.parameters(), p0):
        da, db = (a.detach() - c), (b.detach() - c)
        assert da.abs().max() > 0
        bad = ((da - db).abs() > 0.2 * lr).float().mean().item()
        print("share of entries off by > 0.2 lr:", tuple(a.shape), bad, "max", float((da - db).abs().max()))
        assert bad < 0.02, bad
        assert (da - db).abs().max() <= 4 * 3 * lr
    # the bf16 operands of the next forward follow the fp32 weights; the padded columns stay zero
    w = fus.actor_critic.critic[0].weight.detach()
    assert torch.equal(f.wb[1][0][:, :CO], w.to(torch.bfloat16)) and not f.wb[1][0][:, CO:].float().abs().any()
    assert torch.equal(f.wf[1][0], mfma_mlp.frag_pack(f.wb[1][0], 512))
    # go2_terrain_robust_asym: 427 beside 274
    torch.manual_seed(0)
    big = PPO(ActorCritic(427, 274, A, HID, HID).cuda(), **kw)
    big.init_storage(N, T, [427], [274], [A])
    assert big._fused.fused_fwd and big._fused.fused_loss and big._fused.k0p == [448, 320]


def test_train_then_play_go2_robust_asym():
    """train.py --task go2_robust_asym, then play.py (which turns the noise, the friction
    randomisation and the pushes off: the critic's 87 inputs still load) and its export."""
    import glob
    import os
    from test_gpu_scripts import run
    exp = "pytest_go2_robust_asym"
    out = run("train.py", "--task", "go2_robust_asym", "--num_envs", "64", "--max_iterations", "2", "--headless",
              "--experiment_name", exp, "--run_name", "cli")
    assert "Learning iteration 1/2" in out
    from legged_gym import LEGGED_GYM_ROOT_DIR
    runs = sorted(glob.glob(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "*_cli")))
    assert runs, "train.py wrote no run directory"
    ck = os.path.join(runs[-1], "model_2.pt")
    assert os.path.exists(ck)
    sd = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    assert sd["critic.0.weight"].shape[1] == 87 and sd["actor.0.weight"].shape[1] == 240
    run("play.py", "--task", "go2_robust_asym", "--headless", "--experiment_name", exp, "--load_run",
        os.path.basename(runs[-1]))
    assert os.path.exists(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "exported", "policies", "policy_1.pt"))
