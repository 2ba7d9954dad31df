"""Observation history inside the fused env step, on the GPU.

The CPU oracle does not know the feature and need not: the history row is a pure function of the
rows and reset flags of the same env stepped without it, and the frame's arithmetic and draws do
not move.  So the reference is a twin env -- same task, seed and actions, history off -- with the
numpy restatement of "shift, append, fill after reset" (tests/test_obs_history_host.py, checked
there against hand-written rows) on top of it.  Every comparison is exact.

Shapes: Go2 x 3 (odd: one env per wave) and Go2 x 4 (two envs per wave: 32 lanes for 48 entries,
a partial second pass), each with H = 2 (one old slot: the shift degenerates) and H = 5 (the
task's); G1 x 2 (humanoid layout, privileged row, 47-wide frame); the Go2 handstand x 2 (46 is no
multiple of 4, contact-flag flips, the privileged row is the noisy frame).  Episodes are 7
control steps and the envs' episode counters are staggered, so time-outs fall on different steps.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from legged_gym.envs import task_registry  # noqa: E402
from leggedsim import cabi, native  # noqa: E402
from test_gpu_parity import POST, STATE, assert_exact, env_arrays, make, restore, save  # noqa: E402
from test_gpu_post_physics_branches import split_step  # noqa: E402
from test_obs_history_host import stack_row  # noqa: E402

FRAME = {"go2": 48, "g1": 47, "go2_handstand": 46}
SHAPES = [("go2", 3, 2), ("go2", 3, 5), ("go2", 4, 2), ("go2", 4, 5), ("g1", 2, 5), ("go2_handstand", 2, 5)]
EPISODE = 7
REST = [k for k in STATE + POST if k != "obs"]  # everything but the policy row is the twin's, bitwise


@pytest.fixture
def build():
    envs = []

    def _build(task, n, H, noise=True, **edits):
        c = task_registry.get_cfgs(task)[0]
        edits = dict(edits, noise__add_noise=noise,
                     env__episode_length_s=(EPISODE - 0.5) * c.control.decimation * c.sim.dt)
        if H > 1:
            edits.update(env__history_length=H, env__num_observations=H * FRAME[task])
        env = make(task, n, **edits)
        envs.append(env)
        assert int(env.max_episode_length) == EPISODE and env.num_obs_frame == FRAME[task]
        if H > 1:
            assert env.obs_history.shape == (n, (H - 1) * FRAME[task]) and env.obs_history.dtype == torch.float32
            assert env._obs_history_fill.shape == (n,) and env._obs_history_fill.dtype == torch.int32
            assert env.obs_buf.shape == (n, H * FRAME[task]) and not env._split_step
            assert not env.obs_history.any() and not env._obs_history_fill.any()
        else:
            assert env.obs_history is None and env._obs_history_fill is None
        return env
    yield _build
    for env in envs:
        env.close()
    bridge.set_ground(bridge.ensure_built())


def t2n(t):
    return t.detach().cpu().numpy().copy()


def actions(env, g, scale=0.5):
    return scale * torch.randn(env.num_envs, env.num_actions, device="cuda", generator=g)


class Pair:
    """An env with the history and its twin without, driven in lockstep."""

    def __init__(self, build, task, n, H, noise):
        self.h, self.t = build(task, n, H, noise), build(task, n, 1, noise)
        self.n, self.H, self.F = n, H, FRAME[task]
        self.prev = np.zeros((n, H * self.F), np.float32)
        self.fresh = np.ones(n, bool)      # reset since the env's last row (zeroed buffers: fill on first write)
        self.episode = [[] for _ in range(n)]  # the twin's frames of each env's running episode
        self.resets, self.timeouts, self.alone = np.zeros(n, int), 0, 0

    def both(self, fn):
        for env in (self.h, self.t):
            env._sync_stream()
            fn(env)

    def check(self, what):
        h, t, n, H, F = self.h, self.t, self.n, self.H, self.F
        got, ref = env_arrays(h), env_arrays(t)
        assert_exact(got, ref, REST, n, what + ": everything but the policy row vs the twin")
        frame, row = ref["obs"], got["obs"]
        assert frame.shape == (n, F) and row.shape == (n, H * F)
        reset = ref["reset"].astype(bool).ravel()
        fresh = self.fresh | reset
        want = stack_row(self.prev, frame, fresh, H)
        assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), what + ": the row vs shift / append / fill"
        # the same, slot by slot from the twin's own record: slot k steps back is the twin's row k
        # steps earlier in the episode, or the episode's first one where it is younger than that
        for e in range(n):
            if fresh[e]:
                self.episode[e] = []
            self.episode[e].append(frame[e])
            ep = self.episode[e]
            for k in range(H):
                src = ep[max(len(ep) - 1 - k, 0)]
                assert np.array_equal(row[e, (H - 1 - k) * F:(H - k) * F], src), f"{what}: env {e} slot {k} steps back"
            if fresh[e]:
                assert (row[e].reshape(H, F) == frame[e]).all(), f"{what}: env {e}: the first row of an episode"
        assert np.array_equal(t2n(h.obs_history), row[:, F:]), what + ": obs_history is row[:, F:]"
        assert (t2n(h._obs_history_fill) == 1).all(), what + ": the flags after a row"
        self.prev, self.fresh = row.copy(), np.zeros(n, bool)
        self.resets += reset
        self.timeouts += int(ref["time_out"].astype(bool).sum())
        self.alone += int(n >= 2 and reset[:2].sum() == 1)
        return reset

    def step(self, a, what):
        self.h.step(a)
        self.t.step(a)
        return self.check(what)


def stagger(env):
    env._sync_stream()
    env.episode_length_buf = torch.tensor([EPISODE - 2 - e for e in range(env.num_envs)], device=env.device)


# ------------------------------------------- 1. the rows, on every reset route ---
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("task,n,H", SHAPES)
def test_history_rows_are_the_twins_rows_stacked_on_every_reset_route(build, task, n, H, noise):
    p = Pair(build, task, n, H, noise)
    h, t = p.h, p.t
    assert h.task_params.add_noise == int(noise) and h.task_params.num_obs == H * p.F
    assert (h.task_params.num_privileged_obs, h.privileged_obs_buf is None) == \
           (t.task_params.num_privileged_obs, t.privileged_obs_buf is None)
    h.sim.set_task(h.task_params)  # (the two setters in the other order)
    g = torch.Generator(device="cuda").manual_seed(100 * n + H)
    # BaseTask.reset(): reset_idx of every env (mask byte 1; 2 under a level curriculum), then a
    # zero-action step that writes the episode's first row
    p.both(lambda env: env.reset())
    p.fresh[:] = True
    p.check("reset()")
    for it in range(3):
        assert not p.step(actions(h, g), f"warm step {it}").any()
    # time-outs, one env after the other
    p.both(stagger)
    for it in range(8):
        p.step(actions(h, g), f"time-out run step {it}")
    assert (p.resets >= 1).all() and p.timeouts >= n, "every env times out inside the run"
    assert p.alone >= 1, "a step in which one env of the first wave resets alone"
    # termination: env 0 tipped on its side through the root state
    def tip(env):
        env.root_states[0, 3:7] = torch.tensor([2 ** -0.5, 0.0, 0.0, 2 ** -0.5], device=env.device)
    p.both(tip)
    before = p.resets.copy()
    reset = p.step(actions(h, g), "termination step")
    assert reset[0] and not bool(t.time_out_buf[0]), "env 0 terminates without a time-out"
    for it in range(2):
        p.step(actions(h, g), f"after the termination, step {it}")
    # reset_idx on a subset: the row is written by the next launch
    ids = torch.tensor([n - 1], device=h.device)
    p.both(lambda env: env.reset_idx(ids))
    torch.cuda.synchronize()
    assert t2n(h._obs_history_fill).tolist() == [1] * (n - 1) + [0]
    assert np.array_equal(t2n(h.obs_history), p.prev[:, p.F:]), "a reset leaves the stored frames alone"
    p.fresh[n - 1] = True
    for it in range(2):
        p.step(actions(h, g), f"after reset_idx, step {it}")
    # lgs_reset_all (the C entry point BaseTask.reset does not go through)
    p.both(lambda env: env.sim.reset_all(env._env_structs[env._buf_idx], env.common_step_counter))
    torch.cuda.synchronize()
    assert not t2n(h._obs_history_fill).any()
    p.fresh[:] = True
    for it in range(3):
        p.step(actions(h, g), f"after lgs_reset_all, step {it}")
    assert (p.resets > before).any()


# ------------------------------------------------------ 2. the split path ---
HIST = ("obs_history", "_obs_history_fill")


@pytest.mark.parametrize("task,n,H", [s for s in SHAPES if s[2] == 5])
def test_split_path_is_the_fused_step_bitwise_with_the_history_on(build, task, n, H):
    """lgs_step_physics + lgs_post_physics, and physics + prepare / term_rewards / finish, from the
    same state, history and flags: the fused lgs_step's buffers, rows, history and flags, resets
    included."""
    env = build(task, n, H)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(30 + n)
    for _ in range(2):
        env.step(actions(env, g))
    stagger(env)
    resets = 0
    for it in range(6):
        a = actions(env, g)
        st, h0 = save(env), {k: getattr(env, k).clone() for k in HIST}
        env.step(a)
        fused, hf = env_arrays(env), {k: t2n(getattr(env, k)) for k in HIST}
        resets += int(fused["reset"].sum())
        for three in (False, True):
            restore(env, st)
            for k in HIST:
                getattr(env, k).copy_(h0[k])
            parts = split_step(env, a, three)
            what = f"{task} x{n} step {it}: {'prepare/term_rewards/finish' if three else 'physics + post'}"
            assert_exact(parts, fused, STATE + POST, n, what)
            for k in HIST:
                assert np.array_equal(t2n(getattr(env, k)), hf[k]), f"{what}: {k}"
    assert resets >= n


# ------------------------------------------- 3. the state is the caller's ---
def test_editing_the_history_and_the_flag_between_steps_shows_in_the_next_row(build):
    n, H, F = 4, 3, 48
    env = build("go2", n, H)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(2):
        env.step(actions(env, g))
    env._sync_stream()
    mine = torch.arange(n * (H - 1) * F, device=env.device, dtype=torch.float).view(n, (H - 1) * F) * 0.25 - 7.0
    env.obs_history.copy_(mine)
    env._obs_history_fill[2] = 0  # by hand: env 2's next row fills every slot
    env.step(actions(env, g))
    torch.cuda.synchronize()
    assert not env.reset_buf.any()
    row, mine = t2n(env.obs_buf), t2n(mine)
    frame = row[:, (H - 1) * F:]
    for e in (0, 1, 3):
        assert np.array_equal(row[e, :(H - 1) * F], mine[e]), e          # the older slots: the edited frames
        assert np.array_equal(t2n(env.obs_history)[e], np.concatenate([mine[e, F:], frame[e]])), e
    assert (row[2].reshape(H, F) == frame[2]).all() and not np.array_equal(frame[2], mine[2, :F])
    assert (t2n(env._obs_history_fill) == 1).all()


# ------------------------------------------------------------ the C ABI -----
def test_entry_points_refuse_an_inconsistent_history_before_any_launch(build):
    n, H = 2, 5
    env = build("go2", n, H)
    env.reset()
    env.step(torch.zeros(n, env.num_actions, device="cuda"))
    torch.cuda.synchronize()
    lib, hdl, tp = env.sim.lib, env.sim.handle, env.task_params
    assert lib.lgs_set_observation_history(hdl, None) == -1 and b"null" in lib.lgs_last_error()
    good = cabi.ObsHistory.from_buffer_copy(env.obs_history_params)
    bufs = env.sim._ohist_buffers
    E = env._env_structs[env._buf_idx]
    k = env.common_step_counter
    mask = torch.ones(n, dtype=torch.uint8, device=env.device)
    keep = ("root_states", "dof_state", "obs_buf", "_episode_length", "_d_step_counter", "actions", "obs_history",
            "_obs_history_fill")

    def refused(match):
        before = {key: t2n(getattr(env, key)) for key in keep}
        for call in (lambda: lib.lgs_step(hdl, C.byref(E), k), lambda: lib.lgs_step_deferred(hdl, C.byref(E), k),
                     lambda: lib.lgs_post_physics(hdl, C.byref(E), k),
                     lambda: lib.lgs_post_physics_finish(hdl, C.byref(E), k),
                     lambda: lib.lgs_reset_idx(hdl, C.byref(E), mask.data_ptr(), k),
                     lambda: lib.lgs_reset_all(hdl, C.byref(E), k)):
            assert call() == -1  # LGS_ERR_ARG
            assert match in lib.lgs_last_error().decode(), lib.lgs_last_error().decode()
        torch.cuda.synchronize()
        for key in keep:  # nothing was launched
            np.testing.assert_array_equal(t2n(getattr(env, key)), before[key], err_msg=key)

    def with_desc(edit, match):
        bad = cabi.ObsHistory.from_buffer_copy(good)
        edit(bad)
        env.sim.set_observation_history(bad, bufs)
        refused(match)

    try:
        with_desc(lambda R: setattr(R, "frames", 1), "outside 2 .. LGS_MAX_OBS_FRAMES")
        with_desc(lambda R: setattr(R, "frames", 9), "outside 2 .. LGS_MAX_OBS_FRAMES")
        with_desc(lambda R: setattr(R, "history", None), "needs the history and fill buffers")
        with_desc(lambda R: setattr(R, "fill", None), "needs the history and fill buffers")
        with_desc(lambda R: setattr(R, "frames", 4), "num_obs 240 is not 4 frames of the layout's head (48)")
        env.sim.set_observation_history(good, bufs)
        tp.num_obs = 239
        env.sim.set_task(tp)
        refused("num_obs 239 is not 5 frames of the layout's head (48)")
        tp.num_obs = 240
        env.sim.set_task(tp)
        scan = cabi.HeightObs(1, 0.5, 1.0, 5.0, 0.0)
        env.sim.set_height_observations(scan)
        refused("observation history and height observations do not combine")
        env.sim.set_height_observations(None)
        env.sim.set_observation_history(cabi.ObsHistory())  # off: 240 entries are past the layout's own row
        refused("exceed LGS_MAX_OBS")
    finally:
        tp.num_obs = 240
        env.sim.set_task(tp)
        env.sim.set_height_observations(None)
        env.sim.set_observation_history(good, bufs)
    prev = t2n(env.obs_buf)
    env.step(torch.zeros(n, env.num_actions, device="cuda"))  # consistent again: the step runs
    torch.cuda.synchronize()
    assert np.array_equal(t2n(env.obs_buf)[:, :4 * 48], prev[:, 48:])


def test_the_handstand_row_without_a_history_is_still_its_own_width(build):
    """lgs_set_task lets a whole number of handstand frames through (the history may be set later);
    without a history the entry points hold the row to 6 + 3 A + num_feet, as lgs_set_task did."""
    env = build("go2_handstand", 2, 1)
    env.reset()
    tp = env.task_params
    E = env._env_structs[env._buf_idx]
    try:
        tp.num_obs = 47
        with pytest.raises(native.LeggedSimError, match="handstand layout has"):
            env.sim.set_task(tp)
        tp.num_obs = 92
        env.sim.set_task(tp)
        with pytest.raises(native.LeggedSimError, match="handstand layout has"):
            env.sim.step(E, env.common_step_counter)
    finally:
        tp.num_obs = 46
        env.sim.set_task(tp)
    env.step(torch.zeros(2, env.num_actions, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isfinite(env.obs_buf).all()


# ------------------------------------------------- 4. the captured rollout ---
def test_runner_collects_go2_robust_history_through_the_captured_graph():
    """OnPolicyRunner.learn(2) on go2_robust_history, 64 envs, episodes shorter than a rollout: the
    second iteration's collection replays the captured graph, the update is the fused one on 240
    inputs, and storage, policy, history and flags equal an eager-collecting twin's, bitwise."""
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (True, False):
        env = make("go2_robust_history", 64, env__episode_length_s=0.3)
        assert env.obs_history_params.enabled == 1 and env.num_obs == 240 and env.actuator_rand.enabled == 1
        _, train_cfg = task_registry.get_cfgs("go2_robust_history")
        cfg = copy.deepcopy(class_to_dict(train_cfg))
        assert cfg["runner"]["experiment_name"] == "go2_robust_history"
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
        assert st.observations.shape[-1] == 240
        out[graph] = dict(storage=[t.clone() for t in (st.observations, st.actions, st.actions_log_prob, st.mu, st.sigma,
                                                       st.values, st.rewards, st.dones, st.returns, st.advantages)],
                          params=[p.detach().clone() for p in runner.alg.actor_critic.parameters()],
                          hist=[env.obs_history.clone(), env._obs_history_fill.clone()], obs=env.obs_buf.clone())
        assert st.dones.any(), "episodes end inside the rollout"
        assert all(torch.isfinite(t.float()).all() for t in out[graph]["storage"])
        # the stored rows are histories: a step's four older slots are the previous step's four newest,
        # except where the env's episode ended in between
        o, d = st.observations, st.dones.reshape(st.dones.shape[0], -1).bool()
        same = (o[1:, :, :192] == o[:-1, :, 48:]).all(dim=-1)
        assert same[~d[:-1]].all() and not same[d[:-1]].all()
        first = o[1:][d[:-1]]
        assert (first.reshape(-1, 5, 48) == first[:, None, 192:]).all()
        assert torch.equal(env.obs_history, env.obs_buf[:, 48:]) and (env._obs_history_fill == 1).all()
        env.close()
    for key in ("storage", "params", "hist"):
        for a, b in zip(out[True][key], out[False][key]):
            assert torch.equal(a, b), key
    assert torch.equal(out[True]["obs"], out[False]["obs"])
