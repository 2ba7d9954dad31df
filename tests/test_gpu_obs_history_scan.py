"""The observation history in front of the height scan, on the GPU: the policy row
is [frame(t-H+1) | ... | frame(t) | scan(t)], H * F + P entries.

The CPU oracle knows neither feature.  As in tests/test_gpu_obs_history.py the reference is a twin
env -- same task, map, seed, actions and interventions, scan observed, history off -- with the
numpy restatement of "shift, append, fill after reset" (tests/test_obs_history_host.py) on the
twin's first F entries; the scan's entries are the twin's own, because scan point k keeps noise
draw F + k.  Every comparison is exact.

Shapes: Go2 x 3 (odd: one env per wave) and x 4 (two per wave), each with H = 2 and H = 5; G1
terrain x 2 with H = 2 (humanoid layout, 47-wide frames, 281 / 237 rows: the one-env-per-wave
build with the highest register pressure).  Maps: 3 rows x 2 cols of 8 m tiles.  Resets: forced
time-outs, terminations (a robot rolled past the limit), reset_idx(env_ids) (mask byte 1),
reset() (mask byte 2 under the level curriculum) and lgs_reset_all.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from leggedsim import cabi  # noqa: E402
from test_gpu_height_obs import TERRAIN_STATE, intervene, script  # noqa: E402
from test_gpu_parity import POST, STATE, assert_exact, env_arrays, make, restore, save  # noqa: E402
from test_gpu_post_physics_branches import split_step  # noqa: E402
from test_gpu_terrain_curriculum import MAP, SHORT, t2n  # noqa: E402
from test_obs_history_host import stack_row  # noqa: E402

FRAME = {"go2": 48, "g1": 47}
P = 187
SHAPES = [("go2", 3, 2), ("go2", 3, 5), ("go2", 4, 2), ("go2", 4, 5), ("g1", 2, 2)]
REST = [k for k in STATE + POST if k != "obs"]  # the privileged rows among them: bitwise the twin's
MAP_STATE = TERRAIN_STATE + ("measured_heights",)
HIST = ("obs_history", "_obs_history_fill")


@pytest.fixture
def build():
    envs = []

    def _build(robot, n, H, noise=True):
        F = FRAME[robot]
        kw = dict(MAP, **SHORT, noise__add_noise=noise, terrain__scan_in_observations=True,
                  env__num_observations=H * F + P)
        if H > 1:
            kw.update(env__history_length=H)
        if robot == "go2":
            kw.update(terrain__level_curriculum=True, terrain__scan_heights=True)
            env = make("go2", n, **kw)
        else:
            env = make("g1_terrain", n, **dict(kw, env__num_privileged_obs=50 + P))
        envs.append(env)
        assert env.obs_buf.shape == (n, H * F + P) and env.num_scan_obs == P and not env._split_step
        assert env.height_obs.enabled == 1 and env.task_params.num_obs == H * F + P
        if H > 1:
            assert env.obs_history_params.enabled == 1 and env.num_obs_frame == F
            assert env.obs_history.shape == (n, (H - 1) * F) and env._obs_history_fill.shape == (n,)
        else:
            assert env.obs_history is None
        if robot == "g1":
            assert env.privileged_obs_buf.shape == (n, 50 + P)
        return env
    yield _build
    for env in envs:
        env.close()
    bridge.set_ground(bridge.ensure_built())


class Pair:
    """An env with the history in front of its scan and its twin with the scan alone, in lockstep."""

    def __init__(self, build, robot, n, H, noise):
        self.h, self.t = build(robot, n, H, noise), build(robot, n, 1, noise)
        self.n, self.H, self.F = n, H, FRAME[robot]
        self.prev = np.zeros((n, H * self.F), np.float32)
        self.fresh = np.ones(n, bool)
        self.resets, self.timeouts, self.terminations = np.zeros(n, int), 0, 0

    def both(self, fn):
        for env in (self.h, self.t):
            env._sync_stream()
            fn(env)

    def check(self, what):
        h, t, n, H, F = self.h, self.t, self.n, self.H, self.F
        got, ref = env_arrays(h), env_arrays(t)
        assert_exact(got, ref, REST, n, what + ": everything but the policy row vs the twin")
        for name in MAP_STATE:
            assert np.array_equal(t2n(getattr(h, name)), t2n(getattr(t, name))), f"{what}: {name}"
        row, one = got["obs"], ref["obs"]
        assert row.shape == (n, H * F + P) and one.shape == (n, F + P)
        reset = ref["reset"].astype(bool).ravel()
        fresh = self.fresh | reset
        want = stack_row(self.prev, one[:, :F], fresh, H)
        assert np.array_equal(row[:, :H * F].view(np.uint32), want.view(np.uint32)), \
            what + ": the frames vs shift / append / fill of the twin's head"
        assert np.array_equal(row[:, H * F:].view(np.uint32), one[:, F:].view(np.uint32)), what + ": the scan vs the twin's"
        assert np.abs(row[:, H * F:]).max() > 0, what + ": a scan of zeros shows nothing"
        assert np.array_equal(t2n(h.obs_history), row[:, F:H * F]), what + ": obs_history is row[:, F : H F]"
        assert (t2n(h._obs_history_fill) == 1).all(), what + ": the flags after a row"
        self.prev, self.fresh = row[:, :H * F].copy(), np.zeros(n, bool)
        tout = ref["time_out"].astype(bool).ravel()
        self.resets += reset
        self.timeouts += int((reset & tout).sum())
        self.terminations += int((reset & ~tout).sum())
        return reset

    def step(self, a, what):
        self.h.step(a.clone())
        self.t.step(a.clone())
        return self.check(what)


# ------------------------------------------- 1. the rows, on every reset route ---
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("robot,n,H", SHAPES)
def test_rows_are_the_twins_head_stacked_then_the_twins_scan_on_every_reset_route(build, robot, n, H, noise):
    p = Pair(build, robot, n, H, noise)
    h, t = p.h, p.t
    assert h.task_params.add_noise == int(noise)
    assert h.task_params.num_privileged_obs == t.task_params.num_privileged_obs
    h.sim.set_task(h.task_params)  # (the setters in another order: the pair is checked at the entry points)
    g = torch.Generator(device="cuda").manual_seed(100 * n + H)
    acts = lambda: 0.3 * torch.randn(n, h.num_actions, device="cuda", generator=g)  # noqa: E731
    p.both(lambda env: env.reset())  # reset_idx of every env (mask byte 2: levels held), then a zero-action step
    p.fresh[:] = True
    p.check("reset()")
    for it in range(3):
        assert not p.step(acts(), f"warm step {it}").any()
    for it, what in enumerate(script(n)):  # time-outs, terminations, reset_idx(env_ids) (mask byte 1)
        p.both(lambda env: intervene(env, what))
        for e in what.get("ids", []):
            p.fresh[e] = True
        reset = p.step(acts(), f"script step {it} {what}")
        for e in what.get("timeout", []) + what.get("flip", []):
            assert reset[e], f"script step {it}: env {e} resets"
    assert p.timeouts >= 2 and p.terminations >= 1 and (p.resets > 0).sum() >= 2
    # lgs_reset_all (the C entry point BaseTask.reset does not go through)
    p.both(lambda env: env.sim.reset_all(env._env_structs[env._buf_idx], env.common_step_counter))
    torch.cuda.synchronize()
    assert not t2n(h._obs_history_fill).any()
    p.fresh[:] = True
    for it in range(2):
        p.step(acts(), f"after lgs_reset_all, step {it}")


# ------------------------------------------------------ 2. the split path ---
@pytest.mark.parametrize("robot,n,H", [("go2", 3, 5), ("go2", 4, 5), ("g1", 2, 2)])
def test_split_launches_are_the_one_launch_step_bitwise(build, robot, n, H):
    """lgs_step_physics + lgs_post_physics, and physics + prepare / term_rewards / finish, from the
    same state, map state, history and flags: the fused lgs_step's buffers, rows, history and flags,
    with a time-out and a termination in the step."""
    env = build(robot, n, H)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(30 + n)
    for _ in range(3):
        env.step(0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    extra = HIST + MAP_STATE
    resets = 0
    for it, what in enumerate((dict(), dict(timeout=[0], flip=[1]), dict())):
        env._sync_stream()
        intervene(env, what)
        a = 0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        torch.cuda.synchronize()
        st, x0 = save(env), {k: getattr(env, k).clone() for k in extra}
        env.step(a.clone())
        fused, xf = env_arrays(env), {k: t2n(getattr(env, k)) for k in extra}
        resets += int(fused["reset"].sum())
        for three in (False, True):
            restore(env, st)
            for k in extra:
                getattr(env, k).copy_(x0[k])
            parts = split_step(env, a, three)
            what_ = f"{robot} x{n} step {it}: {'prepare/term_rewards/finish' if three else 'physics + post'}"
            assert_exact(parts, fused, STATE + POST, n, what_)
            for k in extra:
                assert np.array_equal(t2n(getattr(env, k)), xf[k]), f"{what_}: {k}"
    assert resets >= 2


# ------------------------------------------------------------ the C ABI -----
def test_entry_points_refuse_an_inconsistent_pair_before_any_launch(build):
    n, H = 2, 5
    env = build("go2", n, H)
    env.reset()
    env.step(torch.zeros(n, env.num_actions, device="cuda"))
    torch.cuda.synchronize()
    lib, hdl, tp = env.sim.lib, env.sim.handle, env.task_params
    E = env._env_structs[env._buf_idx]
    k = env.common_step_counter
    mask = torch.ones(n, dtype=torch.uint8, device=env.device)
    keep = ("root_states", "dof_state", "obs_buf", "_episode_length", "_d_step_counter", "actions", "obs_history",
            "_obs_history_fill", "measured_heights")
    phrase = "observation history and height observations do not combine"

    def refused(*matches):
        before = {key: t2n(getattr(env, key)) for key in keep}
        for call in (lambda: lib.lgs_step(hdl, C.byref(E), k), lambda: lib.lgs_step_deferred(hdl, C.byref(E), k),
                     lambda: lib.lgs_post_physics(hdl, C.byref(E), k),
                     lambda: lib.lgs_post_physics_finish(hdl, C.byref(E), k),
                     lambda: lib.lgs_reset_idx(hdl, C.byref(E), mask.data_ptr(), k),
                     lambda: lib.lgs_reset_all(hdl, C.byref(E), k)):
            assert call() == -1  # LGS_ERR_ARG
            text = lib.lgs_last_error().decode()
            assert all(m in text for m in matches), text
        torch.cuda.synchronize()
        for key in keep:  # nothing was launched
            np.testing.assert_array_equal(t2n(getattr(env, key)), before[key], err_msg=key)

    good = cabi.ObsHistory.from_buffer_copy(env.obs_history_params)
    bufs = env.sim._ohist_buffers
    try:
        for bad in (426, 428, 5 * 48, 48 + P, 2 * 48 + P):
            tp.num_obs = bad
            env.sim.set_task(tp)
            refused(phrase, f"num_obs is {bad}", "5 frames of the layout's head (48)", "(187) = 427")
        tp.num_obs = 427
        env.sim.set_task(tp)
        four = cabi.ObsHistory.from_buffer_copy(good)
        four.frames = 4
        env.sim.set_observation_history(four, bufs)
        refused(phrase, "num_obs is 427", "(187) = 379")
        env.sim.set_observation_history(good, bufs)
        env.sim.set_height_observations(None)  # the history alone: 427 is not 5 frames
        refused("num_obs 427 is not 5 frames of the layout's head (48)")
        env.sim.set_height_observations(env.height_obs)
        tp.num_obs = (cabi.MAX_OBS_FRAMES * cabi.MAX_OBS + cabi.MAX_SCAN_OBS) + 1  # lgs_set_task's own bound
        assert lib.lgs_set_task(hdl, C.byref(tp)) == -1 and b"exceed limits" in lib.lgs_last_error()
    finally:
        tp.num_obs = 427
        env.sim.set_task(tp)
        env.sim.set_height_observations(env.height_obs)
        env.sim.set_observation_history(good, bufs)
    prev = t2n(env.obs_buf)
    env.step(torch.zeros(n, env.num_actions, device="cuda"))  # consistent again: the step runs
    torch.cuda.synchronize()
    assert np.array_equal(t2n(env.obs_buf)[:, :4 * 48], prev[:, 48:5 * 48])
