"""The rough-terrain path of the fused step on the GPU (csrc/leggedsim.hip): the
level curriculum in the reset stage, extras["episode"]["terrain_level"] from both extras
producers, the height scan, the ground-relative base_height / feet_swing_height terms.

The CPU oracle cannot follow the new switches, so the references are numpy fp32 restatements
of the operation order documented in include/leggedsim.h (lgs_task_params: terrain_curriculum,
measure_heights, ground_relative_heights).  The build has FP contraction off, so the same
operations in the same order give the same bits: levels, origins, the placed roots and the scan
are compared exactly; the two reward terms at 1e-5 (abs and rel: the 187-term mean's order is
the kernel's own, the tolerance the golden tests use for such sums).  With the switches off the
step is compared bit for bit with the oracle.

Maps: 3 rows x 2 cols of 8 m tiles, 5 m border (340 x 260 samples at 0.1 m).  Env counts: Go2
5 (odd: one env per wave) and 8 (two envs per wave), G1 3 and 8 (one env per wave).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bridge  # noqa: E402
from leggedsim import cabi  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from test_gpu_parity import fused_vs_oracle, make, restore, save  # noqa: E402

F = np.float32
MAP = dict(terrain__mesh_type="heightfield", terrain__num_rows=3, terrain__num_cols=2, terrain__border_size=5)
# max_episode_length = 150 control steps; commands resample every 500: a forced time-out (episode
# length 151) never coincides with a command resample
SHORT = dict(env__episode_length_s=3.0)
ROBOTS = [("go2", 5), ("go2", 8), ("g1", 3), ("g1", 8)]


def t2n(x):
    return x.detach().cpu().numpy().copy()


def build(robot, n, **edits):
    if robot == "go2":  # the quadruped on the map with the curriculum and the scan on
        kw = dict(MAP, terrain__level_curriculum=True, terrain__scan_heights=True)
        kw.update(edits)
        env = make("go2", n, **kw)
    else:
        env = make("g1_terrain", n, **dict(MAP, **edits))
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(3):
        env.step(0.3 * torch.randn(env.num_envs, env.num_actions, device="cuda", generator=g))
    return env, g


def begin_step(env, a, terms=None):
    """LeggedRobot.step's preamble for a step issued through the split entry points."""
    env._sync_stream()
    env.flush_extras()
    env._buf_idx ^= 1
    E = env._env_structs[env._buf_idx]
    env.actions.copy_(a)
    E.actions_in = None
    E.ep_snapshot = None
    E.rew_terms = None if terms is None else terms.data_ptr()
    return E, env.common_step_counter


def end_step(env):
    i = env._buf_idx
    env._env_structs[i].rew_terms = None
    env._step_mirror += 1
    env.obs_buf, env.privileged_obs_buf = env._obs_bufs[i], env._priv_bufs[i]
    env.reset_buf, env.time_out_buf = env._reset_bufs[i], env._timeout_bufs[i]


def uniform(env, e, step, stream, index):
    return F(env.sim.lib.lgs_uniform(int(env.task_params.seed), int(e), int(step) & 0xFFFFFFFF, stream, index))


# ------------------------------------------------------------ restatements --
def restate_levels(env, reset, root_xy, cmd, levels, origins, step):
    """The level rule of include/leggedsim.h (terrain_curriculum) in fp32 numpy for the envs of
    `reset`; asserts first that no case lies within 1e-4 relative of either threshold."""
    T = env.task_params
    rows = int(T.terrain_rows)
    dx, dy = root_xy[:, 0] - origins[:, 0], root_xy[:, 1] - origins[:, 1]
    d2 = dx * dx + dy * dy
    half = F(0.5) * F(T.max_episode_length_s)
    up_thr = np.full_like(d2, F(T.terrain_half_length_sq))
    dn_thr = (cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) * (half * half)
    assert d2.dtype == F and dn_thr.dtype == F
    for thr in (up_thr, dn_thr):
        assert (np.abs(d2 - thr)[reset] > F(1e-4) * thr[reset]).all(), "a case sits on a threshold"
    up = d2 > up_thr
    down = ~up & (d2 < dn_thr)
    out = levels.copy()
    for e in np.nonzero(reset)[0]:
        lv = int(levels[e]) + int(up[e]) - int(down[e])
        if lv >= rows:
            lv = min(int(uniform(env, e, step, cabi.STREAM_TERRAIN, 0) * F(rows)), rows - 1)
        else:
            lv = max(lv, 0)
        out[e] = lv
    return out, up, down


def restate_placement(env, e, origin, step):
    """Root xy of a reset env: (base_init + origin) + the U[-1, 1] draw (LGS_STREAM_RESET_ROOT 6, 7)."""
    base = t2n(env.base_init_state).astype(F)
    xy = []
    for k in range(2):
        u = uniform(env, e, step, cabi.STREAM_RESET_ROOT, 6 + k)
        xy.append((base[k] + origin[k]) + ((F(1.0) - F(-1.0)) * u + F(-1.0)))
    return np.array(xy, F)


def restate_scan(env, root):
    """legged_gym's _get_heights in the order of include/leggedsim.h (measure_heights)."""
    tc, H = env.cfg.terrain, env.terrain.heightsamples
    px = np.array(tc.measured_points_x, F)
    py = np.array(tc.measured_points_y, F)
    PX, PY = [a.reshape(1, -1) for a in np.meshgrid(px, py, indexing="ij")]  # point k = ix * ny + iy
    qz, qw = root[:, 5:6], root[:, 6:7]
    nq = np.sqrt(qz * qz + qw * qw)
    z, w = qz / nq, qw / nq
    c, s = w * w - z * z, F(2.0) * w * z
    border, hs = F(tc.border_size), F(tc.horizontal_scale)
    X = ((c * PX - s * PY) + root[:, 0:1]) + border
    Y = ((s * PX + c * PY) + root[:, 1:2]) + border
    assert X.dtype == F and (X / hs).dtype == F
    i = np.clip((X / hs).astype(np.int32), 0, H.shape[0] - 2)
    j = np.clip((Y / hs).astype(np.int32), 0, H.shape[1] - 2)
    hm = np.minimum(np.minimum(H[i, j], H[i + 1, j]), H[i, j + 1])
    return hm.astype(F) * F(tc.vertical_scale), (X / hs, Y / hs)


def restate_ground(env, x, y):
    """The triangle interpolation documented at lgs_set_heightfield: sample (i, j) at
    (i * hs - border, j * hs - border), cell split along its (i, j)-(i+1, j+1) diagonal."""
    tc, H = env.cfg.terrain, env.terrain.heightsamples
    inv, vs, border = F(1.0) / F(tc.horizontal_scale), F(tc.vertical_scale), F(tc.border_size)
    u = np.clip((x + border) * inv, F(0), F(H.shape[0] - 1))
    v = np.clip((y + border) * inv, F(0), F(H.shape[1] - 1))
    i = np.minimum(u.astype(np.int32), H.shape[0] - 2)
    j = np.minimum(v.astype(np.int32), H.shape[1] - 2)
    fu, fv = u - i.astype(F), v - j.astype(F)
    h00, h01 = H[i, j].astype(F) * vs, H[i, j + 1].astype(F) * vs
    h10, h11 = H[i + 1, j].astype(F) * vs, H[i + 1, j + 1].astype(F) * vs
    lower = fu >= fv
    du = np.where(lower, h10 - h00, h11 - h01)
    dv = np.where(lower, h11 - h10, h01 - h00)
    return h00 + fu * du + fv * dv


# ------------------------------------------------------- curriculum cases --
# name, level before, root offset from the tile origin (m), commands xy, expected level change
# (None: graduation past the top row, a random level).  Thresholds at episode_length_s = 3:
# up above 4 m; down below |cmd| * 1.5 m.
CASES = [("up", 0, (5.0, 0.5), (0.5, 0.0), 1),
         ("down", 1, (0.5, -0.25), (1.0, 0.5), -1),
         ("stay", 1, (2.0, 1.0), (0.1, 0.1), 0),
         ("floor", 0, (0.3, 0.2), (1.0, 0.0), 0),
         ("graduate", 2, (-4.5, 2.0), (0.5, 0.5), None)]


def rounds(n):
    """The cases dealt over envs 0 .. n-2, as many rounds as that takes; env n-1 never resets."""
    per = n - 1
    return [{e: CASES[k + e] for e in range(per) if k + e < len(CASES)} for k in range(0, len(CASES), per)]


def place(env, assign):
    levels = t2n(env.terrain_levels)
    for e, c in assign.items():
        levels[e] = c[1]
    env.set_terrain_levels(torch.as_tensor(levels))
    for e, c in assign.items():
        env.root_states[e, 0] = env.env_origins[e, 0] + c[2][0]
        env.root_states[e, 1] = env.env_origins[e, 1] + c[2][1]
        env.root_states[e, 2] += 0.5  # (clear of the slope the new spot may be on)
        env.commands[e, 0], env.commands[e, 1] = c[3]
    torch.cuda.synchronize()


def check_reset(env, assign, reset, pre, step):
    """Levels, origins and placed roots of the envs of `reset` against the restatement (exact);
    the other envs' levels and origins unchanged; the designed cases took their branch."""
    rows = int(env.task_params.terrain_rows)
    want, up, down = restate_levels(env, reset, pre["root"][:, :2], pre["cmd"], pre["levels"], pre["org"], step)
    levels, org = t2n(env.terrain_levels), t2n(env.env_origins)
    table, types = t2n(env.terrain_origins), t2n(env.terrain_types)
    np.testing.assert_array_equal(levels, want)
    np.testing.assert_array_equal(org, table[want, types])
    np.testing.assert_array_equal(org[~reset], pre["org"][~reset])
    root = t2n(env.root_states)
    for e in np.nonzero(reset)[0]:
        np.testing.assert_array_equal(root[e, :2], restate_placement(env, e, org[e], step), err_msg=f"env {e}")
    for e, (name, lv, _, _, delta) in assign.items():
        assert reset[e], f"{name}: env {e} did not reset"
        if delta is None:
            assert up[e] and lv + 1 >= rows and 0 <= levels[e] < rows, name
        else:
            assert levels[e] == lv + delta and (up[e], down[e]) == (name == "up", name in ("down", "floor")), name
    assert int(env._terrain_level_sum) == int(levels.sum())
    assert float(env._ep_means[-1]) == float(env.terrain_levels.float().mean())


def pre_state(env, root=None):
    return dict(root=t2n(env.root_states) if root is None else root, cmd=t2n(env.commands),
                levels=t2n(env.terrain_levels), org=t2n(env.env_origins))


# -------------------------------------------------------------------- tests --
@pytest.mark.parametrize("robot,n", ROBOTS)
def test_reset_idx_moves_the_levels_by_the_rule(robot, n):
    """1. reset_idx(env_ids): up, down, stay, the floor at row 0 and graduation past the top row."""
    env, _ = build(robot, n, **SHORT)
    keep = ("root_states", "dof_state", "commands", "_episode_length", "terrain_levels", "env_origins")
    for assign in rounds(n):
        place(env, assign)
        pre = pre_state(env)
        before = {k: t2n(getattr(env, k)) for k in keep}
        step = env.common_step_counter
        reset = np.zeros(n, bool)
        reset[list(assign)] = True
        env.reset_idx(torch.tensor(sorted(assign), device=env.device))
        torch.cuda.synchronize()
        check_reset(env, assign, reset, pre, step)
        for k in keep:  # the other envs are untouched
            a, b = t2n(getattr(env, k)).reshape(n, -1), before[k].reshape(n, -1)
            np.testing.assert_array_equal(a[~reset], b[~reset], err_msg=k)
        # 3. extras["episode"]["terrain_level"] after reset_idx
        assert float(env.extras["episode"]["terrain_level"]) == float(env.terrain_levels.float().mean())


@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("robot,n", ROBOTS)
def test_control_step_moves_the_levels_by_the_rule(robot, n, path):
    """2. The same cases through a control step (forced time-outs), on the post-physics,
    pre-reset root and the commands after the native callback: the one-launch step (its
    pre-reset root taken from a physics-only run of the same state), and the split launches
    prepare / term_rewards / finish (the reset stage reads back what the first parts left)."""
    env, g = build(robot, n, **SHORT)
    T = env.task_params
    assert int(T.max_episode_length) % T.resample_interval != 0
    for assign in rounds(n):
        place(env, assign)
        env.episode_length_buf[list(assign)] = int(env.max_episode_length)
        assert (int(env.max_episode_length) + 1) % T.resample_interval != 0  # no resample with the time-out
        a = 0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        if path == "fused":
            st = save(env)
            E, k = begin_step(env, a)
            env.sim.step_physics(E, k)
            torch.cuda.synchronize()
            pre = pre_state(env)  # (a time-out env's commands xy: no resample, the heading moves only [2])
            restore(env, st)
            env.step(a)
            torch.cuda.synchronize()
            # 3. extras["episode"]["terrain_level"] after lgs_step
            assert float(env.extras["episode"]["terrain_level"]) == float(env.terrain_levels.float().mean())
        else:
            E, k = begin_step(env, a)
            env.sim.step_physics(E, k)
            env.sim.post_physics_prepare(E, k)
            torch.cuda.synchronize()
            pre = pre_state(env)
            env.sim.post_physics_term_rewards(E, k)
            env.sim.post_physics_finish(E, k)
            end_step(env)
            torch.cuda.synchronize()
        reset = t2n(env.reset_buf).astype(bool)
        assert not reset[n - 1] or n - 1 not in assign
        check_reset(env, assign, reset, pre, k)


@pytest.mark.parametrize("robot,n", [("go2", 8), ("g1", 3)])
def test_terrain_level_extras_from_the_rollout_consumer(robot, n):
    """3. lgs_step_deferred followed by the rollout's consumer (pmlp_store_step_env with the
    step's pmlp_env_extras): the terrain_level slot is the mean of terrain_levels, and until the
    consumer has run it is still the previous step's."""
    env, g = build(robot, n, **SHORT)
    assign = {0: CASES[0], 1: CASES[3]}  # up and floor: the mean level rises by 1 / n
    place(env, assign)
    env.episode_length_buf[list(assign)] = int(env.max_episode_length)
    before, sum_before = float(env.terrain_levels.float().mean()), int(env.terrain_levels.sum())
    assert float(env._ep_means[-1]) == before
    env.defer_extras = True
    _, _, rew, dones, infos = env.step(0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    env.defer_extras = False
    torch.cuda.synchronize()
    after = float(env.terrain_levels.float().mean())
    assert int(env.terrain_levels.sum()) == sum_before + 1 and after != before  # (the `up` case moved)
    assert float(env._ep_means[-1]) == before  # the consumer has not run yet
    job = infos["_deferred_extras"]
    assert job.fields["level_sum"] == env._terrain_level_sum.data_ptr() and job.fields["num_envs"] == n
    ex = mm.EnvExtras(**job.fields)
    job.consumed = True
    value = torch.zeros(n, device="cuda")
    st_rew, st_done = torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    P = mm._p
    mm._ok(mm.load().pmlp_store_step_env(P(rew), P(dones), P(env._time_outs), P(value), P(st_rew), P(st_done), n,
                                         0.99, None, 0, None, 0, C.byref(ex), mm._stream()), "pmlp_store_step_env")
    torch.cuda.synchronize()
    assert float(infos["episode"]["terrain_level"]) == after
    assert float(env._ep_means[-1]) == after
    assert int(env._terrain_level_sum) == int(env.terrain_levels.sum())


def test_captured_runner_on_g1_terrain_moves_levels_across_replays():
    """4. OnPolicyRunner on g1_terrain, small: eager, captured and replayed iterations.  Every env
    starts each iteration on the top row, two steps short of its time-out, so every iteration resets
    envs; levels move inside the captured graph's replays, env_origins follow them, and the logged
    value is the levels' mean."""
    from legged_gym.utils import get_args
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    n = 8
    env = make("g1_terrain", n, **MAP)
    _, train_cfg = task_registry.get_cfgs("g1_terrain")
    runner = OnPolicyRunner(env, class_to_dict(train_cfg), log_dir=None, device="cuda:0")
    top = int(env.task_params.terrain_rows) - 1
    moved = []
    for it in range(3):
        env.set_terrain_levels(torch.full((n,), top))
        env.episode_length_buf = torch.full_like(env.episode_length_buf, int(env.max_episode_length) - 2)
        runner.learn(1)
        env.flush_extras()
        torch.cuda.synchronize()
        levels = env.terrain_levels
        assert ((levels >= 0) & (levels <= top)).all()
        assert torch.equal(env.env_origins, env.terrain_origins[levels, env.terrain_types])
        assert int(env._terrain_level_sum) == int(levels.sum())
        logged = env.extras["episode"]["terrain_level"]
        assert torch.isfinite(logged) and float(logged) == float(levels.float().mean())
        moved.append(bool((levels != top).any()))
    assert runner._rollout_graph is not None
    assert all(moved), moved  # eager, captured, replayed


def odd_poses(env, n):
    """Nonzero yaw, roll and pitch for every env; env 0 and env n-1 near two map edges so that
    both index clips of the scan engage; the others on the hardest row, 2.5 m from the tile
    centre (past the 3 m platform: on the slope or the stairs)."""
    tc = env.cfg.terrain
    far = tc.num_rows * tc.terrain_length + tc.border_size - 0.3
    env.set_terrain_levels(torch.full((n,), tc.num_rows - 1))
    for e in range(1, n - 1):
        env.root_states[e, 0] = env.env_origins[e, 0] + 2.5
        env.root_states[e, 1] = env.env_origins[e, 1] + 1.0
        env.root_states[e, 2] = env.env_origins[e, 2] + env.base_init_state[2] + 0.3
    for e in range(n):
        r, p, y = 0.15 + 0.05 * e, -0.1 - 0.03 * e, 0.7 * (e + 1) * (-1) ** e
        cr, sr, cp, sp, cy, sy = (np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2),
                                  np.sin(y / 2))
        q = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
             cr * cp * cy + sr * sp * sy]
        env.root_states[e, 3:7] = torch.tensor(q, dtype=torch.float, device=env.device)
    env.root_states[0, 0:2] = torch.tensor([-tc.border_size + 0.3, -tc.border_size + 0.2], device=env.device)
    env.root_states[n - 1, 0:2] = torch.tensor([far, tc.num_cols * tc.terrain_width + tc.border_size - 0.2],
                                               device=env.device)
    env.root_states[[0, n - 1], 2] += 0.5
    torch.cuda.synchronize()


@pytest.mark.parametrize("robot,n", ROBOTS)
def test_height_scan_matches_the_restatement_exactly(robot, n):
    """5. measured_heights after a step == legged_gym's _get_heights restated on the post-physics,
    pre-reset root: yawed, rolled and pitched robots, two of them at map edges (index clips)."""
    env, g = build(robot, n)
    odd_poses(env, n)
    a = 0.3 * torch.randn(n, env.num_actions, device="cuda", generator=g)
    E, k = begin_step(env, a)
    env.sim.step_physics(E, k)
    torch.cuda.synchronize()
    root = t2n(env.root_states)
    env.sim.post_physics(E, k)
    end_step(env)
    torch.cuda.synchronize()
    want, (gx, gy) = restate_scan(env, root)
    H = env.terrain.heightsamples
    assert env.measured_heights.shape == want.shape == (n, 187)
    assert (gx < 0).any() and (gx > H.shape[0] - 2).any() and (gy < 0).any() and (gy > H.shape[1] - 2).any()
    assert np.abs(root[:, 3:5]).min() > 1e-3 and np.abs(root[:, 5]).min() > 0.1  # roll / pitch / yaw
    assert len(np.unique(want[1:n - 1])) > 4  # (the envs between the two at the edges: not a flat patch)
    np.testing.assert_array_equal(t2n(env.measured_heights), want)


def _term_rows(env, a):
    """One step up to the reward terms through the split launches; the state the terms read."""
    nr = len(env._native_reward_names)
    terms = torch.zeros(nr, env.num_envs, device="cuda")
    E, k = begin_step(env, a, terms)
    env.sim.step_physics(E, k)
    env.sim.post_physics_prepare(E, k)
    env.sim.post_physics_term_rewards(E, k)
    torch.cuda.synchronize()
    E.rew_terms = None
    feet = t2n(env.feet_indices)
    s = dict(root=t2n(env.root_states), heights=t2n(env.measured_heights),
             feet=t2n(env.rigid_body_states).reshape(env.num_envs, -1, 13)[:, feet, :3],
             cf=t2n(env.contact_forces)[:, feet])
    return t2n(terms), s


@pytest.mark.parametrize("n", [3, 8])
def test_ground_relative_height_terms(n):
    """6. base_height and feet_swing_height through rew_terms on G1: relative to the scanned /
    interpolated ground with the switch on (1e-5), the world-z formulas bit for bit with it off,
    on the same state."""
    env, g = build("g1", n)
    for _ in range(6):  # (feet leave the ground)
        env.step(0.6 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    a = 0.6 * torch.randn(n, env.num_actions, device="cuda", generator=g)
    env.root_states[0, 2] += 0.5  # env 0 in the air: both feet swing
    names = env._native_reward_names
    kb, ks = names.index("base_height"), names.index("feet_swing_height")
    sb, ss = F(env.reward_scales["base_height"]), F(env.reward_scales["feet_swing_height"])
    target, swing = F(env.cfg.rewards.base_height_target), F(env.task_params.swing_height_target)
    st = save(env)
    on, s = _term_rows(env, a)
    restore(env, st)
    tp = env.task_params
    tp.ground_relative_heights = 0
    env.sim.set_task(tp)
    try:
        off, s2 = _term_rows(env, a)
    finally:
        tp.ground_relative_heights = 1
        env.sim.set_task(tp)
        restore(env, st)
    for key in s:
        np.testing.assert_array_equal(s[key], s2[key], err_msg=key)  # the same state
    rz, fz = s["root"][:, 2], s["feet"][:, :, 2]
    free = np.where(np.sqrt((s["cf"] * s["cf"]).sum(axis=2, dtype=F)) > F(1.0), F(0), F(1))
    ground = restate_ground(env, s["feet"][:, :, 0], s["feet"][:, :, 1])
    assert np.abs(ground).max() > 0.01 and np.abs(s["heights"]).max() > 0.01 and free.any()  # (not on z = 0)
    # switch on
    d = (rz[:, None] - s["heights"]).mean(axis=1, dtype=F) - target
    np.testing.assert_allclose(on[kb], d * d * sb, rtol=1e-5, atol=1e-5)
    d = (fz - ground) - swing
    np.testing.assert_allclose(on[ks], (d * d * free).sum(axis=1, dtype=F) * ss, rtol=1e-5, atol=1e-5)
    # switch off: the world-z arithmetic, bit for bit (two feet: one addition, in foot order)
    d = rz - target
    np.testing.assert_array_equal(off[kb], d * d * sb)
    d = fz - swing
    el = d * d * free
    np.testing.assert_array_equal(off[ks], (el[:, 0] + el[:, 1]) * ss)
    others = [k for k in range(len(names)) if k not in (kb, ks)]
    np.testing.assert_array_equal(on[others], off[others])  # no other term reads the switch


@pytest.mark.parametrize("task,n,edits", [("go2", 8, {}), ("go2", 5, {}), ("g1_rough", 8, {}), ("g1_rough", 3, {}),
                                          ("go2", 8, dict(terrain__scan_heights=True))])
def test_switches_off_step_is_the_oracle_bitwise(task, n, edits):
    """7. Heightfield Go2 and G1 with the new switches off: every buffer of the step equals the
    CPU oracle's (which has no such fields) bit for bit.  The scan alone (last case) writes only
    its own buffer, so that env is bitwise the oracle too."""
    env = make(task, n, **dict(MAP, **edits))
    assert env.task_params.terrain_curriculum == 0 and env.task_params.ground_relative_heights == 0
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(5):
        env.step(0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g))
    levels, origins = env.terrain_levels.clone(), env.env_origins.clone()
    try:
        fused_vs_oracle(env, g, 3, f"{task} x{n} switches off")
    finally:
        bridge.set_ground(bridge.ensure_built())
    assert torch.equal(env.terrain_levels, levels) and torch.equal(env.env_origins, origins)
    assert "terrain_level" not in env.extras["episode"]
    assert hasattr(env, "measured_heights") == bool(edits)
