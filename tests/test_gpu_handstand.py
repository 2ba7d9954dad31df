"""The native Go2 handstand task on the GPU (csrc/leggedsim.hip: LGS_OBS_HANDSTAND,
termination_mode 1, the PD target clamp, the unclipped torque record, eleven reward terms).

The CPU oracle does not know these terms, so the reference here is a numpy restatement of
the reference task's formulas (go2_handstand_env.py:140-383), evaluated in fp32 on the state
read between the split launches.  Floats are compared at 1e-5 (abs and rel), the tolerance the
golden-fixture tests use for kernel outputs against torch (lgs_expf tracking terms included);
flags, resets and time-outs exactly.  Sizes: 2 envs (one two-env wave whose halves take
different branches) and 37 (odd: one env per wave).  Every env of every array is compared.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from leggedsim import cabi, native  # noqa: E402
from test_gpu_parity import POST, STATE, assert_exact, env_arrays, fused_vs_oracle, make, restore, save, warm  # noqa: E402

TASK = "go2_handstand"
STEPS = 40
TILT_AT = 3
F = np.float32
TOL = dict(rtol=1e-5, atol=1e-5)


def t2n(x):
    return x.detach().cpu().numpy().copy()


def begin_step(env, a, terms=None):
    """LeggedRobot.step's preamble for a step issued through the split entry points."""
    env._sync_stream()
    env._buf_idx ^= 1
    E = env._env_structs[env._buf_idx]
    env.actions.copy_(a)
    E.actions_in = None
    E.ep_snapshot = None
    E.rew_terms = None if terms is None else terms.data_ptr()
    return E, env.common_step_counter


def end_step(env):
    i = env._buf_idx
    env._step_mirror += 1
    env.obs_buf, env.privileged_obs_buf = env._obs_bufs[i], env._priv_bufs[i]
    env.reset_buf, env.time_out_buf = env._reset_bufs[i], env._timeout_bufs[i]


def put_on_side(env, i):
    """Env i's base rolled by 90 degrees, 0.6 m up: gravity in the base frame has no z part."""
    env._sync_stream()
    s = float(np.sqrt(0.5))
    env.root_states[i, 2] = 0.6
    env.root_states[i, 3:7] = torch.tensor([s, 0.0, 0.0, s], device=env.device)
    env.root_states[i, 7:13] = 0.0
    env.sim.set_root_indexed(env.root_states, torch.tensor([i], dtype=torch.int32, device=env.device), 1)


def norm3(f):
    return np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1] + f[..., 2] * f[..., 2])


def norm2(x, y):
    return np.sqrt(x * x + y * y)


def restate_rewards(env, s):
    """check_termination and compute_reward of the reference task (go2_handstand_env.py:178-383,
    legged_robot.py:770-787) in fp32 numpy on the pre-reset state `s`."""
    cfg, T = env.cfg, env.task_params
    q, qd, cf, tau = s["q"], s["qd"], s["cf"], s["tau"]
    bl, ba, pg = s["bl"], s["ba"], s["pg"]
    feet = env.feet_indices.cpu().numpy()
    front, hind = feet[:2], feet[2:]
    term_b, pen_b = env.termination_contact_indices.cpu().numpy(), env.penalised_contact_indices.cpu().numpy()
    pose = t2n(env.pose_targets)[0]
    lim = t2n(env.dof_pos_limits)
    idx = env.dof_name_to_idx
    front_ids = [idx[f"{leg}_{p}_joint"] for leg in ("FL", "FR") for p in ("hip", "thigh", "calf")]
    hind_ids = [idx[f"{leg}_{p}_joint"] for leg in ("RL", "RR") for p in ("hip", "thigh", "calf")]

    illegal = (norm3(cf[:, term_b]) > F(1.0)).any(axis=1)
    fallen = (pg[:, 2] > F(-0.2)) & (pg[:, 2] < F(0.2))
    time_out = s["ep"].astype(F) > F(env.max_episode_length)
    reset = illegal | fallen | time_out

    lin_xy = norm2(bl[:, 0], bl[:, 1])
    err = q - pose
    sq = (err[:, front_ids] ** 2).sum(axis=1, dtype=F) + F(0.3) * (err[:, hind_ids] ** 2).sum(axis=1, dtype=F)
    gz_err = F(1.0) - np.clip(pg[:, 2], F(-1), F(1))
    h_err = np.maximum(F(cfg.rewards.base_height_target) - s["root"][:, 2], F(0))
    d_xy = s["feet_pos"][:, 0, :2] - s["feet_pos"][:, 1, :2]
    f_err = np.maximum(norm2(d_xy[:, 0], d_xy[:, 1]) - F(0.12), F(0))
    out_lim = -np.minimum(q - lim[:, 0], F(0)) + np.maximum(q - lim[:, 1], F(0))
    terms = {
        "orientation": np.exp(F(-3.0) * gz_err * gz_err),
        "base_height": np.exp(F(-8.0) * h_err * h_err),
        "front_feet_contact": (cf[:, front, 2] > F(5.0)).astype(F).mean(axis=1),
        "hind_feet_no_contact": F(1.0) - (cf[:, hind, 2] > F(5.0)).astype(F).mean(axis=1),
        "pose": np.exp(F(-4.0) * sq),
        "stability": np.exp(F(-2.0) * (lin_xy + F(0.5) * norm2(ba[:, 0], ba[:, 1]))),
        "stay_still": np.exp(-(lin_xy / F(0.05)) ** 2 - (np.abs(ba[:, 2]) / F(0.2)) ** 2),
        "lin_vel_xy": lin_xy,
        "energy": (np.abs(tau) * np.abs(qd)).sum(axis=1, dtype=F),
        "front_hip_neutral": np.exp(F(-4.0) * (q[:, [idx["FL_hip_joint"], idx["FR_hip_joint"]]] ** 2).sum(axis=1, dtype=F)),
        "front_feet_together": np.exp(F(-20.0) * f_err * f_err),
        # the base class's terms the task keeps (legged_robot.py:845-941)
        "lin_vel_z": bl[:, 2] ** 2,
        "ang_vel_xy": ba[:, 0] ** 2 + ba[:, 1] ** 2,
        "torques": (tau ** 2).sum(axis=1, dtype=F),
        "dof_vel": (qd ** 2).sum(axis=1, dtype=F),
        "action_rate": ((s["last_act"] - s["act"]) ** 2).sum(axis=1, dtype=F),
        "dof_pos_limits": out_lim.sum(axis=1, dtype=F),
        "collision": (norm3(cf[:, pen_b]) > F(0.1)).astype(F).sum(axis=1, dtype=F),
    }
    rows = np.stack([(terms[n] * F(env.reward_scales[n])).astype(F) for n in env.reward_names])
    rew = np.zeros(q.shape[0], F)
    for r in rows:
        rew = rew + r
    assert not cfg.rewards.only_positive_rewards
    rt = (reset & ~time_out).astype(F) * F(env.reward_scales["termination"])
    rew = rew + rt
    flags = dict(front=cf[:, front, 2] > F(5.0), hind=cf[:, hind, 2] > F(5.0))
    return dict(rows=rows, rew=rew, term_row=rt, reset=reset, time_out=time_out, illegal=illegal, fallen=fallen,
                flags=flags)


def restate_obs(env, s, k):
    """compute_observations of the reference task (go2_handstand_env.py:140-173) on the post-reset
    state; noise and flag flips from the step's Philox draws (lgs_uniform, noise stream)."""
    T, lib = env.task_params, native.load()
    sc = env.cfg.normalization.obs_scales
    feet = env.feet_indices.cpu().numpy()
    flags = (s["cf"][:, feet, 2] > F(5.0)).astype(F)
    obs = np.concatenate([s["ba"] * F(sc.ang_vel), s["pg"], (s["q"] - t2n(env.default_dof_pos)) * F(sc.dof_pos),
                          s["qd"] * F(sc.dof_vel), s["act"], flags], axis=1).astype(F)
    n, O = obs.shape
    assert O == 46
    flips = np.zeros((n, 4), bool)
    if T.add_noise:
        nv = np.array(list(T.noise_vec)[:O], F)
        u = np.array([[lib.lgs_uniform(T.seed, e, k, cabi.STREAM_NOISE, i) for i in range(O + 4)] for e in range(n)], F)
        obs = obs + (F(2.0) * u[:, :O] - F(1.0)) * nv
        flips = u[:, O:] < F(T.contact_flip_prob)
        obs[:, -4:] = np.logical_xor(obs[:, -4:] > F(0.5), flips).astype(F)
    clip = F(env.cfg.normalization.clip_observations)
    return np.clip(obs, -clip, clip), flips, flags


def scenario(n, add_noise, flip_prob=None, steps=STEPS):
    env = make(TASK, n, env__episode_length_s=0.4, noise__add_noise=add_noise)
    if flip_prob is not None:
        env.task_params.contact_flip_prob = flip_prob
        env.sim.set_task(env.task_params)
    assert not env._split_step and env.task_params.num_rewards == 17
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(100 + n)
    nr = len(env.reward_names)
    terms = torch.zeros(nr, n, device="cuda")
    seen = dict(contact=0, fallen_only=0, time_out=0, both_front=0, hind=0, one_of_wave=0, flips=0, reset_obs=0)
    B = env.num_bodies
    feet = env.feet_indices
    for it in range(steps):
        if it == TILT_AT:
            put_on_side(env, n - 1)
        a = 0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        E, k = begin_step(env, a, terms)
        sums0 = t2n(env._episode_sums)
        ep0 = t2n(env._episode_length)
        pre = dict(last_act=t2n(env.last_actions), last_qd=t2n(env.last_dof_vel))
        env.sim.step_physics(E, k)
        torch.cuda.synchronize()
        s = dict(pre, root=t2n(env.root_states), q=t2n(env.dof_pos), qd=t2n(env.dof_vel),
                 cf=t2n(env._contact_forces).reshape(n, B, 3), tau=t2n(env.torques), act=t2n(env.actions),
                 feet_pos=t2n(env.rigid_body_states_view[:, feet, :3]), ep=ep0 + 1)
        env.sim.post_physics_rewards(E, k)
        torch.cuda.synchronize()
        s.update(bl=t2n(env.base_lin_vel), ba=t2n(env.base_ang_vel), pg=t2n(env.projected_gravity))
        want = restate_rewards(env, s)
        what = f"x{n} step {it}"
        i = env._buf_idx
        np.testing.assert_array_equal(t2n(env._reset_bufs[i]), want["reset"], err_msg=f"{what} reset")
        np.testing.assert_array_equal(t2n(env._timeout_bufs[i]), want["time_out"], err_msg=f"{what} time_out")
        np.testing.assert_array_equal(t2n(env._episode_length), s["ep"], err_msg=f"{what} episode length")
        got_rows = t2n(terms)
        for j, name in enumerate(env.reward_names):
            np.testing.assert_allclose(got_rows[j], want["rows"][j], err_msg=f"{what} term {name}", **TOL)
        np.testing.assert_allclose(t2n(env.rew_buf), want["rew"], err_msg=f"{what} rew", **TOL)
        sums = t2n(env._episode_sums)
        np.testing.assert_allclose(sums[:nr], sums0[:nr] + want["rows"], err_msg=f"{what} episode_sums", **TOL)
        np.testing.assert_allclose(sums[nr], sums0[nr] + want["term_row"], err_msg=f"{what} termination sum", **TOL)
        assert np.isfinite(got_rows).all()
        # observations: the finish part on the post-reset state, the contact forces unchanged
        env.sim.post_physics_finish(E, k)
        end_step(env)
        torch.cuda.synchronize()
        cf1 = t2n(env._contact_forces).reshape(n, B, 3)
        np.testing.assert_array_equal(cf1, s["cf"])
        act1 = t2n(env.actions)
        assert not act1[want["reset"]].any()
        np.testing.assert_array_equal(act1[~want["reset"]], s["act"][~want["reset"]])
        s1 = dict(s, q=t2n(env.dof_pos), qd=t2n(env.dof_vel), act=act1)
        obs_w, flips, flags = restate_obs(env, s1, k)
        obs_g, priv_g = t2n(env.obs_buf), t2n(env.privileged_obs_buf)
        np.testing.assert_allclose(obs_g[:, :42], obs_w[:, :42], err_msg=f"{what} obs", **TOL)
        np.testing.assert_array_equal(obs_g[:, 42:], obs_w[:, 42:], err_msg=f"{what} contact flags")
        np.testing.assert_array_equal(priv_g, obs_g, err_msg=f"{what} priv_obs")
        if not add_noise:
            assert not flips.any()
            np.testing.assert_array_equal(obs_g[:, 42:], flags)
        seen["contact"] += int(want["illegal"].any())
        seen["fallen_only"] += int((want["fallen"] & ~want["illegal"]).any())
        seen["time_out"] += int(want["time_out"].any())
        seen["both_front"] += int(want["flags"]["front"].all(axis=1).any())
        seen["hind"] += int(want["flags"]["hind"].any())
        seen["one_of_wave"] += int(n == 2 and int(want["reset"].sum()) == 1)
        seen["flips"] += int(flips.sum())
        seen["reset_obs"] += int(want["reset"].any())
    env.close()
    return seen


@pytest.mark.parametrize("n", [2, 37])
def test_rewards_termination_and_observations_match_the_restatement(n):
    """Every reward row, rew, episode sums, reset, time_out on the pre-reset state; then obs and
    priv_obs after the finish part, with the noise draws and (at probability 0.25) the flag
    flips reproduced from the host lgs_uniform."""
    seen = scenario(n, add_noise=True, flip_prob=0.25)
    need = ["contact", "fallen_only", "time_out", "both_front", "hind", "flips", "reset_obs"] + (["one_of_wave"] if n == 2 else [])
    missing = [k for k in need if not seen[k]]
    assert not missing, f"x{n}: the run never reached {missing} (seen {seen})"


def test_observations_without_noise_are_the_thresholded_forces():
    seen = scenario(37, add_noise=False, steps=12)
    assert seen["flips"] == 0 and seen["both_front"] and seen["hind"]


@pytest.mark.parametrize("n", [2, 37])
def test_pd_target_clamp_and_unclipped_torque_record(n):
    """decimation 1: torques after the physics half are the PD law on the clamped target from
    the pre-step dof state, unclipped; the joints see the clipped torque with the record on or off."""
    # (from the reset pose: the rear thighs start 1.1 rad or more below their clamped target, so
    # the PD law asks for more than their effort limit)
    env, g = warm(TASK, n, steps=0, seed=n, control__decimation=1)
    T = env.task_params
    assert T.clamp_pd_targets == 1 and T.record_unclipped_torques == 1 and T.decimation == 1
    lo, hi = (t2n(x) for x in env._pd_target_limits())
    kp, kd, dflt = t2n(env.p_gains), t2n(env.d_gains), t2n(env.default_dof_pos)[0]
    eff = t2n(env.torque_limits)
    rear = env.rear_dof_idx.cpu().numpy()
    np.testing.assert_array_equal(np.nonzero(np.isfinite(lo))[0], np.sort(rear))
    seen = dict(active=0, inactive=0, beyond=0)
    for it in range(3):
        a = 0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        st = save(env)
        q0, qd0 = t2n(env.dof_pos), t2n(env.dof_vel)
        E, k = begin_step(env, a)
        env.sim.step_physics(E, k)
        torch.cuda.synchronize()
        raw_t = t2n(a) * F(T.action_scale) + dflt
        tgt = np.minimum(np.maximum(raw_t, lo), hi)
        want = kp * (tgt - q0) - kd * qd0
        got = t2n(env.torques)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=f"x{n} step {it}")
        seen["active"] += int((tgt[:, rear] != raw_t[:, rear]).any())
        seen["inactive"] += int((tgt[:, rear] == raw_t[:, rear]).any())
        seen["beyond"] += int((np.abs(want) > eff).any())
        assert (tgt[:, [j for j in range(12) if j not in rear]] == raw_t[:, [j for j in range(12) if j not in rear]]).all()
        on = {k_: t2n(getattr(env, k_)) for k_ in ("root_states", "dof_state", "_contact_forces", "rigid_body_states")}
        # the same step with the record off: the same motion, the clipped torques in the buffer
        T2 = cabi.TaskParams.from_buffer_copy(T)
        T2.record_unclipped_torques = 0
        restore(env, st)
        env.sim.set_task(T2)
        E, k = begin_step(env, a)
        env.sim.step_physics(E, k)
        torch.cuda.synchronize()
        for k_, v in on.items():
            np.testing.assert_array_equal(t2n(getattr(env, k_)), v, err_msg=f"{k_}: the applied torque depends on the record")
        np.testing.assert_array_equal(t2n(env.torques), np.clip(got, -eff, eff))
        assert (t2n(env.torques) != got).any() == (np.abs(want) > eff).any()
        # on with the task's own params: the run continues from the recorded step
        env.sim.set_task(T)
        restore(env, st)
        env.step(a)
    env.close()
    assert all(seen.values()), seen


def split_step(env, a, three):
    E, k = begin_step(env, a)
    env.sim.step_physics(E, k)
    if three:
        env.sim.post_physics_prepare(E, k)
        env.sim.post_physics_term_rewards(E, k)
        env.sim.post_physics_finish(E, k)
    else:
        env.sim.post_physics(E, k)
    end_step(env)
    return env_arrays(env)


@pytest.mark.parametrize("n", [2, 37])
def test_fused_step_is_the_split_steps_bitwise(n):
    """Every step of the run is compared.  The run must hold steps on which an env resets and
    steps on which an env does not; at 2 envs also a step on which no env resets at all (among
    37 envs on 0.4 s episodes some env resets on every step)."""
    env = make(TASK, n, env__episode_length_s=0.4)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    with_reset = without_reset = no_reset_at_all = 0
    for it in range(20):
        if it == TILT_AT:
            put_on_side(env, n - 1)
        a = 0.5 * torch.randn(n, env.num_actions, device="cuda", generator=g)
        st = save(env)
        env.step(a)
        fused = env_arrays(env)
        for three in (False, True):
            restore(env, st)
            parts = split_step(env, a, three)
            assert_exact(parts, fused, STATE + POST, n,
                         f"x{n} step {it}: {'prepare/term_rewards/finish' if three else 'physics + post'}")
        r = fused["reset"].astype(bool)
        with_reset += int(r.any())
        without_reset += int((~r).any())
        no_reset_at_all += int(not r.any())
    env.close()
    assert with_reset and without_reset, (with_reset, without_reset)
    assert n != 2 or no_reset_at_all


@pytest.mark.parametrize("n", [2, 37])
def test_go2_with_the_new_switches_off_is_still_the_oracle_bitwise(n):
    """The appended task fields shifted nothing: the walking task, whose params have every new
    switch off, is the CPU oracle's step bit for bit."""
    env, g = warm("go2", n, steps=8, seed=n)
    T = env.task_params
    assert (T.clamp_pd_targets, T.record_unclipped_torques, T.termination_mode, T.num_front_feet) == (0, 0, 0, 0)
    assert T.obs_layout == cabi.OBS_QUADRUPED
    fused_vs_oracle(env, g, 8, f"go2 x{n}, handstand switches off")
    env.close()


# ------------------------------------------------------------------ PPO at 46 inputs --
def test_fused_update_at_46_inputs_matches_fp32_autograd():
    """test_fused_step_matches_fp32_autograd_update at the handstand's observation width: 46
    pads to 48 columns in the first layer (rollout forward and first-layer dW)."""
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCritic
    from test_gpu_fused_ppo import _fill_storage
    torch.manual_seed(0)
    N, T, O, A = 256, 8, 46, 12
    ac32 = ActorCritic(O, O, A, [512, 256, 128], [512, 256, 128], mixed_precision=False).cuda()
    acbf = copy.deepcopy(ac32)
    acbf.mixed_precision = True
    kw = dict(num_learning_epochs=1, num_mini_batches=2, learning_rate=1e-3, schedule="fixed", device="cuda")
    ref = PPO(ac32, fused_loss=False, **kw)
    ref.use_graph = False
    fus = PPO(acbf, **kw)
    for alg in (ref, fus):
        alg.init_storage(N, T, [O], [None], [A])
    assert fus._fused is not None and ref._fused is None
    assert fus._fused.k0p[0] == 48
    data = _fill_storage(ref, T, N, O, A, seed=1)
    for k, v in data.items():
        getattr(fus.storage, k).copy_(v)
    fus.storage.step = T
    p0 = [p.detach().clone() for p in ref.actor_critic.parameters()]
    torch.manual_seed(7)
    l_ref = ref.update()
    torch.manual_seed(7)
    l_fus = fus.update()
    np.testing.assert_allclose(l_fus, l_ref, rtol=2e-2, atol=2e-3)
    lr = 1e-3
    for a, b, c in zip(ref.actor_critic.parameters(), fus.actor_critic.parameters(), p0):
        da, db = (a.detach() - c), (b.detach() - c)
        assert da.abs().max() > 0
        bad = ((da - db).abs() > 0.2 * lr).float().mean().item()
        assert bad < 0.02, bad
        assert (da - db).abs().max() <= 4 * 3 * lr


@pytest.mark.parametrize("M,rows", [(256, True), (37, False)])
def test_fused_mlp_forward_at_46_inputs_is_bitwise_the_per_layer_gemms(M, rows):
    """test_fused_mlp_forward_is_bitwise_the_per_layer_gemms at O = 46; also the converted input
    rows themselves: 46 bf16 values, then zero padding up to 48 columns."""
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCritic, mfma_mlp
    torch.manual_seed(0)
    N, T, O, A = 64, 8, 46, 12
    alg = PPO(ActorCritic(O, O, A, [512, 256, 128], [512, 256, 128]).cuda(), num_learning_epochs=1,
              num_mini_batches=1, device="cuda")
    alg.init_storage(N, T, [O], [None], [A])
    f = alg._fused
    assert f.fused_fwd and f.wf is not None and f.k0p[0] == 48
    f.ensure_weights()
    g = torch.Generator(device="cuda").manual_seed(M)
    x = 2.0 * torch.randn(T * N, O, device="cuda", generator=g)
    idx = torch.randperm(T * N, device="cuda", generator=g)[:M] if rows else None
    # the per-layer GEMM's fp32 operand needs a row stride that is a multiple of 4: it reads the
    # same rows from a copy with 48 columns (the fused forward reads the 46-wide rows themselves)
    x48 = torch.zeros(T * N, 48, device="cuda")
    x48[:, :O] = x
    outs = {}
    for fused in ("frag", True, False):
        y = [[torch.full((M, lin.out_features), float("nan"), dtype=torch.bfloat16, device="cuda") for lin in ls[:-1]]
             for ls in f.lins]
        out = [torch.full((M, ls[-1].out_features), float("nan"), device="cuda") for ls in f.lins]
        xa = torch.full((M, f.k0p[0]), float("nan"), dtype=torch.bfloat16, device="cuda")
        if fused:
            mfma_mlp.mlp_forward([dict(x=x, kx=O, rows=idx, xa=xa if i == 0 else None, K0=f.k0p[i], W=f.wb[i],
                                       Wf=f.wf[i] if fused == "frag" else None,
                                       b=[lin.bias.detach() for lin in f.lins[i]],
                                       N=[lin.out_features for lin in f.lins[i]], y=y[i], out=out[i])
                                  for i in range(2)], M)
        else:
            for l in range(4):
                last = l == 3
                gj = []
                for i in range(2):
                    lin = f.lins[i][l]
                    a = dict(af=x48, rows=idx, xa=xa if i == 0 else None) if l == 0 else dict(A=y[i][l - 1])
                    o = dict(cf=out[i]) if last else dict(cb=y[i][l])
                    gj.append(dict(B=f.wb[i][l], M=M, N=lin.out_features, K=f.k0p[i] if l == 0 else lin.in_features,
                                   bias=lin.bias.detach(), **a, **o))
                mfma_mlp._gemm(mfma_mlp.EPI_FWD_OUT if last else mfma_mlp.EPI_FWD_HIDDEN, gj)
        torch.cuda.synchronize()
        outs[fused] = (xa, y, out)
    src = x if idx is None else x[idx]
    for form in ("frag", True):
        (xa1, y1, o1), (xa0, y0, o0) = outs[form], outs[False]
        assert torch.equal(xa1, xa0)
        assert torch.equal(xa1[:, :O], src[:M].to(torch.bfloat16)) and not xa1[:, O:].float().abs().any()
        for i in range(2):
            for a, b in zip(y1[i], y0[i]):
                assert torch.equal(a, b)
            assert torch.equal(o1[i], o0[i])
    # against fp32 torch on the same rows: the padded columns add nothing (bf16 GEMM rounding)
    with torch.no_grad():
        mu = alg.actor_critic.actor(src[:M])
    torch.testing.assert_close(outs["frag"][2][0][:, :A], mu, rtol=0.05, atol=0.05)


# ------------------------------------------------------------------------- runner --
def test_runner_trains_the_task_on_the_captured_path():
    """OnPolicyRunner.learn(2) on 64 envs: the native rollout and update, both captured; finite
    losses; the parameters bitwise those of the same run with graph capture disabled."""
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    params = {}
    for graph in (True, False):
        env = make(TASK, 64)
        _, train_cfg = task_registry.get_cfgs(TASK)
        cfg = class_to_dict(train_cfg)
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        alg = runner.alg
        if not graph:
            alg.use_graph = False
        assert alg._fused is not None and alg._rollout is not None, "native PPO path not active"
        assert not env._split_step
        losses = []
        upd = alg.update
        alg.update = lambda *a, **kw: losses.append(upd(*a, **kw)) or losses[-1]
        runner.learn(2)
        torch.cuda.synchronize()
        # (without a log dir the runner takes the two mean losses as a device tensor)
        losses = [x.tolist() if torch.is_tensor(x) else list(x) for x in losses]
        assert len(losses) == 2 and np.isfinite(np.array(losses, dtype=np.float64)).all(), losses
        if graph:
            assert runner._rollout_graph is not None and not getattr(runner, "_rollout_graph_failed", False)
            assert alg.use_graph and alg._fgraph is not None
        else:
            assert runner._rollout_graph is None and alg._fgraph is None
        assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.rew_buf).all()
        params[graph] = [p.detach().clone() for p in alg.actor_critic.parameters()]
        env.close()
    for a, b in zip(params[True], params[False]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
