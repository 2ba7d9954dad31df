"""Random network distillation on the GPU: the two kernels of csrc/rnd.hip against
tests/rnd_ref.py, pmlp_rnd_loss_step against pmlp_distill_loss_step bit for bit, the fused
predictor step against the plain fp32 path, PPO end to end on the fake env (the reward pass, the
captured update against the eager one, the weight-zero invariance, a load) and the scripts."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rnd_ref as rr  # noqa: E402
from act_ref import check_equal  # noqa: E402
from fake_env import FakeEnv  # noqa: E402
from rsl_rl.algorithms import rnd_step  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from rsl_rl.modules.rnd import RandomNetworkDistillation, parse_cfg  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402

DEV = "cuda"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------------- pmlp_rnd_reward --
def _reward_launch(pred, tgt, w, rew0, T, N, intrinsic):
    M = T * N
    d = dict(pred=_dev(pred), tgt=_dev(tgt), w=_dev(w), rew=_dev(rew0),
             intr=torch.full((M,), 7.0, device=DEV) if intrinsic else None,
             partial=torch.full((2 * rr.num_partials(M),), 7.0, device=DEV), stats=torch.full((2,), 7.0, device=DEV))
    mm.rnd_reward(d["pred"], d["tgt"], d["w"], T, N, d["rew"], d["intr"], d["partial"], d["stats"])
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


@pytest.mark.parametrize("E", rr.WIDTHS)
@pytest.mark.parametrize("T,N", rr.SHAPES)
def test_reward_against_the_reference(T, N, E):
    pred, tgt, w, rew0 = rr.reward_case(T, N, E)
    assert mm.load().pmlp_rnd_parts(T * N) == rr.num_partials(T * N)
    out = _reward_launch(pred, tgt, w, rew0, T, N, True)
    fr = rr.check_reward(out["rew"], out["intr"], out["partial"], out["stats"], pred, tgt, w, rew0, N)
    print(f"[rnd] reward T={T} N={N} E={E}: worst fractions of the bounds {fr}")
    # the in-place add: the zero-weight step's rows are untouched, every other row moved
    assert np.array_equal(out["rew"][N:2 * N], rew0[N:2 * N])
    moved = out["rew"] != rew0
    assert moved[:N].all() and moved[2 * N:].all()
    # no intrinsic output: the same bits everywhere else; a second launch: the same bits
    for intrinsic in (False, True):
        again = _reward_launch(pred, tgt, w, rew0, T, N, intrinsic)
        for k in ("rew", "partial", "stats") + (("intr",) if intrinsic else ()):
            check_equal(again[k], out[k], f"{k} (intrinsic={intrinsic})")
    # the by-element path gives the 16-byte path's bits: the same rows at a misaligned base
    if E % 4 == 0:
        M = T * N
        pad = torch.zeros(M * E + 1, device=DEV)
        pad[1:] = _dev(pred).reshape(-1)
        rew = _dev(rew0)
        partial, stats = torch.empty(2 * rr.num_partials(M), device=DEV), torch.empty(2, device=DEV)
        mm.rnd_reward(pad[1:].view(M, E), _dev(tgt), _dev(w), T, N, rew, None, partial, stats)
        check_equal(rew.cpu().numpy(), out["rew"], "rewards (misaligned pred)")
        check_equal(stats.cpu().numpy(), out["stats"], "stats (misaligned pred)")


def test_reward_refusals():
    lib, P = mm.load(), mm._p
    t = torch.zeros(64 * 40, device=DEV)
    ok = (P(t), P(t), P(t), 2, 8, 8, P(t), None, P(t), P(t), mm._stream())

    def call(**kw):
        names = ("pred", "tgt", "w", "T", "N", "E", "rewards", "intrinsic", "partial", "stats", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.pmlp_rnd_reward(*[a[n] for n in names])
    assert call() == 0
    for k in ("pred", "tgt", "w", "rewards", "partial", "stats"):
        assert call(**{k: None}) == -1, k
    assert call(T=0) == -1 and call(N=0) == -1 and call(E=0) == -1
    assert call(E=33) == -3 and b"E above 32" in lib.pmlp_last_error()
    assert call(T=1 << 20, N=1 << 11) == -4
    torch.cuda.synchronize()


# ---------------------------------------------------------- pmlp_rnd_loss_step --
def _loss_launch(mu, tgt_all, idx, scale, Ap, with_f=True):
    M, E = mu.shape
    d = dict(dmu_b=torch.full((M, Ap), 3.0, dtype=torch.bfloat16, device=DEV),
             dmu_f=torch.full((M, E), 7.0, device=DEV) if with_f else None,
             partial=torch.full((rr.num_partials(M),), 7.0, device=DEV), stats=torch.full((4,), 7.0, device=DEV))
    mm.rnd_loss_step(_dev(mu), _dev(tgt_all), _dev(idx), scale, d["partial"], d["stats"], d["dmu_b"], d["dmu_f"])
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("M", rr.LOSS_ROWS)
@pytest.mark.parametrize("E", rr.WIDTHS)
def test_loss_step_against_the_reference(M, E):
    mu, tgt_all, idx = rr.loss_case(M, E)
    scale = rr.loss_scale(M, E)
    for Ap in rr.LOSS_PADS[E]:
        d = _loss_launch(mu, tgt_all, idx, scale, Ap)
        fr = rr.check_loss_step(_bits(d["dmu_b"]), d["dmu_f"].cpu().numpy(), d["partial"].cpu().numpy(),
                                d["stats"].cpu().numpy(), mu, tgt_all, idx, scale)
        print(f"[rnd] loss M={M} E={E} Ap={Ap}: worst fractions of the bounds {fr}")
        again = _loss_launch(mu, tgt_all, idx, scale, Ap, with_f=False)  # a replay, without the fp32 copy
        for k in ("dmu_b", "partial", "stats"):
            assert torch.equal(again[k].view(torch.int16) if k == "dmu_b" else again[k],
                               d[k].view(torch.int16) if k == "dmu_b" else d[k]), k


@pytest.mark.parametrize("M", rr.LOSS_ROWS + (64,))
@pytest.mark.parametrize("E", rr.WIDTHS)
def test_loss_step_with_the_identity_index_is_the_distillation_kernel(M, E):
    """idx = the identity and R = M: every output is pmlp_distill_loss_step(MSE)'s, bit for bit."""
    mu, tgt_all, idx = rr.loss_case(M, E)
    target = tgt_all[idx]
    scale = rr.loss_scale(M, E)
    for Ap in rr.LOSS_PADS[E]:
        d = _loss_launch(mu, target, np.arange(M, dtype=np.int64), scale, Ap)
        ref = dict(dmu_b=torch.full((M, Ap), 3.0, dtype=torch.bfloat16, device=DEV),
                   dmu_f=torch.full((M, E), 7.0, device=DEV),
                   partial=torch.full((rr.num_partials(M),), 7.0, device=DEV), stats=torch.full((4,), 7.0, device=DEV))
        mm.distill_loss_step(_dev(mu), _dev(target), "mse", scale, ref["partial"], ref["stats"], ref["dmu_b"],
                             ref["dmu_f"])
        torch.cuda.synchronize()
        assert torch.equal(d["dmu_b"].view(torch.int16), ref["dmu_b"].view(torch.int16))
        for k in ("dmu_f", "partial", "stats"):
            check_equal(d[k].cpu().numpy(), ref[k].cpu().numpy(), f"{k} (Ap={Ap})")


def test_loss_step_refusals():
    lib, P = mm.load(), mm._p
    f = torch.zeros(64 * 40, device=DEV)
    b = torch.zeros(64 * 40 + 8, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(64, dtype=torch.int64, device=DEV)
    names = ("mu", "tgt_all", "idx", "M", "R", "A", "scale", "partial", "stats", "dmu_b", "dmu_f", "Ap", "stream")
    ok = dict(zip(names, (P(f), P(f), P(idx), 64, 64, 12, 0.5, P(f), P(f), P(b), None, 16, mm._stream())))

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.pmlp_rnd_loss_step(*[a[n] for n in names])
    assert call() == 0
    for k in ("mu", "tgt_all", "idx", "partial", "stats", "dmu_b"):
        assert call(**{k: None}) == -1, k
    assert call(M=0) == -1 and call(R=0) == -1 and call(A=0) == -1
    assert call(A=33, Ap=40) == -3
    assert call(Ap=8) == -4 and call(Ap=12) == -4 and call(Ap=40) == -4
    assert call(dmu_b=P(b) + 2) == -5
    torch.cuda.synchronize()


# ------------------------------------------------ the fused step, the plain path --
HID, S, E, RSRC, MB = [64, 32, 32], 48, 12, 256, 128


def _rnd(hid=HID, S=S, E=E, lr=1e-3):
    return RandomNetworkDistillation(S, parse_cfg(dict(weight=1.0, num_outputs=E, predictor_hidden_dims=hid,
                                                       target_hidden_dims=hid, learning_rate=lr)), DEV)


def _adam(rnd, lr_t):
    return torch.optim.Adam(list(rnd.predictor.parameters()), lr=lr_t, fused=True, capturable=True)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_fused_step_against_the_plain_path():
    """FusedRndStep.run against the plain autograd step on gathered rows, from equal weights: the
    quantities and bounds of test_gpu_distill's comparison of FusedDistillStep with its plain path
    (per-tensor gradient distance at most twice FusedPPOStep's at the same layer shapes and rows;
    the loss within rtol 2e-2 / atol 2e-3; after n Adam steps the parameters within n x 3 lr)."""
    from test_gpu_distill import _ppo_figures
    lr = 1e-3
    rnd = _rnd()
    plain = copy.deepcopy(rnd)
    twin = copy.deepcopy(rnd)
    g = torch.Generator(device=DEV).manual_seed(5)
    states = torch.randn(RSRC, S, device=DEV, generator=g)
    idx = torch.randperm(RSRC, device=DEV, generator=g)[:MB]
    idx[1] = idx[0]  # a repeated row
    with torch.no_grad():
        tgt_all = rnd.target(states) + 0.5 * torch.randn(RSRC, E, device=DEV, generator=g)
    lr_t = torch.tensor(lr, device=DEV)
    f = rnd_step.FusedRndStep(rnd, _adam(rnd, lr_t), lr_t, MB)
    assert f.k0p == 48 and rnd_step.rnd_k0(87) == 96 and rnd_step.rnd_k0(274) == 320
    acc = torch.zeros(2, device=DEV)
    f.run(idx, states, tgt_all, acc)
    torch.cuda.synchronize()
    loss = torch.nn.functional.mse_loss(plain.predictor(states[idx]), tgt_all[idx])
    loss.backward()
    lins = lambda m: [x for x in m.predictor if isinstance(x, torch.nn.Linear)]  # noqa: E731
    figs = []
    for a, b in zip(lins(rnd), lins(plain)):
        figs += [_rel(f._gview[id(a.weight)], b.weight.grad), _rel(f._gview[id(a.bias)], b.bias.grad)]
    yard = _ppo_figures(S, S)
    print("[rnd] relative L2 distance of the fused gradient from fp32 autograd, per tensor (W0 b0 .. W3 b3)\n"
          "  RND          " + " ".join(f"{v:.3e}" for v in figs) + "\n  PPO (actor)  " + " ".join(f"{v:.3e}" for v in yard))
    np.testing.assert_allclose(float(acc[1]), float(loss), rtol=2e-2, atol=2e-3)
    # -- two steps from the same weights on both paths
    lr2 = torch.tensor(lr, device=DEV)
    f2 = rnd_step.FusedRndStep(twin, _adam(twin, lr2), lr2, MB)
    opt = torch.optim.Adam(list(plain.predictor.parameters()), lr=lr)
    s0 = [p.detach().clone() for p in twin.predictor.parameters()]
    t0 = [p.detach().clone() for p in twin.target.parameters()]
    acc2, tot = torch.zeros(2, device=DEV), 0.0
    for _ in range(2):
        f2.run(idx, states, tgt_all, acc2)
        ls = torch.nn.functional.mse_loss(plain.predictor(states[idx]), tgt_all[idx])
        opt.zero_grad()
        ls.backward()
        opt.step()
        tot += float(ls)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(acc2[1]) / 2, tot / 2, rtol=2e-2, atol=2e-3)
    for a, b, c in zip(twin.predictor.parameters(), plain.predictor.parameters(), s0):
        da, db = a.detach() - c, b.detach() - c
        assert da.abs().max() > 0
        assert (da - db).abs().max() <= 2 * 3 * lr
    assert all(torch.equal(p.detach(), q) for p, q in zip(twin.target.parameters(), t0))
    assert float(f2.step_t) == 2
    for k, (d, y) in enumerate(zip(figs, yard)):
        assert d <= 2.0 * y, f"tensor {k}: RND {d:.3e} above twice PPO's {y:.3e}"


# ------------------------------------------------------- PPO on the fake env --
N, T, O, A = 64, 8, 48, 12
RND_CFG = dict(weight=0.5, num_outputs=E, predictor_hidden_dims=HID, target_hidden_dims=HID, learning_rate=1e-3,
               state="policy")


def _runner(rnd, seed=3):
    cfg = {"runner": {"policy_class_name": "ActorCritic", "algorithm_class_name": "PPO", "num_steps_per_env": T,
                      "save_interval": 50},
           "algorithm": {"num_learning_epochs": 2, "num_mini_batches": 4, "learning_rate": 1e-3},
           "policy": {"actor_hidden_dims": HID, "critic_hidden_dims": HID, "activation": "elu", "init_noise_std": 1.0}}
    if rnd is not None:
        cfg["algorithm"]["rnd_cfg"] = rnd
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    env = FakeEnv(num_envs=N, num_obs=O, num_actions=A, device=DEV)
    return OnPolicyRunner(env, cfg, log_dir=None, device=DEV)


def _collect(runner):
    obs = runner.env.get_observations()
    with torch.inference_mode():
        for _ in range(T):
            obs, _, *_ = runner._collect_step(obs, obs)
    return obs


def test_ppo_reward_pass_and_captured_update(monkeypatch, tmp_path):
    sched = {"mode": "linear", "initial_step": 0, "final_step": 4 * T, "final_value": 0.0}
    runner = _runner(dict(RND_CFG, weight_schedule=sched))
    alg = runner.alg
    assert alg._fused is not None and alg._rnd_fused is not None and alg._rnd_pass is not None
    f, rf, rp = alg._fused, alg._rnd_fused, alg._rnd_pass
    rp.intrinsic = torch.zeros(T * N, device=DEV)
    for it in range(3):
        obs = _collect(runner)
        st = alg.storage
        alg.flush_rollout()
        before = st.rewards.clone()
        rf.ensure_weights()
        rp.ensure_target()
        with torch.inference_mode():
            alg.compute_returns(obs)
        torch.cuda.synchronize()
        # the bonus against the reference, from the kernel's own operands (the forward's outputs)
        w = np.array([alg.rnd.weight_at(it * T + t) for t in range(T)], np.float32)
        check_equal(rp.w.cpu().numpy(), w, "w")
        fr = rr.check_reward(st.rewards.cpu().numpy(), rp.intrinsic.cpu().numpy(), rp.partial.cpu().numpy(),
                             rp.stats.cpu().numpy(), rp.pred.cpu().numpy(), rp.tgt_all.cpu().numpy(), w,
                             before.cpu().numpy(), N)
        print(f"[rnd] PPO reward pass, iteration {it}: worst fractions {fr}")
        # and the forward's outputs against the fp32 nets (bf16 operands: the forward's own tolerance)
        rows = st.observations.flatten(0, 1)
        with torch.no_grad():
            torch.testing.assert_close(rp.tgt_all, alg.rnd.target(rows), rtol=5e-2, atol=5e-2)
            torch.testing.assert_close(rp.pred, alg.rnd.predictor(rows), rtol=5e-2, atol=5e-2)
        assert float(rp.stats[0]) > 0
        if it < 2:
            alg.update()
    # -- the third update: replayed from the captured graph, then eagerly from the same snapshot
    assert alg._fgraph is not None
    state = [f.flat, f.exp_avg, f.exp_avg_sq, f.step_t, alg._lr, rf.flat, rf.exp_avg, rf.exp_avg_sq, rf.step_t,
             st.advantages, st.returns] + [w_ for ws in f.wb for w_ in ws] + \
        ([w_ for ws in f.wf for w_ in ws] if f.wf else []) + list(rf.wb) + list(rf.wf)
    snap = [t.clone() for t in state]
    pred0 = rf.flat.clone()
    alg.update()
    torch.cuda.synchronize()
    got = [f.flat.clone(), f.exp_avg.clone(), rf.flat.clone(), rf.exp_avg.clone(), rf.exp_avg_sq.clone(),
           alg._rnd_acc.clone(), alg._facc.clone()]
    assert not torch.equal(got[2], pred0) and float(rf.step_t) == 3 * 8
    for t, s in zip(state, snap):
        t.copy_(s)
    monkeypatch.setattr(mm, "permutation_", lambda out: None)  # the same mini-batches
    alg.use_graph = False
    alg.storage.step = T
    alg.update()
    torch.cuda.synchronize()
    want = [f.flat, f.exp_avg, rf.flat, rf.exp_avg, rf.exp_avg_sq, alg._rnd_acc, alg._facc]
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), k
    assert float(alg.rnd_loss_mean) > 0
    # -- a load reconverts the target's bf16 copies (and the predictor's)
    monkeypatch.undo()
    path = str(tmp_path / "m.pt")
    runner.save(path)
    other = _runner(dict(RND_CFG, weight_schedule=sched, seed=4), seed=8)
    oa = other.alg
    oa._rnd_pass.ensure_target()
    oa._rnd_fused.ensure_weights()
    stale = [w_.clone() for w_ in oa._rnd_pass.twb]
    other.load(path)
    assert oa._rnd_pass.target_changed and oa._rnd_fused.weights_changed
    oa._rnd_fused.ensure_weights()
    oa._rnd_pass.ensure_target()
    rp.target_changed = True
    rp.ensure_target()
    for a, b, c in zip(oa._rnd_pass.twb, rp.twb, stale):
        assert torch.equal(a, b) and not torch.equal(a, c)
    for a, b in zip(oa._rnd_fused.wb, rf.wb):
        assert torch.equal(a, b)
    assert torch.equal(oa._rnd_fused.exp_avg, rf.exp_avg) and float(oa._rnd_fused.step_t) == float(rf.step_t)


def test_weight_zero_is_bitwise_the_run_without_rnd():
    """The PPO kernels are untouched and the update graph only gained launches: with the weight
    held at 0 the policy after three iterations is the RND-off run's, bit for bit."""
    off = _runner(None)
    off.learn(3)
    on = _runner(dict(RND_CFG, weight=0.0, weight_schedule={"mode": "constant"}))
    on.learn(3)
    torch.cuda.synchronize()
    assert off.alg._fused is not None and on.alg._rnd_fused is not None and on.alg._fgraph is not None
    for p, q in zip(off.alg.actor_critic.parameters(), on.alg.actor_critic.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(off.alg._fused.exp_avg, on.alg._fused.exp_avg)
    assert float(on.alg.rnd_loss_mean) > 0 and float(on.alg._rnd_fused.step_t) == 3 * 8


def test_nets_the_fused_pieces_refuse_take_the_plain_path_untouched():
    """A target of two hidden layers (an ordinary rsl_rl cfg) is not a net the one-launch forward
    takes: beside the fused PPO update the predictor then trains on the plain path, with a warning,
    on an optimizer nothing has rewired.  Each update is compared with a literal fp32 Adam loop on
    the update's own mini-batches.  The tolerance: both sides are fp32 Adam on the same fp32
    gradients and may differ by the rounding of a differently ordered update, orders below
    lr / 50 = 2e-5, while a wrong step count (bias correction) moves a first step by about lr / 2."""
    cfg = dict(RND_CFG, target_hidden_dims=[128, 64])
    with pytest.warns(UserWarning, match="plain fp32 path.*does not take the target's shape"):
        runner = _runner(cfg)
    alg = runner.alg
    assert alg._fused is not None and alg._rnd_fused is None and alg._rnd_pass is None
    assert rnd_step.supported(alg.rnd, N * T // 4) is not None
    params = list(alg.rnd.predictor.parameters())
    ref = copy.deepcopy(alg.rnd.predictor)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    for it in range(3):  # eager, captured, replayed
        obs = _collect(runner)
        st = alg.storage
        alg.flush_rollout()
        before = st.rewards.clone()
        with torch.inference_mode():
            alg.compute_returns(obs)
        rows = st.observations.flatten(0, 1)
        with torch.no_grad():  # the plain reward pass: the torch statement
            d = alg.rnd.target(rows) - alg.rnd.predictor(rows)
            r = torch.sqrt((d * d).sum(dim=1))
        # (two fp32 evaluations of one expression on the device: a few ulps of r, which is of order one)
        torch.testing.assert_close(st.rewards, before + (0.5 * r).view(T, N, 1), rtol=0, atol=1e-6)
        assert not torch.equal(st.rewards, before)
        alg.update()
        torch.cuda.synchronize()
        perm, mb, tot = alg._fperm.clone(), N * T // 4, 0.0
        with torch.no_grad():
            tgt = alg.rnd.target(rows)
        for _ in range(2):
            for i in range(4):
                idx = perm[i * mb:(i + 1) * mb]
                loss = torch.nn.functional.mse_loss(ref(rows[idx]), tgt[idx])
                opt.zero_grad()
                loss.backward()
                opt.step()
                tot += float(loss)
        steps = {float(alg.rnd_optimizer.state[p]["step"]) for p in params}
        assert steps == {8.0 * (it + 1)}, steps  # one count per optimizer step, not one per parameter tensor
        assert len({alg.rnd_optimizer.state[p]["step"].data_ptr() for p in params}) == len(params)
        for a, b in zip(params, ref.parameters()):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(float(alg.rnd_loss_mean), tot / 8, rtol=1e-4)
    assert alg._fgraph is not None  # the PPO steps were captured all the same


@pytest.mark.parametrize("S,k0p", [(87, 96), (274, 320)])
def test_fused_pieces_engage_at_the_tasks_shapes(S, k0p):
    """The privileged rows of go2_robust_rnd / go2_terrain_robust_rnd with the default nets: the
    fused pieces take them (a silent loss of the hot path would show here), the reward pass agrees
    with the fp32 nets to the forward's bf16 tolerance and one step's loss with the plain mse."""
    rnd = RandomNetworkDistillation(S, parse_cfg(dict(weight=1.0)), DEV)
    Tn, Nn, M = 2, 64, 32
    assert rnd_step.supported(rnd, M) is None and rnd_step.rnd_k0(S) == k0p
    lr_t = torch.tensor(1e-3, device=DEV)
    f = rnd_step.FusedRndStep(rnd, _adam(rnd, lr_t), lr_t, M)
    rp = rnd_step.RndRewardPass(f, Tn, Nn)
    assert f.k0p == k0p and rp.k0p == k0p
    g = torch.Generator(device=DEV).manual_seed(S)
    states = torch.randn(Tn * Nn, S, device=DEV, generator=g)
    rew = torch.zeros(Tn, Nn, 1, device=DEV)
    rp.set_weights([1.0, 0.5])
    rp.run(states, rew)
    with torch.no_grad():
        tgt, pred = rnd.target(states), rnd.predictor(states)
        torch.testing.assert_close(rp.tgt_all, tgt, rtol=5e-2, atol=5e-2)
        torch.testing.assert_close(rp.pred, pred, rtol=5e-2, atol=5e-2)
    fr = rr.check_reward(rew.cpu().numpy(), None, rp.partial.cpu().numpy(), rp.stats.cpu().numpy(),
                         rp.pred.cpu().numpy(), rp.tgt_all.cpu().numpy(), np.array([1.0, 0.5], np.float32),
                         np.zeros(Tn * Nn, np.float32), Nn)
    assert max(fr.values()) <= 1.0
    idx = torch.randperm(Tn * Nn, device=DEV, generator=g)[:M].contiguous()
    acc = torch.zeros(2, device=DEV)
    with torch.no_grad():
        want = float(torch.nn.functional.mse_loss(pred[idx], rp.tgt_all[idx]))
    f.run(idx, states, rp.tgt_all, acc)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(acc[1]), want, rtol=2e-2, atol=2e-3)
    assert float(f.step_t) == 1


# -------------------------------------------------------------------- scripts --
def test_train_then_play():
    from test_gpu_scripts import run
    exp = "pytest_go2_robust_rnd"
    out = run("train.py", "--task", "go2_robust_rnd", "--num_envs", "64", "--max_iterations", "2", "--headless",
              "--experiment_name", exp, "--run_name", "cli")
    assert "Learning iteration 1/2" in out and "RND loss:" in out
    from legged_gym import LEGGED_GYM_ROOT_DIR
    runs = sorted(glob.glob(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "*_cli")))
    assert runs, "train.py wrote no run directory"
    ck = torch.load(os.path.join(runs[-1], "model_2.pt"), map_location="cpu", weights_only=True)
    assert {"rnd_state_dict", "rnd_optimizer_state_dict"} <= set(ck)
    assert ck["rnd_state_dict"]["predictor.0.weight"].shape == (256, 87)
    assert ck["rnd_state_dict"]["target.6.weight"].shape == (16, 64)
    run("play.py", "--task", "go2_robust_rnd", "--headless", "--experiment_name", exp, "--load_run",
        os.path.basename(runs[-1]))
    pol = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "exported", "policies", "policy_1.pt")
    assert os.path.exists(pol)
    m = torch.jit.load(pol)
    n_in = ck["model_state_dict"]["actor.0.weight"].shape[1]
    assert n_in == 240 and m(torch.zeros(3, n_in)).shape == (3, 12)
