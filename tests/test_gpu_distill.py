"""Teacher-student distillation on the GPU: the fused optimizer step against the
plain fp32 path, the captured update against the eager one, the teacher and student tasks through
the runner, the checkpoint rule in a captured rollout, imitation of a frozen teacher and the
export of the student."""
import copy
import os
from collections import deque

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from legged_gym.envs import task_registry  # noqa: E402
from legged_gym.utils.helpers import class_to_dict, export_policy_as_jit  # noqa: E402
from rsl_rl.algorithms import PPO, Distillation  # noqa: E402
from rsl_rl.algorithms.distillation import DistillRollout, FusedDistillStep  # noqa: E402
from rsl_rl.modules import ActorCritic, StudentTeacher  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402
from test_gpu_parity import make  # noqa: E402

DEV = "cuda"
HID = [64, 32, 32]
N, T, G, A = 64, 4, 2, 12
# (student inputs, teacher inputs): the narrow forward, and the wide one (K0 448 and 320)
WIDTHS = {"narrow": (48, 32), "wide": (427, 274)}


def _policy(O, P, seed=0, mixed=True):
    torch.manual_seed(seed)
    pol = StudentTeacher(O, P, A, HID, HID, mixed_precision=mixed).to(DEV)
    pol.loaded_teacher = True  # (a random frozen teacher)
    return pol


def _alg(pol, **kw):
    alg = Distillation(pol, num_learning_epochs=1, gradient_length=G, learning_rate=1e-3, loss_type="mse",
                       device=DEV, **kw)
    alg.init_storage(N, T, [pol.student[0].in_features], [pol.teacher[0].in_features], [A])
    return alg


def _fill(alg, seed):
    """Synthetic rows: the teacher's fp32 actions on random privileged rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    st, pol = alg.storage, alg.actor_critic
    st.observations.copy_(torch.randn(st.observations.shape, device=DEV, generator=g))
    tobs = torch.randn(T, N, pol.teacher[0].in_features, device=DEV, generator=g)
    with torch.no_grad():
        st.privileged_actions.copy_(pol.teacher(tobs) + 0.5 * torch.randn(T, N, A, device=DEV, generator=g))
    st.step = T


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _ppo_figures(O, P):
    """The yardstick: FusedPPOStep's flat gradient against PPO's fp32 autograd gradient, per
    parameter tensor of the actor, on one mini-batch of G x N rows at the same layer shapes."""
    torch.manual_seed(0)
    ac32 = ActorCritic(O, P, A, HID, HID, mixed_precision=False).to(DEV)
    acbf = copy.deepcopy(ac32)
    acbf.mixed_precision = True
    kw = dict(num_learning_epochs=1, num_mini_batches=T // G, learning_rate=1e-3, schedule="fixed", device=DEV)
    ref = PPO(ac32, fused_loss=False, **kw)
    fus = PPO(acbf, **kw)
    for alg in (ref, fus):
        alg.init_storage(N, T, [O], [P], [A])
    assert fus._fused is not None and fus._fused.fused_fwd
    g = torch.Generator(device=DEV).manual_seed(3)
    st = ref.storage
    with torch.inference_mode():
        for _ in range(T):
            obs, cobs = torch.randn(N, O, device=DEV, generator=g), torch.randn(N, P, device=DEV, generator=g)
            ref._rollout = None
            ref.act(obs, cobs)
            rew = 0.2 * torch.randn(N, device=DEV, generator=g)
            done = torch.rand(N, device=DEV, generator=g) < 0.05
            ref.process_env_step(rew, done, {"time_outs": done})
        ref.compute_returns(torch.randn(N, P, device=DEV, generator=g))
    names = ("observations", "privileged_observations", "actions", "values", "advantages", "returns",
             "actions_log_prob", "mu", "sigma")
    src = tuple(getattr(st, n).flatten(0, 1).clone() for n in names)
    M = G * N
    rows = torch.arange(M, device=DEV)
    f = fus._fused
    f.run(rows, src, torch.zeros(2, device=DEV))
    torch.cuda.synchronize()
    obs, cobs, actions, values, adv, ret, logp, mu, sigma = [t[:M] for t in src]
    loss, _, _ = ref._reference_loss(obs, cobs, actions, values, adv, ret, logp, mu, sigma, (None, None), None)
    ref.optimizer.zero_grad()
    loss.backward()
    lf = [m for m in acbf.actor if isinstance(m, torch.nn.Linear)]
    lr = [m for m in ac32.actor if isinstance(m, torch.nn.Linear)]
    figs = []
    for a, b in zip(lf, lr):
        figs += [_rel(f._gview[id(a.weight)], b.weight.grad), _rel(f._gview[id(a.bias)], b.bias.grad)]
    return figs


@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_fused_step_against_the_plain_path(width):
    O, P = WIDTHS[width]
    pol = _policy(O, P)
    p32 = copy.deepcopy(pol)
    p32.mixed_precision = False
    fus, ref = _alg(pol), _alg(p32, fused=False)
    assert isinstance(fus._fused, FusedDistillStep) and isinstance(fus._rollout, DistillRollout)
    assert ref._fused is None and ref._rollout is None
    assert fus._fused.k0p == {48: 48, 427: 448}[O] and fus._rollout.tk0p == {32: 32, 274: 320}[P]
    _fill(fus, 1)
    ref.storage.observations.copy_(fus.storage.observations)
    ref.storage.privileged_actions.copy_(fus.storage.privileged_actions)
    ref.storage.step = T
    # -- the gradient of the first optimizer step: the fused flat gradient against fp32 autograd
    f, st = fus._fused, fus.storage
    M = G * N
    obs, tgt = st.observations.flatten(0, 1), st.privileged_actions.flatten(0, 1)
    twin = copy.deepcopy(pol)  # (the step below trains pol: the gradient goes with these weights)
    f.run(obs[:M], tgt[:M], torch.zeros(2, device=DEV))
    torch.cuda.synchronize()
    loss = sum(torch.nn.functional.mse_loss(p32.student(st.observations[t]), st.privileged_actions[t])
               for t in range(G))
    loss.backward()
    figs = []
    for a, b in zip([m for m in pol.student if isinstance(m, torch.nn.Linear)],
                    [m for m in p32.student if isinstance(m, torch.nn.Linear)]):
        figs += [_rel(f._gview[id(a.weight)], b.weight.grad), _rel(f._gview[id(a.bias)], b.bias.grad)]
    yard = _ppo_figures(O, P)
    print(f"[distill] {width}: relative L2 distance of the fused gradient from fp32 autograd, per tensor "
          f"(W0 b0 W1 b1 W2 b2 W3 b3)\n  distillation " + " ".join(f"{v:.3e}" for v in figs) +
          "\n  PPO (actor)  " + " ".join(f"{v:.3e}" for v in yard))
    # -- one whole update from the same weights: the behaviour loss
    fus2 = _alg(twin)
    fus2.storage.observations.copy_(st.observations)
    fus2.storage.privileged_actions.copy_(st.privileged_actions)
    fus2.storage.step = T
    for p in p32.student.parameters():
        p.grad = None
    s0 = [p.detach().clone() for p in twin.student.parameters()]
    t0 = [p.detach().clone() for p in twin.teacher.parameters()]
    l_fus, l_ref = fus2.update(), ref.update()
    print(f"[distill] {width}: behaviour loss fused {l_fus:.6f} plain {l_ref:.6f}")
    np.testing.assert_allclose(l_fus, l_ref, rtol=2e-2, atol=2e-3)
    lr = 1e-3
    for a, b, c in zip(twin.student.parameters(), p32.student.parameters(), s0):
        da, db = a.detach() - c, b.detach() - c
        assert da.abs().max() > 0
        assert (da - db).abs().max() <= 2 * 3 * lr  # two Adam steps of at most ~lr per entry each
    assert all(torch.equal(p.detach(), q) for p, q in zip(twin.teacher.parameters(), t0))
    assert torch.equal(twin.std.detach(), p32.std.detach())
    # nothing new may add error: the same bf16 operands and split-K as PPO's step
    for k, (d, y) in enumerate(zip(figs, yard)):
        assert d <= 2.0 * y, f"tensor {k}: distillation {d:.3e} above twice PPO's {y:.3e}"


def test_captured_update_is_bitwise_the_eager_fused_update():
    O, P = WIDTHS["narrow"]
    pol = _policy(O, P)
    algs = [_alg(copy.deepcopy(pol)), _alg(copy.deepcopy(pol))]
    algs[0].use_graph = False
    _fill(algs[0], 2)
    losses = []
    for alg in algs:
        alg.storage.observations.copy_(algs[0].storage.observations)
        alg.storage.privileged_actions.copy_(algs[0].storage.privileged_actions)
        out = []
        for _ in range(3):  # eager, then (captured and) replayed twice
            alg.storage.step = T
            out.append(alg.update())
        losses.append(out)
    assert algs[0]._fgraph is None and algs[1]._fgraph is not None
    assert losses[0] == losses[1] and losses[0][2] < losses[0][0]
    for a, b in zip(algs[0].actor_critic.state_dict().values(), algs[1].actor_critic.state_dict().values()):
        assert torch.equal(a, b)
    assert torch.equal(algs[0]._fused.exp_avg, algs[1]._fused.exp_avg)
    assert float(algs[1]._fused.step_t) == 3 * (T // G)


# ------------------------------------------------------------------ the tasks --
def _runner(task, n, **runner_cfg):
    env = make(task, n)
    cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(task)[1]))
    cfg["runner"].update(runner_cfg)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    return env, OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")


@pytest.fixture(scope="module")
def teacher_checkpoint(tmp_path_factory):
    """go2_robust_teacher at 64 envs: two PPO iterations on the native path, saved."""
    env, runner = _runner("go2_robust_teacher", 64)
    try:
        assert env.num_obs == 87 and env.num_privileged_obs is None
        assert runner.alg._fused is not None and runner.alg._rollout is not None, "native PPO path not active"
        assert runner.alg.actor_critic.actor[0].in_features == 87 == runner.alg.actor_critic.critic[0].in_features
        obs = env.get_observations()
        assert obs is env.privileged_obs_buf and obs.shape == (64, 87) and env.get_privileged_observations() is None
        runner.learn(2)
        torch.cuda.synchronize()
        assert runner._rollout_graph is not None
        assert env.get_observations() is env.privileged_obs_buf
        assert runner.alg.storage.observations.shape[-1] == 87 and runner.alg.storage.privileged_observations is None
        path = str(tmp_path_factory.mktemp("teacher") / "model_2.pt")
        runner.save(path)
        sd = {k: v.detach().cpu().clone() for k, v in runner.alg.actor_critic.state_dict().items()}
    finally:
        env.close()
    return path, sd


def test_teacher_env_presents_the_asym_envs_privileged_row():
    """Same seed and actions: the teacher env's observation is bitwise the _asym env's privileged row."""
    teacher, asym = make("go2_robust_teacher", 64), make("go2_robust_asym", 64)
    try:
        assert (teacher.num_obs, teacher.num_privileged_obs) == (87, None)
        assert (asym.num_obs, asym.num_privileged_obs) == (240, 87)
        ot, pt = teacher.reset()
        oa, pa = asym.reset()
        assert pt is None and torch.equal(ot, pa)
        g = torch.Generator(device=DEV).manual_seed(4)
        for _ in range(6):
            a = 0.5 * torch.randn(64, 12, device=DEV, generator=g)
            ot, pt, rt, dt, _ = teacher.step(a.clone())
            oa, pa, ra, da, _ = asym.step(a.clone())
            assert pt is None and ot.shape == (64, 87)
            assert torch.equal(ot, pa) and torch.equal(rt, ra) and torch.equal(dt, da)
            assert teacher.get_observations() is ot and teacher.get_privileged_observations() is None
            assert torch.equal(teacher.obs_buf, oa)  # (the inner policy row is still built)
    finally:
        teacher.close()
        asym.close()


def _mlp(sd, x):
    keys = sorted({int(k.split(".")[0]) for k in sd})
    for i, k in enumerate(keys):
        x = torch.nn.functional.linear(x, sd[f"{k}.weight"], sd[f"{k}.bias"])
        if i < len(keys) - 1:
            x = torch.nn.functional.elu(x)
    return x


def test_runner_end_to_end(teacher_checkpoint, tmp_path):
    tpath, tsd = teacher_checkpoint
    env, runner = _runner("go2_robust_distill", 64)
    try:
        alg, pol = runner.alg, runner.alg.actor_critic
        assert isinstance(alg, Distillation) and isinstance(pol, StudentTeacher)
        assert pol.student[0].in_features == 240 and pol.teacher[0].in_features == 87
        assert isinstance(alg._fused, FusedDistillStep) and isinstance(alg._rollout, DistillRollout)
        assert alg._fused.M == 6 * 64 and not runner._defer_env_extras()
        with pytest.raises(ValueError, match="teacher"):
            alg.update()
        runner.load_teacher(tpath)
        assert pol.loaded_teacher and runner.current_learning_iteration == 0
        s0 = [p.detach().clone() for p in pol.student.parameters()]
        runner.learn(3)
        torch.cuda.synchronize()
        assert runner._rollout_graph is not None and alg._fgraph is not None
        assert all(torch.isfinite(p).all() and not torch.equal(p.detach(), q)
                   for p, q in zip(pol.student.parameters(), s0))
        # the teacher and std are bitwise what was loaded / initialised
        for k, v in pol.teacher.state_dict().items():
            assert torch.equal(v.cpu(), tsd["actor." + k])
        assert torch.equal(pol.std.detach().cpu(), torch.full((12,), 0.1))
        # the last stored step: its rows were the env's buffers of the other parity
        Tn = runner.num_steps_per_env
        st, ro = alg.storage, alg._rollout
        obs_last, priv_last = env._obs_bufs[env._buf_idx ^ 1], env._priv_bufs[env._buf_idx ^ 1]
        assert torch.equal(st.observations[Tn - 1], obs_last)
        want = torch.empty(64, 12, device=DEV)
        mm.mlp_forward([ro.teacher_job(priv_last, want)], 64)  # the teacher alone, through mfma_mlp
        torch.cuda.synchronize()
        assert torch.equal(st.privileged_actions[Tn - 1], want)
        with torch.no_grad():
            torch.testing.assert_close(want, pol.teacher(priv_last), rtol=2e-2, atol=2e-3)
            torch.testing.assert_close(mm.mlp_apply(pol.teacher, priv_last), want, rtol=1e-5, atol=1e-6)

        # -- a checkpoint round-trips, and the captured rollout sees loaded student weights
        spath = str(tmp_path / "student" / "model_3.pt")
        runner.save(spath)
        ck = torch.load(spath, map_location="cpu", weights_only=True)
        assert ck["iter"] == 3 and not any(k.startswith("actor.") for k in ck["model_state_dict"])
        for k, v in pol.state_dict().items():
            assert torch.equal(ck["model_state_dict"][k], v.cpu())
        ck["model_state_dict"]["student.6.bias"] = ck["model_state_dict"]["student.6.bias"] + 1.0
        ck["iter"] = 7
        moved = str(tmp_path / "student" / "model_7.pt")
        torch.save(ck, moved)
        before = ro.out[0].clone()
        runner.load(moved)
        assert runner.current_learning_iteration == 7
        obs, priv = env.get_observations(), env.get_privileged_observations()
        with torch.inference_mode():
            runner._collection(obs, priv, [], deque(), deque(), runner._cur_reward_sum, runner._cur_episode_length)
        torch.cuda.synchronize()
        assert runner._rollout_graph is not None  # (the replay, not a new eager loop)
        alg.storage.clear()
        last = env._obs_bufs[env._buf_idx ^ 1]
        with torch.no_grad():
            torch.testing.assert_close(ro.out[0], pol.student(last), rtol=2e-2, atol=2e-3)
        assert float((ro.out[0] - before).mean()) > 0.5  # the moved bias is in the replayed forward

        # -- the export: policy_1.pt is the student, on CPU rows
        out = str(tmp_path / "exported")
        export_policy_as_jit(pol, out)
        m = torch.jit.load(os.path.join(out, "policy_1.pt"))
        x = torch.randn(5, 240)
        sd = {k[len("student."):]: v.cpu() for k, v in pol.state_dict().items() if k.startswith("student.")}
        torch.testing.assert_close(m(x), _mlp(sd, x), rtol=1e-5, atol=1e-6)
        with torch.no_grad():
            torch.testing.assert_close(m(x), copy.deepcopy(pol).cpu().act_inference(x), rtol=1e-5, atol=1e-6)
    finally:
        env.close()


def test_student_imitates_a_frozen_teacher():
    """256 envs, 20 iterations, a fixed seed and a random frozen teacher: the behaviour loss falls."""
    env, runner = _runner("go2_robust_distill", 256)
    try:
        alg = runner.alg
        alg.actor_critic.loaded_teacher = True
        losses, update = [], alg.update

        def recorded(host_means=True):
            losses.append(update(host_means=True))
            return losses[-1]
        alg.update = recorded
        runner.learn(20)
        torch.cuda.synchronize()
        assert runner._rollout_graph is not None and alg._fgraph is not None
        first, last = float(np.mean(losses[:5])), float(np.mean(losses[-5:]))
        print(f"[distill] imitation: mean behaviour loss of iterations 0-4 {first:.6f}, 15-19 {last:.6f}")
        assert np.isfinite(losses).all() and last < first
    finally:
        env.close()
