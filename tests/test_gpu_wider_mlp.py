"""The fused MLP forward past 256 inputs (csrc/ppo_mlp.hip k_mlp_fwd, the WIDER forms; DESIGN
3.13): K0 a multiple of 64 up to 512.  The plain forward, the rollout form and the update forward
with the loss at a 427 / 427 actor-critic (go2_terrain_robust: five 48-entry frames in front of
the 187-point height scan, padded to 448), the rest of the optimizer step at that width, and the
task training on them as captured graphs.

The method and the bars are tests/test_gpu_wide_mlp.py's: the per-layer GEMMs (bitwise), the three
launches pmlp_mlp_forward + pmlp_act + pmlp_store_step_env (bitwise), the fp32 autograd update
(the bars of test_gpu_fused_ppo.py at 48 inputs), and an eager runner on the same seed (bitwise)."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCritic, mfma_mlp  # noqa: E402
from test_gpu_fused_ppo import _fill_storage  # noqa: E402
from test_gpu_parity import make  # noqa: E402
from test_gpu_terrain_curriculum import MAP  # noqa: E402
from test_gpu_wide_mlp import A, HID, _pair, _three_launch_act  # noqa: E402


@functools.lru_cache(maxsize=None)
def _alg(O, CO=None):
    torch.manual_seed(0)
    alg = PPO(ActorCritic(O, CO or O, A, HID, HID).cuda(), num_learning_epochs=1, num_mini_batches=1, device="cuda")
    alg.init_storage(64, 8, [O], [CO], [A])
    f = alg._fused
    assert f is not None and f.fused_fwd and f.wf is not None and (CO is not None or alg._rollout is not None)
    f.ensure_weights()
    return alg


def _per_layer(f, xp, idx, xa, y, out, K0s, M, shared):
    for l in range(4):
        last = l == 3
        gj = []
        for i in range(2):
            lin = f.lins[i][l]
            a = dict(af=xp[i], rows=idx, xa=xa[i] if (i == 0 or not shared) else None) if l == 0 else dict(A=y[i][l - 1])
            o = dict(cf=out[i]) if last else dict(cb=y[i][l])
            gj.append(dict(B=f.wb[i][l], M=M, N=lin.out_features, K=K0s[i] if l == 0 else lin.in_features,
                           bias=lin.bias.detach(), **a, **o))
        mfma_mlp._gemm(mfma_mlp.EPI_FWD_OUT if last else mfma_mlp.EPI_FWD_HIDDEN, gj)


def _forward_all_forms(f, Os, K0s, M, rows, shared, seed):
    """(xs, idx, {form: (xa, y, out)}) of the fused forward with and without fragment-packed weights
    and of the per-layer GEMMs, every output pre-filled with NaN."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    R = M + 64
    xs = [2.0 * torch.randn(R, Os[0], device="cuda", generator=g)]
    xs.append(xs[0] if shared else 2.0 * torch.randn(R, Os[1], device="cuda", generator=g))
    assert [x.stride(0) for x in xs] == list(Os)
    idx = torch.randperm(R, device="cuda", generator=g)[:M] if rows else None
    # the per-layer GEMM's fp32 operand needs a row stride that is a multiple of 4: it reads the
    # same rows from a copy with K0 columns (the fused forward reads the O-wide rows themselves)
    xp = []
    for x, O, K0 in zip(xs, Os, K0s):
        p = torch.zeros(R, K0, device="cuda")
        p[:, :O] = x
        xp.append(p)
    outs = {}
    for fused in ("frag", True, False):
        y = [[torch.full((M, lin.out_features), float("nan"), dtype=torch.bfloat16, device="cuda") for lin in ls[:-1]]
             for ls in f.lins]
        out = [torch.full((M, ls[-1].out_features), float("nan"), device="cuda") for ls in f.lins]
        xa = [torch.full((M, K0), float("nan"), dtype=torch.bfloat16, device="cuda") for K0 in K0s]
        if fused:
            mfma_mlp.mlp_forward([dict(x=xs[i], kx=Os[i], rows=idx, xa=xa[i] if (i == 0 or not shared) else None,
                                       K0=K0s[i], W=f.wb[i], Wf=f.wf[i] if fused == "frag" else None,
                                       b=[lin.bias.detach() for lin in f.lins[i]],
                                       N=[lin.out_features for lin in f.lins[i]], y=y[i], out=out[i])
                                  for i in range(2)], M)
        else:
            _per_layer(f, xp, idx, xa, y, out, K0s, M, shared)
        torch.cuda.synchronize()
        outs[fused] = (xa, y, out)
    return xs, idx, outs


def _assert_bitwise(xs, idx, outs, Os, M, shared):
    for form in ("frag", True):
        (xa1, y1, o1), (xa0, y0, o0) = outs[form], outs[False]
        for i in range(1 if shared else 2):
            src = xs[i][:M] if idx is None else xs[i][idx]
            assert torch.equal(xa1[i], xa0[i])
            assert torch.equal(xa1[i][:, :Os[i]], src.to(torch.bfloat16)) and not xa1[i][:, Os[i]:].float().abs().any()
        for i in range(2):
            for a, b in zip(y1[i], y0[i]):
                assert torch.equal(a, b)
            assert torch.equal(o1[i], o0[i]) and torch.isfinite(o1[i]).all()


# O = 427: row stride 427, read by element; 428: 16-byte loads up to column 424; both K0 = 448 (28
# k-steps: 7 groups, an odd count).  O = 300: K0 = 320 (5 groups, the narrowest).  O = 500: K0 = 512,
# the widest (8 groups, an even count).  M = 37 and 32 * 9: the 32-row form, ragged and whole;
# M = 18432 = 64 * 288: the 64-row form (x staged in the region y1 shares, gathered per job).
@pytest.mark.parametrize("O,K0", [(427, 448), (428, 448), (300, 320), (500, 512)])
@pytest.mark.parametrize("M,rows,shared", [(37, False, True), (288, True, False), (18432, True, True),
                                           (18432, False, False)])
def test_wider_fused_mlp_forward_is_bitwise_the_per_layer_gemms(O, K0, M, rows, shared):
    f = _alg(O)._fused
    assert f.k0p == [K0, K0] and mfma_mlp.mlp_forward_supported(f.lins[0], K0)
    xs, idx, outs = _forward_all_forms(f, (O, O), (K0, K0), M, rows, shared, M + O)
    _assert_bitwise(xs, idx, outs, (O, O), M, shared)
    # against fp32 torch on the same rows (bf16 GEMM rounding over 300 to 500 products: the error of
    # a sum of K rounded products grows as sqrt(K), so test_gpu_wide_mlp.py's 0.1 at K <= 256 is
    # 0.1 * sqrt(512 / 256) here)
    src = xs[0][:M] if idx is None else xs[0][idx]
    with torch.no_grad():
        mu = _alg(O).actor_critic.actor(src)
    torch.testing.assert_close(outs["frag"][2][0][:, :A], mu, rtol=0.05, atol=0.1 * 2 ** 0.5)


@pytest.mark.parametrize("M", [37, 18432])
def test_a_narrower_job_beside_a_wider_one_is_bitwise_too(M):
    """A 281-wide actor row (K0 = 320) beside a 237-wide critic row (K0 = 240: 15 k-steps, the general
    k-loop with its tail) in one launch of the wider forms."""
    f = _alg(281, 237)._fused
    assert f.k0p == [320, 240]
    xs, idx, outs = _forward_all_forms(f, (281, 237), (320, 240), M, True, False, M)
    _assert_bitwise(xs, idx, outs, (281, 237), M, False)


def test_widths_outside_both_classes_are_refused_with_a_text():
    f = _alg(300)._fused
    x = torch.zeros(64, 300, device="cuda")
    for K0, kx in ((272, 260), (528, 300), (576, 300), (432, 300)):
        y = [torch.zeros(32, lin.out_features, dtype=torch.bfloat16, device="cuda") for lin in f.lins[0][:-1]]
        out = torch.full((32, A), float("nan"), device="cuda")
        job = dict(x=x, kx=kx, K0=K0, W=f.wb[0], Wf=None, b=[lin.bias.detach() for lin in f.lins[0]],
                   N=[lin.out_features for lin in f.lins[0]], y=y, out=out)
        with pytest.raises(RuntimeError, match="K0 must be a multiple of 16, kx <= K0 <= 256, or a multiple of 64"):
            mfma_mlp.mlp_forward([job], 32)
        torch.cuda.synchronize()
        assert torch.isnan(out).all()  # nothing was launched
    lib = mfma_mlp.load()
    assert lib.pmlp_mlp_forward_ppo_loss_parts_k0(18432, 12, 448) == 288 * 15 == lib.pmlp_ppo_loss_step_parts(18432, 12)
    assert lib.pmlp_mlp_forward_ppo_loss_parts_k0(18432, 12, 240) == 192 * 15 == lib.pmlp_mlp_forward_ppo_loss_parts(18432, 12)
    assert lib.pmlp_mlp_forward_ppo_loss_parts_k0(18431, 12, 448) == 0


def test_rollout_forward_at_427_inputs_is_bitwise_the_three_launches():
    """pmlp_rollout_forward on go2_terrain_robust's 427-wide rows, 64 envs, with the previous step's
    deferred store and env extras (time-outs in the first step, so the extras' reset branch runs)."""
    T, n = 4, 64
    ac0 = copy.deepcopy(_alg(427).actor_critic)
    runs = []
    for three in (False, True):
        env = make("go2_terrain_robust", n, **MAP)
        assert env.num_obs == 427 and env.obs_history_params.enabled == 1 and env.actuator_rand.enabled == 1
        alg = PPO(copy.deepcopy(ac0), device="cuda")
        alg.init_storage(n, T, [427], [None], [A])
        ro = alg._rollout
        assert alg._fused.fused_fwd and alg._fused.k0p == [448, 448] and ro is not None
        ro.seed = 1234
        if three:
            ro.act = types.MethodType(_three_launch_act, ro)
        env.reset()
        env.episode_length_buf[:2] = int(env.max_episode_length)
        env.defer_extras = True
        obs = env.get_observations()
        with torch.inference_mode():
            for t in range(T):
                assert ro.usable(obs, obs, alg.storage)
                actions = alg.act(obs, obs)
                obs, _, rew, dones, infos = env.step(actions)
                assert "_deferred_extras" in infos
                alg.process_env_step(rew, dones, infos)
            alg.flush_rollout()
        env.defer_extras = False
        env.flush_extras()
        torch.cuda.synchronize()
        st = alg.storage
        runs.append(dict(obs=st.observations, actions=st.actions, logp=st.actions_log_prob, mu=st.mu, sigma=st.sigma,
                         values=st.values, rewards=st.rewards, dones=st.dones, ep_means=env._ep_means.clone(),
                         time_outs=env._time_outs.clone(), last_root_vel=env.last_root_vel.clone(),
                         counter=env._d_step_counter.clone(), draw=ro.draw.clone()))
        env.close()
    one, ref = runs
    assert one["obs"].shape == (T, n, 427) and one["dones"].any() and torch.isfinite(one["obs"]).all()
    assert one["obs"][:, :, 240:].abs().max() > 0  # the scan is in the stored rows
    for k in one:
        assert torch.equal(one[k], ref[k]), k


def test_fused_update_at_427_inputs_matches_the_fp32_autograd_update():
    """test_fused_update_at_235_inputs_matches_the_fp32_autograd_update at O = 427 with mini-batches
    of 18,432 rows: the 64-row forward with the loss in its launch (288 partial rows), the 448-wide
    first layer's weight gradient (masked tiles, slabs with the bias column), slab combine, staged
    copy (427 != 448), fragment mirror and scalar Adam on the odd 427 columns.  The bars are that
    test's."""
    O, N, T = 427, 2048, 18
    ac32, kw, _ = _pair(O, N, T, num_learning_epochs=1, num_mini_batches=2, schedule="adaptive")
    acbf = copy.deepcopy(ac32)
    acbf.mixed_precision = True
    ref = PPO(ac32, fused_loss=False, **kw)
    ref.use_graph = False
    fus = PPO(acbf, **kw)
    for alg in (ref, fus):
        alg.init_storage(N, T, [O], [None], [A])
    f = fus._fused
    assert f is not None and ref._fused is None and f.fused_fwd and f.fused_loss and f.M == 18432
    assert f.k0p == [448, 448] and f.dw_stage[0][0] is not None and f.loss_nb == 288
    data = _fill_storage(ref, T, N, O, A, seed=1)
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
    w = fus.actor_critic.actor[0].weight.detach()
    assert torch.equal(f.wb[0][0][:, :O], w.to(torch.bfloat16)) and not f.wb[0][0][:, O:].float().abs().any()
    assert torch.equal(f.wf[0][0], mfma_mlp.frag_pack(f.wb[0][0], 512))


def test_fused_update_graph_at_427_inputs_is_bitwise_eager():
    O, N, T = 427, 2048, 18
    ac, kw, _ = _pair(O, N, T, num_learning_epochs=2, num_mini_batches=2, schedule="adaptive")
    ac.mixed_precision = True
    algs = []
    for graph in (True, False):
        alg = PPO(copy.deepcopy(ac), **kw)
        alg.use_graph = graph
        alg.init_storage(N, T, [O], [None], [A])
        assert alg._fused.fused_fwd and alg._fused.fused_loss
        algs.append(alg)
    for u in range(3):
        data = _fill_storage(algs[1], T, N, O, A, seed=10 + u)
        for k, v in data.items():
            getattr(algs[0].storage, k).copy_(v)
        algs[0].storage.step = T
        torch.manual_seed(100 + u)
        lg = algs[0].update()
        torch.manual_seed(100 + u)
        le = algs[1].update()
        assert lg == le
        for a, b in zip(algs[0].actor_critic.parameters(), algs[1].actor_critic.parameters()):
            assert torch.equal(a, b)
    assert algs[0]._fgraph is not None and algs[1]._fgraph is None


def test_runner_trains_go2_terrain_robust_on_the_captured_path():
    """OnPolicyRunner on go2_terrain_robust, 64 envs, 2 iterations: the fused forward and the fused
    loss at 448 padded inputs and the one-launch rollout are on, the rollout graph is captured, and
    the replayed iteration is bitwise an eager runner's on the same seed.  64 envs reach the fused
    loss's 18,432-row mini-batch with one mini-batch of 288 steps per env."""
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (True, False):
        env = make("go2_terrain_robust", 64, env__episode_length_s=2.0, **MAP)  # (100 steps: episodes end)
        _, train_cfg = task_registry.get_cfgs("go2_terrain_robust")
        cfg = copy.deepcopy(class_to_dict(train_cfg))
        assert cfg["runner"]["experiment_name"] == "go2_terrain_robust"
        cfg["runner"]["rollout_graph"] = graph
        cfg["runner"]["num_steps_per_env"] = 288
        cfg["algorithm"]["num_mini_batches"] = 1
        cfg["algorithm"]["num_learning_epochs"] = 2
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        alg = runner.alg
        if not graph:
            alg.use_graph = False
        assert alg._fused is not None and alg._rollout is not None, "native PPO path not active"
        assert alg._fused.fused_fwd and alg._fused.fused_loss and alg._fused.k0p == [448, 448]
        assert not env._split_step and env.num_obs == 427 and env.actuator_rand.enabled == 1
        runner.learn(2)
        env.flush_extras()
        torch.cuda.synchronize()
        if graph:
            assert runner._rollout_graph is not None and not getattr(runner, "_rollout_graph_failed", False)
        else:
            assert runner._rollout_graph is None
        st = alg.storage
        out[graph] = dict(params=[p.detach().clone() for p in alg.actor_critic.parameters()],
                          storage=[t.clone() for t in (st.observations, st.actions, st.actions_log_prob, st.mu,
                                                       st.sigma, st.values, st.rewards, st.dones, st.returns,
                                                       st.advantages)],
                          obs=env.obs_buf.clone(), levels=env.terrain_levels.clone(),
                          hist=[env.obs_history.clone(), env._obs_history_fill.clone()])
        assert st.observations.shape == (288, 64, 427) and st.dones.any()
        assert all(torch.isfinite(t.float()).all() for t in out[graph]["storage"] + out[graph]["params"])
        # the stored rows: a step's four older frames are the previous step's four newest, except
        # where the env's episode ended in between; the scan is there and never part of the history
        o, d = st.observations, st.dones.reshape(288, -1).bool()
        same = (o[1:, :, :192] == o[:-1, :, 48:240]).all(dim=-1)
        assert same[~d[:-1]].all()
        assert o[:, :, 240:].abs().max() > 0
        assert torch.equal(env.obs_history, env.obs_buf[:, 48:240]) and (env._obs_history_fill == 1).all()
        env.close()
    for key in ("params", "storage", "hist"):
        for a, b in zip(out[True][key], out[False][key]):
            assert torch.equal(a, b), key
    assert torch.equal(out[True]["obs"], out[False]["obs"]) and torch.equal(out[True]["levels"], out[False]["levels"])
