"""Wide-input LSTM kernels (csrc/lstm_seq.hip, "wide inputs": hidden 64, 64 < I <= 384, the
observation row with the height scan): the input projection against fp64, the sequence
kernels against the torch recurrence, the rollout step against the dense forward, and the
fused recurrent update, the rollout and the runner on g1_terrain_scan's 234 / 237 rows."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCriticRecurrent  # noqa: E402
from rsl_rl.modules import lstm_seq  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from test_gpu_parity import make  # noqa: E402
from test_gpu_recurrent import _synthetic_storage  # noqa: E402
from test_gpu_terrain_curriculum import MAP  # noqa: E402

H = 64


def _weights(rnn):
    return [t.detach().contiguous() for t in (rnn.weight_ih_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, rnn.weight_hh_l0)]


def _fwd_job(rnn, x, h0, c0, T, B):
    """A forward job on fresh output buffers (kept alive in the returned dict)."""
    I = x.shape[-1]
    w = _weights(rnn)
    f = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    buf = dict(w=w, h_out=f(T, B, H), c_out=f(T, B, H), gact=f(T, B, 4 * H), gx=f(T, B, 4 * H), hp=f(T, B, H + 1))
    P = mm._p
    job = lstm_seq.LstmWideJob(I, P(x), P(w[0]), P(w[1]), P(w[2]), P(w[3]), P(h0), P(c0), P(buf["h_out"]),
                               P(buf["c_out"]), P(buf["gact"]), P(buf["gx"]), P(buf["hp"]))
    return job, buf


@pytest.mark.parametrize("M,I", [(37, 65), (37 * 5, 234), (37 * 5, 237), (21, 256), (50, 384)])
def test_wide_projection_matches_fp64(M, I):
    """gx = x W_ih^T + b_ih + b_hh (k_lstm_proj_wide, split-bf16: hi.hi + hi.lo + lo.hi, fp32
    accumulation from the fp32 bias) against the fp64 product.  Per element the omitted lo.lo
    term is <= 2^-16 sum|x||w| and K fp32 additions add <= K 2^-24 sum|x||w|: the bound is
    2^-15 sum_k |x_k||w_k| (a margin of 2 at K = 384).  Row strides of 65 / 237 floats (4-byte
    aligned rows), 234 (8-byte) and 256 / 384 (16-byte); M not a multiple of the 64-row tile,
    more than one workgroup at M = 185."""
    torch.manual_seed(M + I)
    rnn = torch.nn.LSTM(I, H).cuda()
    x = torch.randn(1, M, I, device="cuda")
    job, buf = _fwd_job(rnn, x, None, None, 1, M)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_fwd_wide_jobs(1, job, 1, M, H, None, mm._stream()), "fwd_wide")
    w_ih, b_ih, b_hh, _ = buf["w"]
    x64, w64 = x[0].double(), w_ih.double()
    want = x64 @ w64.t() + (b_ih + b_hh).double()
    bound = 2.0 ** -15 * (x64.abs() @ w64.abs().t())
    err = (buf["gx"][0].double() - want).abs()
    print(f"projection M={M} I={I}: max err / bound = {float((err / bound).max()):.3f}, max |err| = {float(err.max()):.3e}")
    assert bool(torch.isfinite(buf["gx"]).all())
    assert bool((err <= bound).all())


@pytest.mark.parametrize("T,B,I", [(1, 21, 256), (2, 16, 65), (3, 37, 237), (5, 37, 234), (24, 100, 384)])
def test_wide_lstm_kernels_match_torch_to_bf16(T, B, I):
    """The wide forward and all four parameter gradients (through lstm_dense's autograd
    Function) against the torch recurrence, resets inside the sequence (reset[0, :7] = 1) and a
    carried state; the bars are the narrow matrix-core kernels' own
    (test_lstm_mfma_kernels_match_torch_to_bf16): h within 1e-4 absolute and relative (norm),
    the gradients within 1e-3 relative (norm).  The shapes cover B not a multiple of the 16-env
    workgroups, the two-step gx prefetch at T = 1, 2 and 3, 4- / 8- / 16-byte aligned x rows
    and, at (24, 100, 384), several dW_ih row chunks and three column groups."""
    torch.manual_seed(T * 1000 + I)
    rnn = torch.nn.LSTM(I, H).cuda()
    x = torch.randn(T, B, I, device="cuda")
    h0 = 0.5 * torch.randn(1, B, H, device="cuda")
    c0 = 0.5 * torch.randn(1, B, H, device="cuda")
    reset = (torch.rand(T, B, device="cuda") < 0.1).to(torch.uint8)
    reset[0, :7] = 1
    assert lstm_seq.wide_usable(rnn, x)
    y = lstm_seq.lstm_dense(rnn, x, h0, c0, reset)
    y_ref = lstm_seq.lstm_dense_reference(rnn, x, h0, c0, reset)
    d = (y - y_ref).detach()
    err, rel = float(d.abs().max()), float(d.norm() / y_ref.detach().norm())
    print(f"wide lstm T={T} B={B} I={I}: max |dh| {err:.3e}, rel {rel:.3e}")
    assert err < 1e-4 and rel < 1e-4
    g = torch.randn_like(y)
    params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
    gk = torch.autograd.grad(y, params, g)
    gr = torch.autograd.grad(y_ref, params, g)
    for name, a, b in zip(("w_ih", "w_hh", "b_ih", "b_hh"), gk, gr):
        r = float((a - b).norm() / b.norm())
        print(f"wide lstm T={T} B={B} I={I}: grad {name} rel {r:.3e}")
        assert r < 1e-3, (name, r)


@pytest.mark.parametrize("T,B,I", [(3, 37, 237), (24, 100, 384)])
def test_wide_bwd_slabs_sum_to_the_weight_gradients(T, B, I):
    """pmlp_lstm_bwd_wide_jobs, both jobs in one launch (the second on another input width): the
    slab rows [dW_hh | db] and the dW_ih row-chunk partials, summed, are torch autograd's
    gradients through the same recurrence within 1e-4 relative (norm), as the narrow form's
    (test_lstm_bwd_accumulates_the_weight_gradients); dgx is the bias gradient's summand; hp is
    [h_prev | 1]."""
    torch.manual_seed(I + T)
    L, P, st = lstm_seq._lib(), mm._p, mm._stream()
    Is = (I, 65 + (I % 7))
    rnns = [torch.nn.LSTM(i, H).cuda() for i in Is]
    xs = [torch.randn(T, B, i, device="cuda") for i in Is]
    h0 = [0.5 * torch.randn(B, H, device="cuda") for _ in Is]
    c0 = [0.5 * torch.randn(B, H, device="cuda") for _ in Is]
    reset = (torch.rand(T, B, device="cuda") < 0.1).to(torch.uint8)
    gs = [torch.randn(T, B, H, device="cuda") for _ in Is]
    made = [_fwd_job(rnns[n], xs[n], h0[n], c0[n], T, B) for n in range(2)]
    jobs = (lstm_seq.LstmWideJob * 2)(*[m[0] for m in made])
    lstm_seq._ok(L.pmlp_lstm_fwd_wide_jobs(2, jobs, T, B, H, P(reset), st), "fwd_wide")
    nb, nbi = L.pmlp_lstm_bwd_dw_blocks(B), L.pmlp_lstm_wide_dw_blocks(T, B)
    assert nbi == (T * B + 511) // 512
    outs = []
    for n in range(2):
        o = dict(dgx=torch.full((T, B, 4 * H), float("nan"), device="cuda"),
                 slab=torch.full((nb, 4 * H * (H + 1)), float("nan"), device="cuda"),
                 slab_ih=torch.full((nbi, 4 * H * Is[n]), float("nan"), device="cuda"))
        jobs[n].dh_out, jobs[n].dgx, jobs[n].slab, jobs[n].slab_ih = P(gs[n]), P(o["dgx"]), P(o["slab"]), P(o["slab_ih"])
        outs.append(o)
    lstm_seq._ok(L.pmlp_lstm_bwd_wide_jobs(2, jobs, T, B, H, P(reset), st), "bwd_wide")
    for n in range(2):
        rnn, buf, o = rnns[n], made[n][1], outs[n]
        y_ref = lstm_seq.lstm_dense_reference(rnn, xs[n], h0[n], c0[n], reset)
        hp = torch.cat([h0[n].unsqueeze(0), buf["h_out"][:-1]]) * (reset == 0).float().unsqueeze(-1)
        assert torch.equal(buf["hp"][..., :H], hp) and bool((buf["hp"][..., H] == 1).all())
        tot = o["slab"].sum(0)
        got = [o["slab_ih"].sum(0).view(4 * H, Is[n]), tot[:4 * H * H].view(4 * H, H), tot[4 * H * H:]]
        want = torch.autograd.grad(y_ref, [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0], gs[n])
        for name, a, b in zip(("w_ih", "w_hh", "b"), got, want):
            r = float((a - b).norm() / b.norm())
            print(f"wide slabs T={T} B={B} I={Is[n]}: {name} rel {r:.3e}")
            assert r < 1e-4, (name, r)
        r = float((o["dgx"].sum((0, 1)) - want[2]).norm() / want[2].norm())
        assert r < 1e-4, ("dgx", r)


def test_wide_step_is_bitwise_the_dense_forward_at_one_step():
    """pmlp_lstm_step_wide_jobs (both memories per launch, 234 / 237 inputs, B = 37): over three
    steps h, c are updated in place, h_save / c_save receive the state the step started from,
    and the new state is bit for bit the dense forward's h_out[0] / c_out[0] from that state."""
    torch.manual_seed(7)
    B, Is = 37, (234, 237)
    L, P, st = lstm_seq._lib(), mm._p, mm._stream()
    rnns = [torch.nn.LSTM(i, H).cuda() for i in Is]
    h = [0.5 * torch.randn(1, B, H, device="cuda") for _ in Is]
    c = [0.5 * torch.randn(1, B, H, device="cuda") for _ in Is]
    hs = [torch.empty(1, B, H, device="cuda") for _ in Is]
    cs = [torch.empty(1, B, H, device="cuda") for _ in Is]
    gx = [torch.empty(B, 4 * H, device="cuda") for _ in Is]
    for _ in range(3):
        xs = [torch.randn(B, i, device="cuda") for i in Is]
        h_in, c_in = [t.clone() for t in h], [t.clone() for t in c]
        dense = []
        for n in range(2):
            job, buf = _fwd_job(rnns[n], xs[n], h_in[n], c_in[n], 1, B)
            lstm_seq._ok(L.pmlp_lstm_fwd_wide_jobs(1, job, 1, B, H, None, st), "fwd_wide")
            dense.append(buf)
        ptrs = [t.data_ptr() for t in h]
        out = lstm_seq.lstm_step_wide_pair_([(rnns[n], xs[n], h[n], c[n], (hs[n], cs[n]), gx[n]) for n in range(2)])
        for n in range(2):
            assert out[n].data_ptr() == ptrs[n]
            assert torch.equal(hs[n], h_in[n]) and torch.equal(cs[n], c_in[n])
            assert torch.equal(h[n][0], dense[n]["h_out"][0]) and torch.equal(c[n][0], dense[n]["c_out"][0])
            assert bool((h[n] != h_in[n]).any())


@pytest.mark.skipif("PMLP_LSTM_STEP_TILES" in os.environ, reason="the tile count under test is overridden")
@pytest.mark.parametrize("B", [4117, 8213])
def test_wide_step_tile_loop_is_bitwise_the_one_tile_forward(B):
    """The sequence kernel's tile loop with a ragged last tile, gx-fed form (234 / 237 inputs side
    by side): B = 4117 is 2 tiles per workgroup, the last workgroup's second tile with 5 live
    envs; B = 8213 is 4, the last workgroup running one full tile, one with 5 live envs, then
    leaving the loop.  One in-place step (pmlp_lstm_step_wide_jobs with h_save / c_save) leaves
    h, c bit for bit h_out[0] / c_out[0] of the dense forward (pmlp_lstm_fwd_wide_jobs at T = 1:
    one tile per workgroup) from the same state, and saves the state it started from."""
    torch.manual_seed(B)
    Is = (234, 237)
    L, st = lstm_seq._lib(), mm._stream()
    rnns = [torch.nn.LSTM(i, H).cuda() for i in Is]
    xs = [torch.randn(B, i, device="cuda") for i in Is]
    h = [0.5 * torch.randn(1, B, H, device="cuda") for _ in Is]
    c = [0.5 * torch.randn(1, B, H, device="cuda") for _ in Is]
    h_in, c_in = [t.clone() for t in h], [t.clone() for t in c]
    hs = [torch.full((1, B, H), float("nan"), device="cuda") for _ in Is]
    cs = [torch.full((1, B, H), float("nan"), device="cuda") for _ in Is]
    gx = [torch.empty(B, 4 * H, device="cuda") for _ in Is]
    made = [_fwd_job(rnns[n], xs[n], h_in[n], c_in[n], 1, B) for n in range(2)]
    jobs = (lstm_seq.LstmWideJob * 2)(*[m[0] for m in made])
    lstm_seq._ok(L.pmlp_lstm_fwd_wide_jobs(2, jobs, 1, B, H, None, st), "fwd_wide")
    lstm_seq.lstm_step_wide_pair_([(rnns[n], xs[n], h[n], c[n], (hs[n], cs[n]), gx[n]) for n in range(2)])
    for n in range(2):
        dense = made[n][1]
        assert torch.equal(hs[n], h_in[n]) and torch.equal(cs[n], c_in[n])
        assert bool(torch.isfinite(dense["h_out"]).all()) and bool((h[n] != h_in[n]).any())
        assert torch.equal(h[n][0], dense["h_out"][0]) and torch.equal(c[n][0], dense["c_out"][0])


O, P, A = 234, 237, 12  # g1_terrain_scan's rows: 47 / 50 + the 187-point height scan
KW = dict(actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_type="lstm", rnn_hidden_size=H, rnn_num_layers=1,
          init_noise_std=0.8)


def test_wide_recurrent_ppo_update_matches_fp32_cpu_update():
    """One PPO update (5 epochs x 4 mini-batches, adaptive LR) of the 234 / 237-input recurrent
    policy (64 envs, T = 5) on the fused recurrent step with both memories on the wide
    matrix-core kernels, against the same update on the CPU in fp32 with rsl_rl's padded
    trajectories and torch's LSTM; the bars of test_recurrent_ppo_update_matches_fp32_cpu_update."""
    T, N = 5, 64
    torch.manual_seed(0)
    ac_cpu = ActorCriticRecurrent(O, P, A, **KW)
    ac_gpu = copy.deepcopy(ac_cpu).cuda()
    akw = dict(num_learning_epochs=5, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", gamma=0.99,
               lam=0.95, entropy_coef=0.01)
    cpu = PPO(ac_cpu, device="cpu", **akw)
    cpu._dense_recurrent = False  # rsl_rl's own padded-trajectory generator
    gpu = PPO(ac_gpu, device="cuda", **akw)
    for alg in (cpu, gpu):
        alg.init_storage(N, T, [O], [P], [A])
    rf = gpu._rfused
    assert rf is not None and all(rf.mfma) and all(rf.wide)
    last = _synthetic_storage(cpu, T, N, O, P, A, H, seed=1)
    _synthetic_storage(gpu, T, N, O, P, A, H, seed=1)
    cpu.compute_returns(last)
    gpu.compute_returns(last.cuda())
    p0 = [p.detach().clone() for p in ac_cpu.parameters()]
    l_cpu = cpu.update()
    l_gpu = gpu.update()  # eager (first call)
    print("wide update losses gpu", l_gpu, "cpu", l_cpu)
    np.testing.assert_allclose(l_gpu, l_cpu, rtol=1e-3, atol=1e-5)
    assert gpu.learning_rate == pytest.approx(cpu.learning_rate, rel=1e-6)
    lr = 1e-3
    for (name, a), b, c in zip(ac_cpu.named_parameters(), ac_gpu.parameters(), p0):
        da, db = a.detach() - c, b.detach().cpu() - c
        assert da.abs().max() > 0, name
        nbad = int(((da - db).abs() > 0.1 * lr).sum())
        print(f"wide update {name}: {nbad} / {da.numel()} entries off by > 0.1 lr, max {float((da - db).abs().max()):.2e}")
        assert nbad <= max(1, 0.02 * da.numel()), (name, nbad, da.numel())
        assert (da - db).abs().max() <= 2 * 20 * 1.5 * lr, name


@pytest.mark.parametrize("obs", [O, 47])
def test_wide_recurrent_update_graph_matches_eager(obs):
    """The captured fused recurrent update on wide memories replays the eager update (as
    test_recurrent_update_graph_matches_eager); obs = 47: a narrow actor memory next to the
    wide critic memory, each on its own form."""
    T, N = 5, 64
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(obs, P, A, **KW).cuda()
    alg = PPO(ac, device="cuda", num_learning_epochs=2, num_mini_batches=4, learning_rate=3e-4, schedule="fixed")
    alg.init_storage(N, T, [obs], [P], [A])
    assert alg._rfused is not None and all(alg._rfused.mfma) and alg._rfused.wide == [obs > 64, True]
    last = _synthetic_storage(alg, T, N, obs, P, A, H, seed=2).cuda()
    alg.compute_returns(last)
    alg.update()  # eager warm-up
    assert alg._rgraph is None
    saved = {k: v.clone() for k, v in alg.storage.__dict__.items() if torch.is_tensor(v) and not k.startswith("_")}
    params = list(ac.parameters())
    p0 = [p.detach().clone() for p in params]
    st0 = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in alg.optimizer.state[p].items()}
           for p in params}
    alg.storage.step = T
    g_loss = alg.update()  # captured + replayed
    assert alg._rgraph is not None
    p_graph = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, v in zip(params, p0):
            p.copy_(v)
        for p in params:
            for k, v in alg.optimizer.state[p].items():
                if torch.is_tensor(v):
                    v.copy_(st0[id(p)][k])
        for k, v in saved.items():
            getattr(alg.storage, k).copy_(v)
    alg.storage.step = T
    alg.use_graph = False
    e_loss = alg.update()
    np.testing.assert_allclose(g_loss, e_loss, rtol=1e-5, atol=1e-7)
    for a, b, c in zip(params, p_graph, p0):
        assert bool((b != c).any())
        assert (a.detach() - b).abs().max() <= 8 * 3e-4


def test_wide_recurrent_rollout_steps_on_the_update_arithmetic():
    """RecurrentRollout on 234 / 237 rows (200 envs): the memories step on the wide kernels
    (mfma_step), so the new state is bit for bit the update's dense forward from the saved
    state; the stored action means and values are the torch heads on that state within 1e-5
    (test_recurrent_rollout_heads_kernel_matches_torch_heads), and pmlp_heads_forward_act
    copies the 234 / 237-wide rows into the storage."""
    torch.manual_seed(3)
    N, T = 200, 3
    ac = ActorCriticRecurrent(O, P, A, **KW).cuda()
    alg = PPO(ac, device="cuda", num_learning_epochs=1, num_mini_batches=1)
    alg.init_storage(N, T, [O], [P], [A])
    ro, st = alg._rollout, alg.storage
    assert ro is not None and ro.heads is not None and ro.mfma_step and ro.wide == [True, True]
    for t in range(T):
        obs, cobs = torch.randn(N, O, device="cuda"), torch.randn(N, P, device="cuda")
        with torch.inference_mode():
            alg.act(obs, cobs)
            ha, hc = ac.memory_a.hidden_states[0][0], ac.memory_c.hidden_states[0][0]
            mu, value = ac.actor(ha), ac.critic(hc)
            for mem, x, saved, h in ((ac.memory_a, obs, st.saved_hidden_states_a, ha),
                                     (ac.memory_c, cobs, st.saved_hidden_states_c, hc)):
                dense = lstm_seq.lstm_dense(mem.rnn, x.unsqueeze(0), saved[0][t], saved[1][t], None)
                assert torch.equal(dense[0], h)
            alg.process_env_step(torch.zeros(N, device="cuda"), torch.rand(N, device="cuda") < 0.2,
                                 {"time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
        torch.testing.assert_close(st.mu[t], mu, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(st.values[t], value, rtol=1e-5, atol=1e-5)
        assert torch.equal(st.observations[t], obs) and torch.equal(st.privileged_observations[t], cobs)


def test_runner_trains_g1_terrain_scan_on_the_captured_path():
    """OnPolicyRunner on g1_terrain_scan, 64 envs on the small map, 3 iterations: the fused
    recurrent step and the matrix-core rollout step are on at 234 / 237 inputs, and the captured
    collection loop replays the eager loop's rollouts bit for bit (the fields of
    test_recurrent_rollout_graph_matches_eager)."""
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (False, True):
        env = make("g1_terrain_scan", 64, **MAP)
        _, train_cfg = task_registry.get_cfgs("g1_terrain_scan")
        cfg = class_to_dict(train_cfg)
        assert cfg["runner"]["experiment_name"] == "g1_terrain_scan"
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        alg = runner.alg
        assert (env.num_obs, env.num_privileged_obs) == (O, P)
        assert alg._rfused is not None and all(alg._rfused.mfma) and alg._rollout.mfma_step
        alg.use_graph = False  # compare the rollouts, not the update paths
        runner.learn(3, init_at_random_ep_len=True)
        env.flush_extras()
        torch.cuda.synchronize()
        st = alg.storage
        assert st.observations.shape[2] == O and st.privileged_observations.shape[2] == P
        out[graph] = dict(root=env.root_states.clone(), st_obs=st.observations.clone(), st_act=st.actions.clone(),
                          st_rew=st.rewards.clone(), hid=st.saved_hidden_states_a[0].clone(),
                          mem=alg.actor_critic.memory_a.hidden_states[0].clone(),
                          params=[p.detach().clone() for p in alg.actor_critic.parameters()],
                          captured=runner._rollout_graph is not None)
        assert all(bool(torch.isfinite(v).all()) for v in out[graph]["params"])
        env.close()
    e, g = out[False], out[True]
    assert g["captured"] and not e["captured"]
    for k in ("root", "st_obs", "st_act", "st_rew", "hid", "mem"):
        assert torch.equal(e[k], g[k]), k
    for a, b in zip(e["params"], g["params"]):
        assert torch.equal(a, b)
