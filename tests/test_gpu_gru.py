"""ActorCriticRecurrent(rnn_type="gru") on the GPU: the GRU sequence kernels (csrc/gru_seq.hip)
against the dense statement in torch fp32 ops (rsl_rl/modules/gru_seq.py), the in-place step
against the dense forward, the PPO wiring (dense update, captured update, captured rollout)
and train.py / play.py on g1_gru."""
import copy
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCriticRecurrent  # noqa: E402
from rsl_rl.modules import gru_seq  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

H = 64
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _resets(T, B):
    """10 % random, plus: reset[0, :3] discards h0, one reset at T - 1, one env reset on two
    consecutive steps."""
    reset = (torch.rand(T, B, device="cuda") < 0.1).to(torch.uint8)
    reset[0, :3] = 1
    reset[T - 1, B // 2] = 1
    if T >= 2:
        t2 = min(3, T - 2)
        reset[t2:t2 + 2, B - 1] = 1
    return reset


def _rel(a, b):
    """|a - b| / |b|; where the reference is exactly zero (no state ever reaches W_hh), so is a."""
    nb = float(b.norm())
    return float((a - b).norm()) / nb if nb > 0 else float(a.norm())


def _check(rnn, x, h0, reset, what):
    y = gru_seq.gru_dense(rnn, x, h0, reset)
    y_ref = gru_seq.gru_dense_reference(rnn, x, h0, reset)
    err, rel = float((y - y_ref).abs().max()), _rel(y, y_ref)
    print(f"gru {what}: max |dh| {err:.3g} rel {rel:.3g}")
    g = torch.randn_like(y)
    params = [getattr(rnn, n) for n in PARAMS]
    gk = torch.autograd.grad(y, params, g)
    gr = torch.autograd.grad(y_ref, params, g)
    rels = {n: _rel(a, b) for n, a, b in zip(PARAMS, gk, gr)}
    print(f"gru {what}: grad rel", {n: f"{v:.3g}" for n, v in rels.items()})
    assert err < 1e-4 and rel < 1e-4
    for n, v in rels.items():
        assert v < 1e-3, (n, v)


@pytest.mark.parametrize("T,B", [(1, 1), (2, 16), (7, 37)])
@pytest.mark.parametrize("I", [17, 47, 64])
def test_gru_kernels_match_reference(I, T, B):
    """Forward outputs and the four parameter gradients of the dense GRU (pmlp_gru_fwd_jobs /
    pmlp_gru_bwd_jobs: split-bf16 products, fp32 accumulation and state) against the same
    recurrence in torch fp32 ops, with resets inside and a carried state.  B = 37: three tiles,
    the last with 5 envs; I = 17: no multiple of 4.  The bounds are those of
    test_lstm_mfma_kernels_match_torch_to_bf16; a CPU emulation of the split product with exact
    activations gives 9.6e-6 / 6.1e-6."""
    torch.manual_seed(1000 * I + 10 * T + B)
    rnn = torch.nn.GRU(I, H).cuda()
    x = torch.randn(T, B, I, device="cuda")
    h0 = 0.5 * torch.randn(1, B, H, device="cuda")
    _check(rnn, x, h0, _resets(T, B), f"I={I} T={T} B={B}")


@pytest.mark.parametrize("case", ["hn_zero", "hn_alone", "hn_alone_no_input_part"])
def test_gru_keeps_the_hidden_part_of_n_inside_r(case):
    """The n gate's hidden part W_hn h + b_hn is multiplied by r, its input part is not: with
    W_hn and b_hn zero, and with them the only nonzero hidden-side parameters (and then also
    without the n gate's input part), the kernels still match the reference."""
    torch.manual_seed(7)
    T, B, I = 7, 37, 47
    rnn = torch.nn.GRU(I, H).cuda()
    with torch.no_grad():
        if case == "hn_zero":
            rnn.weight_hh_l0[2 * H:].zero_()
            rnn.bias_hh_l0[2 * H:].zero_()
        else:
            rnn.weight_hh_l0[:2 * H].zero_()
            rnn.bias_hh_l0[:2 * H].zero_()
            rnn.bias_hh_l0[2 * H:].add_(0.5)  # a b_hn that matters
            if case == "hn_alone_no_input_part":
                rnn.weight_ih_l0[2 * H:].zero_()
                rnn.bias_ih_l0[2 * H:].zero_()
    x = torch.randn(T, B, I, device="cuda")
    h0 = 0.5 * torch.randn(1, B, H, device="cuda")
    reset = _resets(T, B)
    y = gru_seq.gru_dense(rnn, x, h0, reset)
    y_ref = gru_seq.gru_dense_reference(rnn, x, h0, reset)
    # were b_hn outside r * (.), n would move by b_hn (1 - r), far more than the bound
    err = float((y - y_ref).abs().max())
    print("gru", case, "max |dh|", err)
    assert err < 1e-4 and _rel(y, y_ref) < 1e-4
    if case != "hn_zero":
        _check(rnn, x, h0, reset, case)


def test_gru_forward_saves_the_backward_operands():
    """gact = [r | z | n | gh_n] and xh = [x | h_prev | 1], h_prev the state each step starts
    from (h0 at t = 0, zero after a reset, else the previous output, in fp32)."""
    torch.manual_seed(1)
    T, B, I = 6, 37, 41
    rnn = torch.nn.GRU(I, H).cuda()
    x = torch.randn(T, B, I, device="cuda")
    h0 = torch.randn(B, H, device="cuda")
    reset = (torch.rand(T, B, device="cuda") < 0.3).to(torch.uint8)
    f = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    h_out, gact, xh = f(T, B, H), f(T, B, 4 * H), f(T, B, I + H + 1)
    p = mm._p
    job = gru_seq.GruJob(I, p(x), p(rnn.weight_ih_l0), p(rnn.bias_ih_l0), p(rnn.bias_hh_l0), p(rnn.weight_hh_l0),
                         p(h0), p(h_out), p(gact), p(xh))
    gru_seq._ok(gru_seq._lib().pmlp_gru_fwd_jobs(1, C.byref(job), T, B, H, p(reset), mm._stream()), "fwd")
    torch.cuda.synchronize()
    hp = torch.cat([h0.unsqueeze(0), h_out[:-1]]) * (reset == 0).float().unsqueeze(-1)
    assert torch.equal(xh[..., :I], x)
    assert torch.equal(xh[..., I:I + H], hp)
    assert bool((xh[..., I + H] == 1).all())
    r, z, n, ghn = gact.split(H, dim=-1)
    with torch.no_grad():
        ghn_ref = torch.nn.functional.linear(hp, rnn.weight_hh_l0[2 * H:], rnn.bias_hh_l0[2 * H:])
    assert float((ghn - ghn_ref).abs().max()) < 1e-4
    torch.testing.assert_close(h_out, (1 - z) * n + z * hp, rtol=1e-6, atol=1e-6)
    assert bool(((r > 0) & (r < 1) & (z > 0) & (z < 1) & (n.abs() <= 1)).all())


@pytest.mark.skipif("PMLP_LSTM_STEP_TILES" in os.environ, reason="the tile count under test is overridden")
@pytest.mark.parametrize("B", [37, 4117])
def test_gru_step_is_the_dense_forward_in_place(B):
    """gru_step_pair_ (pmlp_gru_step_jobs): B = 37 is one tile per workgroup with a ragged last
    one; B = 4117 is 2 tiles per workgroup, the last workgroup's second tile with 5 live envs.
    The step leaves h bit for bit the dense forward's h_out[0] from the same state, within
    2e-5 of nn.GRU (the LSTM step's bound), in place, and saves the state it started from."""
    torch.manual_seed(B)
    I = 47
    rnn = torch.nn.GRU(I, H).cuda()
    x = torch.randn(B, I, device="cuda")
    h = 0.5 * torch.randn(1, B, H, device="cuda")
    h_in = h.clone()
    save = torch.full((1, B, H), float("nan"), device="cuda")
    with torch.no_grad():
        y_dense = gru_seq.gru_dense(rnn, x.unsqueeze(0), h_in, None)
        y_ref, h_ref = rnn(x.unsqueeze(0), h_in)
    ptr = h.data_ptr()
    out, = gru_seq.gru_step_pair_([(rnn, x, h, save)])
    assert out.data_ptr() == ptr and h.data_ptr() == ptr
    assert torch.equal(save, h_in)
    assert bool((h != h_in).any())
    assert torch.equal(h, y_dense)
    torch.testing.assert_close(h, h_ref, rtol=2e-5, atol=2e-5)


def _fwd_jobs(rnns, xs, h0s, reset):
    """pmlp_gru_fwd_jobs on len(rnns) memories in one launch -> [(h_out, gact, xh)]."""
    T, B = xs[0].shape[:2]
    p = mm._p
    f = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    outs = [(f(T, B, H), f(T, B, 4 * H), f(T, B, x.shape[2] + H + 1)) for x in xs]
    jobs = (gru_seq.GruJob * len(rnns))()
    for n, (rnn, x, h0, o) in enumerate(zip(rnns, xs, h0s, outs)):
        jobs[n] = gru_seq.GruJob(x.shape[2], p(x), p(rnn.weight_ih_l0), p(rnn.bias_ih_l0), p(rnn.bias_hh_l0),
                                 p(rnn.weight_hh_l0), p(h0), p(o[0]), p(o[1]), p(o[2]))
    gru_seq._ok(gru_seq._lib().pmlp_gru_fwd_jobs(len(rnns), jobs, T, B, H, p(reset), mm._stream()), "fwd")
    torch.cuda.synchronize()
    return outs


def test_gru_two_jobs_are_bitwise_two_launches():
    """Forward, backward and step of two memories (I = 47 and 50) in one launch each equal the
    one-job launches bit for bit."""
    torch.manual_seed(11)
    T, B = 7, 37
    rnns = [torch.nn.GRU(I, H).cuda() for I in (47, 50)]
    xs = [torch.randn(T, B, r.input_size, device="cuda") for r in rnns]
    h0s = [0.5 * torch.randn(B, H, device="cuda") for _ in rnns]
    reset = _resets(T, B)
    pair = _fwd_jobs(rnns, xs, h0s, reset)
    single = [_fwd_jobs([r], [x], [h], reset)[0] for r, x, h in zip(rnns, xs, h0s)]
    for a, b in zip(pair, single):
        for u, v in zip(a, b):
            assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
    # backward
    p, L = mm._p, gru_seq._lib()
    dh = [torch.randn(T, B, H, device="cuda") for _ in rnns]

    def bwd(idx):
        dgs = [torch.full((T, B, 4 * H), float("nan"), device="cuda") for _ in idx]
        jobs = (gru_seq.GruJob * len(idx))()
        for n, i in enumerate(idx):
            jobs[n] = gru_seq.GruJob(rnns[i].input_size, None, None, None, None, p(rnns[i].weight_hh_l0), None, None,
                                     p(pair[i][1]), p(pair[i][2]), p(dh[i]), p(dgs[n]))
        gru_seq._ok(L.pmlp_gru_bwd_jobs(len(idx), jobs, T, B, H, p(reset), mm._stream()), "bwd")
        torch.cuda.synchronize()
        return dgs

    both = bwd([0, 1])
    for i in (0, 1):
        one, = bwd([i])
        assert bool(torch.isfinite(one).all()) and torch.equal(both[i], one)
    # step
    x1 = [x[0].contiguous() for x in xs]
    hp = [h.clone().view(1, B, H) for h in h0s]
    hs = [h.clone().view(1, B, H) for h in h0s]
    sp = [torch.empty(1, B, H, device="cuda") for _ in rnns]
    gru_seq.gru_step_pair_([(r, x, h, s) for r, x, h, s in zip(rnns, x1, hp, sp)])
    for r, x, h, h0, s in zip(rnns, x1, hs, h0s, sp):
        gru_seq.gru_step_pair_([(r, x, h, None)])
        assert torch.equal(s.view(B, H), h0)
    for a, b in zip(hp, hs):
        assert torch.equal(a, b)


KW = dict(actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_type="gru", rnn_hidden_size=H, rnn_num_layers=1,
          init_noise_std=0.8)


def test_gru_policy_takes_the_dense_captured_path():
    O, P, A = 47, 50, 12
    ac = ActorCriticRecurrent(O, P, A, **KW).cuda()
    alg = PPO(ac, device="cuda", num_learning_epochs=1, num_mini_batches=2)
    alg.init_storage(64, 4, [O], [P], [A])
    assert alg._dense_recurrent and alg.use_graph and ac.rollout_capturable() and alg._rollout is not None
    assert alg._rfused is None  # the fused recurrent step stays LSTM-only
    assert alg._rollout.heads is not None  # the heads' launch takes a GRU's output too


@pytest.mark.parametrize("kw", [dict(rnn_hidden_size=128), dict(rnn_num_layers=2)])
def test_other_gru_shapes_keep_the_padded_path(kw):
    """Hidden 128 and two layers: none of the GRU kernels' paths, and one update() still
    completes on rsl_rl's padded generator."""
    torch.manual_seed(0)
    O, P, A, N, T = 47, 50, 12, 64, 6
    ac = ActorCriticRecurrent(O, P, A, **{**KW, **kw}).cuda()
    alg = PPO(ac, device="cuda", num_learning_epochs=1, num_mini_batches=2)
    alg.init_storage(N, T, [O], [P], [A])
    assert not alg._dense_recurrent and not alg.use_graph and not ac.rollout_capturable()
    assert alg._rollout is None or not alg._rollout.usable(torch.zeros(N, O, device="cuda"),
                                                            torch.zeros(N, P, device="cuda"), alg.storage)
    p0 = [p.detach().clone() for p in ac.parameters()]
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.inference_mode():
        for t in range(T):
            obs, cobs = torch.randn(N, O, device="cuda", generator=g), torch.randn(N, P, device="cuda", generator=g)
            alg.act(obs, cobs)
            alg.process_env_step(torch.randn(N, device="cuda", generator=g),
                                 torch.rand(N, device="cuda", generator=g) < 0.2,
                                 {"time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
        alg.compute_returns(cobs)
    vl, sl = alg.update()
    assert np.isfinite(vl) and np.isfinite(sl)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(ac.parameters(), p0))


def _synthetic_storage(alg, T, N, O, P, A, seed):
    """tests/test_gpu_recurrent.py's recipe with one state tensor per memory: a rollout with
    dones and the saved hidden states of a real recurrent rollout (the state at t = 0 is
    carried; after a done it is zero)."""
    g = torch.Generator().manual_seed(seed)
    st = alg.storage
    st.observations.copy_(torch.randn(T, N, O, generator=g))
    st.privileged_observations.copy_(torch.randn(T, N, P, generator=g))
    mu = 0.3 * torch.randn(T, N, A, generator=g)
    sigma = 0.8 * (1 + 0.1 * torch.rand(T, N, A, generator=g))
    act = mu + sigma * torch.randn(T, N, A, generator=g)
    st.mu.copy_(mu)
    st.sigma.copy_(sigma)
    st.actions.copy_(act)
    st.actions_log_prob.copy_(torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True))
    st.values.copy_(0.5 * torch.randn(T, N, 1, generator=g))
    st.rewards.copy_(0.2 * torch.randn(T, N, 1, generator=g))
    dones = (torch.rand(T, N, 1, generator=g) < 0.04)
    st.dones.copy_(dones.to(st.dones.dtype))
    s = 0.5 * torch.randn(T, 1, N, H, generator=g)
    s[1:] *= (~dones[:-1, :, 0]).float().view(T - 1, 1, N, 1)
    dev = st.observations.device
    st.saved_hidden_states_a = [s.to(dev)]
    st.saved_hidden_states_c = [(0.7 * s).to(dev)]
    st.step = T
    return torch.randn(N, P, generator=g)


def test_gru_update_graph_matches_eager():
    """test_recurrent_update_graph_matches_eager for the GRU policy: the captured update (dense
    generator, GRU kernels through autograd, capturable Adam) replays the eager one."""
    T, N, O, P, A = 8, 64, 47, 50, 12
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(O, P, A, **KW).cuda()
    alg = PPO(ac, device="cuda", num_learning_epochs=2, num_mini_batches=4, learning_rate=3e-4, schedule="fixed")
    alg.init_storage(N, T, [O], [P], [A])
    last = _synthetic_storage(alg, T, N, O, P, A, seed=2).cuda()
    alg.compute_returns(last)
    alg.update()  # eager warm-up
    assert alg._rfused is None and alg._graph is None
    saved = {k: v.clone() for k, v in alg.storage.__dict__.items() if torch.is_tensor(v) and not k.startswith("_")}
    params = list(ac.parameters())
    p0 = [p.detach().clone() for p in params]
    st0 = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in alg.optimizer.state[p].items()}
           for p in params}
    alg.storage.step = T
    g_loss = alg.update()  # captured + replayed
    assert alg._graph is not None
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
    assert any(not torch.equal(a.detach(), b) for a, b in zip(params, p0))
    for a, b in zip(params, p_graph):
        assert (a.detach() - b).abs().max() <= 8 * 3e-4


def test_gru_dense_loss_on_the_gpu_matches_the_padded_loss_on_the_cpu():
    """One mini-batch's _reference_loss and parameter gradients: the GPU dense form (GRU
    kernels) against the CPU padded form (torch's nn.GRU on split trajectories), fp32."""
    T, N, O, P, A = 8, 64, 47, 50, 12
    torch.manual_seed(0)
    ac_cpu = ActorCriticRecurrent(O, P, A, **KW)
    ac_gpu = copy.deepcopy(ac_cpu).cuda()
    cpu = PPO(ac_cpu, device="cpu", num_mini_batches=4)
    gpu = PPO(ac_gpu, device="cuda", num_mini_batches=4)
    assert gpu._dense_recurrent and not cpu._dense_recurrent
    for alg in (cpu, gpu):
        alg.init_storage(N, T, [O], [P], [A])
    last = _synthetic_storage(cpu, T, N, O, P, A, seed=1)
    _synthetic_storage(gpu, T, N, O, P, A, seed=1)
    cpu.compute_returns(last)
    gpu.storage.returns.copy_(cpu.storage.returns)
    gpu.storage.advantages.copy_(cpu.storage.advantages)
    padded = next(iter(cpu.storage.reccurent_mini_batch_generator(4, 1)))
    dense = next(iter(gpu.storage.recurrent_dense_mini_batch_generator(4, 1)))
    l_cpu = cpu._reference_loss(*padded)[0]
    l_gpu = gpu._reference_loss(*dense)[0]
    g_cpu = torch.autograd.grad(l_cpu, list(ac_cpu.parameters()))
    g_gpu = torch.autograd.grad(l_gpu, list(ac_gpu.parameters()))
    print("gru loss gpu / cpu", float(l_gpu), float(l_cpu))
    torch.testing.assert_close(l_gpu.detach().cpu(), l_cpu.detach(), rtol=1e-4, atol=0)
    for (name, _), a, b in zip(ac_cpu.named_parameters(), g_gpu, g_cpu):
        rel = _rel(a.cpu(), b)
        print("gru loss grad", name, rel)
        assert rel < 1e-3, (name, rel)


def test_gru_rollout_graph_matches_eager():
    """test_recurrent_rollout_graph_matches_eager on g1_gru: the captured collection loop (GRU
    state stepped in place, masked resets in the store launch) replays the eager loop."""
    import isaacgym  # noqa: F401
    from legged_gym.envs import task_registry
    from legged_gym.utils import get_args
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    out = {}
    for graph in (False, True):
        args = get_args(["--task", "g1_gru", "--num_envs", "64", "--headless"])
        env_cfg, train_cfg = task_registry.get_cfgs("g1_gru")
        env_cfg = copy.deepcopy(env_cfg)
        env_cfg.env.episode_length_s = 0.5  # resets inside every rollout
        env, _ = task_registry.make_env(name="g1_gru", args=args, env_cfg=env_cfg)
        cfg = class_to_dict(train_cfg)
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        ac = runner.alg.actor_critic
        assert isinstance(ac.memory_a.rnn, torch.nn.GRU) and runner.alg._rollout is not None
        runner.alg.use_graph = False  # compare the rollouts, not the update paths
        runner.learn(3, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        st = runner.alg.storage
        assert len(st.saved_hidden_states_a) == 1 and torch.is_tensor(ac.memory_a.hidden_states)
        out[graph] = dict(st_obs=st.observations.clone(), st_act=st.actions.clone(), st_rew=st.rewards.clone(),
                          hid_a=st.saved_hidden_states_a[0].clone(), hid_c=st.saved_hidden_states_c[0].clone(),
                          mem_a=ac.memory_a.hidden_states.clone(), mem_c=ac.memory_c.hidden_states.clone(),
                          dones=st.dones.clone(), params=[p.detach().clone() for p in ac.parameters()],
                          captured=runner._rollout_graph is not None)
        env.close()
    e, g = out[False], out[True]
    assert g["captured"] and not e["captured"]
    assert bool(e["dones"].any()) and bool((e["hid_a"] != 0).any())
    for k in ("st_obs", "st_act", "st_rew", "hid_a", "hid_c", "mem_a", "mem_c"):
        assert torch.equal(e[k], g[k]), k
    for a, b in zip(e["params"], g["params"]):
        assert torch.equal(a, b)
    # the state saved for step t + 1 is zero exactly where step t was done
    d = e["dones"][:-1, :, 0].bool()
    for hid in (e["hid_a"], e["hid_c"]):
        assert bool((hid[1:, 0][d] == 0).all()) and bool((hid[1:, 0][~d] != 0).any(-1).all())


def test_gru_store_zeroes_the_done_envs_memories_as_reset():
    """The store launch zeroes the done envs' h rows of both memories (single-tensor states),
    the other envs' rows untouched, and the torch reset is not needed."""
    torch.manual_seed(5)
    N, T, O, P, A = 256, 3, 47, 50, 12
    ac = ActorCriticRecurrent(O, P, A, **KW).cuda()
    alg = PPO(ac, device="cuda")
    alg.init_storage(N, T, [O], [P], [A])
    g = torch.Generator(device="cuda").manual_seed(2)
    obs, cobs = torch.randn(N, O, device="cuda", generator=g), torch.randn(N, P, device="cuda", generator=g)
    calls = []
    real_reset = ac.reset
    ac.reset = lambda dones=None: (calls.append(1), real_reset(dones))[1]
    for t in range(T):
        with torch.inference_mode():
            prev = [None if m.hidden_states is None else m.hidden_states.clone() for m in (ac.memory_a, ac.memory_c)]
            alg.act(obs, cobs)
            before = [m.hidden_states.clone() for m in (ac.memory_a, ac.memory_c)]
            assert all(bool((h != 0).any()) for h in before)
            dones = torch.rand(N, device="cuda", generator=g) < 0.2
            alg.process_env_step(torch.zeros(N, device="cuda"), dones,
                                 {"time_outs": torch.zeros(N, dtype=torch.bool, device="cuda")})
            after = [m.hidden_states for m in (ac.memory_a, ac.memory_c)]
        for b, a in zip(before, after):
            assert torch.equal(a, b.masked_fill(dones.view(1, -1, 1), 0.0))
        # the storage slot of step t: the state the step started from, written by the step kernel
        st = alg.storage
        for slot, p in zip((st.saved_hidden_states_a[0][t], st.saved_hidden_states_c[0][t]), prev):
            assert bool((slot == 0).all()) if p is None else torch.equal(slot, p)
        # and the stored action means are the heads on the memory's new state
        with torch.inference_mode():
            torch.testing.assert_close(st.mu[t], ac.actor(before[0][0]), rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(st.values[t], ac.critic(before[1][0]), rtol=1e-5, atol=1e-5)
    assert not calls


def test_train_then_play_export_g1_gru():
    """train.py --task g1_gru, then play.py and its export, at 64 envs; the exported
    policy_gru_1.pt reproduces the checkpoint's memory_a.rnn + actor."""
    from test_gpu_scripts import _mlp, run
    exp, n_obs = "pytest_g1_gru", 47
    out = run("train.py", "--task", "g1_gru", "--num_envs", "64", "--max_iterations", "2", "--headless",
              "--experiment_name", exp, "--run_name", "cli")
    assert "Learning iteration 1/2" in out
    from legged_gym import LEGGED_GYM_ROOT_DIR
    runs = sorted(glob.glob(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "*_cli")))
    assert runs, "train.py wrote no run directory"
    ck = os.path.join(runs[-1], "model_2.pt")
    assert os.path.exists(ck)
    run("play.py", "--task", "g1_gru", "--headless", "--experiment_name", exp, "--load_run",
        os.path.basename(runs[-1]))
    pol = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "exported", "policies", "policy_gru_1.pt")
    assert os.path.exists(pol)
    m = torch.jit.load(pol)
    sd = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    actor = {k[len("actor."):]: v for k, v in sd.items() if k.startswith("actor.")}
    rnn = torch.nn.GRU(n_obs, H)
    rnn.load_state_dict({k[len("memory_a.rnn."):]: v for k, v in sd.items() if k.startswith("memory_a.rnn.")})
    x = torch.randn(3, n_obs, generator=torch.Generator().manual_seed(0))
    m.reset_memory()
    h = None
    with torch.no_grad():
        for i in range(3):
            y, h = rnn(x[i:i + 1].unsqueeze(0), h)
            torch.testing.assert_close(m(x[i:i + 1]), _mlp(actor, y[0]), rtol=1e-5, atol=1e-6)
