"""The acting side of the PPO library (csrc/pmlp_noise.h; k_act, k_act4, roll_epilogue,
k_store_step and k_permutation in csrc/ppo_mlp.hip; the ACT branch of k_heads_fwd in
csrc/heads.hip) against the references of tests/act_ref.py at every arm of the host's selection
("The acting anchor").  The C entries are called through mfma_mlp.load() with explicit
seeds and draw counters.  Every output lies between two bands of a sentinel, is filled with
another value before the launch, and the bands are checked after it: a store outside a tensor or
an element never written fails the test.  Actions are held to mu + sigma z of the fp64 noise
within act_bound, st_logp to the fp64 log-density of the stored row within logp_bound, every
copy, the store step and the permutation to equality; the bounds are derived in act_ref.py's
docstring.  Each test prints the worst measured fraction of each bound."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import act_ref as R  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

DEV = "cuda"
P = mm._p
F = np.float32
SEED = 0x9E3779B97F4A7C15        # (the high word set)
GUARD = 64                       # elements (256 bytes of fp32: the tensor stays 16-byte aligned)
SENT = {torch.float32: 1234.5, torch.uint8: 0xA5, torch.int64: -7777}
FILL = {torch.float32: float("nan"), torch.uint8: 0xEE, torch.int64: -1}
WORST = {}


class Out:
    """An output of the given shape between two bands of the sentinel, filled with NaN (fp32),
    0xEE (bytes) or -1 (int64), or with `init`: a buffer the kernel reads and overwrites.  off:
    the tensor starts that many elements past the 16-byte aligned position."""

    def __init__(self, *shape, dtype=torch.float32, init=None, off=0):
        n = int(np.prod(shape))
        self.s = SENT[dtype]
        self.flat = torch.full((n + 2 * GUARD + off,), self.s, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD + off:GUARD + off + n].view(*shape)
        if init is None:
            self.t.fill_(FILL[dtype])
        else:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).view(*shape))
        self.n, self.off = n, off

    def get(self):
        g = torch.cat([self.flat[:GUARD + self.off], self.flat[GUARD + self.off + self.n:]])
        assert bool((g == self.s).all()), "a store outside the tensor (guard band overwritten)"
        return self.t.cpu().numpy()


def dev(a, off=0):
    """a on the device, `off` elements past a 16-byte aligned address."""
    if a is None:
        return None
    a = torch.as_tensor(np.ascontiguousarray(a))
    flat = torch.zeros(a.numel() + off + 4, dtype=a.dtype, device=DEV)
    v = flat[off:off + a.numel()].view(a.shape)
    v.copy_(a)
    assert v.data_ptr() % 16 == (off * a.element_size()) % 16
    return v


def got(outs):
    torch.cuda.synchronize()
    return {k: o.get() for k, o in outs.items() if o is not None}


def sigma_of(A, unit=False):
    """0.8 (1 + 0.1 k / A): never a power of two."""
    return np.ones(A, F) if unit else (0.8 * (1.0 + 0.1 * np.arange(A) / A)).astype(F)


def show(what, fr):
    for k, v in fr.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()), "| so far:",
          ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


ACT_KEYS = ("actions_out", "st_actions", "st_mu", "st_sigma")


# ------------------------------------------------------------------- launchers --
def act_launch(mu, stdv, seed, draw, O=5, CO=3, off=0, in_off=0, obs_off=0, cobs=True, value=None):
    """pmlp_act on mu [N, A]; off / in_off / obs_off: the [N, A] outputs, mu, and obs + st_obs sit
    that many floats past a 16-byte boundary.  Returns the outputs and the inputs it built."""
    N, A = mu.shape
    rng = np.random.default_rng(N * 131 + A)
    inp = dict(mu=mu, stdv=stdv, value=rng.standard_normal(N).astype(F) if value is None else value,
               obs=rng.standard_normal((N, O)).astype(F), cobs=rng.standard_normal((N, CO)).astype(F) if cobs else None)
    d = dict(mu=dev(mu, in_off), stdv=dev(stdv), value=dev(inp["value"]), obs=dev(inp["obs"], obs_off),
             cobs=dev(inp["cobs"]), draw=dev(np.array([draw, 99], np.int64)))
    o = {k: Out(N, A, off=off) for k in ACT_KEYS}
    o.update(st_logp=Out(N), st_value=Out(N), st_obs=Out(N, O, off=obs_off), st_cobs=Out(N, CO) if cobs else None)
    mm._ok(mm.load().pmlp_act(P(d["mu"]), P(d["stdv"]), P(d["value"]), P(d["obs"]), P(d["cobs"]), N, A, O, CO if cobs else 0,
                              P(d["draw"]), seed, P(o["actions_out"].t), P(o["st_actions"].t), P(o["st_logp"].t),
                              P(o["st_mu"].t), P(o["st_sigma"].t), P(o["st_value"].t), P(o["st_obs"].t),
                              P(o["st_cobs"].t) if cobs else None, mm._stream()), "pmlp_act")
    out = got(o)
    assert d["draw"].cpu().tolist() == [draw, 99], "pmlp_act reads the draw counter and does not advance it"
    return out, inp


def check_act_launch(out, inp, seed, draw, what):
    fr = R.check_act_rows(out, inp["stdv"], seed, draw, mu=inp["mu"])
    R.check_equal(out["st_value"], inp["value"], "st_value")
    R.check_equal(out["st_obs"], inp["obs"], "st_obs")
    if inp.get("cobs") is not None:
        R.check_equal(out["st_cobs"], inp["cobs"], "st_cobs")
    show(what, fr)
    return fr


def mu_of(N, A, zero=False):
    rng = np.random.default_rng(N * 17 + A)
    return np.zeros((N, A), F) if zero else rng.standard_normal((N, A)).astype(F)


def _net(gen, K0, nout, x, kx, N, hid=32):
    ks, ns = [K0, hid, hid, hid], [hid, hid, hid, nout]
    W = [(torch.randn(n, k, generator=gen, device=DEV) * (1.2 / k ** 0.5)).to(torch.bfloat16).contiguous()
         for n, k in zip(ns, ks)]
    b = [0.1 * torch.randn(n, generator=gen, device=DEV) for n in ns]
    return dict(x=x, kx=kx, K0=K0, W=W, b=b, N=ns, o=Out(N, nout))


def rollout_launch(N, A, K0, O, CO, seed, draw, parity, stdv, store, time_outs=True, cobs=True):
    """pmlp_rollout_forward: 4-layer nets at the narrowest hidden widths (32); the critic reads
    cobs [N, CO] (obs when cobs is off).  store: the previous step's deferred store rides along."""
    gen = torch.Generator(device=DEV).manual_seed(N * 1000 + A * 10 + K0)
    rng = np.random.default_rng(N * 7 + A)
    obs = torch.randn(N, O, generator=gen, device=DEV)
    cob = torch.randn(N, CO, generator=gen, device=DEV) if cobs else None
    nets = [_net(gen, K0, A, obs, O, N), _net(gen, K0, 1, cob if cobs else obs, CO if cobs else O, N)]
    o = {k: Out(N, A) for k in ACT_KEYS}
    o.update(st_logp=Out(N), st_value=Out(N), st_obs=Out(N, O), st_cobs=Out(N, CO) if cobs else None,
             draw=Out(2, dtype=torch.int64, init=np.array([draw, -5] if parity == 0 else [-5, draw], np.int64)))
    sd = dev(stdv)
    rs = mm.RolloutStep(P(sd), P(obs), P(cob), O, CO if cobs else 0, A, P(o["actions_out"].t), P(o["st_actions"].t),
                        P(o["st_logp"].t), P(o["st_mu"].t), P(o["st_sigma"].t), P(o["st_value"].t), P(o["st_obs"].t),
                        P(o["st_cobs"].t) if cobs else None, P(o["draw"].t), parity, seed)
    st = None
    if store:
        pick = np.array([0, 0, 1, 2, 255], np.uint8)
        st = dict(rew=rng.standard_normal(N).astype(F), dones=pick[rng.integers(0, 5, N)],
                  touts=pick[rng.integers(0, 5, N)] if time_outs else None, value=(3 * rng.standard_normal(N)).astype(F),
                  gamma=0.99)
        sdv = {k: dev(st[k]) for k in ("rew", "dones", "touts", "value")}
        o.update(st_rewards=Out(N), st_dones=Out(N, dtype=torch.uint8))
        rs.rewards, rs.dones, rs.time_outs, rs.prev_value = P(sdv["rew"]), P(sdv["dones"]), P(sdv["touts"]), P(sdv["value"])
        rs.st_rewards, rs.st_dones, rs.gamma = P(o["st_rewards"].t), P(o["st_dones"].t), st["gamma"]
    mm.mlp_forward([dict(n, out=n["o"].t) for n in nets], N, rollout=rs)
    out = got(o)
    out["mu"], out["value"] = nets[0]["o"].get(), nets[1]["o"].get().reshape(-1)
    inp = dict(stdv=stdv, obs=obs.cpu().numpy(), cobs=cob.cpu().numpy() if cobs else None, store=st)
    return out, inp


def check_rollout(out, inp, seed, draw, parity, what):
    R.check_equal(out["st_mu"], out["mu"], "st_mu vs the launch's own mu")
    R.check_equal(out["st_value"], out["value"], "st_value vs the launch's own value")
    assert np.isfinite(out["mu"]).all() and np.isfinite(out["value"]).all()
    fr = R.check_act_rows(out, inp["stdv"], seed, draw)
    R.check_equal(out["st_obs"], inp["obs"], "st_obs")
    if inp["cobs"] is not None:
        R.check_equal(out["st_cobs"], inp["cobs"], "st_cobs")
    want = [draw, draw + 1] if parity == 0 else [draw + 1, draw]
    assert out["draw"].tolist() == want, (out["draw"], want)
    st = inp["store"]
    if st is not None:
        R.check_store(out, st["rew"], st["dones"], st["touts"], st["value"], st["gamma"])
    show(what, fr)


def heads_launch(M, H, A, seed, draw, stdv, O=7, CO=5, cobs=True, N0=(24, 8)):
    """pmlp_heads_forward_act: actor (N0[0] units, A outputs) and critic (N0[1] units, 1 output)."""
    gen = torch.Generator(device=DEV).manual_seed(M * 100 + H + A)
    h = [torch.randn(M, H, generator=gen, device=DEV) for _ in range(2)]
    obs = torch.randn(M, O, generator=gen, device=DEV)
    cob = torch.randn(M, CO, generator=gen, device=DEV) if cobs else None
    jobs, keep, outs = (mm.HeadJob * 2)(), [], []
    for j, (n0, n1) in enumerate(((N0[0], A), (N0[1], 1))):
        w = dict(W0=torch.randn(n0, H, generator=gen, device=DEV) / H ** 0.5, b0=0.1 * torch.randn(n0, generator=gen, device=DEV),
                 W1=torch.randn(n1, n0, generator=gen, device=DEV) / n0 ** 0.5, b1=0.1 * torch.randn(n1, generator=gen, device=DEV))
        oo = dict(y0=Out(M, n0), out=Out(M, n1))
        jobs[j] = mm.HeadJob(P(h[j]), P(w["W0"]), P(w["b0"]), P(w["W1"]), P(w["b1"]), P(oo["y0"].t), P(oo["out"].t), None,
                             None, None, n0, n1)
        keep.append(w)
        outs.append(oo)
    o = {k: Out(M, A) for k in ACT_KEYS}
    o.update(st_logp=Out(M), st_value=Out(M), st_obs=Out(M, O), st_cobs=Out(M, CO) if cobs else None)
    sd, dr = dev(stdv), dev(np.array([draw, 99], np.int64))
    ha = mm.HeadAct(P(sd), P(obs), P(cob), O, CO if cobs else 0, A, P(dr), seed, P(o["actions_out"].t), P(o["st_actions"].t),
                    P(o["st_logp"].t), P(o["st_mu"].t), P(o["st_sigma"].t), P(o["st_value"].t), P(o["st_obs"].t),
                    P(o["st_cobs"].t) if cobs else None)
    mm._ok(mm.load().pmlp_heads_forward_act(jobs, M, H, C.byref(ha), mm._stream()), "pmlp_heads_forward_act")
    out = got(o)
    out["mu"], out["value"] = outs[0]["out"].get(), outs[1]["out"].get().reshape(-1)
    for oo in outs:
        assert np.isfinite(oo["y0"].get()).all()
    assert dr.cpu().tolist() == [draw, 99], "the heads' launch reads the draw counter and does not advance it"
    return out, dict(stdv=stdv, obs=obs.cpu().numpy(), cobs=cob.cpu().numpy() if cobs else None, store=None)


# ------------------------------------------------------------ pmlp_act: k_act4 --
@pytest.mark.parametrize("A", [1, 3, 4, 5, 8, 10, 12, 16])
def test_act4_matches_the_reference(A):
    """k_act4 at N = 1, 63, 64, 65, 257 (one lane group, a block's 64 envs and one more, five
    blocks): aligned buffers (the float4 stores where A % 4 == 0), every [N, A] output 4 bytes off
    (the scalar stores at the same A), mu 4 bytes off; cobs present and NULL; the observation copy
    by float4 (N O a multiple of 4, aligned) and by element (N O odd, and an offset view)."""
    for n, N in enumerate((1, 63, 64, 65, 257)):
        for off, in_off in ((0, 0), (1, 0), (0, 1)):
            O = 4 if (n + off) % 2 == 0 else 5
            out, inp = act_launch(mu_of(N, A), sigma_of(A), SEED, 5 + n, O=O, off=off, in_off=in_off,
                                  obs_off=1 if (O == 4 and off) else 0, cobs=(n + in_off) % 2 == 0)
            check_act_launch(out, inp, SEED, 5 + n, f"k_act4 A={A} N={N} off={off},{in_off} O={O}")
    out, inp = act_launch(mu_of(257, A, zero=True), sigma_of(A, unit=True), SEED, 3)      # the action is z itself
    check_act_launch(out, inp, SEED, 3, f"k_act4 A={A} mu=0 sigma=1")
    assert np.abs(out["actions_out"]).max() <= R.Z_MAX


def test_act4_past_the_block_cap():
    """N = 65,601 at O = 4: 4 N lanes need 1,026 blocks, the grid is capped at 1,024, so the
    grid-stride loop and its two barriers run twice in the first blocks."""
    N, A = 65601, 4
    out, inp = act_launch(mu_of(N, A), sigma_of(A), SEED, 8, O=4)
    check_act_launch(out, inp, SEED, 8, f"k_act4 N={N}")


# ------------------------------------------------------------- pmlp_act: k_act --
@pytest.mark.parametrize("A", [17, 20, 23])
def test_act_wide_matches_the_reference(A):
    """k_act (A > 16, one lane per env) at N = 1, 255, 257, aligned and offset buffers."""
    for n, N in enumerate((1, 255, 257)):
        for off in (0, 1):
            out, inp = act_launch(mu_of(N, A), sigma_of(A), SEED, 11 + n, O=4 + off, off=off, cobs=(n + off) % 2 == 0)
            check_act_launch(out, inp, SEED, 11 + n, f"k_act A={A} N={N} off={off}")
    out, inp = act_launch(mu_of(255, A, zero=True), sigma_of(A, unit=True), SEED, 3)
    check_act_launch(out, inp, SEED, 3, f"k_act A={A} mu=0 sigma=1")


def test_act_wide_past_the_block_cap():
    """N = 262,209 at A = 17, O = 4: 1,025 blocks of lanes, capped at 1,024.  Its 2.6 million radius
    words are also the suite's only sample with words below 2^15, where u01's half is visible."""
    N, A = 262209, 17
    out, inp = act_launch(mu_of(N, A), sigma_of(A), SEED, 9, O=4, cobs=False)
    check_act_launch(out, inp, SEED, 9, f"k_act N={N}")


# ------------------------------------------------------- pmlp_rollout_forward --
@pytest.mark.parametrize("A", [1, 4, 10, 12, 16])
def test_rollout_forward_matches_the_reference(A):
    """k_mlp_fwd<32, ROLL> at K0 = 48, N = 1, 31, 32, 33, 97 (a ragged first tile, a whole one,
    one row more, four workgroups): both parities, the deferred store on (time_outs given and
    NULL) and off, cobs on and off, O = 45 (by element) and 48 (16-byte loads)."""
    for n, N in enumerate((1, 31, 32, 33, 97)):
        parity, store = n % 2, n % 3 != 2
        O = 45 if n % 2 else 48
        out, inp = rollout_launch(N, A, 48, O, 41, SEED, 20 + n, parity, sigma_of(A), store, time_outs=n != 3,
                                  cobs=n % 2 == 0)
        check_rollout(out, inp, SEED, 20 + n, parity, f"ROLL A={A} N={N} parity={parity} store={store}")
    out, inp = rollout_launch(33, A, 48, 48, 48, SEED, 4, 1, sigma_of(A, unit=True), False)
    check_rollout(out, inp, SEED, 4, 1, f"ROLL A={A} sigma=1")


@pytest.mark.parametrize("N,A", [(33, 12), (97, 10)])
def test_rollout_forward_wider_matches_the_reference(N, A):
    """k_mlp_fwd<32, ROLL, WIDER> (K0 = 320, O = 300 inputs)."""
    out, inp = rollout_launch(N, A, 320, 300, 290, SEED, 31, N % 2, sigma_of(A), True)
    check_rollout(out, inp, SEED, 31, N % 2, f"ROLL WIDER A={A} N={N}")


# ------------------------------------------------------ pmlp_heads_forward_act --
@pytest.mark.parametrize("H", [32, 64, 128])
@pytest.mark.parametrize("A", [1, 10, 12, 16])
def test_heads_forward_act_matches_the_reference(H, A):
    """The ACT branch of k_heads_fwd<H> at M = 1, 127, 128, 129 (64 rows per workgroup)."""
    for n, M in enumerate((1, 127, 128, 129)):
        out, inp = heads_launch(M, H, A, SEED, 40 + n, sigma_of(A), cobs=n % 2 == 0)
        R.check_equal(out["st_mu"], out["mu"], "st_mu vs the launch's own mu")
        R.check_equal(out["st_value"], out["value"], "st_value vs the launch's own value")
        fr = R.check_act_rows(out, inp["stdv"], SEED, 40 + n)
        R.check_equal(out["st_obs"], inp["obs"], "st_obs")
        if inp["cobs"] is not None:
            R.check_equal(out["st_cobs"], inp["cobs"], "st_cobs")
        show(f"heads ACT H={H} A={A} M={M}", fr)


def test_heads_forward_act_matrix_core_form_matches_the_reference():
    """From 16,384 rows the heads' forward runs y0 on the matrix cores (64 rows x 128 threads per
    workgroup): its ACT branch at M = 16,421 (a ragged last tile of 37 rows)."""
    M, H, A = 16421, 64, 12
    out, inp = heads_launch(M, H, A, SEED, 51, sigma_of(A))
    R.check_equal(out["st_mu"], out["mu"], "st_mu vs the launch's own mu")
    R.check_equal(out["st_value"], out["value"], "st_value vs the launch's own value")
    fr = R.check_act_rows(out, inp["stdv"], SEED, 51)
    R.check_equal(out["st_obs"], inp["obs"], "st_obs")
    R.check_equal(out["st_cobs"], inp["cobs"], "st_cobs")
    show(f"heads ACT, matrix-core y0, M={M}", fr)


# ------------------------------------------------------------------ cross-arm --
def _same(a, b, what):
    """Bitwise equality of an arm's actions and log-probabilities; the share that differs is printed."""
    for k in ("actions_out", "st_logp"):
        x, y = a[k].view(np.uint32), b[k].view(np.uint32)
        share = float((x != y).mean())
        print(f"{what}: {k} differs in {share:.4%} of {x.size} elements")
        WORST[f"differs {k}"] = max(WORST.get(f"differs {k}", 0.0), share)
    for k in ("actions_out", "st_logp"):
        R.check_equal(a[k], b[k], f"{what}: {k}")


@pytest.mark.parametrize("A", [10, 12])
def test_every_arm_samples_the_same_bits(A):
    """include/ppo_mlp.h: for one (seed, draw) and equal mu, pmlp_act, pmlp_rollout_forward and
    pmlp_heads_forward_act give bitwise the same actions and log-probabilities, at a sigma that is
    no power of two (at sigma = 1 the product is exact and a contracted mu + sigma z cannot
    differ).  The sampling arms are fed the forward arms' own mu.  k_act (A > 16) shares its first
    16 columns' counters with k_act4 at A = 16."""
    stdv = sigma_of(A)
    roll, _ = rollout_launch(97, A, 48, 48, 48, SEED, 77, 0, stdv, False)
    act, _ = act_launch(roll["mu"], stdv, SEED, 77)
    _same(roll, act, f"pmlp_rollout_forward vs pmlp_act A={A}")
    heads, _ = heads_launch(129, 64, A, SEED, 77, stdv)
    act, _ = act_launch(heads["mu"], stdv, SEED, 77)
    _same(heads, act, f"pmlp_heads_forward_act vs pmlp_act A={A}")
    mu = (3.0 * mu_of(257, 20)).astype(F)
    s20 = sigma_of(20)
    wide, _ = act_launch(mu, s20, SEED, 77)
    quad, _ = act_launch(np.ascontiguousarray(mu[:, :16]), s20[:16], SEED, 77)
    R.check_equal(np.ascontiguousarray(wide["actions_out"][:, :16]), quad["actions_out"], "k_act vs k_act4: actions")


def test_the_draw_word_is_the_low_32_bits_and_the_seed_high_word_matters():
    mu, stdv = mu_of(65, 12), sigma_of(12)
    a5, _ = act_launch(mu, stdv, SEED, 5)
    big, inp = act_launch(mu, stdv, SEED, (1 << 32) + 5)
    check_act_launch(big, inp, SEED, (1 << 32) + 5, "draw = 2^32 + 5")
    for k in ("actions_out", "st_logp"):
        R.check_equal(big[k], a5[k], f"draw 2^32 + 5 vs 5: {k}")
    a6, _ = act_launch(mu, stdv, SEED, 6)
    assert (a6["actions_out"] != a5["actions_out"]).mean() > 0.99
    hi, inp = act_launch(mu, stdv, SEED ^ (1 << 40), 5)
    check_act_launch(hi, inp, SEED ^ (1 << 40), 5, "another high seed word")
    assert (hi["actions_out"] != a5["actions_out"]).mean() > 0.99


# ------------------------------------------------------------------ store step --
def store_launch(N, entry, time_outs, nstates, H, with_draw, gamma=0.99):
    rng = np.random.default_rng(N * 10 + nstates)
    pick = np.array([0, 0, 0, 1, 2, 255], np.uint8)
    c = dict(rew=rng.standard_normal(N).astype(F), dones=pick[rng.integers(0, 6, N)],
             touts=pick[rng.integers(0, 6, N)] if time_outs else None, value=(3 * rng.standard_normal(N)).astype(F),
             gamma=gamma, states=[(rng.standard_normal((N, H)) + 3).astype(F) for _ in range(nstates)])
    if N > 4:
        c["dones"][:4] = (0, 1, 2, 255)
        if time_outs:
            c["touts"][:4] = (1, 0, 255, 2)       # a time-out alone, a done alone, both
    d = {k: dev(c[k]) for k in ("rew", "dones", "touts", "value")}
    o = dict(st_rewards=Out(N), st_dones=Out(N, dtype=torch.uint8))
    so = [Out(N, H, init=s) for s in c["states"]]
    dr = Out(1, dtype=torch.int64, init=np.array([41], np.int64)) if with_draw else None
    ptrs = (C.c_void_p * max(nstates, 1))(*[P(s.t) for s in so])
    L = mm.load()
    head = (P(d["rew"]), P(d["dones"]), P(d["touts"]), P(d["value"]), P(o["st_rewards"].t), P(o["st_dones"].t), N, gamma,
            P(dr.t) if dr else None)
    if entry == "plain":
        rc = L.pmlp_store_step(*head, mm._stream())
    elif entry == "reset":
        rc = L.pmlp_store_step_reset(*head, nstates, ptrs if nstates else None, H, mm._stream())
    else:
        rc = L.pmlp_store_step_env(*head, nstates, ptrs if nstates else None, H, None, mm._stream())
    mm._ok(rc, "pmlp_store_step")
    out = got(o)
    R.check_store(out, c["rew"], c["dones"], c["touts"], c["value"], gamma)
    for s0, s1 in zip(c["states"], so):
        R.check_equal(s1.get(), R.reset_ref(s0, c["dones"]), "memory state")     # live envs' rows untouched
    if dr:
        assert dr.get().tolist() == [42]
    return out


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_store_step_matches_the_reference(N):
    """pmlp_store_step, _reset and _env (ex = NULL): time_outs NULL and given; done and time-out
    bytes of 0, 1, 2, 255; 0, 1 and 4 memory states at H = 4, 64, 128; draw NULL and given."""
    store_launch(N, "plain", True, 0, 0, True)
    store_launch(N, "plain", False, 0, 0, False)
    store_launch(N, "reset", True, 0, 0, False)
    store_launch(N, "reset", True, 1, 4, True)
    store_launch(N, "reset", False, 4, 64, False)
    store_launch(N, "env", True, 4, 128, True)
    store_launch(N, "env", True, 1, 64, False)
    store_launch(N, "env", False, 0, 0, True)


# ----------------------------------------------------------------- permutation --
PERM_N = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 4096, 4097, 98304, 100003)


@pytest.mark.parametrize("n", PERM_N)
def test_permutation_matches_the_reference(n):
    for seed in (0x123456789abcdef, 0xFEDCBA9800000007):
        o = Out(n, dtype=torch.int64)
        mm._ok(mm.load().pmlp_permutation(P(o.t), n, seed, mm._stream()), "pmlp_permutation")
        torch.cuda.synchronize()
        R.check_permutation(o.get(), n, seed)


def test_permutation_refuses_sizes_outside_its_domain():
    o = Out(8, dtype=torch.int64)
    for n in (0, -3, (1 << 40) + 1):
        assert mm.load().pmlp_permutation(P(o.t), n, 5, mm._stream()) != 0
    torch.cuda.synchronize()
    assert (o.get() == FILL[torch.int64]).all()
