"""The scalar half of the PPO update -- the loss kernels (csrc/ppo_loss.hip and the loss epilogue
in csrc/ppo_mlp.hip, all on the one core of csrc/ppo_loss.h), the GAE kernels, the Adam kernels
(csrc/ppo_mlp.hip) and the three callers of the KL learning-rate rule -- against the fp64 references
of tests/ppo_ref.py, at every arm of the host's selection, with the bounds derived there (never
fitted to what a kernel returns).  tests/test_ppo_ref_host.py applies the same comparison
functions to deliberately wrong outputs and asserts the input conditions of every case below.

Every output sits in a sentinel-prefilled buffer with a band before and after it; nothing
outside the stated extent may change.  Tests print their worst error as a fraction of its
bound (pytest -s shows them; DESIGN.md section 4 records them).

Arms reached, to tick against loss_step_launch, pmlp_adam_mirror_n and the GAE entries:
  pmlp_ppo_loss_step   each (A, Ap) below at M = 1, 37, 64, 65, 257, 517 (the listed M is the
                       kernel's M: its last min(12, M - 1) rows are the grid rows of
                       ppo_ref.edge_rows(); M = 1 has room for none), with per M the toggles
                       (rows gathered, clipped_value, dmu_t and dvalue_t given) =
                       (0,1,0) (1,0,1) (1,1,1) (0,0,0) (1,1,0) (0,1,1), and at M = 64 once more
                       with stats = dstd = NULL (partials only):
      k_ppo_loss_step_q       (4, 4) first quad only; (4, 8) quad lane 1 writes zeros;
                              (12, 16) three quads of data, one of zeros; (16, 16) all four
      k_ppo_loss_step_reg<16> scalar loads (10, 16), (1, 8), (3, 8); float4 loads (12, 24), (8, 32)
      k_ppo_loss_step         (10, 12), (17, 17), (20, 24)
  pmlp_ppo_loss_step_f32   A = 12 quad, 10 register (scalar loads), 20 generic, at M = 65, 257;
                       the unaligned dmu refusal
  pmlp_ppo_loss_fwd / _bwd   M = 1, 255, 256, 257, 517 x A = 1, 10, 12, 20, gout 1 and 0.5, rows
                       and clipped_value alternating (ppo_ref.bwd_toggles)
  pmlp_reduce_slabs_step   the folded finish on the step kernel's partials (M = 101, A = 12), and
                       its copy of the KL rule
  pmlp_mlp_forward_ppo_loss  M = 18469 (a ragged last group), the three instantiations:
                       k_mlp_fwd<96, LOSS> (K0 16), <96, LOSS, WIDE> (K0 80), <64, LOSS, WIDER> (K0 320)
  k_gae                pmlp_gae_local, pmlp_gae: N = 1, 63, 64, 65, 255, 256, 257, 333 x T = 1, 2, 7
                       x five done patterns on the exact grid; N = 257, 333 at T = 24 realistic
  k_adv_norm           its own moments (gstats NULL, through pmlp_gae) and given moments
  k_adam_vec<4>        n = 3 (no whole group), 4, 1021, 4098, 4099 (tails 0..3); the grid-stride
                       reload at n = 4096 * 256 * 4 + 1203; mirrors (dst + frag)
  k_adam_vec<2>        views 2 floats into an aligned allocation, n odd and even; a mirror offset
                       that is a multiple of 2 only
  k_adam               views 1 float in; a mirror with odd cols; n = 1024 * 256 + 259 (the
                       grid-stride loop past the 1024-block cap); pmlp_adam
  KL rule              k_loss_bookkeeping, k_opt_prepare (grad_scale 0.5), reduce_step_finish
Not reached: the PMLP_ADAM_VEC switch (read once per process; the arms are reached by alignment);
k_ppo_loss_step_reg's float4 loads through pmlp_ppo_loss_step_f32 (A % 4 == 0, A <= 16 always
takes the quad kernel there, Ap being 0); the grid rows in the loss inside the forward (a grid
row needs a chosen value, and there the value is the launch's own output; loss_quad_rows'
branches are covered through k_ppo_loss_step_q); normalising T N = 1 advantages with their own
moments (the unbiased std of one number is undefined and pmlp_gae refuses the size); what is
out of scope (pmlp_act, the Philox noise, the store-step family, the sequence kernels, the heads).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

import ppo_ref as R  # noqa: E402

DEV = "cuda"
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
P = mm._p
VCOEF, ECOEF = 0.5, 0.01


def _sync():
    torch.cuda.synchronize()


class Band:
    """n elements starting `off` elements into an aligned, sentinel-prefilled allocation with
    64 elements in front and behind: .v is the view a kernel is given."""

    def __init__(self, n, dtype=F32, off=0):
        self.lo, self.n = 64 + off, n
        self.flat = torch.full((64 + off + n + 64,), R.SENTINEL, dtype=dtype, device=DEV)
        self.v = self.flat[self.lo:self.lo + n]
        self.sentinel = torch.tensor(R.SENTINEL, dtype=dtype, device=DEV)

    def untouched(self, what):
        m = torch.ones_like(self.flat, dtype=torch.bool)
        m[self.lo:self.lo + self.n] = False
        bad = m & (self.flat != self.sentinel)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the buffer were written"

    def all_sentinel(self):
        return bool((self.flat == self.sentinel).all())

    def none_sentinel(self):
        return not bool((self.v == self.sentinel).any())


def _mat(rows, cols, dtype):
    return R.Guarded(rows, cols, cols, dtype, DEV)


def _dev(inp):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}


def _largs(d, mu=None, value=None):
    return (P(d["mu"] if mu is None else mu), P(d["std"]), P(d["value"] if value is None else value), P(d["act"]),
            P(d["old_logp"]), P(d["old_mu"]), P(d["old_sigma"]), P(d["adv"]), P(d["ret"]), P(d["target"]), P(d["rows"]))


def _show(what, fr):
    print(f"[ppo-ref] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fr.items())))


# ------------------------------------------------------- pmlp_ppo_loss_step --
def _run_step(d, M, A, Ap, Vp, cv, transposed, with_stats=True):
    L = mm.load()
    g = dict(partial=Band(L.pmlp_ppo_loss_step_parts(M, A)), stats=Band(4), dstd=Band(A),
             dmu=_mat(M, Ap, BF), dv=_mat(M, Vp, BF))
    if transposed:
        g.update(dmu_t=_mat(Ap, M, BF), dv_t=_mat(Vp, M, BF))
    pt = lambda k: P(g[k].mat) if k in g else None  # noqa: E731
    mm._ok(L.pmlp_ppo_loss_step(*_largs(d), M, A, R.CLIP, cv, VCOEF, ECOEF, P(g["partial"].v),
                                P(g["stats"].v) if with_stats else None, P(g["dstd"].v) if with_stats else None,
                                pt("dmu"), pt("dmu_t"), Ap, pt("dv"), pt("dv_t"), Vp, mm._stream()),
           "pmlp_ppo_loss_step")
    _sync()
    for k, b in g.items():
        b.untouched(k) if isinstance(b, Band) else b.assert_untouched(k)
    out = {k: g[k].got().cpu() for k in ("dmu", "dv", "dmu_t", "dv_t") if k in g}
    assert g["partial"].none_sentinel(), "partials not all written"
    if with_stats:
        out.update(stats=g["stats"].v.cpu(), dstd=g["dstd"].v.cpu())
    else:
        assert g["stats"].all_sentinel() and g["dstd"].all_sentinel(), "stats / dstd written with NULL given"
    out["partial"] = g["partial"].v.clone()
    return out


@pytest.mark.parametrize("arm,A,Ap", R.LOSS_ARMS)
def test_loss_step_arm_matches_fp64(arm, A, Ap):
    assert R.loss_arm(A, Ap) == arm
    worst = {}
    for M, (rows, cv, tr) in zip(R.LOSS_M, R.LOSS_TOGGLES):
        inp = R.loss_inputs(M, A, R.loss_seed(M, A), bool(rows))
        ref = R.loss_ref(inp, clipped_value=cv, vcoef=VCOEF, ecoef=ECOEF)
        d = _dev(inp)
        what = f"{arm} A={A} Ap={Ap} M={M} rows={rows} cv={cv} t={tr}"
        out = _run_step(d, M, A, Ap, 8, cv, bool(tr))
        fr = R.check_loss_step(out, ref, what)
        for k, v in fr.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if M == 64:  # partials only: the same partials and outputs, stats / dstd untouched
            o2 = _run_step(d, M, A, Ap, 1, cv, bool(tr), with_stats=False)
            assert R.same_bits(o2["partial"], out["partial"]), what + ": partials differ without stats"
            assert R.same_bits(o2["dmu"], out["dmu"]) and R.same_bits(o2["dv"][:, 0], out["dv"][:, 0].contiguous())
            R.check_loss_step(o2, ref, what + " (stats NULL)")
    _show(f"loss step {arm} ({A}, {Ap})", worst)


# --------------------------------------------------- pmlp_ppo_loss_step_f32 --
def _run_f32(d, M, A, cv, dmu_ptr=None):
    L = mm.load()
    g = dict(partial=Band(L.pmlp_ppo_loss_step_parts(M, A)), stats=Band(4), dstd=Band(A), dmu=_mat(M, A, F32),
             dv=Band(M))
    st = L.pmlp_ppo_loss_step_f32(*_largs(d), M, A, R.CLIP, cv, VCOEF, ECOEF, P(g["partial"].v), P(g["stats"].v),
                                  P(g["dstd"].v), P(g["dmu"].mat) if dmu_ptr is None else dmu_ptr(g["dmu"]),
                                  P(g["dv"].v), mm._stream())
    _sync()
    return st, g


@pytest.mark.parametrize("A,M", R.F32_CASES)
def test_loss_step_f32_matches_fp64_and_the_bf16_form(A, M):
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), True)
    ref = R.loss_ref(inp, clipped_value=1, vcoef=VCOEF, ecoef=ECOEF)
    d = _dev(inp)
    st, g = _run_f32(d, M, A, 1)
    assert st == 0, mm.load().pmlp_last_error()
    for k, b in g.items():
        b.untouched(k) if isinstance(b, Band) else b.assert_untouched(k)
    out = dict(dmu=g["dmu"].got().cpu(), dv=g["dv"].v.cpu(), stats=g["stats"].v.cpu(), dstd=g["dstd"].v.cpu())
    fr = R.check_loss_f32(out, ref, f"f32 A={A} M={M}")
    _show(f"loss step f32 A={A} M={M}", fr)
    # the bf16 form on the same arm rounds these very numbers (the two forms share dlogp)
    Ap = {12: 16, 10: 16, 20: 24}[A]
    assert R.loss_arm(A, Ap) == R.loss_arm(A, 0)
    b16 = _run_step(d, M, A, Ap, 8, 1, False)
    R.check_loss_step(b16, ref, f"bf16 form A={A} Ap={Ap} M={M}")
    assert R.same_bits(out["dmu"].to(BF).contiguous(), b16["dmu"][:, :A].contiguous()), "bf16 dmu != RNE(fp32 dmu)"
    assert R.same_bits(out["dv"].to(BF).contiguous(), b16["dv"][:, 0].contiguous()), "bf16 dvalue != RNE(fp32 dvalue)"
    assert R.same_bits(out["stats"], b16["stats"]) and R.same_bits(out["dstd"], b16["dstd"])


def test_loss_step_f32_refuses_an_unaligned_dmu():
    M, A = 65, 12
    d = _dev(R.loss_inputs(M, A, R.loss_seed(M, A), True))
    st, g = _run_f32(d, M, A, 1, dmu_ptr=lambda G: P(G.mat) + 4)
    assert st == -1 and b"16-byte" in mm.load().pmlp_last_error()
    assert all(b.all_sentinel() for b in g.values() if isinstance(b, Band))
    assert bool((g["dmu"].flat == g["dmu"].sentinel).all())


# --------------------------------------- pmlp_ppo_loss_fwd / pmlp_ppo_loss_bwd --
@pytest.mark.parametrize("ia", range(len(R.BWD_A)))
def test_autograd_path_loss_matches_fp64(ia):
    L = mm.load()
    A = R.BWD_A[ia]
    worst = {}
    for im, M in enumerate(R.BWD_M):
        rows, cv, gout = R.bwd_toggles(im, ia)
        inp = R.loss_inputs(M, A, R.loss_seed(M, A), rows)
        ref = R.loss_ref(inp, clipped_value=cv, vcoef=VCOEF, ecoef=ECOEF, gout=gout)
        ref1 = R.loss_ref(inp, clipped_value=cv, vcoef=VCOEF, ecoef=ECOEF)
        d = _dev(inp)
        nb = L.pmlp_ppo_loss_blocks(M)
        g = dict(partial=Band(4 * nb), loss=Band(1), stats=Band(4), dmu=_mat(M, A, F32), dv=Band(M),
                 pstd=Band(A * nb), dstd=Band(A))
        go = torch.tensor([gout], device=DEV)
        a = _largs(d)
        mm._ok(L.pmlp_ppo_loss_fwd(*a, M, A, R.CLIP, cv, VCOEF, ECOEF, P(g["partial"].v), P(g["loss"].v),
                                   P(g["stats"].v), mm._stream()), "pmlp_ppo_loss_fwd")
        mm._ok(L.pmlp_ppo_loss_bwd(*a, M, A, R.CLIP, cv, VCOEF, ECOEF, P(go), P(g["dmu"].mat), P(g["dv"].v),
                                   P(g["pstd"].v), P(g["dstd"].v), mm._stream()), "pmlp_ppo_loss_bwd")
        _sync()
        for k, b in g.items():
            b.untouched(k) if isinstance(b, Band) else b.assert_untouched(k)
        what = f"fwd/bwd A={A} M={M} rows={rows} cv={cv} gout={gout}"
        fr = R.check_loss_f32(dict(dmu=g["dmu"].got().cpu(), dv=g["dv"].v.cpu(), dstd=g["dstd"].v.cpu()), ref, what)
        fr.update(R.check_loss_stats(g["stats"].v.cpu(), g["dstd"].v.cpu(), dict(ref1, dstd=ref["dstd"], bound=dict(
            ref1["bound"], dstd=ref["bound"]["dstd"])), what, loss=g["loss"].v.cpu()))
        for k, v in fr.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _show(f"loss fwd/bwd A={A}", worst)


# -------------------------------------------------- pmlp_reduce_slabs_step --
def _reduce_step(partial, nb, A, M, std, norm_cap, step, lr, acc, desired, adaptive, slab=None):
    """pmlp_reduce_slabs_step on loss partials, with one small slab job beside it.  Returns
    (stats, dstd, norm partials written, out, nparts)."""
    if slab is None:
        slab = torch.zeros(1, 4, device=DEV)
    ns, n = slab.shape
    g = dict(stats=Band(4), dstd=Band(A), out=Band(n), norm=Band(norm_cap))
    rs = mm.ReduceStep(P(partial), nb, A, M, ECOEF, P(std), P(g["stats"].v), P(g["dstd"].v),
                       P(g["norm"].v) if norm_cap else None, P(step), P(lr), P(acc), desired, adaptive, norm_cap)
    nparts = mm._reduce_step([(slab, g["out"].v, n, ns)], rs)
    _sync()
    for k, b in g.items():
        b.untouched(k)
    return g["stats"].v.cpu(), g["dstd"].v.cpu(), g["norm"].v[:nparts].cpu(), g["out"].v.cpu(), nparts, g["norm"]


def test_folded_finish_is_bitwise_the_final_kernel():
    M, A, Ap = 64 + 37, 12, 16
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), True)
    ref = R.loss_ref(inp, clipped_value=1, vcoef=VCOEF, ecoef=ECOEF)
    d = _dev(inp)
    full = _run_step(d, M, A, Ap, 8, 1, True)
    R.check_loss_step(full, ref, "step kernel before the folded finish")
    part = _run_step(d, M, A, Ap, 8, 1, True, with_stats=False)
    assert R.same_bits(part["partial"], full["partial"])
    gen = torch.Generator(device=DEV).manual_seed(5)
    slab = torch.randint(-16, 17, (3, 37), generator=gen, device=DEV).float() / 8
    step, lr, acc = torch.tensor([4.0], device=DEV), torch.tensor([1e-3], device=DEV), torch.tensor([2.0, 3.0], device=DEV)
    stats, dstd, norm, out, nparts, nb_ = _reduce_step(part["partial"], (M + 63) // 64, A, M, d["std"], 8, step, lr, acc,
                                                       0.0, 0, slab=slab)
    assert R.same_bits(stats, full["stats"]) and R.same_bits(dstd, full["dstd"]), "folded finish != k_ppo_loss_step_final"
    R.check_loss_stats(stats, dstd, ref, "folded finish")
    assert nparts == 2 and not bool((nb_.v[nparts:] != nb_.sentinel).any())
    assert torch.equal(out, slab.sum(0).cpu())
    sq = torch.cat([out.double() ** 2, dstd.double() ** 2])
    err = abs(float(norm.double().sum()) - float(sq.sum()))
    bound = R.sum_bound(sq) + R.U * float(sq.sum())
    assert err <= bound, (err, bound)
    _show("folded finish norm partials", dict(norm=err / bound))
    # step advances by one; acc accumulates in the order [value, surrogate]
    assert float(step) == 5.0 and float(lr) == float(np.float32(1e-3))
    f = np.float32
    assert acc.cpu().numpy().tolist() == [f(2.0) + stats[1].numpy(), f(3.0) + stats[0].numpy()]


# ------------------------------------------ pmlp_mlp_forward_ppo_loss (LOSS) --
@pytest.mark.parametrize("K0,form", [(16, "k_mlp_fwd<96, LOSS>"), (80, "k_mlp_fwd<96, LOSS, WIDE>"),
                                     (320, "k_mlp_fwd<64, LOSS, WIDER>")])
def test_loss_inside_the_forward_matches_fp64(K0, form):
    L = mm.load()
    M, A, Ap, Vp = R.FWD_LOSS_M, 12, 16, 8
    Rn, seed = M + R.STORE_EXTRA, R.loss_seed(M, A)
    gen = torch.Generator(device=DEV).manual_seed(K0)
    kx, H = K0 - 3, 32
    x = torch.randn(Rn, K0, generator=gen, device=DEV)
    rows_cpu = R.loss_inputs(M, A, seed, True)["rows"]   # (the builder's gather does not depend on mu)
    rows = rows_cpu.to(DEV)

    def net(nout):
        ks = [K0, H, H, H]
        ns = [H, H, H, nout]
        W = [(torch.randn(n, k, generator=gen, device=DEV) * (1.2 / k ** 0.5)).to(BF).contiguous() for n, k in zip(ns, ks)]
        b = [0.1 * torch.randn(n, generator=gen, device=DEV) for n in ns]
        return dict(x=x, kx=kx, rows=rows, K0=K0, W=W, b=b, N=ns, out=_mat(M, nout, F32))

    nets = [net(A), net(1)]
    jobs = [dict(n, out=n["out"].mat) for n in nets]
    mm.mlp_forward(jobs, M)                      # the plain forward: mu and value to build the rollout side from
    _sync()
    mu0, v0 = nets[0]["out"].got().clone(), nets[1]["out"].got().clone()
    inp = R.loss_inputs(M, A, seed, True, mu=mu0, value=v0)
    assert torch.equal(inp["rows"], rows_cpu)
    d = _dev(inp)
    for n in nets:
        n["out"].flat.fill_(R.SENTINEL)
    nparts = L.pmlp_mlp_forward_ppo_loss_parts_k0(M, A, K0)
    grp = 64 if K0 > 256 else 96
    assert nparts == ((M + grp - 1) // grp) * (3 + A)
    g = dict(partial=Band(nparts), dmu=_mat(M, Ap, BF), dv=_mat(M, Vp, BF), dmu_t=_mat(Ap, M, BF), dv_t=_mat(Vp, M, BF))
    loss = (P(d["std"]), P(d["act"]), P(d["old_logp"]), P(d["old_mu"]), P(d["old_sigma"]), P(d["adv"]), P(d["ret"]),
            P(d["target"]), P(d["rows"]), A, R.CLIP, 1, VCOEF, ECOEF, P(g["partial"].v), P(g["dmu"].mat),
            P(g["dmu_t"].mat), Ap, P(g["dv"].mat), P(g["dv_t"].mat), Vp, mm._stream())
    mm.mlp_forward(jobs, M, loss=loss)
    _sync()
    for k, b in g.items():
        b.untouched(k) if isinstance(b, Band) else b.assert_untouched(k)
    for n in nets:
        n["out"].assert_untouched("out")
    mu, value = nets[0]["out"].got().clone(), nets[1]["out"].got().clone().reshape(-1)
    assert R.same_bits(mu, mu0) and R.same_bits(value, v0.reshape(-1)), "the loss launch's forward differs"
    ref = R.loss_ref(inp, clipped_value=1, vcoef=VCOEF, ecoef=ECOEF, mu=mu, value=value)
    assert g["partial"].none_sentinel()
    step, lr = torch.tensor([0.0], device=DEV), torch.tensor([1e-3], device=DEV)
    stats, dstd, _, _, _, _ = _reduce_step(g["partial"].v, nparts // (3 + A), A, M, d["std"], 0, step, lr, None, 0.0, 0)
    out = {k: g[k].got().cpu() for k in ("dmu", "dv", "dmu_t", "dv_t")}
    out.update(stats=stats, dstd=dstd)
    _show(f"loss in the forward {form}", R.check_loss_step(out, ref, form))


# ------------------------------------------------------------------------ GAE --
def _gae_bufs(T, N):
    L = mm.load()
    return dict(ret=_mat(T, N, F32), adv=_mat(T, N, F32), partial=Band(2 * L.pmlp_gae_parts(N), F64), mom=Band(3, F64))


def _gae_local(x, gamma, lam):
    L = mm.load()
    T, N = x[0].shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in x]
    g = _gae_bufs(T, N)
    mm._ok(L.pmlp_gae_local(*[P(a) for a in t], P(g["ret"].mat), P(g["adv"].mat), T, N, gamma, lam, P(g["partial"].v),
                            P(g["mom"].v), mm._stream()), "pmlp_gae_local")
    _sync()
    for k, b in g.items():
        b.untouched(k) if isinstance(b, Band) else b.assert_untouched(k)
    return t, g


def _normalize(adv_t, moments_t):
    b = Band(adv_t.numel())
    b.v.copy_(adv_t.reshape(-1))
    mm._ok(mm.load().pmlp_adv_normalize(P(b.v), adv_t.numel(), P(moments_t), mm._stream()), "pmlp_adv_normalize")
    _sync()
    b.untouched("normalised advantages")
    return b.v.clone()


def _gae_full(t, T, N, gamma, lam):
    L = mm.load()
    g = _gae_bufs(T, N)
    st = L.pmlp_gae(*[P(a) for a in t], P(g["ret"].mat), P(g["adv"].mat), T, N, gamma, lam, P(g["partial"].v),
                    mm._stream())
    _sync()
    return st, g


@pytest.mark.parametrize("T", R.GAE_T)
def test_gae_on_the_exact_grid_equals_fp64(T):
    worst = 0.0
    for N in R.GAE_N:
        for pat in R.DONE_PATTERNS:
            what = f"GAE T={T} N={N} {pat}"
            x = R.gae_grid_inputs(T, N, 7 * N + T, pat)
            r64, a64 = R.gae_ref(*x, 0.5, 0.5)
            t, g = _gae_local(x, 0.5, 0.5)
            adv, mom = g["adv"].got().clone(), g["mom"].v.clone()
            R.check_gae_exact(g["ret"].got().cpu().numpy(), adv.cpu().numpy(), mom.cpu().numpy(), r64, a64, what)
            m = R.moments_ref(a64)
            n2 = _normalize(adv, mom * 2)
            worst = max(worst, R.check_normalized(n2.cpu().numpy().reshape(T, N), a64, 2 * m, what + " doubled moments"))
            st, gf = _gae_full(t, T, N, 0.5, 0.5)
            if T * N < 2:
                assert st == -1, "pmlp_gae must refuse T N < 2"
                assert all((b.all_sentinel() if isinstance(b, Band) else bool((b.flat == b.sentinel).all()))
                           for b in gf.values())
                continue
            assert st == 0
            n1 = _normalize(adv, mom)
            worst = max(worst, R.check_normalized(n1.cpu().numpy().reshape(T, N), a64, m, what + " own moments"))
            for k in ("ret", "adv"):
                gf[k].assert_untouched(what + " pmlp_gae " + k)
            gf["partial"].untouched(what + " pmlp_gae partial")
            assert R.same_bits(gf["ret"].got().contiguous(), g["ret"].got().contiguous()), what + ": pmlp_gae returns"
            assert R.same_bits(gf["adv"].got().contiguous().reshape(-1), n1), what + ": pmlp_gae != local + normalize"
    _show(f"GAE normalise T={T}", dict(norm=worst))


@pytest.mark.parametrize("N", [257, 333])
def test_gae_realistic_case_within_four_times_the_float32_recursion(N):
    """T = 24, gamma 0.99, lam 0.95, normal data: the recursion is sequential, so only contraction
    and the grouping of operations can differ from a float32 numpy run; 4 x its error against
    float64 covers a regrouped chain of this length."""
    T = 24
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((T, N)).astype(np.float32), (rng.random((T, N)) < 0.1).astype(np.uint8),
         rng.standard_normal((T, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    r64, a64 = R.gae_ref(*x, 0.99, 0.95)
    r32, a32 = R.gae_ref(*x, 0.99, 0.95, dtype=np.float32)
    e32 = max(np.abs(r32 - r64).max(), np.abs(a32 - a64).max())
    _, g = _gae_local(x, 0.99, 0.95)
    ret, adv = g["ret"].got().cpu().numpy(), g["adv"].got().cpu().numpy()
    eg = max(np.abs(ret - r64).max(), np.abs(adv - a64).max())
    print(f"[ppo-ref] GAE realistic N={N}: float32 numpy vs float64 {e32:.3g}, kernel vs float64 {eg:.3g}")
    assert eg <= 4 * e32, (eg, e32)
    m = R.moments_ref(adv)   # double sums of the kernel's own advantages, in another order
    tol = adv.size * 2.0 ** -53 * np.array([np.abs(adv).sum(dtype=np.float64), m[1], 0.0])
    assert (np.abs(g["mom"].v.cpu().numpy() - m) <= tol).all()
    n1 = _normalize(g["adv"].got().clone(), g["mom"].v)
    R.check_normalized(n1.cpu().numpy().reshape(T, N), adv.astype(np.float64), g["mom"].v.cpu().numpy(), "realistic")


# ----------------------------------------------------------------------- Adam --
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
CLIPPED, UNCLIPPED = 2.0 ** -12, 2.0 ** 12


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _sent_bf():
    return np.uint16(torch.tensor([R.SENTINEL], dtype=BF).view(torch.int16).numpy().view(np.uint16)[0])


class AdamState:
    def __init__(self, p0, off):
        n = p0.size
        self.n, self.off = n, off
        self.b = {k: Band(n, F32, off) for k in ("p", "g", "m", "v")}
        self.b["p"].v.copy_(torch.from_numpy(p0))
        self.b["m"].v.zero_()
        self.b["v"].v.zero_()
        self.step = torch.zeros(1, device=DEV)
        self.lr = torch.tensor([LR], device=DEV)
        self.part = Band(mm.load().pmlp_opt_parts())

    def run(self, g, scale, max_norm, mirrors=(), partial=None, entry="mirror_n"):
        L = mm.load()
        s = mm._stream()
        self.b["g"].v.copy_(torch.from_numpy(g))
        b = self.b
        if partial is None:
            mm._ok(L.pmlp_opt_prepare(P(b["g"].v), self.n, scale, P(self.part.v), P(self.step), None, P(self.lr), None,
                                      0.0, 0, s), "pmlp_opt_prepare")
            part, nparts = self.part.v, self.part.n
        else:
            self.step += 1
            part, nparts = partial, partial.numel()
        arr = (mm.MirrorJob * max(len(mirrors), 1))(*[mm.MirrorJob(o, r, c, ld, P(dst), P(fr))
                                                     for o, r, c, ld, dst, fr in mirrors])
        if entry == "adam":
            mm._ok(L.pmlp_adam(P(b["p"].v), P(b["g"].v), P(b["m"].v), P(b["v"].v), self.n, scale, P(part), P(self.step),
                               P(self.lr), max_norm, B1, B2, EPS, s), "pmlp_adam")
        else:
            mm._ok(L.pmlp_adam_mirror_n(P(b["p"].v), P(b["g"].v), P(b["m"].v), P(b["v"].v), self.n, scale, P(part),
                                        nparts, P(self.step), P(self.lr), max_norm, B1, B2, EPS, len(mirrors),
                                        arr if mirrors else None, s), "pmlp_adam_mirror_n")
        _sync()
        for k, x in b.items():
            x.untouched(k)
        self.part.untouched("norm partials")
        return tuple(b[k].v.cpu().numpy() for k in ("p", "m", "v"))


def _adam_data(n, seed):
    rng = np.random.default_rng(seed)
    g0 = R.adam_grid_grads(n, seed)
    return rng.standard_normal(n).astype(np.float32), [g0, g0 * np.float32(0.5), g0]


def _adam_steps(n, off, scale, max_norm, seed=3, steps=3, entry="mirror_n"):
    """`steps` steps through the kernels, each checked against adam_ref; returns the states."""
    p0, grads = _adam_data(n, seed)
    grads = grads[:steps]
    z = np.zeros(n, np.float32)
    ref = R.adam_ref(p0, z, z, grads, grad_scale=scale, max_norm=max_norm, lr=LR, b1=B1, b2=B2, eps=EPS)
    st = AdamState(p0, off)
    got, worst = [], {}
    for s, g in enumerate(grads):
        got.append(st.run(g, scale, max_norm, entry=entry))
        fr = R.check_adam(*got[-1], ref[s], f"n={n} off={off} scale={scale} max_norm={max_norm} step {s + 1}")
        for k, v in fr.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert float(st.step) == steps
    return got, ref, worst


ADAM_ARMS = [("vec4", 0, n) for n in R.ADAM_VEC4_N] + [("vec2", 2, 4099), ("vec2", 2, 4100),
                                                       ("scalar", 1, 4099), ("scalar", 1, 4100)]


@pytest.mark.parametrize("arm,off,n", ADAM_ARMS)
def test_adam_arm_matches_fp64_and_the_other_arms(arm, off, n):
    worst = {}
    for scale in (1.0, 0.5):
        for max_norm, clipped in ((CLIPPED, True), (UNCLIPPED, False), (0.0, False)):
            got, ref, w = _adam_steps(n, off, scale, max_norm)
            assert all(r["clipped"] == clipped for r in ref)
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if arm != "scalar" and scale == 0.5 and max_norm == CLIPPED:
                # the kernel comment's claim: per element the bits of the scalar kernel
                sc, _, _ = _adam_steps(n, 1, scale, max_norm)
                for a, b in zip(got, sc):
                    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), \
                        f"{arm} differs from the scalar kernel"
    _show(f"Adam {arm} n={n}", worst)


def test_adam_scalar_grid_stride_past_the_block_cap():
    _, _, w = _adam_steps(R.ADAM_SCALAR_CAP_N, 1, 0.5, CLIPPED, steps=2)
    _show("Adam scalar past the cap", w)
    _, _, w = _adam_steps(R.ADAM_SCALAR_CAP_N, 0, 1.0, UNCLIPPED, steps=1, entry="adam")
    _show("pmlp_adam past the cap", w)


def test_adam_vec4_reload_path():
    _, _, w = _adam_steps(R.ADAM_RELOAD_N, 0, 1.0, CLIPPED, steps=1)
    _show("Adam vec4 reload", w)


@pytest.mark.parametrize("nparts", [1, 7, 300])
def test_adam_mirror_n_takes_any_count_of_norm_partials(nparts):
    n, scale = 4099, 0.5
    p0, grads = _adam_data(n, 3)
    z = np.zeros(n, np.float32)
    ref = R.adam_ref(p0, z, z, grads[:1], grad_scale=scale, max_norm=CLIPPED, lr=LR, b1=B1, b2=B2, eps=EPS)
    a = AdamState(p0, 0)
    base = a.run(grads[0], scale, CLIPPED)
    S = ref[0]["sumsq"]
    u = 2.0 ** -16                       # every scaled square is a multiple of 2^-16
    assert S / u == round(S / u) and S > nparts * u
    hand = Band(nparts)
    hand.v.fill_(u)
    hand.v[0] = S - (nparts - 1) * u
    assert float(hand.v.double().sum()) == S
    b = AdamState(p0, 0)
    got = b.run(grads[0], scale, CLIPPED, partial=hand.v)
    hand.untouched("hand-made partials")
    R.check_adam(*got, ref[0], f"nparts={nparts}")
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got, base))


def _mirror_case(offs, cols0, what):
    """Two disjoint mirror jobs per call (job 0 with a fragment-packed copy) over three steps."""
    rows0, ld0, rows1, cols1, ld1 = 40, 32, 16, 32, 40
    n = offs[1] + rows1 * cols1 + 13
    assert offs[0] + rows0 * cols0 <= offs[1]
    p0, grads = _adam_data(n, 9)
    z = np.zeros(n, np.float32)
    ref = R.adam_ref(p0, z, z, grads, grad_scale=1.0, max_norm=CLIPPED, lr=LR, b1=B1, b2=B2, eps=EPS)
    st = AdamState(p0, 0)
    dst0, frag0, dst1 = Band(rows0 * ld0, BF), Band(64 * ld0, BF), Band(rows1 * ld1, BF)
    jobs = [(offs[0], rows0, cols0, ld0, dst0.v, frag0.v), (offs[1], rows1, cols1, ld1, dst1.v, None)]
    got = []
    for s, g in enumerate(grads):
        got.append(st.run(g, 1.0, CLIPPED, mirrors=jobs))
        R.check_adam(*got[-1], ref[s], f"{what} step {s + 1}")   # parameters outside the mirrors too
        for b in (dst0, frag0, dst1):
            b.untouched(what)
        p = got[-1][0]
        R.check_mirror(_bits(dst0.v).reshape(rows0, ld0), _bits(frag0.v), p, (offs[0], rows0, cols0, ld0), _sent_bf(),
                       what + " job 0")
        R.check_mirror(_bits(dst1.v).reshape(rows1, ld1), None, p, (offs[1], rows1, cols1, ld1), _sent_bf(),
                       what + " job 1")
    return got


def test_adam_mirrors_hold_the_rounded_parameters_on_every_arm():
    v4 = _mirror_case((8, 1000), 24, "vec4 mirrors")          # offsets, widths, strides multiples of 4
    v2 = _mirror_case((10, 1000), 24, "vec2 mirrors")         # an offset that is a multiple of 2 only
    sc = _mirror_case((8, 1000), 23, "scalar mirrors")        # odd cols
    for a, b, c in zip(v4, v2, sc):
        for x, y, w in zip(a, b, c):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "the mirror offset changed the results"
            assert np.array_equal(x.view(np.uint32), w.view(np.uint32)), "the mirror width changed the results"


# -------------------------------------------------------------------- KL rule --
def _kl_cases():
    return [(float(kl), lr) for kl in R.kl_table() for lr in R.LR_TABLE]


S0, S1, ACC0 = 0.375, 1.25, (2.0, 3.0)


def _kl_expect(kl, lr, adaptive, acc, scale=1.0, stats_scale=1.0):
    f = np.float32
    stats = [f(S0) * f(stats_scale), f(S1) * f(stats_scale), f(kl) * f(stats_scale), f(0)]
    return R.bookkeeping_ref(stats, lr, ACC0 if acc else None, R.DESIRED_KL, adaptive, scale)


@pytest.mark.parametrize("copy", ["pmlp_loss_bookkeeping", "pmlp_opt_prepare", "pmlp_reduce_slabs_step"])
def test_kl_rule_at_its_thresholds(copy):
    L = mm.load()
    s = mm._stream()
    cases = [(kl, lr, 1, True) for kl, lr in _kl_cases()] + [(float(R.kl_table()[1]), 1e-3, 0, True),
                                                             (float(R.kl_table()[3]), 1e-3, 1, False)]
    n = len(cases)
    A, M = 4, 64
    mult = {"pmlp_loss_bookkeeping": 1.0, "pmlp_opt_prepare": 2.0, "pmlp_reduce_slabs_step": float(M)}[copy]
    stats = torch.zeros(n, 3 + A, device=DEV)
    for i, (kl, lr, ad, acc) in enumerate(cases):
        stats[i, :3] = torch.tensor([S0, S1, kl], dtype=F64).to(F32) * mult   # (power-of-two factors: exact)
    assert all(float(stats[i, 2]) == float(np.float32(c[0])) * mult for i, c in enumerate(cases))
    lrs = Band(n)
    lrs.v.copy_(torch.tensor([c[1] for c in cases]))
    accs = Band(2 * n)
    accs.v.copy_(torch.tensor(ACC0).repeat(n))
    steps = Band(n)
    steps.v.fill_(3.0)
    std = torch.ones(A, device=DEV)
    grad, part = torch.ones(8, device=DEV), torch.empty(L.pmlp_opt_parts(), device=DEV)
    for i, (kl, lr, ad, acc) in enumerate(cases):
        a = accs.v[2 * i:2 * i + 2] if acc else None
        if copy == "pmlp_loss_bookkeeping":
            mm._ok(L.pmlp_loss_bookkeeping(P(stats[i]), P(lrs.v[i:]), P(a), R.DESIRED_KL, ad, s), copy)
        elif copy == "pmlp_opt_prepare":
            mm._ok(L.pmlp_opt_prepare(P(grad), 8, 0.5, P(part), P(steps.v[i:]), P(stats[i]), P(lrs.v[i:]), P(a),
                                      R.DESIRED_KL, ad, s), copy)
        else:
            st, _, _, _, nparts, _ = _reduce_step(stats[i], 1, A, M, std, 4, steps.v[i:], lrs.v[i:], a, R.DESIRED_KL, ad)
            assert nparts == 2 and float(st[2]) == float(np.float32(kl))
    _sync()
    for b in (lrs, accs, steps):
        b.untouched(copy)
    scale = 0.5 if copy == "pmlp_opt_prepare" else 1.0
    for i, (kl, lr, ad, acc) in enumerate(cases):
        want_lr, want_acc = _kl_expect(kl, lr, ad, acc, scale, 2.0 if copy == "pmlp_opt_prepare" else 1.0)
        got_lr = lrs.v[i].cpu().numpy()
        assert got_lr == want_lr, f"{copy}: kl={kl!r} lr={lr!r} adaptive={ad}: lr {got_lr!r} != {want_lr!r}"
        got_acc = accs.v[2 * i:2 * i + 2].cpu().numpy().tolist()
        assert got_acc == ([float(x) for x in want_acc] if acc else list(ACC0)), (copy, kl, lr, got_acc, want_acc)
        if copy != "pmlp_loss_bookkeeping":
            assert float(steps.v[i]) == 4.0
