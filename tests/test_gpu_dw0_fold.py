"""The first layer's weight gradient formed inside layer 1's input-gradient tiles
(pmlp_gemm_pair_dw0, csrc/ppo_mlp.hip): bitwise the two launches it replaces (pmlp_gemm_pair,
then pmlp_gemm(PARTIAL_TN) on the stored input gradient), within the fp32 accumulation bound of
the fp64 products on its own, the fall-through for shapes it does not take, and the optimizer
step with the fold on and off.

Shapes are the smallest that reach every index of the folded tile: slabs of two and three
128-row tiles (more than one tile per workgroup, more than one slab), one and two 128-wide
column tiles, one and two 64-deep k-tiles of the input gradient, first-layer widths of 16, 48
and 56 (the bias column in the first and in the second 32-column block of the slab piece,
column quads cut by N), one job and two unlike jobs, the input gradient stored and not."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.modules import mfma_mlp  # noqa: E402

import gemm_ref as R  # noqa: E402

DEV = "cuda"
PT = mfma_mlp.EPI_PARTIAL_TN
F32, BF = torch.float32, torch.bfloat16
KS1 = 256  # rows per slab of layer 1's own weight gradient


def _case(M, width, depth, k0ps, seed):
    """Layer 1's backward (dz2 [M, depth] through W1 [depth, width], ELU'(y0)) and the first
    layer's inputs xb [M, k0p], one set per job, on the exact grids of gemm_ref."""
    g = R.gen(seed, DEV)
    return [dict(dz2=R.grid_act((M, depth), g, DEV), w1=R.grid_weight((depth, width), depth, g, DEV),
                 y0=R.grid_yprev((M, width), g, DEV), xb=R.grid_weight((M, k0p), 128, g, DEV), k0p=k0p)
            for k0p in k0ps]


def _outputs(case, M, width, depth, ks0, with_cb, pad=8):
    S1, S0 = (M + KS1 - 1) // KS1, (M + ks0 - 1) // ks0
    return [dict(cf1=R.Guarded(depth, width, width + 8, F32, DEV, slabs=S1),
                 cf0=R.Guarded(width, c["k0p"], c["k0p"] + pad, F32, DEV, slabs=S0),
                 cb=R.Guarded(M, width, width + 8, BF, DEV) if with_cb else None) for c in case]


def _jobs(case, outs, M, width, depth):
    jw = [dict(A=c["dz2"], B=c["y0"], M=depth, N=width, K=M, cf=o["cf1"].t, sum_col=width) for c, o in zip(case, outs)]
    jx = [dict(A=c["dz2"], B=c["w1"], b_kn=1, M=M, N=width, K=depth, yprev=c["y0"],
               cb=None if o["cb"] is None else o["cb"].mat) for c, o in zip(case, outs)]
    j0 = [dict(B=c["xb"], M=width, N=c["k0p"], K=M, cf=o["cf0"].t, sum_col=c["k0p"]) for c, o in zip(case, outs)]
    return jw, jx, j0


def _two_launches(case, M, width, depth, ks0, pad=8):
    """The reference of the bitwise comparisons: pmlp_gemm_pair, then PARTIAL_TN on its cb."""
    outs = _outputs(case, M, width, depth, ks0, True, pad)
    jw, jx, j0 = _jobs(case, outs, M, width, depth)
    mfma_mlp._gemm_pair(jw, KS1, jx)
    mfma_mlp._gemm(PT, [dict(j, A=o["cb"].mat) for j, o in zip(j0, outs)], ksplit=ks0)
    torch.cuda.synchronize()
    return outs


def _same(outs, ref, what):
    for i, (o, r) in enumerate(zip(outs, ref)):
        for k in ("cf1", "cf0", "cb"):
            if o[k] is not None:  # (the whole buffers: the guard bands and the unwritten columns too)
                assert R.same_bits(o[k].flat, r[k].flat), f"{what}: job {i} {k} differs from the two launches"


@pytest.mark.parametrize("M,ks0", [(768, 384), (512, 256)])
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("depth", [64, 128])
def test_fold_is_bitwise_the_two_launches(M, ks0, width, depth):
    """Slabs and the sum_col column of the folded path against the two launches at the same
    ksplit, with the input gradient stored (it must be the same too) and not stored."""
    for k0ps in ((16,), (48,), (56,), (48, 16)):
        case = _case(M, width, depth, k0ps, 51000 + M + width + depth + sum(k0ps))
        ref = _two_launches(case, M, width, depth, ks0)
        for with_cb in (False, True):
            outs = _outputs(case, M, width, depth, ks0, with_cb)
            jw, jx, j0 = _jobs(case, outs, M, width, depth)
            assert mfma_mlp._gemm_pair_dw0(jw, KS1, jx, j0, ks0, plan=True)
            assert mfma_mlp._gemm_pair_dw0(jw, KS1, jx, j0, ks0) is True
            torch.cuda.synchronize()
            _same(outs, ref, f"M {M} ks {ks0} width {width} depth {depth} K0p {k0ps} cb {with_cb}")


@pytest.mark.parametrize("M,ks0,width,depth,k0ps", [(768, 384, 256, 128, (48, 16)), (512, 256, 128, 64, (56,))])
def test_fold_against_fp64(M, ks0, width, depth, k0ps):
    """On its own: the stored input gradient is the exact-grid BWD_DX result, every slab is
    within e_acc of the fp64 product of that stored gradient and xb over the slab's rows, the
    bias column within e_acc of its column sum, and nothing else is written."""
    case = _case(M, width, depth, k0ps, 52000 + M)
    outs = _outputs(case, M, width, depth, ks0, True)
    jw, jx, j0 = _jobs(case, outs, M, width, depth)
    assert mfma_mlp._gemm_pair_dw0(jw, KS1, jx, j0, ks0) is True
    torch.cuda.synchronize()
    for i, (c, o) in enumerate(zip(case, outs)):
        k0p = c["k0p"]
        o["cb"].assert_untouched(f"cb {i}")
        o["cf0"].assert_untouched(f"first-layer slabs {i}", extra_cols=(k0p,))
        o["cf1"].assert_untouched(f"layer-1 slabs {i}", extra_cols=(width,))
        dz1 = o["cb"].got()
        R.check_bwd_dx(dz1, c["dz2"], c["w1"].t(), c["y0"], f"dz1 {i}")
        R.check_partial(o["cf1"].t[:, :, :width], c["dz2"], c["y0"], KS1, o["cf1"].t[:, :, width], f"dW1 {i}")
        ones = torch.ones(1, ks0, dtype=BF, device=DEV)
        for s in range(M // ks0):
            a, x = dz1[s * ks0:(s + 1) * ks0].t(), c["xb"][s * ks0:(s + 1) * ks0].t()  # [width, rows], [k0p, rows]
            v, e = R.preact(a, x), R.e_acc(a, x)
            R.assert_between(o["cf0"].t[s, :, :k0p], v - e, v + e, f"dW0 {i} slab {s}")
            v, e = R.preact(a, ones)[:, 0], R.e_acc(a, ones)[:, 0]
            R.assert_between(o["cf0"].t[s, :, k0p], v - e, v + e, f"db0 {i} slab {s}")


@pytest.mark.parametrize("M,ks0,k0p,pad", [(700, 384, 48, 8), (640, 320, 48, 8), (768, 384, 64, 8)])
def test_other_shapes_take_the_two_launches(M, ks0, k0p, pad):
    """Rows that are no whole slabs, a slab extent that is no multiple of 128 and a slab wider
    than 64 floats (72) run pmlp_gemm_pair and the PARTIAL_TN launch, and say so: the same
    results, nothing written outside them."""
    width, depth = 128, 64
    case = _case(M, width, depth, (k0p,), 53000 + M)
    ref = _two_launches(case, M, width, depth, ks0, pad)
    outs = _outputs(case, M, width, depth, ks0, True, pad)
    jw, jx, j0 = _jobs(case, outs, M, width, depth)
    assert outs[0]["cf0"].ld == (72 if k0p == 64 else 56)
    assert not mfma_mlp._gemm_pair_dw0(jw, KS1, jx, j0, ks0, plan=True)
    assert mfma_mlp._gemm_pair_dw0(jw, KS1, jx, j0, ks0) is False
    torch.cuda.synchronize()
    _same(outs, ref, f"M {M} ks {ks0} K0p {k0p}")
    outs[0]["cb"].assert_untouched("cb")
    outs[0]["cf0"].assert_untouched("first-layer slabs", extra_cols=(k0p,))
    outs[0]["cf1"].assert_untouched("layer-1 slabs", extra_cols=(width,))
    with pytest.raises(RuntimeError, match="cb"):  # the two launches cannot do without the stored gradient
        mfma_mlp._gemm_pair_dw0(jw, KS1, [dict(j, cb=None) for j in jx], j0, ks0)


def test_optimizer_step_is_bitwise_with_the_fold_on_and_off(monkeypatch):
    """Two optimizer steps (mini-batches of 768 rows) of a 48-input 512-256-128 pair from the
    same weights and rollout with PMLP_DW0_FOLD 1 and 0, at the same slab extents: the
    parameters, Adam's moments and the loss statistics are bitwise equal."""
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCritic

    torch.manual_seed(0)
    N, T, O, A = 192, 8, 48, 12
    ac0 = ActorCritic(O, O, A, [512, 256, 128], [512, 256, 128]).cuda()
    algs = []
    for fold in ("1", "0"):
        monkeypatch.setenv("PMLP_DW0_FOLD", fold)
        alg = PPO(copy.deepcopy(ac0), num_learning_epochs=1, num_mini_batches=2, learning_rate=1e-3, device="cuda")
        alg.init_storage(N, T, [O], [None], [A])
        f = alg._fused
        assert f is not None and f.M == 768 and f.dw0_fold == (fold == "1")
        assert (f.dz[0][1] is None) == f.dw0_fold
        algs.append(alg)
    assert algs[0]._fused.ks == algs[1]._fused.ks
    g = torch.Generator(device=DEV).manual_seed(5)
    st = algs[0].storage
    st.observations.copy_(torch.randn(st.observations.shape, device=DEV, generator=g))
    st.actions.copy_(torch.randn(st.actions.shape, device=DEV, generator=g))
    st.mu.copy_(st.actions + 0.3 * torch.randn(st.actions.shape, device=DEV, generator=g))
    st.sigma.fill_(1.0)
    st.actions_log_prob.copy_(-torch.rand(st.actions_log_prob.shape, device=DEV, generator=g) * A)
    for name in ("values", "returns", "advantages"):
        getattr(st, name).copy_(torch.randn(getattr(st, name).shape, device=DEV, generator=g))
    for k, v in st.__dict__.items():
        if torch.is_tensor(v) and not k.startswith("_"):
            getattr(algs[1].storage, k).copy_(v)
    for alg in algs:
        alg.storage.step = T
        torch.manual_seed(7)
        alg.update()
    torch.cuda.synchronize()
    a, b = algs[0]._fused, algs[1]._fused
    assert float(a.step_t) == 2.0 and float(b.step_t) == 2.0
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert R.same_bits(getattr(a, name), getattr(b, name)), name
    assert R.same_bits(a.grad[a.n:].contiguous(), b.grad[b.n:].contiguous()), "statistics tail"
    assert bool(a.exp_avg.abs().max() > 0)
