"""The checks of tests/ppo_ref.py are themselves tested (CPU): a float32 evaluation of each
statement, written out by hand as the kernels do it, passes the comparison functions that
tests/test_gpu_ppo_reference.py applies to the kernels, and deliberately wrong outputs -- the
mistakes a hand-kept copy of this arithmetic can make -- are rejected by the same functions.
The input conditions (the 2 % cap on rows left out, the quadrant counts, the exactness of the
GAE and Adam grids) are asserted for every case the GPU file runs."""
import math

import numpy as np
import pytest
import torch

import ppo_ref as R

f = np.float32
BF = torch.bfloat16


# ------------------------------------------------------------------------ loss --
def eval32(inp, cv=1, vcoef=0.5, ecoef=0.01, gout=1.0, Ap=None, Vp=8, mut=""):
    """The loss statement and its gradient in numpy float32, operation for operation as
    k_ppo_loss_step writes it; `mut` plants one mistake."""
    n = lambda t: t.numpy().astype(f)  # noqa: E731
    mu, std, value = n(inp["mu"]), n(inp["std"]), n(inp["value"])
    M, A = mu.shape
    Ap = A if Ap is None else Ap
    idx = np.arange(M) if (inp["rows"] is None or mut == "rows") else inp["rows"].numpy()
    act, om, os_ = (n(inp[k])[idx] for k in ("act", "old_mu", "old_sigma"))
    olp, adv, ret, tgt = (n(inp[k])[idx] for k in ("old_logp", "adv", "ret", "target"))
    clip, lo, hi = f(R.CLIP), f(1 - R.CLIP), f(1 + R.CLIP)
    vcoef, ecoef, gout, c = f(vcoef), f(ecoef), f(gout), f(R.HALF_LOG_2PI)
    d = act - mu
    logp = np.zeros(M, f)
    kl = np.zeros(M, f)
    for k in range(A):
        logp += -(d[:, k] * d[:, k]) / (f(2) * std[k] * std[k]) - np.log(std[k]) - c
        x = std[k] / os_[:, k] + (f(0) if mut == "kl_eps" else f(1e-5))
        kl += np.log(x) + (os_[:, k] ** 2 + (om[:, k] - mu[:, k]) ** 2) / (f(2) * std[k] * std[k]) - f(0.5)
    ratio = np.exp(logp - olp)
    s1, s2 = -adv * ratio, -adv * np.clip(ratio, lo, hi)
    w1 = np.where(s1 > s2, f(1), np.where(s1 == s2, f(0.5), f(0)))
    w2 = np.where(s2 > s1, f(1), np.where(s1 == s2, f(0.5), f(0)))
    dcl = ((ratio >= lo) & (ratio <= hi)).astype(f)
    Mk = (M + 63) // 64 * 64 if mut == "m64" else M
    gs, gv = gout / f(Mk), gout * vcoef / f(Mk)
    dlogp = gs * (-adv) * (w1 + w2 * dcl) * ratio
    sg_g = np.roll(std, 1) if mut == "sigma" else std
    dmu = dlogp[:, None] * d / (sg_g * sg_g)[None, :]
    x1 = value - ret
    if cv and mut != "unclipped":
        vc = tgt + np.clip(value - tgt, -clip, clip)
        x2 = vc - ret
        a, b = x1 * x1, x2 * x2
        vl = np.maximum(a, b)
        if mut == "tie":
            u1, u2 = (a >= b).astype(f), (b > a).astype(f)
        else:
            u1 = np.where(a > b, f(1), np.where(a == b, f(0.5), f(0)))
            u2 = np.where(b > a, f(1), np.where(a == b, f(0.5), f(0)))
        vt = value - tgt
        dcv = ((vt > -clip) & (vt < clip)) if mut == "edge" else ((vt >= -clip) & (vt <= clip))
        dv = gv * (u1 * f(2) * x1 + u2 * f(2) * x2 * dcv.astype(f))
    else:
        vl = x1 * x1
        dv = gv * f(2) * x1
    dstd = np.array([np.sum(dlogp * (d[:, k] ** 2 / std[k] ** 3 - f(1) / std[k]), dtype=f) for k in range(A)], f)
    if mut != "no_entropy":
        dstd = dstd - ecoef * gout / std
    ent = np.sum(f(0.5) + c + np.log(std), dtype=f)
    inv = f(1) / f(M)
    surr, vlm = np.sum(np.maximum(s1, s2), dtype=f) * inv, np.sum(vl, dtype=f) * inv
    stats = np.array([surr, vlm, np.sum(kl, dtype=f) * inv, ent], f)
    t = torch.from_numpy
    dmu_b = torch.zeros(M, Ap, dtype=BF)
    dmu_b[:, :A] = t(dmu).to(BF)
    dv_b = torch.zeros(M, Vp, dtype=BF)
    dv_b[:, 0] = t(dv).to(BF)
    if mut == "pad" and Ap > A:
        dmu_b[:, A] = dmu_b[:, A - 1]
    dmu_t = dmu_b.reshape(Ap, M).clone() if mut == "untransposed" else dmu_b.t().contiguous()
    return dict(dmu=dmu_b, dv=dv_b, dmu_t=dmu_t, dv_t=dv_b.t().contiguous(), stats=t(stats), dstd=t(dstd),
                dmu32=t(dmu), dv32=t(dv), loss=t(np.array(surr + vcoef * vlm - ecoef * ent, f)))


def _f32_out(o):
    return dict(dmu=o["dmu32"], dv=o["dv32"], stats=o["stats"], dstd=o["dstd"], loss=o["loss"])


HOST_CASES = [(257, 12, 16, True, 1), (65, 10, 16, False, 1), (517, 20, 24, True, 0), (37, 4, 8, True, 1),
              (101, 12, 16, True, 1)]


@pytest.mark.parametrize("M,A,Ap,rows,cv", HOST_CASES)
def test_float32_evaluation_passes_the_loss_checks(M, A, Ap, rows, cv):
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), rows)
    for gout in (1.0, 0.5):
        ref = R.loss_ref(inp, clipped_value=cv, gout=gout)
        o = eval32(inp, cv=cv, gout=gout, Ap=Ap)
        fr = R.check_loss_f32(_f32_out(o), ref, f"host M={M} A={A}")
        if gout == 1.0:
            fr.update(R.check_loss_step(o, ref, f"host M={M} A={A}"))
        # a correct float32 evaluation sits well inside the derived bounds (dvalue: the grid rows'
        # bound is two roundings, which two roundings can nearly fill)
        assert max(v for k, v in fr.items() if k != "dvalue") < 0.5, fr


def test_grid_rows_take_the_stated_branches():
    """loss_ref on the rows of edge_rows(): the value gradient is the stated multiple of
    vcoef / M (torch's tie and clamp conventions), the adv = 0 rows give 0, not NaN."""
    M, A = 64, 4
    inp = R.loss_inputs(M, A, 5, True)
    ref = R.loss_ref(inp, clipped_value=1, vcoef=0.5)
    assert int(inp["grid"].sum()) == R.N_EDGE and bool(inp["grid"][-R.N_EDGE:].all())
    for j, (v, t, r, a0, sh, c) in enumerate(R.edge_rows()):
        i = M - R.N_EDGE + j
        if c is not None:
            assert float(ref["dvalue"][i]) == 0.5 / M * c, (j, float(ref["dvalue"][i]) * M / 0.5, c)
        if a0 is not None:
            assert bool((ref["dmu"][i] == 0).all()) and abs(float(ref["diag"]["ratio"][i]) - 1) > 0.5
    un = R.loss_ref(inp, clipped_value=0, vcoef=0.5)
    g = inp["gridv"]
    want = 0.5 / M * 2 * (inp["value"].double() - inp["ret"][inp["rows"]].double())
    assert torch.equal(un["dvalue"][g], want[g])


LOSS_MUTATIONS = ["m64", "sigma", "kl_eps", "tie", "edge", "pad", "untransposed", "rows", "no_entropy", "unclipped"]


@pytest.mark.parametrize("mut", LOSS_MUTATIONS)
def test_wrong_loss_outputs_are_rejected(mut):
    M, A, Ap = 257, 12, 16
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), True)
    ref = R.loss_ref(inp, clipped_value=1)
    R.check_loss_step(eval32(inp, Ap=Ap), ref, "unmutated")
    with pytest.raises(AssertionError):
        R.check_loss_step(eval32(inp, Ap=Ap, mut=mut), ref, mut)
    if mut not in ("pad", "untransposed"):  # the fp32 form has neither padding nor a transpose
        with pytest.raises(AssertionError):
            R.check_loss_f32(_f32_out(eval32(inp, Ap=Ap, mut=mut)), ref, mut)


@pytest.mark.parametrize("mut", ["tie", "edge"])
def test_branch_mistakes_are_caught_by_the_grid_rows_alone(mut):
    """Random rows never sit on a tie or a clamp edge: only the grid rows see these."""
    M, A = 64, 4
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), False)
    ref = R.loss_ref(inp, clipped_value=1)
    o = eval32(inp, mut=mut)
    bad = (o["dv32"].double() - ref["dvalue"]).abs() > 1e-6
    assert bool(bad.any()) and bool((bad <= inp["gridv"]).all())
    with pytest.raises(AssertionError):
        R.check_loss_step(o, ref, mut)


def test_input_conditions_hold_for_every_gpu_loss_case():
    cases = R.loss_cases()
    assert len(cases) > 60
    for M, A, seed, rows, cv in cases:
        inp = R.loss_inputs(M, A, seed, rows)          # (asserts the quadrant counts for M >= 128)
        ref = R.loss_ref(inp, clipped_value=cv)
        R.assert_ambiguous_cap(ref, f"M={M} A={A} seed={seed}")
        assert int(inp["grid"].sum()) == min(R.N_EDGE, M - 1)
        if M >= 128:
            assert min(R.quadrants(inp)) >= 2
    for _, A, Ap in R.LOSS_ARMS:
        assert R.loss_arm(A, Ap) == _


def test_forward_loss_case_meets_the_cap():
    """The M = 18469 case of the loss inside the forward: its mu and value come from the launch,
    so the cap is asserted there again; here on the builder's own mu / value."""
    inp = R.loss_inputs(R.FWD_LOSS_M, 12, R.loss_seed(R.FWD_LOSS_M, 12), True)
    R.assert_ambiguous_cap(R.loss_ref(inp), "forward loss")


# ------------------------------------------------------------------------- GAE --
def _gae32(rew, done, val, last, gamma, lam, mut=""):
    T, N = rew.shape
    ret, adv = np.zeros((T, N), f), np.zeros((T, N), f)
    a = np.zeros(N, f)
    g, l = f(gamma), f(lam)
    for t in range(T - 1, -1, -1):
        if mut == "last_t2":
            nxt = last if t == T - 2 else val[min(t + 1, T - 1)]
        else:
            nxt = last if t == T - 1 else val[t + 1]
        nt = f(1) - (done[t] != 0).astype(f)
        boot = f(g) * nxt if mut == "no_cut" else (nt * g) * nxt
        a = (rew[t] + boot - val[t]) + ((nt * g) * l) * a
        ret[t] = a + val[t]
        adv[t] = ret[t] - val[t]
    return ret, adv


def _norm32(adv, moments, mut=""):
    s, ss, c = moments
    if mut == "per_env":
        mean = adv.astype(np.float64).mean(0, keepdims=True)
    else:
        mean = s / c
    var = (ss - c * (s / c) ** 2) / (c if mut == "biased" else c - 1.0)
    den = f(math.sqrt(max(var, 0.0))) + f(1e-8)
    return ((adv - mean.astype(f) if mut == "per_env" else adv - f(mean)) / den).astype(f)


@pytest.mark.parametrize("T", [1, 2, 7, 8])
def test_gae_grid_is_exact_in_float32(T):
    """The exactness claim of gae_grid_inputs: the float32 recursion equals the float64 one, and
    the moments are exact doubles, for every (N, pattern) the GPU file runs."""
    for N in R.GAE_N:
        for pat in R.DONE_PATTERNS:
            x = R.gae_grid_inputs(T, N, 7 * N + T, pat)
            r64, a64 = R.gae_ref(*x, 0.5, 0.5)
            r32, a32 = R.gae_ref(*x, 0.5, 0.5, dtype=np.float32)
            R.check_gae_exact(r32, a32, R.moments_ref(a32), r64, a64, f"T={T} N={N} {pat}")
            assert np.array_equal(a64 * 2.0 ** 20, np.round(a64 * 2.0 ** 20))  # <= 20 fraction bits
            if T * N >= 2:
                R.check_normalized(_norm32(a32, R.moments_ref(a64)), a64, R.moments_ref(a64), "normalise")
                R.check_normalized(_norm32(a32, 2 * R.moments_ref(a64)), a64, 2 * R.moments_ref(a64), "doubled")


@pytest.mark.parametrize("mut", ["no_cut", "last_t2"])
def test_wrong_gae_recursions_are_rejected(mut):
    x = R.gae_grid_inputs(7, 65, 3, "random")
    r64, a64 = R.gae_ref(*x, 0.5, 0.5)
    r32, a32 = _gae32(*x, 0.5, 0.5)
    R.check_gae_exact(r32, a32, R.moments_ref(a32), r64, a64, "unmutated")
    rm, am = _gae32(*x, 0.5, 0.5, mut=mut)
    with pytest.raises(AssertionError):
        R.check_gae_exact(rm, am, R.moments_ref(am), r64, a64, mut)


def test_cut_at_the_last_step_is_seen_by_its_pattern():
    """Dones only at t = T - 1 cut last_values off: a recursion that ignores the done there is
    rejected by that pattern."""
    x = R.gae_grid_inputs(2, 64, 11, "last")
    r64, a64 = R.gae_ref(*x, 0.5, 0.5)
    rm, am = _gae32(*x, 0.5, 0.5, mut="no_cut")
    with pytest.raises(AssertionError):
        R.check_gae_exact(rm, am, None, r64, a64, "no_cut")


@pytest.mark.parametrize("mut", ["biased", "per_env"])
def test_wrong_normalisations_are_rejected(mut):
    x = R.gae_grid_inputs(7, 63, 5, "random")
    _, a64 = R.gae_ref(*x, 0.5, 0.5)
    mom = R.moments_ref(a64)
    a32 = a64.astype(f)
    R.check_normalized(_norm32(a32, mom), a64, mom, "unmutated")
    with pytest.raises(AssertionError):
        R.check_normalized(_norm32(a32, mom, mut), a64, mom, mut)


# ------------------------------------------------------------------------ Adam --
def _adam32(p, m, v, grads, scale, max_norm, lr, b1=0.9, b2=0.999, eps=1e-8, mut=""):
    """adam_elem and k_adam's coefficients in numpy float32 (fma as a double product rounded once)."""
    p, m, v = (np.asarray(x, f).copy() for x in (p, m, v))
    b1, b2, eps, lr, scale, max_norm = f(b1), f(b2), f(eps), f(lr), f(scale), f(max_norm)
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f)  # noqa: E731
    out = []
    for s, g in enumerate(grads):
        t = s + 1
        sq = f(np.sum((g.astype(np.float64) * (1.0 if mut == "no_scale" else float(scale))) ** 2))
        coef = scale
        if max_norm > 0:
            coef = scale * min(max_norm / (np.sqrt(sq) + f(1e-6)), f(1))
        tb = t - 1 if mut == "bias_t1" else t
        bc1 = f(1) - f(b1 ** f(tb))
        bc2s = np.sqrt(f(1) - f(b2 ** f(tb)))
        with np.errstate(divide="ignore", invalid="ignore"):
            step = lr / bc1
            gi = g * coef
            m = fma(gi - m, f(1) - b1, m)
            v = fma(v, b2, ((f(1) - b2) * gi) * gi)
            p = fma(m / (np.sqrt(v) / bc2s + eps), -step, p)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def _adam_case(n, scale, max_norm, seed=3):
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(f)
    g0 = R.adam_grid_grads(n, seed)
    grads = [g0, g0 * f(0.5), g0]
    z = np.zeros(n, f)
    return p0, z, z, grads, dict(grad_scale=scale, max_norm=max_norm, lr=1e-3)


@pytest.mark.parametrize("max_norm,clipped", [(2.0 ** -12, True), (2.0 ** 12, False), (0.0, False)])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_float32_adam_passes_the_budgets(max_norm, clipped, scale):
    p0, m0, v0, grads, kw = _adam_case(4099, scale, max_norm)
    ref = R.adam_ref(p0, m0, v0, grads, **kw)
    got = _adam32(p0, m0, v0, grads, scale, max_norm, 1e-3)
    for s in range(3):
        assert ref[s]["clipped"] == clipped
        fr = R.check_adam(*got[s], ref[s], f"step {s + 1}")
        assert max(fr.values()) < 0.5, fr


@pytest.mark.parametrize("mut", ["no_scale", "bias_t1"])
def test_wrong_adam_coefficients_are_rejected(mut):
    p0, m0, v0, grads, kw = _adam_case(4099, 0.5, 2.0 ** -12)
    ref = R.adam_ref(p0, m0, v0, grads, **kw)
    got = _adam32(p0, m0, v0, grads, 0.5, 2.0 ** -12, 1e-3, mut=mut)
    with pytest.raises(AssertionError):
        for s in range(3):
            R.check_adam(*got[s], ref[s], mut)


def test_adam_grid_sums_are_exact_in_any_order():
    """The exactness claim of adam_grid_grads for every n the GPU file uses: each square is a
    multiple of a unit u, and the whole sum is below 2^24 u, so every partial sum of any order
    is an fp32 number.  Holds under the power-of-two grad scales and step scales too."""
    ns = R.ADAM_VEC4_N + (4099, 4100, 4101, 4102, R.ADAM_SCALAR_CAP_N, R.ADAM_RELOAD_N)
    for n in ns:
        g = R.adam_grid_grads(n, n % 1000)
        sq = g.astype(np.float64) ** 2
        u = sq.min()
        assert np.array_equal(sq / u, np.round(sq / u)) and sq.sum() / u <= 2.0 ** 24, n
        assert f(sq.sum()) == sq.sum()
        rng = np.random.default_rng(0)
        for _ in range(2 if n < 10 ** 6 else 0):
            assert float(np.cumsum(rng.permutation(g * g), dtype=f)[-1]) == sq.sum()


def test_mirror_and_fragment_checks():
    rows, cols, ld, off = 40, 24, 32, 8
    rng = np.random.default_rng(1)
    p = rng.standard_normal(off + rows * cols + 5).astype(f)
    sent = np.uint16(0xC641)
    want = R.bf16_bits_rne(p[off:off + rows * cols]).reshape(rows, cols)
    # the restated index agrees with the packing the forward reads (rsl_rl.modules.mfma_mlp.frag_pack)
    from rsl_rl.modules import mfma_mlp
    w = torch.arange(64 * ld, dtype=torch.float32).reshape(64, ld)
    packed = mfma_mlp.frag_pack(w, 64).numpy()
    r, c = np.divmod(np.arange(64 * ld), ld)
    assert np.array_equal(packed[R.frag_index_ref(r, c, ld)], w.numpy().reshape(-1))
    assert torch.equal(torch.from_numpy(want.astype(np.int16)).view(BF),
                       torch.from_numpy(p[off:off + rows * cols]).to(BF).reshape(rows, cols))

    def build(trunc=False, swap=False):
        dst = np.full((rows, ld), sent, np.uint16)
        bits = (p[off:off + rows * cols].view(np.uint32) >> 16).astype(np.uint16).reshape(rows, cols) if trunc else want
        dst[:, :cols] = bits
        frag = np.full(64 * ld, sent, np.uint16)
        r, c = np.divmod(np.arange(rows * cols), cols)
        frag[R.frag_index_ref(r, (c ^ 8) if swap else c, ld)] = bits.reshape(-1)
        return dst, frag

    job = (off, rows, cols, ld)
    R.check_mirror(*build(), p, job, sent, "unmutated")
    for kw in (dict(trunc=True), dict(swap=True)):
        with pytest.raises(AssertionError):
            R.check_mirror(*build(**kw), p, job, sent, str(kw))
    dst, frag = build()
    dst[3, cols] = 0
    with pytest.raises(AssertionError):
        R.check_mirror(dst, frag, p, job, sent, "guard column")


# --------------------------------------------------------------------- KL rule --
def _rule(kl, lr, desired, mut=""):
    kl, lr, desired = f(kl), f(lr), f(desired)
    up = kl >= desired * f(2) if mut == "ge" else kl > desired * f(2)
    if up:
        lr = lr / f(1.5) if mut == "no_clamp" else max(lr / f(1.5), f(1e-5))
    elif kl < desired / f(2) and (mut == "no_guard" or kl > 0):
        lr = lr * f(1.5) if mut == "no_clamp" else min(lr * f(1.5), f(1e-2))
    return f(lr)


def _table(mut):
    return [(float(kl), lr, _rule(kl, lr, R.DESIRED_KL, mut)) for kl in R.kl_table() for lr in R.LR_TABLE]


def test_lr_rule_table_reaches_every_branch():
    got = _table("")
    assert all(out == R.lr_rule_ref(kl, lr, R.DESIRED_KL) for kl, lr, out in got)
    outs = {(kl, lr): out for kl, lr, out in got}
    kls = [float(k) for k in R.kl_table()]
    assert outs[(kls[0], 1e-3)] == f(1e-3) and outs[(kls[1], 1e-3)] == f(1e-3) / f(1.5)       # > is strict
    assert outs[(kls[2], 1e-3)] == f(1e-3) and outs[(kls[3], 1e-3)] == f(1e-3) * f(1.5)       # < is strict
    assert outs[(kls[4], 1e-3)] == f(1e-3) and outs[(kls[5], 1e-3)] == f(1e-3)                # 0, negative
    assert outs[(kls[6], 1e-3)] == f(1e-3) * f(1.5)                                           # subnormal > 0
    assert outs[(kls[1], 1.2e-5)] == f(1e-5) and outs[(kls[3], 8e-3)] == f(1e-2)              # both clamps bind


@pytest.mark.parametrize("mut", ["ge", "no_guard", "no_clamp"])
def test_wrong_lr_rules_are_rejected(mut):
    bad = [(kl, lr) for kl, lr, out in _table(mut) if out != R.lr_rule_ref(kl, lr, R.DESIRED_KL)]
    assert bad, mut
