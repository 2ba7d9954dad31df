"""fp64 references, input builders and comparison functions for the scalar half of the PPO
update: the loss kernels on the core of csrc/ppo_loss.h (pmlp_ppo_loss_fwd / _bwd / _step /
_step_f32 in csrc/ppo_loss.hip; in csrc/ppo_mlp.hip the loss epilogue of pmlp_mlp_forward_ppo_loss
and the folded finish of pmlp_reduce_slabs_step), and in csrc/ppo_mlp.hip the GAE kernels, the
Adam kernels and the three callers of the KL learning-rate rule.  Plain torch /
numpy on the CPU; tests/test_ppo_ref_host.py tests these checks themselves (a float32 CPU
evaluation passes, deliberately wrong outputs are rejected) and tests/test_gpu_ppo_reference.py
applies them to the kernels.

U = 2^-24 is one fp32 rounding (relative).  Every bound below is derived from the reference's
fp64 terms and the number formats, never from what a kernel returns.

LOSS.  loss_ref is rsl_rl v1.0.2's PPO.update statement in torch float64 autograd (torch.max
and clamp: ties split the gradient, a clamp passes it on its closed interval).  The constants
a kernel receives as floats (clip, the coefficients, the 1e-5 of the KL logarithm) enter the
reference as those float values.

Per-row gradients of mu.  g = dlogp d / sigma^2 with dlogp = -(adv / M) w ratio and
ratio = exp(logp - old_logp).  The exponent is a sum of A + 1 fp32 terms, each term a few
operations on fp32 inputs: its absolute error is at most E_i = (A + 8) 2^-23 S_i with
S_i = sum_k |logp term_k| + |old_logp_i|, which is the relative error it puts on the ratio;
expf, logf, 1/M, the products with adv, d and 1/sigma^2 (precomputed or divided) add a few
roundings, 16 U.  So |g - g_ref| <= |g_ref| (E_i + 16 U) + 2^-126 (the floor covers a result in
the denormal range).  A bf16 output must lie between the round-to-nearest bf16 values of the two
ends of that interval; padding must be +0 bit for bit.

Per-row gradients of the value.  With x1 = v - r, vc = t + clamp(v - t), x2 = vc - r every
difference is one rounding of its result and vc carries U (|v - t| + |vc|), so the bracket
u1 2 x1 + u2 2 x2 dcv is within 2 U (|x1| + |v - t| + |vc| + |x2|); the factor vcoef / M and
the two remaining operations are relative: |dv - dv_ref| <= (vcoef / M) 2 U (|x1| + |v - t| +
|vc| + |x2|) + 4 U |dv_ref|.  (A relative bound alone is wrong here: x2 cancels.)  On the grid
rows of edge_rows() every operation before the factor vcoef / M is exact, the factor and the
product are two roundings: |dv - dv_ref| <= 2 U |dv_ref|.

Rows left out.  A row whose fp64 ratio is within DELTA = 1e-4 of 1 -+ clip, or whose value terms
are within DELTA of a branch change (| |v - t| - clip | < DELTA, or the clamp active and
|(v - r)^2 - (vc - r)^2| < DELTA) may take the other branch in fp32: ambiguous() marks them, the
per-row comparisons skip them, at most 2 % of a batch (asserted per case).  The grid rows sit
on the branch points on purpose, are exact in fp32, and are never left out.

stats and dstd are sums over the M rows: the any-order fp32 summation bound
(ceil(log2 M) + 8) U sum_i |term_i| from the fp64 terms, plus the per-row bounds summed (the
surrogate term inherits the ratio's relative bound; a value-loss term max(x1^2, x2^2) is within
2 max|x| U (|x1| + |v - t| + |vc| + |x2|) + 2 U of itself; a row's KL, a sum of A terms
log(sigma / os + 1e-5) + (os^2 + om^2) / (2 sigma^2) - 0.5: each term's own operations are within
8 U of its pieces' magnitudes plus 3 U for the logarithm's argument, the running sum adds
(A - 1) U sum_k |term_k|: (A + 7) U sum_k (|log term| + quadratic term + 0.5) + 3 A U), divided by
M for the means.  The entropy
sum_k (0.5 + log sqrt(2 pi) + log sigma_k) gets (A + 4) ulp: (A + 4) 2^-23 sum_k |term_k|.
dstd_k = sum_i dlogp_i (d^2 / sigma^3 - 1 / sigma) - ecoef g / sigma_k: the summation bound and
the row bounds (E_i + 24 U) are taken on |dlogp_i| (d^2 / sigma^3 + 1 / sigma), which also covers
the cancellation inside the bracket; the entropy term adds 2 U of itself; an ambiguous row adds
the whole of its alternative contribution.  The loss surr + vcoef vl - ecoef ent takes the three
bounds in that combination plus 3 U of the terms' magnitudes.

GAE.  gae_ref is the recursion in numpy at a chosen precision (float64: the reference;
float32: the measured error of a realistic case).  gae_grid_inputs gives rewards, values and
last values k/4, |k| <= 8, with gamma = lam = 0.5: delta is a multiple of 1/8 below 7, the
advantage gains two fraction bits per step, so for T <= 8 it has at most 3 + 2 (T - 1) + 3
<= 20 significant bits below 8 and every fp32 operation of k_gae is exact whatever is
contracted; the squares have at most 40 bits and their double sums are exact.  The
normalisation (adv - mean) / (std + 1e-8): mean and std come from exact double moments, are
rounded once to float, the sum and the quotient round once each:
|got - ref| <= ((|adv| + |mean|) / den) 4 U.

ADAM.  adam_ref is clip_grad_norm_ + torch.optim.Adam in float64 (amsgrad off, no weight
decay) on the float values of beta1, beta2, eps and lr.  adam_grid_grads makes the squared norm
exact in fp32 in any order (magnitudes 2^-3, 2^-5, 2^-7 below 65536 elements: the squares are
multiples of 2^-14 and the sum stays below 2^10; one magnitude 2^-4 above; a power-of-two
grad_scale keeps that), so the clip coefficient's input has no summation error.  Budgets count
roundings (each at most U relative, which is below one ulp of the reference value) and are
doubled:
  coef  sqrtf, + 1e-6, the division, x scale: 4; the gradient g coef: 5.
  m     per step 1 - b1, gi - m, the fma: 3 on top of the larger of the carried error and the
        gradient's 5 (m is a convex combination of same-sign terms here: the gradient keeps its
        signs over the steps, so nothing cancels): e_m(t) = 5 + 3 t; budget 2 e_m ulp(m_ref).
  v     gi^2 carries 10; 1 - b2, two products, the fma: e_v(t) = 10 + 4 t; budget 2 e_v ulp(v_ref).
  p     the update u = step_size m / (sqrt(v) / bc2s + eps): e_m + (e_v / 2 + 1) for sqrtf(v);
        bc1 = 1 - powf(b1, t) with powf good to 1 ulp (2 U) amplified by k1 = b1^t / (1 - b1^t)
        and one rounding, the division lr / bc1: 2 k1 + 2; bc2s = sqrtf(1 - powf(b2, t)):
        k2 + 1.5 with k2 = b2^t / (1 - b2^t) (999 at t = 1: the honest cost of an fp32 bias
        correction); two divisions and the eps sum: 3.  R_u(t) = e_m + e_v / 2 + 2 k1 + k2 + 7.5,
        and |p - p_ref| <= sum over the steps so far of 2 R_u U |u_ref| + ulp(p_ref) / 2 (the
        final rounding of each step, not doubled).
The mirrors must hold exactly the round-to-nearest bf16 of the fp32 parameter the kernel wrote,
the fragment-packed copy at frag_index_ref, a separate restatement of the header's formula.

KL RULE.  lr_rule_ref is the rule in numpy float32, operation for operation; results are
compared for equality.
"""
import math

import numpy as np
import torch

from gemm_ref import SENTINEL, Guarded, round_bf16, same_bits  # noqa: F401  (shared with the GEMM anchor)

F64 = torch.float64
U = 2.0 ** -24
CLIP = 0.25          # exact in fp32; 1 - clip and 1 + clip too
DELTA = 1e-4
FLOOR = 2.0 ** -126
STORE_EXTRA = 311    # rows of the rollout store beyond the mini-batch when rows are gathered
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def f32(x):
    """The value a kernel receives for a float argument."""
    return float(np.float32(x))


KL_EPS = f32(1e-5)


# ------------------------------------------------------------------ loss: inputs --
def edge_rows():
    """Rows on an exact dyadic grid whose branch is known: (v, t, r, adv0, shift, c) with
    dv = (vcoef / M) c under clipped_value = 1 (c = None: a random value row), adv0 = the row's
    advantage is this zero (else random) and shift = old_logp - logp."""
    e = []
    # v - t = -+0.25: on the clamp edge, vc == v, the gradient passes: dv = gv 2 (v - r)
    e += [(0.75, 0.5, 0.0, None, 0.0, 1.5), (0.25, 0.5, 1.0, None, 0.0, -1.5)]
    # |v - t| = 0.125: inside the clamp, vc == v, a tie of the two terms
    e += [(1.125, 1.0, 0.25, None, 0.0, 1.75), (0.875, 1.0, 2.0, None, 0.0, -2.25)]
    # |v - t| = 0.5 (vc = t +- 0.25, the clamp closed): r on the far side (the clipped term
    # wins: 0), r midway (a tie: gv (v - r)), r on the near side (the unclipped term wins)
    e += [(0.5, 0.0, 1.0, None, 0.0, 0.0), (0.5, 0.0, 0.375, None, 0.0, 0.125), (0.5, 0.0, -1.0, None, 0.0, 3.0)]
    e += [(-0.5, 0.0, -1.0, None, 0.0, 0.0), (-0.5, 0.0, -0.375, None, 0.0, -0.125), (-0.5, 0.0, 1.0, None, 0.0, -3.0)]
    # adv = +-0 with the ratio well outside the clip (e^-+1): s1 == s2 == -+0, gradient 0, not NaN
    e += [(None, None, None, 0.0, -1.0, None), (None, None, None, -0.0, 1.0, None)]
    return e


N_EDGE = len(edge_rows())


def loss_inputs(M, A, seed, rows, mu=None, value=None):
    """Random inputs shaped like tests/test_gpu_fused_ppo.py's (CPU float32 tensors): mu [M, A],
    std [A], value [M]; the rollout side act / old_mu / old_sigma [R, A] and old_logp / adv /
    ret / target [R], with R = M + STORE_EXTRA and rows a permutation gather when `rows`, else
    R = M and rows None.  old_logp is the current log-probability plus 0.25 times a normal draw,
    so that ratios fall on both sides of the clip for both signs of the advantage.  The last
    min(N_EDGE, M - 1) mini-batch rows are the grid rows of edge_rows().  mu / value given (the
    outputs of a forward launch): they replace the random ones and no grid rows are placed (a
    grid row needs its own value)."""
    g = torch.Generator().manual_seed(seed)
    R = M + STORE_EXTRA if rows else M
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    given = mu is not None
    mu_r, std, value_r = rn(M, A), 0.5 + torch.rand(A, generator=g), rn(M)
    mu, value = (mu.detach().cpu().float(), value.detach().cpu().float().reshape(-1)) if given else (mu_r, value_r)
    act, old_mu = rn(R, A), rn(R, A)
    old_sigma = 0.5 + torch.rand(R, A, generator=g)
    adv, ret = rn(R), rn(R)
    target = ret + 0.3 * rn(R)
    idx = torch.randperm(R, generator=g)[:M].contiguous() if rows else torch.arange(M)
    shift = 0.25 * rn(M).to(F64)
    ne = 0 if given else min(N_EDGE, M - 1)
    grid, gridv = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
    for j, (v, t, r, a0, sh, _) in enumerate(edge_rows()[:ne]):
        i = M - ne + j
        grid[i] = True
        shift[i] = sh
        if v is not None:
            gridv[i] = True
            value[i], target[idx[i]], ret[idx[i]] = v, t, r
        if a0 is not None:
            adv[idx[i]] = a0
    logp = torch.distributions.Normal(mu.to(F64), std.to(F64)).log_prob(act[idx].to(F64)).sum(-1)
    old_logp = rn(R)
    old_logp[idx] = (logp + shift).to(torch.float32)
    inp = dict(mu=mu, std=std, value=value, act=act, old_logp=old_logp, old_mu=old_mu, old_sigma=old_sigma, adv=adv,
               ret=ret, target=target, rows=idx if rows else None, grid=grid, gridv=gridv)
    if M >= 128:
        q = quadrants(inp)
        assert min(q) >= 2, f"loss_inputs({M}, {A}, {seed}): quadrant counts {q}"
    return inp


def quadrants(inp):
    """Rows with the ratio (above hi, below lo) x (adv > 0, adv < 0)."""
    d = loss_ref(inp)["diag"]
    hi, lo = d["ratio"] > 1 + CLIP, d["ratio"] < 1 - CLIP
    pos, neg = d["adv"] > 0, d["adv"] < 0
    return [int((a & b).sum()) for a in (hi, lo) for b in (pos, neg)]


# --------------------------------------------------------------- loss: reference --
def loss_ref(inp, clipped_value=1, vcoef=0.5, ecoef=0.01, clip=CLIP, gout=1.0, mu=None, value=None):
    """The fp64 statement on `inp` (loss_inputs' dict; mu / value override the dict's: the
    forward launch's own outputs).  Returns loss, stats [4], dmu [M, A], dvalue [M], dstd [A],
    the per-row diagnostics `diag` and the derived bounds `bound` (see the module docstring)."""
    d = lambda t: t.detach().to("cpu", F64)  # noqa: E731
    rows = inp.get("rows")
    ga = (lambda t: d(t)[rows.cpu()]) if rows is not None else d  # noqa: E731
    vcoef, ecoef, clip, gout = f32(vcoef), f32(ecoef), f32(clip), f32(gout)
    tm = d(inp["mu"] if mu is None else mu).clone().requires_grad_(True)
    ts = d(inp["std"]).clone().requires_grad_(True)
    tv = d(inp["value"] if value is None else value).reshape(-1).clone().requires_grad_(True)
    act, om, os_ = ga(inp["act"]), ga(inp["old_mu"]), ga(inp["old_sigma"])
    olp, adv, ret, tgt = (ga(inp[k]).reshape(-1) for k in ("old_logp", "adv", "ret", "target"))
    M, A = tm.shape
    dist = torch.distributions.Normal(tm, tm * 0 + ts)
    lp_terms = dist.log_prob(act)
    logp = lp_terms.sum(-1)
    logp.retain_grad()
    ratio = torch.exp(logp - olp)
    s_rows = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip))
    if clipped_value:
        vc = tgt + (tv - tgt).clamp(-clip, clip)
        v_rows = torch.max((tv - ret).pow(2), (vc - ret).pow(2))
    else:
        vc = tv
        v_rows = (ret - tv).pow(2)
    surr, vl = s_rows.mean(), v_rows.mean()
    ent = dist.entropy().sum(-1).mean()
    loss = surr + vcoef * vl - ecoef * ent
    (gout * loss).backward()
    with torch.no_grad():
        m, s, v = tm.detach(), ts.detach(), tv.detach()
        kl_log = torch.log(s / os_ + KL_EPS)
        kl_quad = (os_ ** 2 + (om - m) ** 2) / (2 * s ** 2)
        kl_rows = (kl_log + kl_quad - 0.5).sum(-1)
        vcd = vc.detach()
        x1, x2, vt = v - ret, vcd - ret, v - tgt
        S = lp_terms.detach().abs().sum(-1) + olp.abs()
        diag = dict(ratio=ratio.detach(), S=S, vt=vt, vdiff=x1 ** 2 - x2 ** 2, adv=adv, clipped=bool(clipped_value),
                    grid=inp["grid"].clone() if "grid" in inp else torch.zeros(M, dtype=torch.bool),
                    gridv=inp["gridv"].clone() if "gridv" in inp else torch.zeros(M, dtype=torch.bool))
        # ---- derived bounds
        lg = math.ceil(math.log2(M)) if M > 1 else 0
        ssum = (lg + 8) * U
        rel = (A + 8) * 2 * U * S + 16 * U                          # per row, on dmu (relative)
        xmag = x1.abs() + vt.abs() + vcd.abs() + x2.abs()
        gv = gout * vcoef / M
        dv_abs = gv * 2 * U * xmag + 4 * U * tv.grad.abs()            # per row, on dvalue (absolute)
        v_err = 2 * torch.maximum(x1.abs(), x2.abs()) * U * xmag + 2 * U * v_rows.detach()
        kl_err = (A + 7) * U * (kl_log.abs() + kl_quad + 0.5).sum(-1) + 3 * U * A
        ent_terms = (0.5 + HALF_LOG_2PI + torch.log(s)).abs().sum()
        b_stats = torch.stack([
            (ssum * s_rows.detach().abs().sum() + (s_rows.detach().abs() * rel).sum()) / M,
            (ssum * v_rows.detach().sum() + v_err.sum()) / M,
            (ssum * kl_rows.abs().sum() + kl_err.sum()) / M,
            (A + 4) * 2 * U * ent_terms])
        amb = ambiguous(diag)
        dd = act - m
        full = (gout / M) * adv.abs() * ratio.detach()                 # |dlogp| had the branch passed it
        dl = logp.grad.abs()                                          # |dlogp| per row
        cabs = dd ** 2 / s ** 3 + 1 / s                              # [M, A]
        b_dstd = (ssum * (dl[:, None] * cabs).sum(0) + (dl[:, None] * cabs * (rel + 24 * U)[:, None]).sum(0)
                  + (full[:, None] * cabs)[amb].sum(0) + 2 * U * ecoef * gout / s)
        b_loss = (b_stats[0] + vcoef * b_stats[1] + ecoef * b_stats[3]
                  + 3 * U * (surr.detach().abs() + vcoef * vl.detach() + ecoef * ent.detach().abs()))
        stats = torch.stack([surr.detach(), vl.detach(), kl_rows.mean(), ent.detach()])
    return dict(loss=loss.detach(), stats=stats, dmu=tm.grad, dvalue=tv.grad, dstd=ts.grad, diag=diag, M=M, A=A,
                bound=dict(rel=rel, dv_abs=dv_abs, stats=b_stats, dstd=b_dstd, loss=b_loss))


def ambiguous(diag, delta=DELTA):
    """Rows that may take another branch in fp32 (module docstring); never a grid row."""
    r = diag["ratio"]
    amb = ((r - (1 - CLIP)).abs() < delta) | ((r - (1 + CLIP)).abs() < delta)
    if diag["clipped"]:
        avt = diag["vt"].abs()
        amb |= ((avt - CLIP).abs() < delta) | ((avt > CLIP) & (diag["vdiff"].abs() < delta))
    return amb & ~diag["grid"]


def assert_ambiguous_cap(ref, what):
    amb = ambiguous(ref["diag"])
    assert int(amb.sum()) <= 0.02 * ref["M"], f"{what}: {int(amb.sum())} of {ref['M']} rows are ambiguous (> 2 %)"
    return amb


# ------------------------------------------------------------- loss: comparisons --
def _frac(err, bound):
    """Worst error as a fraction of its bound (0 where both are 0)."""
    b = torch.where(bound > 0, bound, torch.ones_like(bound))
    f = torch.where(bound > 0, err / b, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(f.max()) if f.numel() else 0.0


def _first_bad(bad, what, **vals):
    idx = tuple(int(i) for i in bad.nonzero()[0])
    shown = ", ".join(f"{k}={float(v[idx])!r}" for k, v in vals.items())
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; first at {idx}: {shown}"


def check_close(got, want, bound, what, keep=None):
    """|got - want| <= bound elementwise (rows where keep is False are skipped); returns the
    worst error as a fraction of its bound."""
    g, w, b = got.detach().to("cpu", F64), want.to(F64), bound.to(F64)
    assert tuple(g.shape) == tuple(w.shape), (what, tuple(g.shape), tuple(w.shape))
    b = b.expand_as(w)
    err = (g - w).abs()
    bad = ~(err <= b)  # (NaN fails)
    if keep is not None:
        k = keep.reshape([-1] + [1] * (w.dim() - 1)).expand_as(w)
        bad &= k
        err = torch.where(k, err, torch.zeros_like(err))
    if bool(bad.any()):
        raise AssertionError(_first_bad(bad, what, got=g, want=w, bound=b))
    return _frac(torch.nan_to_num(err, nan=float("inf")), b)


def check_bf16(got, want, bound, what, keep=None):
    """A bf16 output: between the round-to-nearest bf16 values of want -+ bound."""
    g, w, b = got.detach().to("cpu", F64), want.to(F64), bound.to(F64).expand_as(want)
    assert got.dtype == torch.bfloat16 and tuple(g.shape) == tuple(w.shape), (what, got.dtype, tuple(g.shape))
    lo, hi = round_bf16(w - b), round_bf16(w + b)
    bad = ~((g >= lo) & (g <= hi))
    if keep is not None:
        bad &= keep.reshape([-1] + [1] * (w.dim() - 1)).expand_as(w)
    if bool(bad.any()):
        raise AssertionError(_first_bad(bad, what, got=g, lo=lo, hi=hi))
    return 0.0


def assert_zero_bits(t, what):
    """Padding: +0 bit for bit."""
    iv = {2: torch.int16, 4: torch.int32}[t.element_size()]
    n = int((t.contiguous().view(iv) != 0).sum())
    assert n == 0, f"{what}: {n} padding elements are not +0"


def row_bounds(ref):
    """(dmu bound [M, A], dvalue bound [M], rows kept [M]): the per-row bounds, the grid rows'
    value gradients on their tight bound under clipped_value (exact arithmetic up to the
    scaling's two roundings)."""
    b = ref["bound"]
    keep = ~ambiguous(ref["diag"])
    bm = ref["dmu"].abs() * b["rel"][:, None] + FLOOR
    bv = b["dv_abs"] + FLOOR
    grid = ref["diag"]["gridv"]
    bv = torch.where(grid, 2 * U * ref["dvalue"].abs() + FLOOR, bv)
    return bm, bv, keep


def check_loss_stats(stats, dstd, ref, what, loss=None):
    fr = {}
    fr["stats"] = check_close(stats, ref["stats"], ref["bound"]["stats"], what + " stats")
    fr["dstd"] = check_close(dstd, ref["dstd"], ref["bound"]["dstd"], what + " dstd")
    if loss is not None:
        fr["loss"] = check_close(loss.reshape(()), ref["loss"], ref["bound"]["loss"], what + " loss")
    return fr


def check_loss_step(out, ref, what):
    """The outputs of pmlp_ppo_loss_step (CPU tensors: dmu bf16 [M, Ap], dv bf16 [M, Vp],
    dmu_t [Ap, M] / dv_t [Vp, M] or None, stats, dstd or None) against loss_ref's result."""
    A = ref["A"]
    assert_ambiguous_cap(ref, what)
    bm, bv, keep = row_bounds(ref)
    check_bf16(out["dmu"][:, :A], ref["dmu"], bm, what + " dmu", keep)
    check_bf16(out["dv"][:, 0], ref["dvalue"], bv, what + " dvalue", keep)
    assert_zero_bits(out["dmu"][:, A:], what + " dmu padding")
    assert_zero_bits(out["dv"][:, 1:], what + " dvalue padding")
    if out.get("dmu_t") is not None:
        assert same_bits(out["dmu_t"].contiguous(), out["dmu"].t().contiguous()), what + ": dmu_t is not dmu^T"
    if out.get("dv_t") is not None:
        assert same_bits(out["dv_t"].contiguous(), out["dv"].t().contiguous()), what + ": dvalue_t is not dvalue^T"
    if out.get("stats") is not None:
        return check_loss_stats(out["stats"], out["dstd"], ref, what)
    return {}


def check_loss_f32(out, ref, what):
    """fp32 output gradients dmu [M, A], dv [M] (pmlp_ppo_loss_step_f32, pmlp_ppo_loss_bwd);
    stats / dstd / loss where given."""
    assert_ambiguous_cap(ref, what)
    bm, bv, keep = row_bounds(ref)
    fr = dict(dmu=check_close(out["dmu"], ref["dmu"], bm, what + " dmu", keep),
              dvalue=check_close(out["dv"].reshape(-1), ref["dvalue"], bv, what + " dvalue", keep))
    if out.get("stats") is not None:
        fr.update(check_loss_stats(out["stats"], out["dstd"], ref, what, out.get("loss")))
    elif out.get("dstd") is not None:
        fr["dstd"] = check_close(out["dstd"], ref["dstd"], ref["bound"]["dstd"], what + " dstd")
    return fr


def sum_bound(terms, n=None):
    """Any-order fp32 summation bound of the fp64 terms."""
    n = terms.numel() if n is None else n
    return (math.ceil(math.log2(max(n, 2))) + 8) * U * float(terms.abs().sum())


# -------------------------------------------------------------------------- GAE --
DONE_PATTERNS = ("none", "all", "last", "first", "random")


def gae_grid_inputs(T, N, seed, pattern="random"):
    """Rewards, values [T, N] and last values [N] of the form k/4, |k| <= 8, and dones [T, N]
    (uint8) in one of DONE_PATTERNS; to be run with gamma = lam = 0.5 and T <= 8."""
    assert T <= 8
    g = np.random.default_rng(seed)
    q = lambda *s: (g.integers(-8, 9, size=s) / 4.0).astype(np.float32)  # noqa: E731
    rew, val, last = q(T, N), q(T, N), q(N)
    done = np.zeros((T, N), np.uint8)
    if pattern == "all":
        done[:] = 1
    elif pattern == "last":
        done[T - 1] = 1
    elif pattern == "first":
        done[0] = 1
    elif pattern == "random":
        done = (g.random((T, N)) < 0.2).astype(np.uint8)
    else:
        assert pattern == "none"
    return rew, done, val, last


def gae_ref(rew, done, val, last, gamma, lam, dtype=np.float64):
    """RolloutStorage.compute_returns' recursion at precision `dtype`, in k_gae's grouping of
    the operations: (returns, un-normalised advantages) [T, N]."""
    f = dtype
    rew, val, last = rew.astype(f), val.astype(f), last.astype(f)
    gamma, lam = f(np.float32(gamma)), f(np.float32(lam))
    T, N = rew.shape
    ret, adv = np.zeros((T, N), f), np.zeros((T, N), f)
    a = np.zeros(N, f)
    for t in range(T - 1, -1, -1):
        nxt = last if t == T - 1 else val[t + 1]
        nt = f(1) - (done[t] != 0).astype(f)
        delta = (rew[t] + (nt * gamma) * nxt) - val[t]
        a = delta + ((nt * gamma) * lam) * a
        ret[t] = a + val[t]
        adv[t] = ret[t] - val[t]
    return ret, adv


def moments_ref(adv):
    a = adv.astype(np.float64)
    return np.array([a.sum(), (a * a).sum(), float(a.size)])


def normalize_ref(adv, moments):
    """(adv - mean) / (std + 1e-8) with the mean and unbiased std of the given {sum, sum of
    squares, count}; returns (normalised fp64, the bound ((|adv| + |mean|) / den) 4 U)."""
    s, ss, c = (float(x) for x in moments)
    mean = s / c
    var = max((ss - c * mean * mean) / (c - 1.0), 0.0)
    den = math.sqrt(var) + f32(1e-8)
    a = adv.astype(np.float64)
    return (a - mean) / den, (np.abs(a) + abs(mean)) / den * 4 * U


def check_gae_exact(ret, adv, moments, ref_ret, ref_adv, what):
    """On the exact grid: returns, advantages and the moments equal the fp64 reference."""
    for name, got, want in (("returns", ret, ref_ret), ("advantages", adv, ref_adv)):
        bad = ~(got.astype(np.float64) == want)
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} of {bad.size} differ from fp64; first at " \
                              f"{tuple(int(i[0]) for i in np.nonzero(bad))}"
    if moments is not None:
        want = moments_ref(ref_adv)
        assert np.array_equal(np.asarray(moments, np.float64), want), f"{what} moments: {moments} != {want}"


def check_normalized(got, adv, moments, what):
    want, bound = normalize_ref(adv, moments)
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} normalised advantages outside " \
                          f"((|adv| + |mean|) / den) 4 U; worst {float(np.nanmax(err / np.maximum(bound, 1e-300))):.3g} x"
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------- Adam --
def adam_grid_grads(n, seed):
    """Gradients whose sum of squares is exact in fp32 in any order (module docstring)."""
    g = np.random.default_rng(seed)
    sign = np.where(g.random(n) < 0.5, -1.0, 1.0)
    if n < 65536:
        mag = np.array([2.0 ** -3, 2.0 ** -5, 2.0 ** -7])[g.integers(0, 3, size=n)]
    else:
        mag = np.full(n, 2.0 ** -4)
    return (sign * mag).astype(np.float32)


def ulp32(x):
    """One fp32 ulp at |x| (fp64 array), the denormal spacing at the bottom."""
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return np.where(ax > 0, np.maximum(2.0 ** (e - 23), 2.0 ** -149), 2.0 ** -149)


def adam_budgets(t, b1, b2):
    """(e_m, e_v, R_u): rounding counts after step t (module docstring), before doubling."""
    b1, b2 = f32(b1), f32(b2)
    k1, k2 = b1 ** t / (1 - b1 ** t), b2 ** t / (1 - b2 ** t)
    em, ev = 5 + 3 * t, 10 + 4 * t
    return em, ev, em + ev / 2 + 2 * k1 + k2 + 7.5


def adam_ref(p, m, v, grads, grad_scale=1.0, max_norm=1.0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step0=0):
    """clip_grad_norm_ + Adam in float64 over the steps `grads` (a list of fp32 arrays), from
    fp32 state p, m, v.  Per step a dict p, m, v (fp64), the bounds bp, bm, bv on the fp32
    results, and `clipped`."""
    p, m, v = (np.asarray(x, np.float64).copy() for x in (p, m, v))
    b1, b2, eps, lr, scale, max_norm = f32(b1), f32(b2), f32(eps), f32(lr), f32(grad_scale), f32(max_norm)
    out = []
    bp = np.zeros_like(p)
    for s, g in enumerate(grads):
        t = step0 + s + 1
        gs = np.asarray(g, np.float64) * scale
        norm = math.sqrt(float((gs * gs).sum()))
        coef = min(1.0, max_norm / (norm + f32(1e-6))) if max_norm > 0 else 1.0
        gi = gs * coef
        m = m + (1 - b1) * (gi - m)
        v = b2 * v + (1 - b2) * gi * gi
        u = (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
        p = p - u
        em, ev, ru = adam_budgets(t, b1, b2)
        bp = bp + 2 * ru * U * np.abs(u) + 0.5 * ulp32(p)
        out.append(dict(p=p.copy(), m=m.copy(), v=v.copy(), bp=bp.copy(), bm=2 * em * ulp32(m), bv=2 * ev * ulp32(v),
                        clipped=coef < 1.0, sumsq=float((gs * gs).sum())))
    return out


def check_adam(p, m, v, ref, what):
    """fp32 results (numpy) of a step against adam_ref's entry for it; returns the worst
    fractions of the budgets."""
    fr = {}
    for name, got, want, bound in (("m", m, ref["m"], ref["bm"]), ("v", v, ref["v"], ref["bv"]),
                                   ("p", p, ref["p"], ref["bp"])):
        err = np.abs(np.asarray(got, np.float64) - want)
        bad = ~(err <= bound)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            raise AssertionError(f"{what} {name}: {int(bad.sum())} of {bad.size} outside the budget; first at {i}: "
                                 f"got={float(got[i])!r} want={want[i]!r} bound={bound[i]!r}")
        fr[name] = float((err / bound).max())
    return fr


def frag_index_ref(r, c, ld):
    """Index of element (r, c) in the fragment-packed copy of a weight with row stride ld
    (include/ppo_mlp.h pmlp_mirror_job.frag): blocks of 32 rows x 16 columns, 64 groups of 8
    elements each -- group = row within the block, + 32 for the block's upper 8 columns."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    block = (r // 32) * (ld // 16) + c // 16
    group = r % 32 + 32 * ((c // 8) % 2)
    return (block * 64 + group) * 8 + c % 8


def bf16_bits_rne(x32):
    """The bf16 bit patterns (uint16) of fp32 numbers under round-to-nearest-even (finite)."""
    b = np.asarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def check_mirror(dst_bits, frag_bits, p32, job, sentinel_bits, what):
    """A mirror job's copies (uint16 arrays: dst [rows, ld], frag flat or None) of the fp32
    parameter p32 the kernel wrote: dst[:, :cols] and the frag entries at frag_index_ref are
    exactly the RNE bf16; the guard columns and the frag padding still hold the sentinel."""
    off, rows, cols, ld = job
    want = bf16_bits_rne(p32[off:off + rows * cols]).reshape(rows, cols)
    assert np.array_equal(dst_bits[:, :cols], want), \
        f"{what} dst: {int((dst_bits[:, :cols] != want).sum())} entries are not the RNE bf16 of the parameter"
    assert (dst_bits[:, cols:] == sentinel_bits).all(), f"{what} dst: guard columns were written"
    if frag_bits is not None:
        r, c = np.divmod(np.arange(rows * cols), cols)
        idx = frag_index_ref(r, c, ld)
        assert np.array_equal(frag_bits[idx], want.reshape(-1)), f"{what} frag: entries are not at frag_index_ref"
        rest = np.ones(frag_bits.shape, bool)
        rest[idx] = False
        assert (frag_bits[rest] == sentinel_bits).all(), f"{what} frag: padding entries were written"


# ---------------------------------------------------------------------- KL rule --
def lr_rule_ref(kl, lr, desired):
    """rsl_rl v1.0.2's KL-adaptive schedule in numpy float32, operation for operation."""
    f = np.float32
    kl, lr, desired = f(kl), f(lr), f(desired)
    if kl > desired * f(2):
        lr = max(lr / f(1.5), f(1e-5))
    elif kl < desired / f(2) and kl > f(0):
        lr = min(lr * f(1.5), f(1e-2))
    return f(lr)


DESIRED_KL = 2.0 ** -7


def kl_table():
    """kl values around the rule's thresholds for desired_kl = 2^-7."""
    f = np.float32
    up, dn = f(2.0 ** -6), f(2.0 ** -8)
    return [up, np.nextafter(up, f(1)), dn, np.nextafter(dn, f(0)), f(0), f(-0.01), f(2.0 ** -140)]


LR_TABLE = (1e-3, 1.2e-5, 8e-3)


def bookkeeping_ref(stats, lr, acc, desired, adaptive, scale=1.0):
    """(lr, acc) after one step's bookkeeping in numpy float32 from stats = [surrogate, value,
    kl, entropy] (k_opt_prepare's form: the stats scaled by `scale` first)."""
    f = np.float32
    st = [f(x) * f(scale) for x in stats]
    new_acc = None if acc is None else [f(acc[0]) + st[1], f(acc[1]) + st[0]]
    return (lr_rule_ref(st[2], lr, desired) if adaptive else f(lr)), new_acc


# --------------------------------------------------------- the GPU file's cases --
# tests/test_ppo_ref_host.py asserts the input conditions (the 2 % cap, the quadrant counts,
# the exactness claims) for every case listed here; tests/test_gpu_ppo_reference.py runs them.
LOSS_M = (1, 37, 64, 65, 257, 517)
LOSS_ARMS = (  # (arm of loss_step_launch, A, Ap)
    ("quad", 4, 4), ("quad", 4, 8), ("quad", 12, 16), ("quad", 16, 16),
    ("reg-scalar", 10, 16), ("reg-scalar", 1, 8), ("reg-scalar", 3, 8),
    ("reg-vec", 12, 24), ("reg-vec", 8, 32),
    ("generic", 10, 12), ("generic", 17, 17), ("generic", 20, 24))
# per M of LOSS_M: (rows gathered, clipped_value, dmu_t / dvalue_t given); every arm runs all six,
# so every arm sees both values of each toggle
LOSS_TOGGLES = ((0, 1, 0), (1, 0, 1), (1, 1, 1), (0, 0, 0), (1, 1, 0), (0, 1, 1))
F32_CASES = tuple((A, M) for A in (12, 10, 20) for M in (65, 257))   # quad, register, generic
BWD_M, BWD_A = (1, 255, 256, 257, 517), (1, 10, 12, 20)
FWD_LOSS_M = 18432 + 37


def loss_arm(A, Ap):
    """The arm loss_step_launch (csrc/ppo_loss.hip) takes."""
    if A % 4 == 0 and A <= 16 and Ap <= 16 and Ap % 4 == 0:
        return "quad"
    if A <= 16 and Ap % 8 == 0:
        return "reg-vec" if A % 4 == 0 else "reg-scalar"
    return "generic"


def loss_seed(M, A):
    return 1000 * A + M


def loss_cases():
    """(M, A, seed, rows, clipped_value) of every loss case the GPU file runs."""
    out = []
    for _, A, _ in LOSS_ARMS:
        for M, (rows, cv, _) in zip(LOSS_M, LOSS_TOGGLES):
            out.append((M, A, loss_seed(M, A), bool(rows), cv))
    for A, M in F32_CASES:
        out.append((M, A, loss_seed(M, A), True, 1))
    for im, M in enumerate(BWD_M):
        for ia, A in enumerate(BWD_A):
            out.append((M, A, loss_seed(M, A), *bwd_toggles(im, ia)[:2]))
    out.append((64 + 37, 12, loss_seed(64 + 37, 12), True, 1))       # the folded finish
    return sorted(set(out))


def bwd_toggles(im, ia):
    """(rows gathered, clipped_value, gout) of the autograd-path case (BWD_M[im], BWD_A[ia])."""
    return bool((im + ia) % 2), 0 if (im + 2 * ia) % 3 == 0 else 1, 1.0 if (im + ia) % 2 == 0 else 0.5


GAE_N, GAE_T = (1, 63, 64, 65, 255, 256, 257, 333), (1, 2, 7)
ADAM_VEC4_N = (3, 4, 255 * 4 + 1, 4096 + 2, 4096 + 3)
ADAM_SCALAR_CAP_N = 1024 * 256 + 259
ADAM_RELOAD_N = 4096 * 256 * 4 + 4 * 300 + 3
