"""fp64 references for the two kernels of random network distillation (pmlp_rnd_reward and
pmlp_rnd_loss_step, csrc/rnd.hip) and the comparisons built on them.  numpy only:
nothing here needs a GPU or the libraries.  tests/test_rnd_ref_host.py tests this file itself;
tests/test_gpu_rnd.py holds the kernels to it.

U = 2^-24 is one fp32 rounding (relative).  No bound below is fitted to a kernel's output: every
one is a count of the fp32 roundings between the reference's operands and the kernel's result,
doubled.  The kernels are compiled without contraction, so every product and sum is one rounding.

The loss kernel is pmlp_distill_loss_step's mse arm with the target row read through an index:
its references and bounds are distill_ref's (grad_ref / grad_bound, terms, partials_ref, loss_ref),
imported and applied to the gathered target tgt_all[idx] (check_loss_step below).

The reward kernel.  The reference's operands are the kernel's own fp32 inputs pred, tgt [M, E],
w [T], the rewards before the launch [M] and inv_m = float32(1) / float32(M) (the host's operand
of the finish), all widened to fp64.  Per row m of storage step t = m // N:

    r = sqrt(sum_k (tgt_k - pred_k)^2)      bonus = w[t] r      rewards_out = rewards_in + bonus

Roundings of r: d_k is one (U); d_k * d_k carries it twice and rounds once (3 U of the term); the
terms are non-negative, so each of the E - 1 additions adds at most U of the running sum, itself
at most s: (E - 1) U of s.  So s is within (E + 2) U s.  The library is compiled without fast-math
(csrc/Makefile's HIPFLAGS: -O3, no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt),
so sqrtf is the correctly rounded square root: it halves the relative error of s and rounds once,
((E + 2) / 2 + 1) U r.  The product with w rounds once more.  Doubled:
    B_r     = (E + 4) U r
    B_bonus = (E + 6) U |bonus|
The addition into the rewards rounds once, U |rewards_out|.  Doubled:
    B_rew   = B_bonus + 2 U |rewards_in + bonus|
A partial: the bonuses (or the r's) of 64 consecutive rows, n of them, summed by a butterfly (any
order of n - 1 additions is within (n - 1) U sum |x| to first order), as distill_ref's B_partial:
    B_part  = sum B_x + 2 (n - 1) U sum |x|
A mean stats[j] = (sum of the P partials) inv_m, as distill_ref's B_loss:
    B_mean  = inv_m (sum B_part + 2 (P - 1) U sum |partial| + 2 U |sum|)
(the values of the cases are far above the subnormal range; nothing is added for underflow).
"""
import numpy as np

from act_ref import U, check_close
import distill_ref as dr

GROUP = 64  # rows per partial


def num_partials(M):
    return (M + GROUP - 1) // GROUP


def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _groups(x):
    M = x.shape[0]
    return [x[g * GROUP:min(M, (g + 1) * GROUP)] for g in range(num_partials(M))]


def inv_rows(M):
    """The finish's fp32 operand float(1) / float(M)."""
    return np.float32(1.0) / np.float32(M)


# ------------------------------------------------------------------- the reward --
def reward_ref(pred, tgt, w, rewards_in, N):
    """dict of fp64 references and bounds of one pmlp_rnd_reward launch over M = T N rows:
    r, bonus, rewards [M] with B_r, B_bonus, B_rew; partial [2 P] with B_part; stats [2] with B_mean."""
    pred, tgt = _f64(pred), _f64(tgt)
    M, E = pred.shape
    d = tgt - pred
    r = np.sqrt((d * d).sum(axis=1))
    wt = np.repeat(_f64(w), N)
    assert wt.shape[0] == M, (wt.shape, M)
    bonus = wt * r
    rew = _f64(rewards_in).reshape(M) + bonus
    b_r = (E + 4.0) * U * r
    b_bonus = (E + 6.0) * U * np.abs(bonus)
    b_rew = b_bonus + 2.0 * U * np.abs(rew)

    def parts(x, bx):
        ref = np.array([g.sum() for g in _groups(x)])
        bound = np.array([b.sum() + 2.0 * (g.size - 1) * U * np.abs(g).sum() for g, b in zip(_groups(x), _groups(bx))])
        return ref, bound

    def mean(p, pb):
        s, total = float(inv_rows(M)), p.sum()
        return total * s, s * (pb.sum() + 2.0 * (p.size - 1) * U * np.abs(p).sum() + 2.0 * U * abs(total))

    pb_, pbb = parts(bonus, b_bonus)
    pr_, prb = parts(r, b_r)
    mb, mbb = mean(pb_, pbb)
    mr, mrb = mean(pr_, prb)
    return dict(r=r, b_r=b_r, bonus=bonus, b_bonus=b_bonus, rewards=rew, b_rew=b_rew,
                partial=np.concatenate([pb_, pr_]), b_partial=np.concatenate([pbb, prb]),
                stats=np.array([mb, mr]), b_stats=np.array([mbb, mrb]))


def check_reward(rewards_out, intrinsic, partial, stats, pred, tgt, w, rewards_in, N):
    """The outputs of one launch (float32; intrinsic may be None) against reward_ref.  Returns the
    worst fractions of the bounds."""
    ref = reward_ref(pred, tgt, w, rewards_in, N)
    M = ref["r"].shape[0]
    fr = dict(rewards=check_close(np.asarray(rewards_out, np.float32).reshape(M), ref["rewards"], ref["b_rew"],
                                  "rewards"))
    if intrinsic is not None:
        fr["bonus"] = check_close(np.asarray(intrinsic, np.float32).reshape(M), ref["bonus"], ref["b_bonus"],
                                  "intrinsic")
    fr["partial"] = check_close(np.asarray(partial, np.float32), ref["partial"], ref["b_partial"], "partials")
    fr["stats"] = check_close(np.asarray(stats, np.float32), ref["stats"], ref["b_stats"], "stats")
    return fr


def reward_f32(pred, tgt, w, rewards_in, N):
    """The kernel's arithmetic in numpy float32, in its order (k order, the butterfly of
    csrc/rnd.hip's wave_sum per 64 rows, the finish's strided sums): (rewards_out, bonus, partial,
    stats) float32."""
    f = np.float32
    pred, tgt = np.asarray(pred, f), np.asarray(tgt, f)
    M, E = pred.shape
    s = np.zeros(M, f)
    for k in range(E):
        d = (tgt[:, k] - pred[:, k]).astype(f)
        s = (s + (d * d).astype(f)).astype(f)
    r = np.sqrt(s).astype(f)
    bonus = (np.repeat(np.asarray(w, f), N) * r).astype(f)
    rew = (np.asarray(rewards_in, f).reshape(M) + bonus).astype(f)
    P = num_partials(M)

    def butterfly(x):
        v = np.zeros(GROUP, f)
        v[:x.shape[0]] = x
        sft = GROUP // 2
        while sft:
            v = (v + v[np.arange(GROUP) ^ sft]).astype(f)
            sft //= 2
        return v[0]

    def finish(p):
        lane = np.zeros(GROUP, f)
        for i in range(p.shape[0]):
            lane[i % GROUP] = f(lane[i % GROUP] + p[i])
        return f(butterfly(lane) * inv_rows(M))

    pb = np.array([butterfly(g) for g in _groups(bonus)], f)
    pr = np.array([butterfly(g) for g in _groups(r)], f)
    assert pb.shape[0] == P
    return rew, bonus, np.concatenate([pb, pr]), np.array([finish(pb), finish(pr)], f)


# --------------------------------------------------------------------- the loss --
def loss_scale(M, E):
    """The kernel's fp32 scale operand 1 / (M E)."""
    return np.float32(1.0 / (M * E))


def check_loss_step(dmu_b_bits, dmu_f, partial, stats, mu, tgt_all, idx, scale):
    """One pmlp_rnd_loss_step launch against distill_ref's mse references on the gathered
    target: the gradient (bf16 bits [M, Ap] and the optional fp32 copy), the padded zeros, the
    partials and stats.  Returns the worst fractions."""
    target = np.asarray(tgt_all, np.float32)[np.asarray(idx, np.int64)]
    fr = dr.check_grad(dmu_b_bits, dmu_f, mu, target, dr.MSE, scale)
    fr.update(dr.check_loss(partial, stats, mu, target, dr.MSE, scale))
    return fr


# --------------------------------------------------------------------- the cases --
WIDTHS = (1, 8, 12, 32)                 # scalar, the 16-byte path, by element, the limit
SHAPES = ((3, 8), (25, 8), (2, 64))     # 24 rows < one group; 200 = three groups and a ragged one; 128 = two
LOSS_PADS = {1: (8, 16, 32), 8: (8, 16, 32), 12: (16, 32), 32: (32,)}
LOSS_ROWS = (24, 200)
LOSS_SOURCE_ROWS = 256


def reward_case(T, N, E, seed=0):
    """(pred, tgt [T N, E], w [T], rewards_in [T N]) float32: outputs of order one, a distinct
    weight per step with w[1] = 0, rewards non-zero."""
    rng = np.random.default_rng(10000 * T + 100 * N + E + seed)
    M = T * N
    pred = rng.standard_normal((M, E)).astype(np.float32)
    tgt = rng.standard_normal((M, E)).astype(np.float32)
    w = (0.25 + 0.125 * np.arange(T)).astype(np.float32)
    w[1] = 0.0
    rewards = (rng.standard_normal(M) - 0.5).astype(np.float32)
    rewards[rewards == 0] = np.float32(0.5)
    return pred, tgt, w, rewards


def loss_case(M, E, seed=0):
    """(mu [M, E], tgt_all [R, E], idx [M]) with R = LOSS_SOURCE_ROWS: distill_ref's grid values
    (every difference exactly representable); idx out of order, with repeated rows."""
    R = LOSS_SOURCE_ROWS
    rng = np.random.default_rng(77000 + 100 * M + E + seed)
    idx = rng.integers(0, R, M).astype(np.int64)
    idx[:4] = (R - 1, 0, R - 1, 5)[:M]  # the ends, a repeat, out of order
    _, tgt_all = dr.loss_case(R, E, dr.MSE, seed)
    mu_src, tgt_src = dr.loss_case(M, E, dr.MSE, seed + 1)
    mu = (tgt_all[idx] + (mu_src - tgt_src)).astype(np.float32)
    return mu, tgt_all, idx
