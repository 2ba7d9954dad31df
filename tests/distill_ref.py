"""fp64 references for the behaviour-cloning loss of teacher-student distillation
(pmlp_distill_loss_step, csrc/distill.hip) and the comparisons built on them.  numpy
only: nothing here needs a GPU or the libraries.  tests/test_distill_ref_host.py tests this file
itself; tests/test_gpu_distill_reference.py holds the kernel to it.  The acting side
(pmlp_distill_act) is held to tests/act_ref.py's noise_ref / act_bound as they are.

U = 2^-24 is one fp32 rounding (relative).  No bound below is fitted to a kernel's output: every
one is a count of the fp32 roundings between the reference's operands and the kernel's result,
doubled.  The kernel is compiled without contraction, so every product and sum is one rounding.

The reference's operands are the kernel's own fp32 inputs mu, target [M, A] and the fp32 scale
= float32(1 / (N A)), all widened to fp64.  Per entry, with d = mu - target:

    mse:    term = d^2               gradient = 2 d scale
    huber:  |d| <= 1: term = d^2 / 2,   gradient = d scale          (delta = 1)
            |d| >  1: term = |d| - 1/2, gradient = sign(d) scale
    (at |d| = 1 both branches give term 1/2 and gradient +-scale: the reference is unambiguous)

The gradient (grad_bound).  d is one rounding; 2 d is exact and its product with scale one more;
the huber's d * scale likewise; the huber's outer branch is +-scale itself, no rounding, but an
entry within one rounding of |d| = 1 may take the other branch, whose value differs by
|d - 1| scale <= U scale: inside the same count.  Counted 2 U |g|, doubled:
    B_g32 = 4 U |g|
The bf16 operand dmu_b is that fp32 value rounded to nearest even at 8 significant bits: half an
ulp of the value v it rounds, 2^(floor(log2 |v|) - 8) -- between 2^-9 |v| (the top of a binade)
and 2^-8 |v| (its bottom) -- of a value within B_g32 of g.  The format's own figure, not doubled:
    B_g16 = half_ulp_bf16(|g| + B_g32) + B_g32
(the gradients of the cases are far above the subnormal range; nothing is added for underflow).
Padded columns A .. Ap - 1 are zeros, compared for equality.

A term (term_bound).  Quadratic: d carries its rounding twice into d * d, which rounds once
(0.5 d is exact): 3 U |term|.  Linear: |d| carries one rounding, U |d|, and the subtraction
rounds once, U |term|.  Doubled:
    B_term = 6 U |term|  (quadratic),   2 U (|d| + |term|)  (linear)
An entry within one rounding of |d| = 1 may take the other branch; the two agree there to
(|d| - 1)^2 / 2 <= U^2, below every bound above.

A partial (partial_bound): the unscaled terms of 64 consecutive rows, n = rows x A of them, summed
in fp32 (a row's in k order, the rows' by a butterfly: any order of n - 1 additions is within
(n - 1) U sum |term| to first order).  Doubled:
    B_partial = sum B_term + 2 (n - 1) U sum |term|
The finished loss stats[0] = (sum of the P partials) scale: the partials' bounds, (P - 1) U sum
|partial| for the additions and one rounding of the product.  Doubled where not already:
    B_loss = scale (sum B_partial + 2 (P - 1) U sum |partial| + 2 U |sum|)
"""
import numpy as np

from act_ref import U, check_close, check_equal

GROUP = 64  # rows per loss partial
MSE, HUBER = "mse", "huber"


def entry_scale(N, A):
    """The kernel's fp32 scale operand 1 / (N A)."""
    return np.float32(1.0 / (N * A))


def _d(mu, target):
    return np.asarray(mu, np.float32).astype(np.float64) - np.asarray(target, np.float32).astype(np.float64)


def terms_ref(mu, target, loss_type):
    """(term, linear) fp64 / bool [M, A]: the unscaled loss terms and where the huber is linear."""
    d = _d(mu, target)
    if loss_type == MSE:
        return d * d, np.zeros(d.shape, bool)
    lin = np.abs(d) > 1.0
    return np.where(lin, np.abs(d) - 0.5, 0.5 * d * d), lin


def grad_ref(mu, target, loss_type, scale):
    """The fp64 gradient [M, A] of the step's loss with respect to mu."""
    d, s = _d(mu, target), float(np.float32(scale))
    if loss_type == MSE:
        return 2.0 * d * s
    return np.where(np.abs(d) > 1.0, np.sign(d) * s, d * s)


def half_ulp_bf16(v):
    """Half a unit in the last place of bf16 (8 significant bits) at |v|; 0 at 0."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (e - 8.0), 0.0)


def grad_bound(g, bf16=False):
    b32 = 4.0 * U * np.abs(g)
    return half_ulp_bf16(np.abs(g) + b32) + b32 if bf16 else b32


def term_bound(mu, target, loss_type):
    term, lin = terms_ref(mu, target, loss_type)
    return np.where(lin, 2.0 * U * (np.abs(_d(mu, target)) + np.abs(term)), 6.0 * U * np.abs(term))


def num_partials(M):
    return (M + GROUP - 1) // GROUP


def _groups(x):
    M = x.shape[0]
    return [x[g * GROUP:min(M, (g + 1) * GROUP)] for g in range(num_partials(M))]


def partials_ref(mu, target, loss_type):
    """(partials, bounds) fp64 [ceil(M / 64)]."""
    term, _ = terms_ref(mu, target, loss_type)
    tb = term_bound(mu, target, loss_type)
    ref = np.array([t.sum() for t in _groups(term)])
    bound = np.array([b.sum() + 2.0 * (t.size - 1) * U * np.abs(t).sum() for t, b in zip(_groups(term), _groups(tb))])
    return ref, bound


def loss_ref(mu, target, loss_type, scale):
    """(loss, bound): the step's loss, sum of the terms times scale."""
    p, pb = partials_ref(mu, target, loss_type)
    s = float(np.float32(scale))
    total = p.sum()
    return total * s, s * (pb.sum() + 2.0 * (p.size - 1) * U * np.abs(p).sum() + 2.0 * U * abs(total))


def bf16_to_f64(bits):
    """uint16 bf16 bit patterns -> fp64."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def check_grad(dmu_b_bits, dmu_f, mu, target, loss_type, scale):
    """dmu_b (uint16 bits [M, Ap]) and dmu_f (float32 [M, A] or None) of one launch against
    grad_ref: the A columns within grad_bound, the padded columns exactly +0.  Returns the worst
    fractions of the bounds."""
    g = grad_ref(mu, target, loss_type, scale)
    M, A = g.shape
    bits = np.asarray(dmu_b_bits, np.uint16)
    assert bits.shape[0] == M and bits.shape[1] >= A and bits.shape[1] % 8 == 0, bits.shape
    fr = dict(b=check_close(bf16_to_f64(bits[:, :A]), g, grad_bound(g, True), f"dmu_b ({loss_type})"))
    if bits.shape[1] > A:
        check_equal(bits[:, A:], np.zeros((M, bits.shape[1] - A), np.uint16), "dmu_b padded columns")
    if dmu_f is not None:
        fr["f"] = check_close(np.asarray(dmu_f, np.float32), g, grad_bound(g), f"dmu_f ({loss_type})")
    return fr


def check_loss(partial, stats, mu, target, loss_type, scale):
    """The partials [ceil(M / 64)] and stats [4] of one launch against partials_ref / loss_ref;
    stats[1:4] are exactly zero.  Returns the worst fractions."""
    p, pb = partials_ref(mu, target, loss_type)
    fr = dict(partial=check_close(np.asarray(partial, np.float32), p, pb, f"partials ({loss_type})"))
    want, wb = loss_ref(mu, target, loss_type, scale)
    stats = np.asarray(stats, np.float32)
    fr["loss"] = check_close(stats[:1], np.array([want]), np.array([wb]), f"stats[0] ({loss_type})")
    check_equal(stats[1:4], np.zeros(3, np.float32), "stats[1:4]")
    return fr


# --------------------------------------------------------------------- the cases --
ROWS = (1, 37, 64, 65, 257)
WIDTHS = ((12, 16), (16, 16), (4, 8), (10, 16), (1, 8), (20, 24))
ENVS = 8  # the N of scale = 1 / (N A) in the loss cases


def loss_case(M, A, loss_type, seed=0):
    """(mu, target) float32 [M, A] on a grid of multiples of 1/8 (every d exactly representable),
    most |d| below 1, some above; the huber cases carry entries with |d| exactly 1 of both signs
    in their first row.  The entries are far from the subnormal range."""
    rng = np.random.default_rng(1000 * M + 10 * A + seed + (1 if loss_type == HUBER else 0))
    target = rng.integers(-8, 9, (M, A)).astype(np.float32) / np.float32(8.0)
    d = rng.integers(-7, 8, (M, A)).astype(np.float32) / np.float32(8.0)     # |d| < 1
    far = rng.random((M, A)) < 0.25
    d = np.where(far, np.sign(d + np.float32(0.01)) * (np.abs(d) + np.float32(1.25)), d).astype(np.float32)
    flat = d.reshape(-1)
    # fixed entries: |d| = 1 (both signs where there is room), one inside, one outside
    # (M = 1, A = 1 has one entry: |d| = 1; every other case has at least four)
    fixed = [1.0, -1.0, 0.5, -2.5][:flat.size]
    flat[:len(fixed)] = np.asarray(fixed, np.float32)
    mu = (target + d).astype(np.float32)
    return mu, target


def case_conditions(M, A, loss_type):
    """What every GPU case's inputs satisfy (asserted by the host test): exact differences, and for
    the huber cases with at least four entries |d| < 1, |d| > 1 and |d| == 1 all present."""
    mu, target = loss_case(M, A, loss_type)
    d32 = mu - target
    exact = np.array_equal(d32.astype(np.float64), _d(mu, target))
    a = np.abs(d32)
    return dict(exact=bool(exact), inside=bool((a < 1).any()), outside=bool((a > 1).any()), at=bool((a == 1).any()),
                entries=int(a.size))
