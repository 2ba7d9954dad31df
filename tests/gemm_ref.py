"""Inputs and fp64 references for the bf16 GEMM family of csrc/ppo_mlp.hip (pmlp_gemm,
pmlp_gemm_pair) and its helper kernels, in plain torch; runs on the CPU and on the GPU.

Exact-grid inputs.  Activations / A operands are k/8 (k a uniform integer in [-16, 16]),
weights / B operands j/s (j in [-16, 16], s = 2^ceil(log2(19.2 sqrt(K)))) and biases i/8
(i in [-8, 8]); all are bf16 numbers.  Every product is a multiple of 1/(8 s) and every
partial sum, the bias included, is below K * 2 * (16/s) * 8 s + 8 s = 256 K + 8 s < 2^24 such
units, so an fp32 accumulator holds every partial sum exactly WHATEVER the order of the
additions (the order inside the matrix instruction included): the linear part of every
epilogue is compared with the fp64 product without a tolerance.  s is chosen so that the
pre-activations have a standard deviation of about 0.75: half of a hidden layer's outputs
are on the ELU's negative branch, and nearly all of those away from its ends.

What is compared (got == want is numeric equality of finite numbers: bit equality up to the
sign of a zero):
  FWD_OUT     A B^T + b                                     == the fp64 value
  FWD_HIDDEN  v = A B^T + b > 0:                            == RNE-bf16 of the fp64 value
              v < 0: bf16(expm1(v) - e) <= got <= bf16(expm1(v) + e), e = 2^-21
              v = 0: |got| <= e
  BWD_DX      bf16(acc * (y > 0 ? 1 : y + 1)), y = m/128    == RNE-bf16 of the fp64 value
              (m in [-128, 255]: y + 1 and the product are fp32 numbers)
  PARTIAL(_TN) each slab == the fp64 product over its own k range; the sum_col column ==
              the column sum of that range

The ELU margin e.  The kernel's negative branch is __expf(v) - 1 (elu() in
csrc/ppo_mlp.hip): v_exp_f32 on v log2(e).  The hardware exponential is good to about 1 ulp
(relative 2^-23 ... 2^-24 of e^v <= 1), scaling the argument adds a relative |v| 2^-24 to
e^v, i.e. at most |v| e^v 2^-24 <= 2^-24 / e absolute, and the subtraction of 1 is exact or
rounds to within 2^-25; together below 2^-23 absolute.  e = 2^-21 is four times that, still
a 1/64 of the bf16 spacing below -0.5 and at most one spacing near zero, so at most two bf16
values are ever acceptable and for all but a fraction of a percent of the elements only one.

Random-normal inputs (the second class: full-mantissa fp32 rows through the af operand form,
randn weights rounded to bf16) are compared with the fp64 product of the bf16-rounded
operands within e_acc = (K + 1) 2^-23 (sum_k |a_k w_k| + |b|): the forward error bound of a
length-K fp32 sum plus the bias in any order, with the unit roundoff doubled because the
matrix instruction's internal rounding is not documented.  bf16 outputs take the interval
[bf16(ELU(v - e_acc) - e), bf16(ELU(v + e_acc) + e)] (ELU and the rounding are monotonic;
e only where the negative branch can be taken).
"""
import math

import torch

BF16 = torch.bfloat16
E_ELU = 2.0 ** -21
SENTINEL = -12345.0  # prefill of guarded outputs; no result of these inputs comes near it

# k extents the GPU sweep uses (tests/test_gpu_gemm_reference.py); tests/test_gemm_ref_host.py
# asserts the exactness claim and the input conditions for every one of them
K_CLASSES = (16, 32, 40, 48, 64, 72, 128, 200, 256, 320)
LAYER_K = (48, 64, 128, 256, 448, 512)          # the PPO layer shapes (K0 and the hidden widths)
PARTIAL_KS = ((1000, 320), (1024, 256))          # (K, ksplit) of the slab-by-slab sweep
PAIR_KS = (512, 1024)                            # slab extents of the pmlp_gemm_pair cases
ALL_K = tuple(sorted(set(K_CLASSES + LAYER_K + tuple(ks for _, ks in PARTIAL_KS) + PAIR_KS)))


def grid_scale(k):
    return 2.0 ** math.ceil(math.log2(19.2 * math.sqrt(k)))


def gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def _ints(shape, lo, hi, g, device):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=device).to(torch.float32)


def grid_act(shape, g, device, dtype=BF16):
    """k/8, k in [-16, 16] (exact in bf16 and fp32)."""
    return (_ints(shape, -16, 16, g, device) / 8.0).to(dtype)


def grid_weight(shape, k, g, device, dtype=BF16):
    """j/s, j in [-16, 16], s = grid_scale(k) for a sum over k terms."""
    return (_ints(shape, -16, 16, g, device) / grid_scale(k)).to(dtype)


def grid_bias(n, g, device):
    return _ints((n,), -8, 8, g, device) / 8.0


def grid_yprev(shape, g, device):
    """m/128, m in [-128, 255]: ELU outputs with y + 1 exact; holds exactly -1 and (with more
    than one element) exactly 0."""
    y = _ints(shape, -128, 255, g, device) / 128.0
    f = y.view(-1)
    f[0] = -1.0
    if f.numel() > 1:
        f[-1] = 0.0
    return y.to(BF16)


def round_bf16(x):
    """Round-to-nearest-even of fp64 x to a bf16 number, returned as fp64 (one rounding from
    the fp64 value: no double rounding through fp32).  Normal range only."""
    b = x.to(torch.float64).contiguous().view(torch.int64)
    low = 1 << 45  # 52 - 7 mantissa bits dropped
    r = (b + (low // 2 - 1) + ((b >> 45) & 1)) & ~(low - 1)
    return r.view(torch.float64)


def bf16_ordinal(x):
    """Position of the bf16 numbers x (fp64) in the ordered list of bf16 numbers."""
    t = x.to(BF16).view(torch.int16).to(torch.int32)
    return torch.where(t < 0, -(t & 0x7FFF), t)


def _d(t):
    return t.to(torch.float64)


def _first_bad(bad, what, **vals):
    idx = tuple(int(i) for i in bad.nonzero()[0])
    shown = ", ".join(f"{k}={float(v[idx])!r}" for k, v in vals.items())
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first at {idx}: {shown}"


def assert_equal(got, want64, what):
    """Every element of got is finite and numerically equal to want64 (fp64 holding numbers
    of got's type)."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    g = _d(got)
    bad = ~(g == want64)  # (NaN compares unequal)
    if bool(bad.any()):
        raise AssertionError(_first_bad(bad, what, got=g, want=want64))


def assert_between(got, lo, hi, what):
    assert tuple(got.shape) == tuple(lo.shape), (what, tuple(got.shape), tuple(lo.shape))
    g = _d(got)
    bad = ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        raise AssertionError(_first_bad(bad, what, got=g, lo=lo, hi=hi))


def assert_fp32_exact(x64, what):
    """A condition of the exact-grid inputs: the fp64 value is an fp32 number."""
    assert bool((x64.to(torch.float32).to(torch.float64) == x64).all()), f"{what}: inputs are not on an exact grid"


def preact(a, w, bias=None):
    """fp64 A B^T (+ b): a [M, K], w [N, K]."""
    v = _d(a) @ _d(w).t()
    return v if bias is None else v + _d(bias)[None, :]


def elu_bounds(v, margin):
    """[lo, hi] (bf16 numbers as fp64) for bf16(ELU(v)) with the absolute margin on the negative
    branch: v > 0 -> lo = hi = bf16(v); v < 0 -> bf16(expm1(v) -+ margin); v = 0 -> -+ margin."""
    pos = v > 0
    ref = torch.where(pos, v, torch.expm1(v))
    m = torch.where(pos, torch.zeros_like(v), torch.zeros_like(v) + margin)
    lo, hi = round_bf16(ref - m), round_bf16(ref + m)
    zero = v == 0
    return torch.where(zero, -m, lo), torch.where(zero, m, hi)


class Conditions:
    """The conditions the exact-grid FWD_HIDDEN inputs must meet, counted over the cases of a
    test and asserted on the total (a single small output cannot meet a share)."""

    def __init__(self):
        self.n = self.neg = self.mid = self.amb = self.wide = 0

    def add(self, v, lo, hi):
        neg = v < 0
        elu = torch.expm1(v)
        width = bf16_ordinal(hi) - bf16_ordinal(lo)
        self.n += v.numel()
        self.neg += int(neg.sum())
        self.mid += int((neg & (elu > -0.95) & (elu < -0.05)).sum())
        self.amb += int((neg & (width == 1)).sum())
        self.wide += int(((v != 0) & (width > 1)).sum())
        assert self.wide == 0, "an acceptance interval holds more than two bf16 values"

    def assert_ok(self):
        assert self.n > 0
        assert 0.3 <= self.neg / self.n <= 0.7, f"negative-branch share {self.neg / self.n:.3f}"
        assert self.mid / self.n >= 0.3, f"share of ELU values in (-0.95, -0.05): {self.mid / self.n:.3f}"
        assert self.amb <= 0.01 * self.neg, f"{self.amb} of {self.neg} negative-branch intervals hold two bf16 values"
        assert self.wide == 0


def check_fwd_out(got, a, w, bias, what="FWD_OUT"):
    v = preact(a, w, bias)
    assert_fp32_exact(v, what)
    assert_equal(got, v, what)


def check_fwd_hidden(got, a, w, bias, cond=None, what="FWD_HIDDEN"):
    """got [M, N] bf16 against the exact-grid reference; every element is compared.  cond
    (a Conditions) collects the input conditions over a test's cases; an output of at least
    32 x 128 must meet them on its own.  (A column's bias, of the size of the product's
    standard deviation, moves the whole column: the shares are means over N independent
    columns, and below about a hundred columns one draw can leave 30-70 % by chance.)"""
    v = preact(a, w, bias)
    assert_fp32_exact(v, what)
    lo, hi = elu_bounds(v, E_ELU)
    own = Conditions()
    own.add(v, lo, hi)
    if v.shape[0] >= 32 and v.shape[1] >= 128:
        own.assert_ok()
    if cond is not None:
        cond.add(v, lo, hi)
    assert_between(got, lo, hi, what)


def bwd_dx_ref(dz, wt, yprev):
    """fp64 acc * (y > 0 ? 1 : y + 1): dz [M, K], wt [N, K] (the weight transposed), yprev [M, N]."""
    acc = preact(dz, wt)
    y = _d(yprev)
    return acc * torch.where(y > 0, torch.ones_like(y), y + 1.0)


def check_bwd_dx(got, dz, wt, yprev, what="BWD_DX"):
    y = _d(yprev)
    if y.numel() > 1:
        assert bool((y == -1).any()) and bool((y == 0).any()), f"{what}: yprev must hold -1 and 0"
    r = bwd_dx_ref(dz, wt, yprev)
    assert_fp32_exact(r, what)
    assert_equal(got, round_bf16(r), what)


def check_ct(ct, cb, what="ct"):
    """The transposed output [N, M] is the row-major output [M, N] transposed."""
    assert_equal(ct, _d(cb).t(), what + " == cb^T")


def check_partial(slabs, a_km, b_kn, ksplit, sums=None, what="PARTIAL"):
    """slabs [S, M, N] fp32: slab s == a_km[k0:k1]^T b_kn[k0:k1] over its own k range (a_km
    [K, M], b_kn [K, N]); sums [S, M] == the column sums of a_km over that range."""
    K = a_km.shape[0]
    S = (K + ksplit - 1) // ksplit
    assert slabs.shape[0] == S, (what, slabs.shape, S)
    a, b = _d(a_km), _d(b_kn)
    for s in range(S):
        k0, k1 = s * ksplit, min(K, (s + 1) * ksplit)
        ref = a[k0:k1].t() @ b[k0:k1]
        assert_fp32_exact(ref, what)
        assert_equal(slabs[s], ref, f"{what} slab {s} (k {k0}..{k1})")
        if sums is not None:
            assert_equal(sums[s], a[k0:k1].sum(0), f"{what} sum_col of slab {s}")


# ---- the random-normal class
def e_acc(a, w, bias=None):
    """(K + 1) 2^-23 (sum_k |a_k w_k| + |b|) per output element (fp64)."""
    K = a.shape[1]
    mag = _d(a).abs() @ _d(w).abs().t()
    if bias is not None:
        mag = mag + _d(bias).abs()[None, :]
    return (K + 1) * 2.0 ** -23 * mag


def check_fwd_out_bound(got, a, w, bias, what="FWD_OUT (randn)"):
    v, ea = preact(a, w, bias), e_acc(a, w, bias)
    assert_between(got, v - ea, v + ea, what)


def hidden_bounds_bound(a, w, bias):
    v, ea = preact(a, w, bias), e_acc(a, w, bias)
    lo_v, hi_v = v - ea, v + ea
    m = torch.where(lo_v <= 0, torch.zeros_like(v) + E_ELU, torch.zeros_like(v))
    elu = lambda x: torch.where(x > 0, x, torch.expm1(x))  # noqa: E731
    return round_bf16(elu(lo_v) - m), round_bf16(elu(hi_v) + m)


def check_fwd_hidden_bound(got, a, w, bias, what="FWD_HIDDEN (randn)"):
    lo, hi = hidden_bounds_bound(a, w, bias)
    assert_between(got, lo, hi, what)


# ---- outputs with a guard band
class Guarded:
    """An output [slabs, rows, ld] inside a larger buffer prefilled with SENTINEL: `guard`
    elements in front of it, `extra` rows and `guard` elements behind it.  .t is the tensor a
    kernel is given (.mat = its first slab), .got(cols) what it wrote, and assert_untouched
    checks that everything outside [rows, cols] (+ the named extra columns) still holds the
    sentinel: the columns cols..ld-1, the rows past the last, the band around the buffer."""

    def __init__(self, rows, cols, ld, dtype, device, slabs=1, extra=2, guard=64):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.slabs, self.guard = rows, cols, ld, slabs, guard
        self.n = slabs * rows * ld
        self.flat = torch.full((guard + self.n + extra * ld + guard,), SENTINEL, dtype=dtype, device=device)
        self.t = self.flat[guard:guard + self.n].view(slabs, rows, ld)
        self.mat = self.t[0]
        self.sentinel = torch.tensor(SENTINEL, dtype=dtype, device=device)

    def got(self, col=None):
        """The written region [slabs, rows, cols] ([rows, cols] of a single slab), or the one
        column `col` [slabs, rows]."""
        r = self.t[:, :, :self.cols] if col is None else self.t[:, :, col]
        return r[0] if self.slabs == 1 and col is None else r

    def assert_untouched(self, what, extra_cols=()):
        mask = torch.ones(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        m = mask[self.guard:self.guard + self.n].view(self.slabs, self.rows, self.ld)
        m[:, :, :self.cols] = False
        for c in extra_cols:
            m[:, :, c] = False
        bad = mask & ~(self.flat == self.sentinel)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the output were written " \
                                    f"(first at flat offset {int(bad.nonzero()[0]) - self.guard}, ld {self.ld})"


def same_bits(a, b):
    """Two buffers of one type hold the same bits."""
    iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(iv), b.view(iv))


def tile_config(epi, M, N, K, njobs):
    """The tile configuration pmlp_gemm's selection (csrc/ppo_mlp.hip) picks for a batch with
    these maxima: (BM, BN, WM, WN).  epi as include/ppo_mlp.h's enum."""
    part = epi in (3, 4)
    if M <= 32:
        return (32, 128, 1, 4)
    if N <= 32:
        return (128, 32, 4, 1)
    if N <= 64:
        return (128, 64, 4, 1)
    if not part and ((M + 127) // 128) * ((N + 127) // 128) * njobs < 512:
        return (64, 64, 2, 2)
    return (128, 128, 2, 2) if (epi == 0 and K >= 256) else (128, 128, 2, 4)
