"""fp64 references, input builders, bounds and comparison functions for the recurrent kernels
(csrc/lstm_seq.hip, gru_seq.hip, heads.hip, seq_mfma.h), in the pattern of ppo_ref.py.  Plain
numpy on the CPU.  tests/test_gpu_seq_reference.py applies the checks to the kernels,
tests/test_seq_ref_host.py applies them to float32 emulations (which must pass) and to
deliberately wrong emulations (which must be rejected).

One step at a time.  A free-running comparison over T steps needs a bound that compounds; the
kernels save the state every step starts from, so the checks go by induction instead:

  chain     the saved operand row is what the recurrence says, bitwise: xh[t, :, :I] == x[t],
            the h columns (or hp) are h0 at t = 0, zero where reset[t], else h_out[t-1], the last
            column is 1; h_save / c_save are the state step 0 started from.  Absent h0 / c0 /
            reset mean zeros / no resets.
  gate      gact[t] against the activation of the fp64 pre-activation of the operand row the
            kernel saved (for the wide form: of its own gx[t] and hp[t]).
  cell      c_out[t] from the kernel's own gact[t] and the carried c (c0, zero where reset[t],
            else the kernel's c_out[t-1]).
  out       h_out[t] from the kernel's own gact[t] and c_out[t].

u = 2^-24 is the unit roundoff of fp32 throughout.

Pre-activation of the matrix-core forms (SPLIT = 2^-15).  Every operand v is split into
hi = bf16(v), lo = bf16(v - hi): |lo| <= 2^-9 |v| and the residual |v - hi - lo| <= 2^-18 |v|.
The product keeps hi.hi + hi.lo + lo.hi; what it omits of a.w is lo.lo plus the two residual
cross terms, <= 3 * 2^-18 |a||w| < 2^-16 |a||w|.  The products are exact in fp32 (8 x 8 bit
significands) and are accumulated in fp32 from the fp32 bias; the project's derivation
(test_wide_projection_matches_fp64) allows K 2^-24 sum|a||w| <= 2^-17 sum|a||w| for K <= 128
additions and takes, as this file does,
    e_z = 2^-15 sum_k |a_k||w_k|
over the operand row [x | h_prev | 1] . [W_ih | W_hh | b_ih + b_hh] (the bias is the product
with the ones column).  The gx-fed (wide) form starts the accumulators from the kernel's own gx,
an fp32 number that is not split and takes part in the additions only.  The 3 * 64 products are
added to it, so it passes through at most 192 fp32 additions, each of which rounds the running
sum by at most u times its magnitude; the share of those roundings that falls on the products is
inside 2^-15 sum|h||w| as above, the share that falls on gx is at most 192 u |gx|:
    e_z = 2^-15 sum|h||w| + 192 u |gx|.
Emulated on the CPU with correctly rounded splits the worst element sits below a tenth of e_z;
an emulation that drops the hi.lo term leaves it on most elements (test_seq_ref_host.py prints
both).

Pre-activation of the fp32 VALU kernels: an fmaf chain from the fp32 sum b_ih + b_hh (or from gx)
over n = I + H products: the any-order fp32 summation bound (n + 1) u (sum|a||w| + |b_ih| + |b_hh|),
as gemm_ref.py's e_acc without its doubling (fmaf and the fp32 addition are IEEE operations).

Activations.  ASSUMPTIONS: no document on the accuracy of v_exp_f32, v_rcp_f32, expf, tanhf or
expm1f was at hand when this was written.  The hardware exp2 and reciprocal are ASSUMED accurate
to 1 ulp = 2u relative, expf to 1 ulp, tanhf and expm1f to 2 ulp, and the fp32 division is
ASSUMED correctly rounded.  None of these figures is taken from a source; if one turns up, the
budgets below are to be recomputed from it.  Each budget counts the roundings to first order and
is then doubled, as ppo_ref.py does for Adam.
  fsig(x) = rcp(1 + __expf(-x)), __expf(y) = exp2(y * log2e): the rounded constant and the
    rounded product move the exponent by 2u |x| log2e, i.e. e = exp(-x) by 2u |x| relative; exp2
    adds 2u; the sum 1 + e adds u and the reciprocal 2u, both relative to the result s.  The
    result's sensitivity to e is s (1 - s):
        B_sig(x) = 2 u (3 s + s (1 - s) (2 |x| + 2)).
  ftanh(x) = 2 rcp(1 + __expf(-2x)) - 1 (the factors of 2 are exact), r = (1 + t) / 2:
    r is off by u (3 r + r (1 - r) (4 |x| + 2)), the result by twice that plus u |t| for the
    last subtraction:
        B_tanh(x) = 2 u (3 (1 + t) + (1 - t^2) (2 |x| + 1) + |t|),
    which keeps an absolute term near 0 (8u at x = 0), where 2r - 1 cancels.  With every
    operation correctly rounded a numpy emulation stays within 1.6u (fsig) and 3.1u (ftanh) on
    [-20, 20]; the budgets are 4u and 8u at 0 and clear that floor everywhere
    (test_seq_ref_host.py asserts it).
  VALU: sigm(x) = 1 / (1 + expf(-x)): B = 2 u (2 s + 2 s (1 - s)); tanhf: B = 8 u |t|.
A gate is compared with act(z) where z is known to e_z only.  The activations are monotonic, so
the gate lies in [act(z - e_z) - B, act(z + e_z) + B] exactly, no linearisation.

Cell and output, from the kernel's own fp32 gates: c = f c_prev + i g is two products and a sum
(or an fma): 3 roundings of at most u (|f c_prev| + |i g|), doubled: 6 u (|f c_prev| + |i g|).
h = o ftanh(c): o B_tanh(c) + 2 u |h|.  Where the gates are not saved (the in-place steps) the
gates' bounds are multiplied through: |c_prev| e_f + |g| e_i + |i| e_g + e_i e_g, and the
output takes tanh over [c - e_c, c + e_c].

Backward.  Its inputs are plain arrays.  Where the kernel writes the gate gradients they are
checked step by step: the matrix part of the carried gradient, dh_{t-1} = dG_t . W_hh, is formed
in fp64 from the kernel's own dgx[t] with the split bound 2^-15 sum|dg||w| (the fp32 kernel:
(4H + 3) u sum|dg||w|); the elementwise carry the kernel does not write (the LSTM's dc . f, the
GRU's dh . z) runs free in fp64 with its bound propagated, which stays small because it is
multiplied by gate values below 1.  Every product of the gate-gradient formulas contributes
one rounding, doubled; 1 - g^2 and 1 - tanh(c)^2 cancel and get the absolute term
u (g^2 + |1 - g^2|).  Nothing flows across a reset or into the state before step 0: there the
reference's carried terms and their bounds are exactly zero, so the bound that remains is the
few roundings of that one step.

Weight-gradient slabs.  Where dgx is written too (the wide form) slab row b is the fp64 sum of
dgx_kernel^T [h_prev | 1] over workgroup b's 16 envs and the T steps, and slab_ih row c the sum
of dgx_kernel^T x over its 512 rows, torch row order, row by row, within
(2^-15 + n u) sum|dg||xh| (n terms: the split bound and the any-order summation bound).  The
narrow form does not write dgx: its reference is the free-running fp64 backward, the gate
gradients' bound propagated to first order through |W_hh| and the actual gate values and
doubled for the second-order terms.  The condition of that check (T <= 4) is asserted for
every case: the bound of every slab element stays below a quarter of 2^-9 sum|dg||xh|, what a
dropped cross term is worth there.

Exact grids.  x and h0 are k/8 (|k| <= 16), weights j/64 (|j| <= 8), biases i/8: all bf16
numbers (lo = 0), every product a multiple of 2^-9 and every partial sum of K <= 128 of them
an fp32 number, in any order, so the pre-activations are exact and the gates are left with
the activation budget alone.  The heads' grids make every sum of the forward (on rows whose y0
is positive) and of the backward exact, so those are compared for equality, per block of 128
rows; the ELU's negative branch calls expm1f, assumed 2 ulp (above), doubled: B = 8 u |expm1(z)|.
"""
import numpy as np

U = 2.0 ** -24
SPLIT = 2.0 ** -15
MH = 64
ME = 16          # envs per workgroup of the matrix-core kernels
WDR = 512        # rows per slab_ih chunk (k_lstm_dwih_wide)
HEAD_ROWS = 128  # rows per slab row of pmlp_heads_backward
F = np.float32
D = np.float64


class CheckFailed(AssertionError):
    """A comparison failed; .check names which one (chain, gate, cell, out, save, dgx, slab ...)."""

    def __init__(self, check, msg):
        super().__init__(f"[{check}] {msg}")
        self.check = check


class Stats(dict):
    """Worst measured fraction of each bound, by check name."""

    def add(self, name, frac):
        self[name] = max(self.get(name, 0.0), float(frac))

    def line(self, what):
        return f"{what}: worst fraction of the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.items()))


def d(a):
    return None if a is None else np.asarray(a, dtype=D)


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def equal(check, got, want, what):
    """Every element finite and numerically equal (-0 == 0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise CheckFailed(check, f"{what}: shape {got.shape} != {want.shape}")
    bad = ~(np.isfinite(got) & (got == want))
    if bad.any():
        i = _first(bad)
        raise CheckFailed(check, f"{what}: {int(bad.sum())} of {bad.size} differ, first at {i}: "
                                 f"got {got[i]!r}, want {want[i]!r}")


def within(check, got, want, bound, what, stats=None):
    """|got - want| <= bound per element, got finite.  Records the worst err / bound."""
    got, want, bound = d(got), d(want), d(bound)
    if got.shape != want.shape:
        raise CheckFailed(check, f"{what}: shape {got.shape} != {want.shape}")
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got - want)
    bad = ~np.isfinite(got) | ~(err <= bound)
    if stats is not None and not bad.any():
        pos = bound > 0
        if pos.any():
            stats.add(check, (err[pos] / bound[pos]).max())
    if bad.any():
        i = _first(bad)
        raise CheckFailed(check, f"{what}: {int(bad.sum())} of {bad.size} outside the bound, first at {i}: "
                                 f"got {got[i]!r}, want {want[i]!r}, |err| {err[i]:.3e}, bound {bound[i]:.3e}")


# ------------------------------------------------------------------ activations --
def sig(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-d(z)))


def b_fsig(z):
    s = sig(z)
    return 2 * U * (3 * s + s * (1 - s) * (2 * np.abs(z) + 2))


def b_ftanh(z):
    t = np.tanh(z)
    return 2 * U * (3 * (1 + t) + (1 - t * t) * (2 * np.abs(z) + 1) + np.abs(t))


def b_vsig(z):
    s = sig(z)
    return 2 * U * (2 * s + 2 * s * (1 - s))


def b_vtanh(z):
    return 8 * U * np.abs(np.tanh(z))


ACT = {"mfma": (b_fsig, b_ftanh), "valu": (b_vsig, b_vtanh)}


def act_bound(fn, budget, z, ez):
    """(act(z), bound) for an activation of a pre-activation known to ez: monotonic fn, so the
    interval is [fn(z - ez), fn(z + ez)] widened by the function's own budget."""
    v, lo, hi = fn(z), fn(z - ez), fn(z + ez)
    return v, np.maximum(hi - v, v - lo) + np.maximum(budget(z), np.maximum(budget(z - ez), budget(z + ez)))


# ----------------------------------------------------------------- input builders --
RESET_PATTERNS = ("none", "t0", "last", "twice", "all", "tail", "mixed")


def reset_pattern(name, T, B, rng):
    """[T, B] uint8 or None.  t0: some envs at t = 0; last: some at T - 1; twice: one env on two
    consecutive steps; all: every env at one step; tail: env B - 1; mixed: all of these and 15 %."""
    if name == "none":
        return None
    r = np.zeros((T, B), np.uint8)
    some = rng.random(B) < 0.4
    some[rng.integers(B)] = True
    if name in ("t0", "mixed"):
        r[0, some] = 1
    if name in ("last", "mixed"):
        r[T - 1, np.roll(some, 1)] = 1
    if name in ("twice", "mixed"):
        e = int(rng.integers(B))
        r[max(T - 2, 0), e] = r[T - 1, e] = 1
        r[0, e] = r[min(1, T - 1), e] = 1
    if name in ("all",):
        r[T // 2, :] = 1
    if name in ("tail", "mixed"):
        r[T // 2, B - 1] = 1
        r[T - 1, B - 1] = 1
    if name == "mixed":
        r |= (rng.random((T, B)) < 0.15).astype(np.uint8)
    return r


def seq_case(seed, T, B, I, H=MH, gates=4, h0=True, c0=True, reset="mixed", wscale=0.25):
    """Random-normal inputs of one memory (gates = 4: LSTM, 3: GRU), float32."""
    rng = np.random.default_rng(seed)
    c = dict(T=T, B=B, I=I, H=H,
             x=rng.standard_normal((T, B, I)).astype(F),
             w_ih=rng.uniform(-wscale, wscale, (gates * H, I)).astype(F),
             w_hh=rng.uniform(-wscale, wscale, (gates * H, H)).astype(F),
             b_ih=rng.uniform(-wscale, wscale, gates * H).astype(F),
             b_hh=rng.uniform(-wscale, wscale, gates * H).astype(F),
             h0=(0.5 * rng.standard_normal((B, H))).astype(F) if h0 else None,
             c0=(0.5 * rng.standard_normal((B, H))).astype(F) if (c0 and gates == 4) else None,
             reset=reset_pattern(reset, T, B, rng),
             dh_out=rng.standard_normal((T, B, H)).astype(F))
    return c


def ones_case(seed, B, I, gates=4):
    """T = 1, every operand positive with an all-ones mantissa, (2 - 2^-23) 2^e, biases zero.  A
    round-to-nearest split of such a value is exact (hi = 2^(e+1), lo = -2^(e-23)); a truncating
    split leaves 2^-16 of it behind and every product's error has the same sign, about
    3 * 2^-16 |a||w|, 1.5 times the bound.  The pre-activations stay between 1 and 4, where the
    sigmoid still passes a sixteenth to a fifth of that on."""
    rng = np.random.default_rng(seed)
    one = np.float32(2.0) - np.float32(2.0 ** -23)
    k = (I + MH) / 111.0
    pw = lambda lo, hi, shape: (one * np.exp2(rng.integers(lo, hi + 1, shape))).astype(F)  # noqa: E731
    c = seq_case(seed, 1, B, I, gates=gates, reset="none")
    c["x"], c["h0"] = pw(-2, -1, (1, B, I)), pw(-2, -1, (B, MH))
    wexp = -6 if k > 0.75 else -5
    c["w_ih"], c["w_hh"] = pw(wexp - 1, wexp, (gates * MH, I)), pw(wexp - 1, wexp, (gates * MH, MH))
    c["b_ih"], c["b_hh"] = np.zeros(gates * MH, F), np.zeros(gates * MH, F)
    return c


def narrow_bwd_case(seed, T, B, I, c0=True, reset="mixed"):
    """Test-built inputs of pmlp_lstm_bwd_dw_mfma_jobs (plain arrays: gact, c_out, xh, dh_out, c0,
    reset, w_hh), every factor of the gate-gradient formulas bounded away from 0 and from the
    cancelling ends (|c| in [0.2, 1.2], sigmoid gates in [0.1, 0.9], |g| in [0.1, 0.9], |dh| in
    [0.25, 1] with one sign per (env, unit) over the steps, so that dc = dc . f + .. adds terms of
    one sign; |W_hh| <= 1/32 so that the carried dG . W_hh and its split bound stay small beside
    dh_out), so that no slab element is a small difference of large terms and the free-running
    reference's bound stays far below a dropped cross term (narrow_slab_condition)."""
    rng = np.random.default_rng(seed)
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    c = dict(T=T, B=B, I=I, H=MH, w_hh=rng.uniform(-2.0 ** -5, 2.0 ** -5, (4 * MH, MH)).astype(F),
             c0=(sgn((B, MH)) * rng.uniform(0.2, 1.2, (B, MH))).astype(F) if c0 else None,
             reset=reset_pattern(reset, T, B, rng),
             dh_out=(sgn((1, B, MH)) * rng.uniform(0.25, 1.0, (T, B, MH))).astype(F))
    s = lambda: rng.uniform(0.1, 0.9, (T, B, MH))  # noqa: E731
    fwd = dict(gact=np.concatenate([s(), s(), sgn((T, B, MH)) * s(), s()], -1).astype(F),
               c_out=(sgn((T, B, MH)) * rng.uniform(0.2, 1.2, (T, B, MH))).astype(F),
               xh=np.concatenate([rng.standard_normal((T, B, I)), 0.5 * rng.standard_normal((T, B, MH)),
                                  np.ones((T, B, 1))], -1).astype(F))
    return c, fwd


def _sig_bits(v, unit):
    """Significant bits of the largest |v| counted in units."""
    m = float(np.abs(v).max()) / unit
    return 0 if m < 1 else int(np.floor(np.log2(m))) + 1


def grid_case(seed, B, I, gates=4, reset0=False):
    """T = 1 on the exact grid: x, h0 = k/8 (|k| <= 16), weights j/64 (|j| <= 8), biases i/8
    (|i| <= 8), c0 = k/8.  Asserts the exactness: every value is a bf16 number, the fp64
    pre-activation survives float32, and the largest sum of |products| (which bounds every
    partial sum in any order) needs at most 24 bits of the products' unit 2^-9."""
    rng = np.random.default_rng(seed)
    gi = lambda lo, hi, shape, den: (rng.integers(lo, hi + 1, shape) / den).astype(F)  # noqa: E731
    c = dict(T=1, B=B, I=I, H=MH, x=gi(-16, 16, (1, B, I), 8.0), w_ih=gi(-8, 8, (gates * MH, I), 64.0),
             w_hh=gi(-8, 8, (gates * MH, MH), 64.0), b_ih=gi(-8, 8, gates * MH, 8.0), b_hh=gi(-8, 8, gates * MH, 8.0),
             h0=gi(-16, 16, (B, MH), 8.0), c0=gi(-16, 16, (B, MH), 8.0) if gates == 4 else None,
             reset=None, dh_out=gi(-16, 16, (1, B, MH), 8.0))
    if reset0:
        c["reset"] = np.zeros((1, B), np.uint8)
        c["reset"][0, ::3] = 1
    assert_grid_exact(c, gates)
    return c


def assert_grid_exact(c, gates=4):
    import torch
    for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0"):
        t = torch.from_numpy(c[k])
        assert bool((t.to(torch.bfloat16).to(torch.float32) == t).all()), f"{k}: not bf16 numbers"
    hp = h_prev_expected(c, None)[0]
    row = np.concatenate([d(c["x"][0]), d(hp)], axis=1)
    w = np.concatenate([d(c["w_ih"]), d(c["w_hh"])], axis=1)
    b = d(c["b_ih"]) + d(c["b_hh"])
    z = row @ w.T + b
    assert (z.astype(F).astype(D) == z).all(), "the pre-activation is not an fp32 number"
    total = np.abs(row) @ np.abs(w).T + np.abs(d(c["b_ih"])) + np.abs(d(c["b_hh"]))
    bits = _sig_bits(total, 2.0 ** -9)
    assert bits <= 24, f"partial sums need {bits} bits"
    # (gates == 3: the n gate's n_x and n_h halves are separate sums over subsets of the terms
    # counted in `total`, so their partial sums need no more bits than checked here)
    return bits


# ------------------------------------------------------------------- the recurrence --
def h_prev_expected(c, h_out):
    """[T, B, H]: the state every step starts from, given the kernel's h_out."""
    T, B, H = c["T"], c["B"], c["H"]
    hp = np.zeros((T, B, H), F)
    if c.get("h0") is not None:
        hp[0] = c["h0"]
    if T > 1:
        hp[1:] = h_out[:-1]
    if c.get("reset") is not None:
        hp[c["reset"] != 0] = 0
    return hp


def c_prev_expected(c, c_out):
    T, B, H = c["T"], c["B"], c["H"]
    cp = np.zeros((T, B, H), F)
    if c.get("c0") is not None:
        cp[0] = c["c0"]
    if T > 1:
        cp[1:] = c_out[:-1]
    if c.get("reset") is not None:
        cp[c["reset"] != 0] = 0
    return cp


def check_chain(c, out, what, saved_after_reset=True):
    """The saved operand rows and the saved initial state, bitwise."""
    I, H = c["I"], c["H"]
    hp = h_prev_expected(c, out["h_out"])
    if out.get("xh") is not None:
        xh = out["xh"]
        equal("chain", xh[..., :I], c["x"], f"{what}: xh[..., :I] == x")
        equal("chain", xh[..., I:I + H], hp, f"{what}: xh's h columns == h_prev")
        equal("chain", xh[..., I + H], np.ones(xh.shape[:2], F), f"{what}: xh's last column == 1")
    if out.get("hp") is not None:
        equal("chain", out["hp"][..., :H], hp, f"{what}: hp == h_prev")
        equal("chain", out["hp"][..., H], np.ones(hp.shape[:2], F), f"{what}: hp's last column == 1")
    for k, src in (("h_save", "h0"), ("c_save", "c0")):
        if out.get(k) is not None:
            s = np.zeros((c["B"], H), F) if c.get(src) is None else c[src].copy()
            if saved_after_reset and c.get("reset") is not None:
                s[c["reset"][0] != 0] = 0
            equal("save", out[k], s, f"{what}: {k} == the state step 0 starts from")
    return hp


def _row_w(c, hp):
    """fp64 operand rows [T, B, I + H + 1] and weights [G, I + H + 1] = [W_ih | W_hh | b_ih + b_hh]."""
    row = np.concatenate([d(c["x"]), d(hp), np.ones(hp.shape[:2] + (1,))], axis=-1)
    w = np.concatenate([d(c["w_ih"]), d(c["w_hh"]), (d(c["b_ih"]) + d(c["b_hh"]))[:, None]], axis=1)
    return row, w


def lstm_preact(c, hp, form, gx=None):
    """(z, e_z) [T, B, 4H] of the form: 'x' (matrix-core, x-fed), 'gx' (matrix-core from the
    kernel's gx), 'valu_x', 'valu_gx' (fp32 kernels)."""
    H = c["H"]
    if form in ("x", "valu_x"):
        row, w = _row_w(c, hp)
        z = row @ w.T
        if form == "x":
            return z, SPLIT * (np.abs(row) @ np.abs(w).T)
        wa = np.concatenate([np.abs(d(c["w_ih"])), np.abs(d(c["w_hh"])),
                             (np.abs(d(c["b_ih"])) + np.abs(d(c["b_hh"])))[:, None]], axis=1)
        return z, (c["I"] + H + 1) * U * (np.abs(row) @ wa.T)
    hw = np.abs(d(hp)) @ np.abs(d(c["w_hh"])).T
    z = d(gx) + d(hp) @ d(c["w_hh"]).T
    if form == "gx":
        return z, SPLIT * hw + 3 * H * U * np.abs(d(gx))
    return z, (H + 1) * U * (hw + np.abs(d(gx)))


def check_wide_gx(c, gx, what, stats=None):
    """The wide form's projection gx = x W_ih^T + b_ih + b_hh within 2^-15 (sum|x||w| + |b|)."""
    x, w = d(c["x"]), d(c["w_ih"])
    b = d(c["b_ih"]) + d(c["b_hh"])
    within("gx", gx, x @ w.T + b, SPLIT * (np.abs(x) @ np.abs(w).T + np.abs(b)), f"{what}: gx", stats)


def lstm_fwd_check(c, out, form="x", stats=None, what="lstm fwd", exact=False):
    """The LSTM forward of any form, step by step (module docstring).  out: h_out, c_out
    [T, B, H]; gact [T, B, 4H], xh / hp, gx, h_save, c_save where the entry writes them (None or
    absent otherwise: the in-place steps save no gates and their bounds are multiplied through).
    exact: the inputs are on the exact grid, the pre-activation carries no error."""
    H = c["H"]
    kind = "valu" if form.startswith("valu") else "mfma"
    bs, bt = ACT[kind]
    hp = check_chain(c, out, what, saved_after_reset=(kind == "mfma"))
    z, ez = lstm_preact(c, hp, form, out.get("gx") if form == "gx" else c.get("gx"))
    if exact:
        ez = np.zeros_like(ez)
    want, eb = [], []
    for q in range(4):
        zz, ee = z[..., q * H:(q + 1) * H], ez[..., q * H:(q + 1) * H]
        v, b = act_bound(np.tanh, bt, zz, ee) if q == 2 else act_bound(sig, bs, zz, ee)
        want.append(v)
        eb.append(b)
    gact = out.get("gact")
    if gact is not None:
        within("gate", gact, np.concatenate(want, -1), np.concatenate(eb, -1), f"{what}: gact", stats)
        ig, fg, gg, og = (d(gact[..., q * H:(q + 1) * H]) for q in range(4))
        ei = ef = eg = eo = 0.0
    else:
        (ig, fg, gg, og), (ei, ef, eg, eo) = want, eb
    if gact is not None or c["T"] == 1:
        cp = d(c_prev_expected(c, out["c_out"]))
    else:
        raise ValueError("a sequence without gact cannot be checked step by step")
    cw = fg * cp + ig * gg
    ec = np.abs(cp) * ef + np.abs(gg) * ei + np.abs(ig) * eg + ei * eg + 6 * U * (np.abs(fg * cp) + np.abs(ig * gg))
    within("cell", out["c_out"], cw, ec, f"{what}: c_out", stats)
    if gact is not None:
        ck, ech = d(out["c_out"]), 0.0
    else:
        ck, ech = cw, ec
    tc, et = act_bound(np.tanh, bt, ck, ech)
    hw = og * tc
    eh = np.abs(tc) * eo + (og + eo) * et + 2 * U * np.abs(hw)
    within("out", out["h_out"], hw, eh, f"{what}: h_out", stats)


def grid_lstm_check(c, out, stats=None, what="lstm grid"):
    """T = 1 on the exact grid: the gates within the activation budget alone."""
    assert_grid_exact(c, 4)
    lstm_fwd_check(c, out, "x", stats, what, exact=True)


def grid_act_errors(c, out):
    """(max |fsig error|, max |ftanh error|) in units of u over an exact-grid LSTM case's gates:
    the activations measured alone."""
    H = c["H"]
    z, _ = lstm_preact(c, h_prev_expected(c, out["h_out"]), "x")
    g = d(out["gact"])
    es = max(float(np.abs(g[..., q * H:(q + 1) * H] - sig(z[..., q * H:(q + 1) * H])).max()) for q in (0, 1, 3))
    et = float(np.abs(g[..., 2 * H:3 * H] - np.tanh(z[..., 2 * H:3 * H])).max())
    return es / U, et / U


# ------------------------------------------------------------------ LSTM backward --
def lstm_bwd_ref(c, fwd, dgx_k=None, kind="mfma"):
    """fp64 gate gradients [T, B, 4H] and their bound from the backward's own inputs (fwd: gact,
    c_out; c: w_hh, c0, reset, dh_out).  dgx_k: the kernel's gate gradients; the matrix part of the
    carried dh is then formed from them (step-by-step check).  None: free-running, the bound of
    dG . W_hh propagated through |W_hh|."""
    T, B, H = c["T"], c["B"], c["H"]
    bt = ACT[kind][1]
    w = d(c["w_hh"])
    wa = np.abs(w)
    em = SPLIT if kind == "mfma" else (4 * H + 3) * U
    gact, c_out, dh_out = d(fwd["gact"]), d(fwd["c_out"]), d(c["dh_out"])
    cp_all = d(c_prev_expected(c, fwd["c_out"]))
    rs = np.zeros((T, B), bool) if c.get("reset") is None else c["reset"] != 0
    dg, eg = np.zeros((T, B, 4 * H)), np.zeros((T, B, 4 * H))
    dhn = e_dhn = dcn = e_dcn = np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        ig, fg, gg, og = (gact[t][:, q * H:(q + 1) * H] for q in range(4))
        cp = cp_all[t]
        dh = dh_out[t] + dhn
        e_dh = e_dhn + 2 * U * np.abs(dh)
        tc = np.tanh(c_out[t])
        e_tc = bt(c_out[t])
        q1 = 1 - tc * tc
        e_q1 = 2 * np.abs(tc) * e_tc + 2 * U * (tc * tc + np.abs(q1))
        s = dh * og * q1
        e_s = e_dh * np.abs(og * q1) + np.abs(dh * og) * e_q1 + 4 * U * np.abs(s)
        dc = dcn + s
        e_dc = e_dcn + e_s + 2 * U * np.abs(dc)
        q2 = 1 - gg * gg
        e_q2 = 2 * U * (gg * gg + np.abs(q2))
        v = [dc * gg * ig * (1 - ig), dc * cp * fg * (1 - fg), dc * ig * q2, dh * tc * og * (1 - og)]
        e = [e_dc * np.abs(gg * ig * (1 - ig)) + 8 * U * np.abs(v[0]),
             e_dc * np.abs(cp * fg * (1 - fg)) + 8 * U * np.abs(v[1]),
             e_dc * np.abs(ig * q2) + np.abs(dc * ig) * e_q2 + 4 * U * np.abs(v[2]),
             e_dh * np.abs(tc * og * (1 - og)) + np.abs(dh * og * (1 - og)) * e_tc + 8 * U * np.abs(v[3])]
        dg[t], eg[t] = np.concatenate(v, 1), np.concatenate(e, 1)
        keep = ~rs[t][:, None]
        dcn = np.where(keep, dc * fg, 0.0)
        e_dcn = np.where(keep, e_dc * fg + 2 * U * np.abs(dc * fg), 0.0)
        src = dg[t] if dgx_k is None else d(dgx_k[t])
        e_src = eg[t] if dgx_k is None else np.zeros_like(eg[t])
        dhn = np.where(keep, src @ w, 0.0)
        e_dhn = np.where(keep, e_src @ wa + em * (np.abs(src) @ wa), 0.0)
    return dg, eg


def lstm_bwd_check(c, fwd, dgx, kind="mfma", stats=None, what="lstm bwd"):
    """dgx [T, B, 4H] step by step against the fp64 formulas on the kernel's own dgx[t + 1]."""
    dg, eg = lstm_bwd_ref(c, fwd, dgx, kind)
    within("dgx", dgx, dg, eg, f"{what}: dgx", stats)


def slab_terms(dg, rows, B, I, H=MH):
    """The per-workgroup sums dG^T rows over the T steps: [nblk, 4H, RL] and the same of the
    absolute values (dg [T, B, 4H], rows [T, B, RL])."""
    nblk = (B + ME - 1) // ME
    out = np.zeros((nblk, dg.shape[-1], rows.shape[-1]))
    mag = np.zeros_like(out)
    for b in range(nblk):
        g = dg[:, b * ME:(b + 1) * ME].reshape(-1, dg.shape[-1])
        r = rows[:, b * ME:(b + 1) * ME].reshape(-1, rows.shape[-1])
        out[b] = g.T @ r
        mag[b] = np.abs(g).T @ np.abs(r)
    return out, mag


def slab_layout(s, I, H=MH):
    """[nblk, 4H, I + H + 1] -> the kernel's slab rows [dW_ih (4H x I) | dW_hh (4H x H) | db (4H)]."""
    n = s.shape[0]
    return np.concatenate([s[:, :, :I].reshape(n, -1), s[:, :, I:I + H].reshape(n, -1), s[:, :, I + H]], axis=1)


def wide_slab_check(c, hp, dgx, slab, slab_ih, stats=None, what="wide bwd"):
    """slab [nblk, 256 * 65] and slab_ih [chunks, 256 * I] from the kernel's own dgx, row by row."""
    T, B, I = c["T"], c["B"], c["I"]
    s, m = slab_terms(d(dgx), d(hp), B, 0)
    within("slab", slab, slab_layout(s, 0), (SPLIT + ME * T * U) * slab_layout(m, 0), f"{what}: slab", stats)
    g, x = d(dgx).reshape(T * B, -1), d(c["x"]).reshape(T * B, I)
    nch = (T * B + WDR - 1) // WDR
    want = np.stack([g[k * WDR:(k + 1) * WDR].T @ x[k * WDR:(k + 1) * WDR] for k in range(nch)])
    mag = np.stack([np.abs(g[k * WDR:(k + 1) * WDR]).T @ np.abs(x[k * WDR:(k + 1) * WDR]) for k in range(nch)])
    within("slab_ih", slab_ih, want.reshape(nch, -1), (SPLIT + WDR * U) * mag.reshape(nch, -1), f"{what}: slab_ih",
           stats)


def narrow_slab_ref(c, fwd):
    """(want, bound, cross) of pmlp_lstm_bwd_dw_mfma_jobs' slab rows from the free-running fp64
    backward; cross = 2^-9 sum|dg||xh|, what a dropped hi.lo term is worth."""
    T, B, I = c["T"], c["B"], c["I"]
    dg, eg = lstm_bwd_ref(c, fwd, None, "mfma")
    rows = d(fwd["xh"])
    s, m = slab_terms(dg, rows, B, I)
    e, _ = slab_terms(eg, np.abs(rows), B, I)
    bound = 2 * (e + (SPLIT + ME * T * U) * m)
    return slab_layout(s, I), slab_layout(bound, I), slab_layout(2.0 ** -9 * m, I)


def narrow_slab_condition(c, fwd):
    """The reference's own bound stays below a quarter of a dropped cross term on every element."""
    assert c["T"] <= 4
    _, bound, cross = narrow_slab_ref(c, fwd)
    pos = cross > 0
    worst = float((bound[pos] / cross[pos]).max())
    assert worst < 0.25, f"slab bound / cross term = {worst:.3f}"
    assert (bound[~pos] == 0).all()
    return worst


def narrow_slab_check(c, fwd, slab, stats=None, what="lstm bwd_dw"):
    want, bound, _ = narrow_slab_ref(c, fwd)
    within("slab", slab, want, bound, f"{what}: slab", stats)


# ---------------------------------------------------------------------------- GRU --
def gru_fwd_check(c, out, stats=None, what="gru fwd", exact=False):
    """The GRU forward step by step.  out: h_out; gact = [r | z | n | gh_n] and xh where written
    (T = 1 without gact: the bounds are multiplied through); h_save."""
    H, I = c["H"], c["I"]
    hp = check_chain(c, out, what)
    x, h = d(c["x"]), d(hp)
    wi, wh, bi, bh = d(c["w_ih"]), d(c["w_hh"]), d(c["b_ih"]), d(c["b_hh"])
    gi, e_gi = x @ wi.T + bi, SPLIT * (np.abs(x) @ np.abs(wi).T + np.abs(bi))
    gh, e_gh = h @ wh.T + bh, SPLIT * (np.abs(h) @ np.abs(wh).T + np.abs(bh))
    if exact:
        e_gi, e_gh = np.zeros_like(e_gi), np.zeros_like(e_gh)
    sl = lambda a, q: a[..., q * H:(q + 1) * H]  # noqa: E731
    rw, er = act_bound(sig, b_fsig, sl(gi, 0) + sl(gh, 0), sl(e_gi, 0) + sl(e_gh, 0))
    zw, ezz = act_bound(sig, b_fsig, sl(gi, 1) + sl(gh, 1), sl(e_gi, 1) + sl(e_gh, 1))
    gact = out.get("gact")
    if gact is not None:
        within("gate", gact[..., :H], rw, er, f"{what}: r", stats)
        within("gate", gact[..., H:2 * H], zw, ezz, f"{what}: z", stats)
        within("ghn", gact[..., 3 * H:], sl(gh, 2), sl(e_gh, 2), f"{what}: gh_n", stats)
        r, z, ghn = d(gact[..., :H]), d(gact[..., H:2 * H]), d(gact[..., 3 * H:])
        e_r = e_z = e_ghn = 0.0
    else:
        assert c["T"] == 1
        r, z, ghn, e_r, e_z, e_ghn = rw, zw, sl(gh, 2), er, ezz, sl(e_gh, 2)
    # n = ftanh(gi_n + r gh_n): the n_x half from the operand row, the n_h half as the kernel
    # saved it; the product and the sum are two roundings, doubled
    an = sl(gi, 2) + r * ghn
    e_an = sl(e_gi, 2) + np.abs(ghn) * e_r + (np.abs(r) + e_r) * e_ghn + 4 * U * (np.abs(sl(gi, 2)) + np.abs(r * ghn))
    nw, en = act_bound(np.tanh, b_ftanh, an, e_an)
    if gact is not None:
        within("n", gact[..., 2 * H:3 * H], nw, en, f"{what}: n", stats)
        n, e_n = d(gact[..., 2 * H:3 * H]), 0.0
    else:
        n, e_n = nw, en
    # h = (1 - z) n + z h_prev: 1 - z, two products, a sum: 4 roundings, doubled
    hw = (1 - z) * n + z * h
    eh = np.abs(h - n) * e_z + (1 - z + e_z) * e_n + 8 * U * (np.abs((1 - z) * n) + np.abs(z * h))
    within("out", out["h_out"], hw, eh, f"{what}: h_out", stats)


def gru_bwd_ref(c, fwd, dg_k=None):
    """fp64 [da_r | da_z | da_n | da_hn] and bound; the matrix part of the carried dh from the
    kernel's own dg (dg_k) or free-running."""
    T, B, H, I = c["T"], c["B"], c["H"], c["I"]
    w = d(c["w_hh"])
    wa = np.abs(w)
    gact, hp_all, dh_out = d(fwd["gact"]), d(fwd["xh"][..., I:I + H]), d(c["dh_out"])
    rs = np.zeros((T, B), bool) if c.get("reset") is None else c["reset"] != 0
    dg, eg = np.zeros((T, B, 4 * H)), np.zeros((T, B, 4 * H))
    dhn = e_dhn = np.zeros((B, H))
    cols = np.r_[0:2 * H, 3 * H:4 * H]  # the operand's columns, W_hh's row order
    for t in range(T - 1, -1, -1):
        r, z, n, ghn = (gact[t][:, q * H:(q + 1) * H] for q in range(4))
        hp = hp_all[t]
        dh = dh_out[t] + dhn
        e_dh = e_dhn + 2 * U * np.abs(dh)
        q1 = 1 - n * n
        e_q1 = 2 * U * (n * n + np.abs(q1))
        dn = dh * (1 - z)
        da_n = dn * q1
        e_dan = e_dh * np.abs((1 - z) * q1) + np.abs(dn) * e_q1 + 6 * U * np.abs(da_n)
        dz = dh * (hp - n)
        v = [da_n * ghn * r * (1 - r), dz * z * (1 - z), da_n, da_n * r]
        e = [e_dan * np.abs(ghn * r * (1 - r)) + 8 * U * np.abs(v[0]),
             e_dh * np.abs((hp - n) * z * (1 - z)) + 10 * U * np.abs(v[1]),
             e_dan,
             e_dan * np.abs(r) + 2 * U * np.abs(v[3])]
        dg[t], eg[t] = np.concatenate(v, 1), np.concatenate(e, 1)
        keep = ~rs[t][:, None]
        src = dg[t] if dg_k is None else d(dg_k[t])
        e_src = eg[t] if dg_k is None else np.zeros_like(eg[t])
        mat = src[:, cols] @ w
        e_mat = e_src[:, cols] @ wa + SPLIT * (np.abs(src[:, cols]) @ wa)
        dhz = dh * z
        dhn = np.where(keep, dhz + mat, 0.0)
        e_dhn = np.where(keep, e_dh * z + e_mat + 2 * U * np.abs(dhz) + 2 * U * np.abs(dhz + mat), 0.0)
    return dg, eg


def gru_bwd_check(c, fwd, dg, stats=None, what="gru bwd"):
    want, e = gru_bwd_ref(c, fwd, dg)
    within("dg", dg, want, e, f"{what}: dg", stats)


def grid_gru_check(c, out, stats=None, what="gru grid"):
    """T = 1 on the exact grid: r, z within the activation budget alone and gh_n exactly."""
    assert_grid_exact(c, 3)
    gru_fwd_check(c, out, stats, what, exact=True)


# -------------------------------------------------------------------------- heads --
def heads_case(seed, M, H, N0, N1):
    """The heads' exact grid.  h = k/8, W0 / W1 = j/64, b0 / b1 = i/8, dout = k/8.  Every third
    row has few non-zero inputs, so with b0 >= 1/2 its y0 is positive in every unit (those rows'
    out is exact).  y0b, the backward's y0 input, is m/8 in [-1, 2] with both signs, 0 and -1:
    elu' from the output is 1 or y0 + 1, exact.  Asserts that every sum is exact: sum|terms| of
    every output, which bounds every partial sum in any order, needs at most 23 bits of the
    terms' unit."""
    rng = np.random.default_rng(seed)
    gi = lambda lo, hi, shape, den: (rng.integers(lo, hi + 1, shape) / den).astype(F)  # noqa: E731
    h = gi(-16, 16, (M, H), 8.0)
    pos = np.arange(M) % 3 == 0
    sparse = np.zeros((M, H), F)
    for r in np.nonzero(pos)[0]:
        sparse[r, rng.choice(H, 4, replace=False)] = gi(-2, 2, 4, 8.0)
    h[pos] = sparse[pos]
    c = dict(M=M, H=H, N0=N0, N1=N1, h=h, W0=gi(-8, 8, (N0, H), 64.0), b0=gi(4, 8, N0, 8.0),
             W1=gi(-8, 8, (N1, N0), 64.0), b1=gi(-8, 8, N1, 8.0), dout=gi(-8, 8, (M, N1), 8.0),
             y0b=gi(-8, 16, (M, N0), 8.0), pos=pos)
    c["y0b"][0, 0] = 0.0
    c["y0b"][M - 1, N0 - 1] = -1.0
    heads_assert_exact(c)
    return c


def heads_ref(c):
    """fp64: z0, y0, out of the forward; dz0, dh and the slab rows of the backward (from y0b)."""
    h, W0, b0, W1, b1 = (d(c[k]) for k in ("h", "W0", "b0", "W1", "b1"))
    z0 = h @ W0.T + b0
    y0 = np.where(z0 > 0, z0, np.expm1(np.minimum(z0, 0)))
    y0b, dout = d(c["y0b"]), d(c["dout"])
    dy = dout @ W1
    dz0 = dy * np.where(y0b > 0, 1.0, y0b + 1.0)
    dh = dz0 @ W0
    M = c["M"]
    nblk = (M + HEAD_ROWS - 1) // HEAD_ROWS
    rows = []
    for b in range(nblk):
        s = slice(b * HEAD_ROWS, min(M, (b + 1) * HEAD_ROWS))
        rows.append(np.concatenate([(dz0[s].T @ h[s]).reshape(-1), dz0[s].sum(0), (dout[s].T @ y0b[s]).reshape(-1),
                                    dout[s].sum(0)]))
    return dict(z0=z0, y0=y0, dy=dy, dz0=dz0, dh=dh, slab=np.stack(rows))


def heads_assert_exact(c):
    h, W0, b0, W1, dout, y0b = (d(c[k]) for k in ("h", "W0", "b0", "W1", "dout", "y0b"))
    r = heads_ref(c)
    bits = {}
    bits["z0"] = _sig_bits(np.abs(h) @ np.abs(W0).T + np.abs(b0), 2.0 ** -9)
    assert (r["z0"][c["pos"]] > 0).all() and c["pos"].any(), "the positive rows are not positive"
    assert c["M"] < 8 or (r["z0"][~c["pos"]] < 0).any(), "no negative branch"
    bits["out"] = _sig_bits(np.abs(r["y0"][c["pos"]]) @ np.abs(W1).T + np.abs(d(c["b1"])), 2.0 ** -15)
    bits["dy"] = _sig_bits(np.abs(dout) @ np.abs(W1), 2.0 ** -9)
    fac = np.abs(np.where(y0b > 0, 1.0, y0b + 1.0))
    bits["dz0"] = _sig_bits(np.abs(r["dy"]) * fac, 2.0 ** -12)
    bits["dh"] = _sig_bits(np.abs(r["dz0"]) @ np.abs(W0), 2.0 ** -18)
    M = c["M"]
    worst = 0.0
    for b in range(0, M, HEAD_ROWS):
        s = slice(b, min(M, b + HEAD_ROWS))
        worst = max(worst, float((np.abs(r["dz0"][s]).T @ np.abs(h[s])).max()))
    bits["dW0"] = _sig_bits(np.array([worst]), 2.0 ** -15)
    for k, v in bits.items():
        assert v <= 23, f"heads grid: {k} needs {v} bits"
    assert (y0b == 0).any() and (y0b < 0).any() and (y0b > 0).any()
    return bits


def heads_fwd_check(c, y0, out, stats=None, what="heads fwd"):
    """y0: equal where z0 > 0, within 8u |expm1(z0)| on the negative branch (z0 is exact);
    out: equal on the rows whose y0 is positive in every unit, else the any-order fp32 bound
    from the kernel's own y0."""
    r = heads_ref(c)
    posm = r["z0"] > 0
    equal("y0", np.where(posm, y0, 0), np.where(posm, r["y0"], 0).astype(F), f"{what}: y0 (z0 > 0)")
    within("elu", np.where(posm, 0, y0), np.where(posm, 0, r["y0"]), np.where(posm, 0, 8 * U * np.abs(r["y0"])),
           f"{what}: y0 (z0 <= 0)", stats)
    W1, b1 = d(c["W1"]), d(c["b1"])
    rowpos = posm.all(1)
    assert rowpos[c["pos"]].all()
    o64 = d(y0) @ W1.T + b1
    equal("out", out[rowpos], o64[rowpos].astype(F), f"{what}: out on the positive rows")
    assert (o64[rowpos].astype(F).astype(D) == o64[rowpos]).all()
    eb = (c["N0"] + 1) * U * (np.abs(d(y0)) @ np.abs(W1).T + np.abs(b1))
    within("out_neg", out, o64, eb, f"{what}: out", stats)


def heads_bwd_check(c, dh, slab, what="heads bwd"):
    """dh and every slab row [dW0 | db0 | dW1 | db1] equal the fp64 values, block by block."""
    r = heads_ref(c)
    for k in ("dh", "slab"):
        assert (r[k].astype(F).astype(D) == r[k]).all(), f"{k}: the reference is not an fp32 number"
    equal("dh", dh, r["dh"].astype(F), f"{what}: dh")
    for b in range(r["slab"].shape[0]):
        equal("slab", slab[b], r["slab"][b].astype(F), f"{what}: slab row {b}")


# ------------------------------------------------- the cases both test files run --
MF_I = (1, 3, 4, 32, 47, 63, 64)
MF_B = (1, 15, 16, 17, 37)
MF_T = (1, 2, 3, 4, 7)
GRU_I = (1, 3, 32, 47, 64)
DW_I = (1, 31, 32, 63)
DW_B = (1, 15, 17, 37)
DW_T = (1, 2, 3, 4)
BWD_B = (1, 16, 17, 37)
BWD_T = (1, 2, 3, 7)
WIDE = ((65, 1, 1), (65, 7, 73), (237, 4, 128), (237, 3, 171), (234, 2, 37), (384, 3, 171), (384, 1, 21))  # I, T, B
VALU_H = (32, 64, 128)
VALU_I = (0, 1, 32, 33, 48, 49, 64)  # 0: gx-fed
VALU_B = (1, 4, 5)
HEADS_M = (1, 63, 64, 65, 127, 128, 129, 16383, 16421)
HEADS_N = ((8, 1), (24, 12), (32, 16))


def presence(n):
    """Which optional inputs combination n of a sweep has: every one of h0, c0 and reset is
    present in some and NULL in others, and every reset pattern occurs."""
    return dict(h0=bool(n & 1), c0=bool(n & 2), reset=RESET_PATTERNS[(n // 2) % len(RESET_PATTERNS)] if n % 5 else "mixed")


def sweep(seed, Ts, Bs, I, gates=4, **kw):
    """The cases of one input width over Ts x Bs, the optional inputs rotating."""
    n = 0
    for T in Ts:
        for B in Bs:
            p = presence(n)
            p.update(kw)
            yield seq_case(seed * 1000 + n, T, B, I, gates=gates, **p)
            n += 1


WIDE_RESETS = ("t0", "none", "mixed", "all", "last", "tail", "twice")


def wide_cases():
    """The wide cases: every reset pattern once (NULL at T = 7, every env at one step at T = 3),
    h0 and c0 each present and NULL."""
    for n, (I, T, B) in enumerate(WIDE):
        yield seq_case(I + T, T, B, I, h0=bool(n & 1), c0=bool(n & 2), reset=WIDE_RESETS[n])


def wide_pair_cases():
    """Two wide jobs (I = 65, 300) over one [T, B]: every env reset at one step, h0 / c0 NULL in one each."""
    a, b = seq_case(1, 2, 21, 65, h0=False, reset="all"), seq_case(2, 2, 21, 300, c0=False)
    b["reset"] = a["reset"]
    return a, b


def wide_pair_null_cases():
    """The same pair without resets (reset == NULL with two jobs)."""
    a, b = seq_case(3, 3, 21, 65, reset="none"), seq_case(4, 3, 21, 300, h0=False, c0=False, reset="none")
    return a, b


def lstm_pair_cases():
    a, b = seq_case(1, 3, 37, 3), seq_case(2, 3, 37, 64)
    b["reset"] = a["reset"]
    return a, b


def narrow_pair_cases():
    (n1, f1), (n2, f2) = narrow_bwd_case(3, 3, 37, 1), narrow_bwd_case(4, 3, 37, 63)
    n2["reset"] = n1["reset"]
    return (n1, f1), (n2, f2)


def bwd_cases(T):
    """pmlp_lstm_bwd_mfma's cases of one T: B = 1, 16, 17, 37, c0 given and NULL."""
    for n, B in enumerate(BWD_B):
        for c0 in (True, False):
            yield seq_case(T * 10 + n, T, B, 47, c0=c0, reset=RESET_PATTERNS[(n + T + c0) % 7])


def step_cases(B, gates=4):
    return [seq_case(B + I, 1, B, I, gates=gates, reset="none") for I in (47, 4)]


def wide_step_case(B):
    return seq_case(B, 1, B, 237, reset="none")


def valu_case(seed, T, B, I, H, **p):
    """(case, form): I = 0 is the gx-fed form, gx a float32 product made on the CPU."""
    c = seq_case(seed, T, B, max(I, 1), H=H, **p)
    if I == 0:
        c["gx"] = (c["x"] @ c["w_ih"].T + c["b_ih"] + c["b_hh"]).astype(F)
    return c, ("valu_gx" if I == 0 else "valu_x")


def valu_cases(H):
    """(case, form, xh present) over VALU_I x VALU_B at T = 3.  The reset pattern is
    RESET_PATTERNS[(3 hidx + n) % 7]: over the three hidden sizes every form, the gx-fed one
    included, meets every pattern; h0 / c0 present and NULL by the bits of n."""
    n, hidx = 0, VALU_H.index(H)
    for I in VALU_I:
        for B in VALU_B:
            c, form = valu_case(H + n, 3, B, I, H, h0=bool(n & 1), c0=bool(n & 2),
                                reset=RESET_PATTERNS[(3 * hidx + n) % len(RESET_PATTERNS)])
            yield c, form, bool(n % 2)
            n += 1


VALU_SWITCH_RESETS = {4088: ("all", "none"), 4089: ("none", "twice")}


def valu_switch_cases(B):
    """T = 2 at the switch of the env block: I = 33 and gx-fed, with and without resets."""
    for k, I in enumerate((33, 0)):
        yield valu_case(B + I, 2, B, I, 64, h0=bool(k), c0=not k, reset=VALU_SWITCH_RESETS[B][k])


def valu_step_case(H):
    return valu_case(H, 1, 37, 0, H, reset="none")


def heads_cases(M):
    """Per hidden size the two jobs of one launch."""
    for n, H in enumerate(VALU_H):
        yield H, [heads_case(M + H + k, M, H, *HEADS_N[(n + k) % 3]) for k in range(2)]


def pattern_cases(pattern):
    """The reset-pattern cases: (LSTM case, (narrow backward case, arrays), two GRU jobs)."""
    a, b = seq_case(7, 7, 21, 3, gates=3, reset=pattern), seq_case(8, 7, 21, 64, gates=3)
    b["reset"] = a["reset"]
    return seq_case(5, 7, 21, 47, reset=pattern), narrow_bwd_case(6, 4, 21, 31, reset=pattern), (a, b)


def narrow_cases(I):
    """pmlp_lstm_bwd_dw_mfma_jobs' sweep of one input width: test-built arrays over DW_T x DW_B."""
    n = 0
    for T in DW_T:
        for B in DW_B:
            p = presence(n)
            yield narrow_bwd_case(I * 100 + n, T, B, I, c0=p["c0"], reset=p["reset"])
            n += 1
