"""Reference and bounds for the empirical observation normalisation (pmlp_obs_norm_step,
rsl_rl/modules/normalizer.py): what tests/test_obsnorm_host.py and tests/test_gpu_obsnorm.py
compare against.

Reference.  Batch moments by the two-pass formulas (mean_x = sum x / N, M2_x = sum (x - mean_x)^2)
accumulated in numpy's extended precision (64-bit significand on x86, never below fp64), then
the merge of the C ABI:
    n' = count + N, r = N / n', delta = mean_x - mean, mean' = mean + delta r,
    var' = (var count + M2_x + delta^2 count r) / n', count' = n',
and the tables mean32 = (float) mean', inv32 = (float) (1 / (sqrt(var') + eps)).

Bounds.  The code under test sums d = x - s and d^2 in fp64 with the shift s = x[0, k], in an
order of its own.  With u = 2^-53 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., eq. 4.4: any order of summation), A1 = sum |d| and A2 = sum d^2:
    |S1^ - S1| <= gamma_{N+1} A1        (one rounding for d, N - 1 additions)
    |S2^ - S2| <= gamma_{N+3} A2        (d, its square, N - 1 additions)
    mean_x = s + S1 / N:   e_mx <= gamma_{N+4} A1 / N + 2 u max(|s|, |mean_x|)
    M2_x = S2 - S1^2 / N:  S1^2 / N <= A1^2 / N <= A2 (Cauchy-Schwarz), so the error of S1^2 / N is
                           <= 2 gamma_{N+1} A2 (+ second order), and e_M2 <= 4 gamma_{N+8} A2
and through the merge, with e_d = e_mean + e_mx the error of delta:
    e_mean' <= (1 - r) e_mean + r e_mx + 4 u (|mean'| + |mean| + |delta|)
    e_var'  <= (count e_var + e_M2 + count r (2 |delta| e_d + e_d^2)) / n' + 8 u var'
(every term of var' is non-negative, so 8 u var' covers the roundings of its five operations and
of the reference's result).  The bounds come from the inputs alone; nothing is fitted to a kernel.
`count` must be exact, and the tables must be within 1 fp32 ulp of the reference's roundings.
"""
import numpy as np

U = 2.0 ** -53
EPS = 1e-2
LD = np.longdouble


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- inputs ----
KINDS = ("unit", "const100", "const0.1", "mean100", "zero")


def make_batch(rng, N, D, offset=0):
    """fp32 rows [N, D]; column k is of kind KINDS[(k + offset) % 5]: ordinary unit-scale, constant
    100.0, constant 0.1f, mean 100 with spread 1e-3, all-zero."""
    x = np.empty((N, D), dtype=np.float32)
    for k in range(D):
        kind = KINDS[(k + offset) % 5]
        if kind == "unit":
            x[:, k] = rng.standard_normal(N).astype(np.float32) * np.float32(1.0 + 0.1 * (k % 7)) + np.float32(0.3 * (k % 3))
        elif kind == "const100":
            x[:, k] = np.float32(100.0)
        elif kind == "const0.1":
            x[:, k] = np.float32(0.1)
        elif kind == "mean100":
            x[:, k] = (100.0 + 1e-3 * rng.uniform(-1.0, 1.0, N)).astype(np.float32)
        else:
            x[:, k] = 0.0
    return x


def make_sequence(seed, N, D, ncalls=4, offset=0):
    rng = np.random.default_rng(seed)
    return [make_batch(rng, N, D, offset) for _ in range(ncalls)]


# ---- reference ----
class State:
    """Reference state with the bounds on what a conforming implementation may hold."""

    def __init__(self, D):
        self.count = 0
        self.mean = np.zeros(D)
        self.var = np.ones(D)
        self.e_mean = np.zeros(D)
        self.e_var = np.zeros(D)

    def copy(self):
        s = State(len(self.mean))
        s.count, s.mean, s.var = self.count, self.mean.copy(), self.var.copy()
        s.e_mean, s.e_var = self.e_mean.copy(), self.e_var.copy()
        return s


def update(st, x):
    """Merge the rows x [N, D] (fp32) into st: the reference and the bounds, in place."""
    N = x.shape[0]
    xl = x.astype(LD)
    mean_x = xl.sum(0) / LD(N)
    m2 = ((xl - mean_x) ** 2).sum(0)
    c, n = LD(st.count), LD(N)
    nn = c + n
    r = n / nn
    mean, var = st.mean.astype(LD), st.var.astype(LD)
    delta = mean_x - mean
    mean_new = mean + delta * r
    var_new = (var * c + m2 + delta * delta * c * r) / nn
    # bounds, from the shifted sums of the code under test
    s = x[0].astype(np.float64)
    d = x.astype(np.float64) - s
    A1, A2 = np.abs(d).sum(0), (d * d).sum(0)
    e_mx = gamma(N + 4) * A1 / N + 2 * U * np.maximum(np.abs(s), np.abs(mean_x.astype(np.float64)))
    e_m2 = 4 * gamma(N + 8) * A2
    rf, cf, nf = float(r), float(c), float(nn)
    ad = np.abs(delta.astype(np.float64))
    e_d = st.e_mean + e_mx
    e_mean = (1 - rf) * st.e_mean + rf * e_mx + 4 * U * (np.abs(mean_new.astype(np.float64)) + np.abs(st.mean) + ad)
    e_var = (cf * st.e_var + e_m2 + cf * rf * (2 * ad * e_d + e_d * e_d)) / nf + 8 * U * var_new.astype(np.float64)
    st.count += N
    st.mean, st.var = mean_new.astype(np.float64), var_new.astype(np.float64)
    st.e_mean, st.e_var = e_mean, e_var
    return st


def tables(st, eps=EPS):
    """(mean32, inv32) of the reference state: its fp32 roundings."""
    inv = LD(1.0) / (np.sqrt(st.var.astype(LD)) + LD(eps))
    return st.mean.astype(np.float32), inv.astype(np.float32)


def rows(x, mean32, inv32):
    """y = (x - mean32) * inv32, fp32 with two roundings."""
    return ((x.astype(np.float32) - mean32.astype(np.float32)).astype(np.float32) * inv32.astype(np.float32)).astype(np.float32)


def run(batches, update_flags=None, until=None, eps=EPS, st=None):
    """The reference over a sequence of calls: per call (state after it, (mean32, inv32))."""
    st = State(batches[0].shape[1]) if st is None else st
    out = []
    for i, x in enumerate(batches):
        upd = True if update_flags is None else update_flags[i]
        if upd and (until is None or st.count < until):
            update(st, x)
        out.append((st.copy(), tables(st, eps)))
    return out


# ---- comparisons (raise AssertionError) ----
def check_state(count, mean, var, ref):
    """count exact; mean and var within the reference's bounds."""
    assert int(count) == ref.count, f"count {int(count)} != {ref.count}"
    mean, var = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(var, dtype=np.float64).reshape(-1)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    em, ev = np.abs(mean - ref.mean), np.abs(var - ref.var)
    k = int(np.argmax(em - ref.e_mean))
    assert (em <= ref.e_mean).all(), f"mean[{k}] off by {em[k]:.3e} > bound {ref.e_mean[k]:.3e}"
    k = int(np.argmax(ev - ref.e_var))
    assert (ev <= ref.e_var).all(), f"var[{k}] off by {ev[k]:.3e} > bound {ref.e_var[k]:.3e}"
    assert (var >= 0).all()


def check_tables(mean32, inv32, ref_tables):
    """Within 1 fp32 ulp of the reference's fp32 roundings."""
    for name, got, want in (("mean32", mean32, ref_tables[0]), ("inv32", inv32, ref_tables[1])):
        got = np.asarray(got).reshape(-1)
        assert got.dtype == np.float32 and np.isfinite(got).all(), name
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32))
        bad = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
        assert not bad.any(), f"{name}[{int(np.argmax(bad))}] more than 1 ulp from the reference"


def check_rows(y, x, mean32, inv32):
    """Bitwise the fp32 restatement with the call's own tables."""
    y = np.asarray(y)
    want = rows(x, np.asarray(mean32).reshape(-1), np.asarray(inv32).reshape(-1))
    assert y.dtype == np.float32 and y.shape == want.shape
    bad = y.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} row elements differ from (x - mean32) * inv32"


# ---- the kernel test's cases (N, D, ldx); the host test runs the restatement on the same ----
NS = (1, 63, 64, 65, 257, 4096)
WIDTHS = ((1, 1), (46, 46), (48, 48), (235, 236), (427, 448), (512, 512))
