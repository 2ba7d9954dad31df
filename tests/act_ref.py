"""fp64 / exact references for the acting side of the PPO library (csrc/pmlp_noise.h; k_act,
k_act4, roll_epilogue, k_store_step and k_permutation in csrc/ppo_mlp.hip; the ACT branch of
k_heads_fwd in csrc/heads.hip; the env step's philox_uniform), and the comparisons built on them
("The acting anchor").  numpy only: nothing here needs a GPU or the libraries.
tests/test_act_ref_host.py tests this file itself; tests/test_gpu_act_reference.py holds the
kernels to it.

U = 2^-24 is one fp32 rounding (relative).  No bound below is fitted to a kernel's output:
every one is a count of the fp32 roundings between the reference's operands and the kernel's
result, doubled.

Integer parts (compared for equality).  philox4x32_10 is Philox4x32-10 of Salmon et al.
(Random123): per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1,
lo(M0 c0)) with M0 = 0xD2511F53, M1 = 0xCD9E8D57, then k0 += 0x9E3779B9, k1 += 0xBB67AE85; the
host tests hold it to the three known-answer vectors of Random123's kat_vectors.  The policy
noise's counter is (uint32(draw), row, quad, 0x5050) and its key (seed low, seed high); the env
step's counter is (env, step, stream, index).  permutation_ref is pmlp_permutation's host
arithmetic (b = max(2, ceil(log2 n)) bits, a = b / 2 high and c = b - a low) and k_permutation's
four alternating Feistel rounds (counter (half, round, 0x9e11, 0x7e37), word 0 of the output)
with the cycle walk.

u01_ref is the exact float32 value of ((float)x + 0.5f) * 2^-32: the conversion rounds to nearest
even, the add is one rounding and the scaling by a power of two is exact, and numpy's float32
does each of them the same way, so the uniforms are compared for equality and the references
below start from the kernel's own fp32 uniforms.  What it implies: the smallest uniform is
(0 + 0.5) 2^-32 = 2^-33, so the radius is at most sqrt(-2 ln 2^-33) = sqrt(66 ln 2) = 6.7637 and
|z| <= 6.7637; every x >= 0xffffff80 converts to 2^32 (round to nearest even at 24 bits), the
add leaves it and the uniform is exactly 1.0, where log is 0, the radius 0 and z a signed zero,
never a NaN.  (So u lies in [2^-33, 1], both ends included.)

noise_ref: z in fp64 from those fp32 uniforms: for quad c of a row, elements 4c and 4c + 1 are
cos and sin of 2 pi u(r.y) times sqrt(-2 ln u(r.x)), elements 4c + 2 and 4c + 3 the same from
r.w and r.z (Box-Muller; the kernel's sincospif(2 u) is sin and cos of pi (2 u)).

ASSUMPTIONS.  No document on the accuracy of the device's logf, sqrtf and sincospif, or of the
fp32 division, was at hand when this was written.  ASSUMED: logf within E_LOG = 1 ulp,
sincospif within E_SINCOS = 1 ulp, sqrtf and the fp32 division correctly rounded (half an ulp).
None of these figures is taken from a source; if one turns up, change the constants, not the
tests.  One ulp is charged at 2 U relative (its size at the bottom of a binade), and for the
sine and cosine, whose magnitude is at most 1, at 2 U absolute, so that an argument near a zero
of either needs no relative accuracy.

z (z_bound).  The uniforms are exact and 2.f * u is exact.  logf's E_LOG ulp on L = -2 ln u
is E_LOG / 2 ulp on the radius (the square root halves a relative error); sqrtf's rounding and
the product's are half an ulp each, one ulp together; the sine or cosine carries E_SINCOS ulp
absolute, times the radius.  Counted: 2 U ((E_LOG / 2 + 1) |z| + E_SINCOS rad).  Doubled:
    B_z = 4 U ((E_LOG / 2 + 1) |z| + E_SINCOS rad)            (6 U |z| + 4 U rad)

The action (act_bound).  The reference is mu + sigma z in fp64 from the kernel's own stored mu
and sigma.  The kernel adds sigma times its z, then rounds the product and the sum (one rounding
where the two are contracted into an fma: less): U |sigma z| + U |act|, doubled:
    B_act = sigma B_z + 2 U (|sigma z| + |act|)

The log-probability (logp_ref, logp_bound).  The reference is the fp64 Gaussian log-density of
the kernel's own stored action, mean and sigma, term_k = -d^2 / (2 sigma^2) - ln sigma -
ln sqrt(2 pi) with d = act - mu, summed over A.  The kernel's term: d is one rounding (none
where Sterbenz applies), d * d carries it twice and rounds once, 2.f * sigma is exact and
(2 sigma) sigma rounds once, the division (ASSUMED correctly rounded) once: 5 U on q = d^2 /
(2 sigma^2); logf(sigma) E_LOG ulp = 2 E_LOG U |ln sigma|; the constant kHalfLog2Pi is the
float nearest ln sqrt(2 pi): U K; the two subtractions round to s = -q - ln sigma and to the
term: U |s| + U |term|.  Doubled:
    B_term = 2 U (5 q + 2 E_LOG |ln sigma| + K + |s| + |term|)
and the row's sequential fp32 sum over k = 0 .. A - 1 (all the arms sum in k order from 0.f)
adds (A - 1) U sum_k |term_k|:
    B_logp = sum_k B_term_k + (A - 1) U sum_k |term_k|

store_ref is k_store_step's statement in numpy float32 in the kernel's order (contraction off
there): rewards + gamma * (value * time_out) with time_out 1.0 where the byte is nonzero, the
reward itself where time_outs is NULL, and dones != 0 as bytes; compared for equality.  Memory
rows are zeroed exactly where dones != 0 (a time-out alone zeroes nothing).

uniform_ref is the env step's draw: float(word0 >> 8) * 2^-24 of the counter (env, step, stream,
index) under the key (seed low, seed high): a 24-bit integer times a power of two, exact.

Each check_* returns the worst measured error as a fraction of its bound (0.0 where the
comparison is for equality) and raises AssertionError naming the first bad element.
"""
import math

import numpy as np

U = 2.0 ** -24
E_LOG = 1.0      # ASSUMED: logf within 1 ulp
E_SINCOS = 1.0   # ASSUMED: sincospif within 1 ulp
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
Z_MAX = math.sqrt(66.0 * math.log(2.0))
NOISE_TAG = 0x5050
PERM_TAG = (0x9e11, 0x7e37)

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: four arrays (broadcast together) of 32-bit words, key: two.
    Returns the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(x) for x in counter])
    k0, k1 = _u64(key[0]), _u64(key[1])
    for _ in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2     # (32 x 32 bits: no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _W0) & _M32, (k1 + _W1) & _M32
    return c0, c1, c2, c3


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def u01_ref(x):
    """((float)x + 0.5f) * 2^-32 in float32, exactly as the device rounds it."""
    x = np.asarray(x, dtype=np.uint64)
    return (x.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def uniform_ref(seed, env, step, stream, index):
    """The env step's draw (leggedsim's philox_uniform, lgs_uniform on the host), float32."""
    w0 = philox4x32_10((env, step, stream, index), seed_key(seed))[0]
    return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniform_cases():
    """(seed, env, step, stream, index) for the env draw's comparisons: every counter word at 0 and
    0xffffffff, and 300 random ones under seeds with the high word set."""
    rng = np.random.default_rng(7)
    edge = (0, 0xffffffff)
    cases = [(0xFFFFFFFF00000001, e, s, t, i) for e in edge for s in edge for t in edge for i in edge]
    for _ in range(300):
        seed = int(rng.integers(1 << 62, 1 << 63)) * 2 + 1       # the high word set, bit 63 included
        cases.append((seed, *[int(v) for v in rng.integers(0, 1 << 32, 4)]))
    return cases


def _rows(rows):
    return np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64).reshape(-1)


def noise_parts(seed, draw, rows, A):
    """(z, rad), fp64 [N, A]: the policy noise of rows (a count N, or an array of row indices)
    and the Box-Muller radius each element was scaled by."""
    r = _rows(rows)
    Q = (A + 3) // 4
    i, c = np.repeat(r, Q), np.tile(np.arange(Q, dtype=np.uint64), r.size)
    w = philox4x32_10((int(draw) & 0xFFFFFFFF, i, c, NOISE_TAG), seed_key(seed))
    ux, uy, uz, uw = [u01_ref(x).astype(np.float64) for x in w]
    rad0, rad1 = np.sqrt(-2.0 * np.log(ux)), np.sqrt(-2.0 * np.log(uz))
    a0, a1 = 2.0 * np.pi * uy, 2.0 * np.pi * uw
    z = np.stack([np.cos(a0) * rad0, np.sin(a0) * rad0, np.cos(a1) * rad1, np.sin(a1) * rad1], 1)
    rad = np.stack([rad0, rad0, rad1, rad1], 1)
    return z.reshape(r.size, 4 * Q)[:, :A], rad.reshape(r.size, 4 * Q)[:, :A]


def noise_ref(seed, draw, rows, A):
    return noise_parts(seed, draw, rows, A)[0]


def z_bound(z, rad):
    return 4.0 * U * ((E_LOG / 2.0 + 1.0) * np.abs(z) + E_SINCOS * rad)


def act_bound(mu, sigma, z, rad):
    """The bound on |act_kernel - (mu + sigma z)|; mu [N, A], sigma [A] or [N, A] (fp64)."""
    sz = sigma * z
    return np.abs(sigma) * z_bound(z, rad) + 2.0 * U * (np.abs(sz) + np.abs(mu + sz))


def logp_terms(act, mu, sigma):
    """The fp64 log-density terms [N, A] and their bounds."""
    act, mu, sigma = [np.asarray(x, dtype=np.float64) for x in (act, mu, sigma)]
    d = act - mu
    q = d * d / (2.0 * sigma * sigma)
    ls = np.log(sigma) + 0.0 * q
    s = -q - ls
    term = s - HALF_LOG_2PI
    bound = 2.0 * U * (5.0 * q + 2.0 * E_LOG * np.abs(ls) + HALF_LOG_2PI + np.abs(s) + np.abs(term))
    return term, bound


def logp_ref(act, mu, sigma):
    return logp_terms(act, mu, sigma)[0].sum(1)


def logp_bound(act, mu, sigma):
    term, bound = logp_terms(act, mu, sigma)
    return bound.sum(1) + (term.shape[1] - 1) * U * np.abs(term).sum(1)


def store_ref(rewards, dones, time_outs, value, gamma):
    """(st_rewards float32 [N], st_dones uint8 [N]) of k_store_step."""
    f = np.float32
    r = np.asarray(rewards, dtype=f)
    if time_outs is not None:
        to = (np.asarray(time_outs) != 0).astype(f)
        r = r + f(gamma) * (np.asarray(value, dtype=f) * to)
    return r.astype(f), (np.asarray(dones) != 0).astype(np.uint8)


def reset_ref(state, dones):
    """A memory state [N, H] after the store step: rows zeroed exactly where dones != 0."""
    out = np.array(state, copy=True)
    out[np.asarray(dones) != 0] = 0
    return out


def perm_split(n):
    """pmlp_permutation's host arithmetic: (a, c), the high and low halves' widths."""
    b = 2
    while (1 << b) < n:
        b += 1
    a = b // 2
    return a, b - a


def permutation_ref(n, seed, steps=False):
    """pmlp_permutation(out, n, seed) as an int64 array (and the longest cycle walk with steps)."""
    a, c = perm_split(n)
    ma, mc, sc = np.uint64((1 << a) - 1), np.uint64((1 << c) - 1), np.uint64(c)
    key = seed_key(seed)
    x = np.arange(n, dtype=np.uint64)
    out = np.zeros(n, dtype=np.uint64)
    todo = np.arange(n)
    walk = 0
    while todo.size:
        H, L = (x >> sc) & ma, x & mc
        for r in range(4):
            if r % 2 == 0:
                H = H ^ (philox4x32_10((L, r, PERM_TAG[0], PERM_TAG[1]), key)[0] & ma)
            else:
                L = L ^ (philox4x32_10((H, r, PERM_TAG[0], PERM_TAG[1]), key)[0] & mc)
        x = (H << sc) | L
        walk += 1
        assert walk <= (1 << (a + c)), "the cycle walk did not return"
        done = x < np.uint64(n)
        out[todo[done]] = x[done]
        todo, x = todo[~done], x[~done]
    out = out.astype(np.int64)
    return (out, walk) if steps else out


# ------------------------------------------------------------------ comparisons --
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _first_bad(bad, what, **vals):
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside, first at {i}: " +
                         ", ".join(f"{k}={np.asarray(v)[i]!r}" for k, v in vals.items()))


def check_close(got, want, bound, what):
    """|got - want| <= bound elementwise (a NaN fails); the worst fraction of the bound."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        _first_bad(bad, what, got=got, want=want, err=err, bound=bound)
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))
    bad = bad.any(-1)
    if bad.any():
        _first_bad(bad, what + " (bitwise)", got=got, want=want)
    return 0.0


def check_act_rows(out, stdv, seed, draw, rows=None, mu=None):
    """The sampling outputs of one launch: out holds actions_out, st_actions, st_mu, st_sigma
    [N, A] and st_logp [N] (float32).  st_sigma is the broadcast of stdv, st_actions is
    actions_out and (where mu is given) st_mu is mu, bitwise; the actions lie within act_bound
    of mu + sigma z and st_logp within logp_bound of the log-density of the stored row.  Returns
    the worst fractions."""
    act, smu, ssg = out["actions_out"], out["st_mu"], out["st_sigma"]
    N, A = act.shape
    check_equal(out["st_actions"], act, "st_actions vs actions_out")
    check_equal(ssg, np.broadcast_to(np.asarray(stdv, np.float32), (N, A)), "st_sigma vs stdv")
    if mu is not None:
        check_equal(smu, np.asarray(mu, np.float32).reshape(N, A), "st_mu vs mu")
    z, rad = noise_parts(seed, draw, N if rows is None else rows, A)
    m64, s64 = smu.astype(np.float64), ssg.astype(np.float64)
    fr = dict(act=check_close(act, m64 + s64 * z, act_bound(m64, s64, z, rad), "actions"))
    fr["logp"] = check_close(out["st_logp"], logp_ref(act, smu, ssg), logp_bound(act, smu, ssg), "st_logp")
    return fr


def check_store(out, rewards, dones, time_outs, value, gamma):
    """st_rewards / st_dones of one store step against store_ref, for equality."""
    r, d = store_ref(rewards, dones, time_outs, value, gamma)
    check_equal(out["st_rewards"], r, "st_rewards")
    check_equal(out["st_dones"], d, "st_dones")
    return 0.0


def check_permutation(got, n, seed):
    return check_equal(np.asarray(got), permutation_ref(n, seed), f"permutation n={n}")


def permutation_batch(n, seeds):
    """permutation_ref(n, seed) for every seed at once: int64 [len(seeds), n]."""
    a, c = perm_split(n)
    ma, mc, sc = np.uint64((1 << a) - 1), np.uint64((1 << c) - 1), np.uint64(c)
    keys = np.array([seed_key(s) for s in seeds], dtype=np.uint64)
    S = len(seeds)
    x = np.tile(np.arange(n, dtype=np.uint64), S)
    k0, k1 = np.repeat(keys[:, 0], n), np.repeat(keys[:, 1], n)
    out = np.zeros(S * n, dtype=np.uint64)
    todo = np.arange(S * n)
    walk = 0
    while todo.size:
        H, L = (x >> sc) & ma, x & mc
        for r in range(4):
            if r % 2 == 0:
                H = H ^ (philox4x32_10((L, r, PERM_TAG[0], PERM_TAG[1]), (k0, k1))[0] & ma)
            else:
                L = L ^ (philox4x32_10((H, r, PERM_TAG[0], PERM_TAG[1]), (k0, k1))[0] & mc)
        x = (H << sc) | L
        walk += 1
        assert walk <= (1 << (a + c)), "the cycle walk did not return"
        done = x < np.uint64(n)
        out[todo[done]] = x[done]
        keep = ~done
        todo, x, k0, k1 = todo[keep], x[keep], k0[keep], k1[keep]
    return out.astype(np.int64).reshape(S, n)


def perm_uniformity(n, seeds, chunk=500):
    """The standardised chi-square of the (index, value) counts of permutation_ref(n, seed) over
    the seeds against the uniform null: (chi2 - dof) / sqrt(2 dof), dof = (n - 1)^2."""
    cnt = np.zeros(n * n)
    idx = np.arange(n) * n
    for s0 in range(0, len(seeds), chunk):
        p = permutation_batch(n, seeds[s0:s0 + chunk])
        cnt += np.bincount((p + idx).ravel(), minlength=n * n)
    e = len(seeds) / n
    chi, dof = ((cnt - e) ** 2 / e).sum(), (n - 1) ** 2
    return (chi - dof) / math.sqrt(2 * dof)


def perm_seeds(count):
    return [(s * 0x9E3779B97F4A7C15 + 12345) & 0xFFFFFFFFFFFFFFFF for s in range(count)]


def noise_statistics(seed, N=1 << 18, A=12):
    """The statistics of the distribution test on noise_ref (A a multiple of 4), each in units of
    its standard error under the null: the first four moments and the Kolmogorov-Smirnov statistic
    (times sqrt n) of draw 0's N A values, and the correlations between the cos and sin members of
    a pair, the two halves of a quad, neighbouring quads, neighbouring rows and draws 0 and 1.
    Returns (statistics, n)."""
    z0, z1 = noise_ref(seed, 0, N, A), noise_ref(seed, 1, N, A)
    x = z0.ravel()
    n = x.size
    rn = math.sqrt(n)
    st = dict(mean=x.mean() * rn, var=((x * x).mean() - 1.0) * rn / math.sqrt(2.0),
              third=(x ** 3).mean() * rn / math.sqrt(15.0), fourth=((x ** 4).mean() - 3.0) * rn / math.sqrt(96.0))

    def corr(a, b):
        return np.corrcoef(a.ravel(), b.ravel())[0, 1] * math.sqrt(a.size)
    q = z0.reshape(N, A // 4, 4)
    st["pair"] = corr(z0[:, 0::2], z0[:, 1::2])
    st["halves"] = corr(q[:, :, :2], q[:, :, 2:])
    st["quads"] = corr(q[:, :-1], q[:, 1:])
    st["rows"] = corr(z0[:-1], z0[1:])
    st["draws"] = corr(z0, z1)
    # KS at every 8th order statistic: between two of them the empirical distribution function
    # moves by 8 / n, 3e-6 at the test's n against a threshold of 1.5e-3
    k = np.arange(0, n, 8)
    xs = np.sort(x)[k]
    cdf = 0.5 * (1.0 + np.frompyfunc(math.erf, 1, 1)(xs / math.sqrt(2.0)).astype(np.float64))
    st["ks"] = max((cdf - k / n).max(), ((k + 1) / n - cdf).max()) * rn
    st["max"] = np.abs(x).max()
    return {k: float(v) for k, v in st.items()}, n
