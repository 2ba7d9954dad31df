"""tests/act_ref.py itself, on the CPU: Philox against the published known answers, the env
step's draw against them, the policy noise's distribution proved on the statement (fixed seeds:
deterministic), the permutation's bijection and uniformity, and the comparison functions against
a float32 numpy emulation of the kernels with one deliberate mistake at a time: each must fail
on the mutant and pass on the unmutated emulation ("The acting anchor")."""
import ctypes as C
import math

import numpy as np
import pytest

import act_ref as R

F = np.float32
SEED = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------- known answers --
KAT = [  # Random123 kat_vectors, philox4x32 10
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_reproduces_the_published_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert " ".join("%08x" % int(w) for w in got) == want
    # vectorised: the same words at every position of an array of counters
    arr = R.philox4x32_10([np.full(5, c) for c in counter], key)
    assert all((a == g).all() for a, g in zip(arr, got))


def _rne24(x):
    """(float)x of a 32-bit unsigned x in integer arithmetic: round to nearest even at 24 bits."""
    if x < (1 << 24):
        return x
    sh = x.bit_length() - 24
    q, r = x >> sh, x & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return q << sh


def test_u01_is_the_exact_float32_value_and_its_edges():
    rng = np.random.default_rng(1)
    xs = [0, 1, 255, 256, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, 0x7fffffff, 0x80000000, 0xffffff7f,
          0xffffff80, 0xffffff81, 0xffffffff] + [int(v) for v in rng.integers(0, 1 << 32, 4000)]
    got = R.u01_ref(np.array(xs, np.uint64))
    assert got.dtype == np.float32
    for x, g in zip(xs, got):
        s = _rne24(x) + 0.5                     # exact in fp64 (at most 33 bits)
        want = F(s) * F(2.0 ** -32)             # one rounding of the sum; the scaling is exact
        assert g == want and float(want) == float(F(s)) * 2.0 ** -32, hex(x)
    assert float(R.u01_ref(0)) == 2.0 ** -33
    assert float(R.u01_ref(0xffffff7f)) < 1.0 and all(float(R.u01_ref(x)) == 1.0 for x in (0xffffff80, 0xffffffff))
    # what it implies: |z| <= sqrt(66 ln 2), and u = 1 gives a zero radius, never a NaN
    assert math.sqrt(-2.0 * math.log(2.0 ** -33)) == pytest.approx(R.Z_MAX, rel=1e-15) and 6.76 < R.Z_MAX < 6.77
    assert math.sqrt(-2.0 * math.log(float(R.u01_ref(0xffffffff)))) == 0.0


def test_oracle_uniform_rests_on_the_known_answers(oracle_lib):
    """orc_uniform == uniform_ref (which test_philox_reproduces_... ties to Random123), with the
    seed's high word set and every counter word at 0 and 0xffffffff."""
    oracle_lib.orc_uniform.restype = C.c_float
    oracle_lib.orc_uniform.argtypes = [C.c_uint64] + [C.c_uint32] * 4
    for seed, *args in R.uniform_cases():
        want = R.uniform_ref(seed, *args)
        got = F(oracle_lib.orc_uniform(seed, *args))
        assert got == want and 0.0 <= got < 1.0, (hex(seed), args)
    # the draw is the high 24 bits of word 0
    w0 = int(R.philox4x32_10((1, 2, 3, 4), R.seed_key(SEED))[0])
    assert float(R.uniform_ref(SEED, 1, 2, 3, 4)) == (w0 >> 8) / 2.0 ** 24


# ------------------------------------------------------------------ distribution --
def test_policy_noise_is_standard_normal_and_uncorrelated():
    """N = 2^18 rows x A = 12: 3,145,728 values of draw 0 (and draw 1 for the correlation between
    draws).  Moments within 5 standard errors of 0, 1, 0, 3; correlations within 5 / sqrt n; the
    Kolmogorov-Smirnov statistic below 2.7 / sqrt n (the 1e-6 level).  Measured at this seed:
    moments 0.49, -0.44, 0.21, -0.58; correlations -0.72 .. +0.37; KS 0.50."""
    st, n = R.noise_statistics(SEED)
    print(st)
    assert n == (1 << 18) * 12
    for k in ("mean", "var", "third", "fourth", "pair", "halves", "quads", "rows", "draws"):
        assert abs(st[k]) < 5.0, (k, st[k])
    assert st["ks"] < 2.7, st["ks"]
    assert st["max"] <= R.Z_MAX


def test_noise_ref_layout_rows_and_draw_word():
    z = R.noise_ref(SEED, 5, 7, 10)
    assert z.shape == (7, 10) and np.isfinite(z).all()
    # a row's noise depends on its index alone, and A only cuts the last quad
    assert R.same_bits(R.noise_ref(SEED, 5, np.array([3, 6]), 10), z[[3, 6]])
    assert R.same_bits(R.noise_ref(SEED, 5, 7, 12)[:, :10], z)
    # the draw word is the low 32 bits; the seed's high word is the second key word
    assert R.same_bits(R.noise_ref(SEED, (1 << 32) + 5, 7, 10), z)
    assert not R.same_bits(R.noise_ref(SEED, 6, 7, 10), z)
    assert not R.same_bits(R.noise_ref(SEED ^ (1 << 40), 5, 7, 10), z)
    # each pair lies on its radius' circle
    zz, rad = R.noise_parts(SEED, 5, 7, 12)
    np.testing.assert_allclose(zz[:, 0::2] ** 2 + zz[:, 1::2] ** 2, rad[:, 0::2] ** 2, rtol=1e-12)


# ------------------------------------------------------------------- permutation --
PERM_N = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 4096, 4097, 98304, 100003)


@pytest.mark.parametrize("n", PERM_N)
def test_permutation_ref_is_a_bijection(n):
    for seed in (0x123456789abcdef, 0xFEDCBA9800000007):
        p, walk = R.permutation_ref(n, seed, steps=True)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n))
        a, c = R.perm_split(n)
        assert a >= 1 and c >= a and c - a <= 1 and (1 << (a + c)) >= n and ((1 << (a + c)) < 2 * n or n <= 2)
        assert walk <= 40, walk     # (13 at n = 4097 with the first seed: the domain is below 2 n)
    assert R.same_bits(R.permutation_batch(n, [5, 0xFEDCBA9800000007])[1], p)


@pytest.mark.parametrize("n,count", [(64, 4000), (1000, 3000)])
def test_permutation_is_uniform_over_seeds(n, count):
    """The (index, value) counts over the seeds against the uniform null: chi-square has mean dof =
    (n - 1)^2 and sd sqrt(2 dof); within 5 sigma.  Measured -0.2 (n = 64) and +1.2 (n = 1000)."""
    s = R.perm_uniformity(n, R.perm_seeds(count))
    print(n, s)
    assert abs(s) < 5.0, s


def test_permutation_is_not_uniform_at_tiny_n():
    """With halves of one or two bits the four-round network is visibly non-uniform: +7.3, +30.7,
    +29.6 sigma at n = 3, 5, 6 over 4,000 seeds (and +5.8 at 12, +4.4 at 17).  The update calls it
    with n = 98,304 and include/ppo_mlp.h says so; this assertion is here so that a change of the
    network shows up (if it starts failing because the network became uniform: good, move the
    sizes into the test above)."""
    for n in (3, 5, 6):
        s = R.perm_uniformity(n, R.perm_seeds(4000))
        print(n, s)
        assert s > 5.0, (n, s)


# ------------------------------------------------ the emulation and its mutants --
def emu_philox(counter, key, rounds=10, swap_mul=False, advance=True):
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [np.asarray(x, np.uint64) & m32 for x in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter])]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    ma, mb = (0xCD9E8D57, 0xD2511F53) if swap_mul else (0xD2511F53, 0xCD9E8D57)
    for _ in range(rounds):
        p0, p1 = np.uint64(ma) * c[0], np.uint64(mb) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & m32, (p0 >> s32) ^ c[3] ^ k1, p0 & m32]
        if advance:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c


def _f(x):
    return np.asarray(x, np.float64).astype(F)


def emu_act(seed, draw, mu, stdv, mut="", fma=False, rows=None):
    """k_act4 / k_act / roll_epilogue / the heads' ACT branch in float32 numpy (logf, sqrtf,
    sincospif and the division as the correctly rounded fp64 value); mut names one mistake.
    fma: mu + sigma z in one rounding (the contracted form the sampling arms had)."""
    mu = np.asarray(mu, F)
    N, A = mu.shape
    Q = (A + 3) // 4
    key = R.seed_key(seed)
    if mut == "key_swapped":
        key = key[::-1]
    rows = np.arange(N, dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    i, c = np.repeat(rows, Q), np.tile(np.arange(Q, dtype=np.uint64), N)
    cnt = [np.uint64(int(draw) & 0xFFFFFFFF), i, c, np.uint64(0x5050)]
    if mut == "row_draw_exchanged":
        cnt[0], cnt[1] = cnt[1], cnt[0]
    if mut == "quad_zero":
        cnt[2] = np.zeros_like(c)
    if mut == "no_tag":
        cnt[3] = np.uint64(0)
    w = emu_philox(cnt, key, rounds=9 if mut == "nine_rounds" else 10, swap_mul=mut == "multipliers_swapped",
                   advance=mut != "key_not_advanced")

    def u01(x):
        if mut == "u01_no_half":
            return x.astype(F) * F(2.0 ** -32)
        if mut == "u01_24_bits":
            return ((x >> np.uint64(8)).astype(F) + F(0.5)) * F(2.0 ** -24)
        return (x.astype(F) + F(0.5)) * F(2.0 ** -32)
    ux, uy, uz, uw = [u01(x) for x in w]
    with np.errstate(divide="ignore"):
        rad0 = _f(np.sqrt(_f(-2.0 * _f(np.log(ux.astype(np.float64)))).astype(np.float64)))
        rad1 = _f(np.sqrt(_f(-2.0 * _f(np.log(uz.astype(np.float64)))).astype(np.float64)))
    a0, a1 = (F(2) * uy).astype(np.float64) * np.pi, (F(2) * uw).astype(np.float64) * np.pi
    cs = [_f(np.cos(a0)), _f(np.sin(a0)), _f(np.cos(a1)), _f(np.sin(a1))]
    if mut == "sin_cos_exchanged":
        cs = [cs[1], cs[0], cs[3], cs[2]]
    rr = [rad1, rad1, rad0, rad0] if mut == "other_radius" else [rad0, rad0, rad1, rad1]
    z = np.stack([t * r for t, r in zip(cs, rr)], 1).astype(F).reshape(N, 4 * Q)[:, :A]
    sg = np.broadcast_to(np.asarray(stdv, F), (N, A))
    sg_used = np.roll(sg, -1, axis=1) if mut == "neighbour_sigma" else sg
    if fma:
        act = _f(mu.astype(np.float64) + sg_used.astype(np.float64) * z.astype(np.float64))
    else:
        act = mu + sg_used * z
    d = (sg_used * z) if mut == "logp_from_sigma_z" else (act - mu)
    den = sg if mut == "sigma_for_two_sigma_squared" else (F(2) * sg) * sg
    q = _f((d * d).astype(np.float64) / den.astype(np.float64))
    term = -q
    if mut != "no_log_sigma":
        term = term - _f(np.log(sg.astype(np.float64)))
    term = term - F(R.HALF_LOG_2PI)
    terms = np.full((N, 16), F(-0.7))           # (an LDS row's other slots: whatever was there)
    terms[:, :min(A, 16)] = term[:, :16]
    logp = np.zeros(N, F)
    for k in range(16 if mut == "sum_over_16" else A):
        logp = logp + (terms[:, k] if k < 16 else term[:, k])
    return dict(actions_out=act.astype(F), st_actions=act.astype(F).copy(), st_mu=mu.copy(), st_sigma=sg.copy(),
                st_logp=logp.astype(F))


def _act_case(A=10, N=257, scale=1.0):
    rng = np.random.default_rng(A * 1000 + N)
    mu = (scale * rng.standard_normal((N, A))).astype(F)
    stdv = (0.8 * (1.0 + 0.1 * np.arange(A) / A)).astype(F)
    return mu, stdv


ACT_MUTANTS = ("nine_rounds", "multipliers_swapped", "key_not_advanced", "row_draw_exchanged", "quad_zero", "no_tag",
               "u01_no_half", "u01_24_bits", "sin_cos_exchanged", "other_radius", "neighbour_sigma", "no_log_sigma",
               "sigma_for_two_sigma_squared", "sum_over_16", "logp_from_sigma_z", "key_swapped")


@pytest.mark.parametrize("A", [1, 3, 4, 10, 12, 16, 17, 23])
@pytest.mark.parametrize("fma", [False, True])
def test_the_unmutated_emulation_passes_the_checks(A, fma):
    mu, stdv = _act_case(A)
    fr = R.check_act_rows(emu_act(SEED, 5, mu, stdv, fma=fma), stdv, SEED, 5, mu=mu)
    print(A, fma, fr)
    assert 0.0 < fr["act"] < 1.0 and 0.0 < fr["logp"] < 1.0
    mu, stdv = np.zeros_like(mu), np.ones_like(stdv)       # sigma 1, mu 0: the action is z itself
    out = emu_act(SEED, 5, mu, stdv)
    R.check_act_rows(out, stdv, SEED, 5, mu=mu)
    assert np.abs(out["actions_out"]).max() <= R.Z_MAX


def small_radius_word_rows(seed, draw, A, below=1 << 13, among=1 << 20):
    """The rows (of the first `among`) one of whose radius words (r.x, r.z of a quad < ceil(A / 4))
    is below `below`: u01's half is a relative 1 / (2 x) of the uniform, beyond the bound on z only
    for x below about 2^15 (it is there so that x = 0 gives a finite radius)."""
    Q = (A + 3) // 4
    i, c = np.repeat(np.arange(among, dtype=np.uint64), Q), np.tile(np.arange(Q, dtype=np.uint64), among)
    w = R.philox4x32_10((int(draw) & 0xFFFFFFFF, i, c, R.NOISE_TAG), R.seed_key(seed))
    small = (np.minimum(w[0], w[2]) < np.uint64(below)).reshape(among, Q).any(1)
    return np.nonzero(small)[0]


@pytest.mark.parametrize("mut", ACT_MUTANTS)
def test_the_checks_reject_a_wrong_sampling(mut):
    # (logp_from_sigma_z differs from the stored act - mu by the rounding of act: visible where
    # |mu| is large against sigma, as for a trained policy's means in joint units)
    mu, stdv = _act_case(10, scale=60.0 if mut == "logp_from_sigma_z" else 1.0)
    rows = None
    if mut == "u01_no_half":                    # (only a small radius word shows it: see above)
        rows = small_radius_word_rows(SEED, 5, 10)
        assert 4 <= rows.size <= 40
        mu = mu[:rows.size]
    R.check_act_rows(emu_act(SEED, 5, mu, stdv, rows=rows), stdv, SEED, 5, mu=mu, rows=rows)
    with pytest.raises(AssertionError):
        R.check_act_rows(emu_act(SEED, 5, mu, stdv, mut=mut, rows=rows), stdv, SEED, 5, mu=mu, rows=rows)


def test_the_checks_reject_a_few_ulps_and_a_stale_copy():
    mu, stdv = _act_case(12)
    good = emu_act(SEED, 5, mu, stdv)
    bad = {k: v.copy() for k, v in good.items()}
    i = np.unravel_index(np.abs(good["actions_out"]).argmax(), mu.shape)
    for _ in range(16):
        bad["actions_out"][i] = np.nextafter(bad["actions_out"][i], F(np.inf))
    bad["st_actions"] = bad["actions_out"].copy()
    with pytest.raises(AssertionError):
        R.check_act_rows(bad, stdv, SEED, 5, mu=mu)
    for k in ("st_actions", "st_mu", "st_sigma"):
        bad = {j: v.copy() for j, v in good.items()}
        bad[k][3, 1] = np.nextafter(bad[k][3, 1], F(np.inf))
        with pytest.raises(AssertionError):
            R.check_act_rows(bad, stdv, SEED, 5, mu=mu)
    bad = {j: v.copy() for j, v in good.items()}
    bad["st_logp"][7] = np.nan
    with pytest.raises(AssertionError):
        R.check_act_rows(bad, stdv, SEED, 5, mu=mu)


def emu_store(rew, dones, touts, value, gamma, states, mut=""):
    f = F
    r = np.asarray(rew, f).copy()
    if touts is not None:
        src = dones if mut == "dones_for_time_outs" else touts
        to = (np.asarray(src) != 0).astype(f)
        v = np.roll(value, 1) if mut == "value_of_wrong_step" else value
        g = f(1.0) if mut == "no_gamma" else f(gamma)
        r = r + g * (np.asarray(v, f) * to)
    d = np.asarray(dones).astype(np.uint8) if mut == "done_byte_kept" else (np.asarray(dones) != 0).astype(np.uint8)
    z = (np.asarray(dones) != 0)
    if mut == "reset_on_time_out":
        z = z | (np.asarray(touts) != 0)
    outs = []
    for s in states:
        s = s.copy()
        s[z] = 0
        outs.append(s)
    return dict(st_rewards=r.astype(f), st_dones=d), outs


def _store_case(N=257, H=4):
    rng = np.random.default_rng(N)
    pick = np.array([0, 0, 0, 1, 2, 255], np.uint8)
    return dict(rew=rng.standard_normal(N).astype(F), dones=pick[rng.integers(0, 6, N)],
                touts=pick[rng.integers(0, 6, N)], value=(3.0 * rng.standard_normal(N)).astype(F), gamma=0.99,
                states=[rng.standard_normal((N, H)).astype(F) + F(3) for _ in range(2)])


def _check_store_case(c, out, states):
    R.check_store(out, c["rew"], c["dones"], c["touts"], c["value"], c["gamma"])
    for s0, s1 in zip(c["states"], states):
        R.check_equal(s1, R.reset_ref(s0, c["dones"]), "memory state")


@pytest.mark.parametrize("mut", ["", "dones_for_time_outs", "no_gamma", "value_of_wrong_step", "done_byte_kept",
                                 "reset_on_time_out"])
def test_the_checks_reject_a_wrong_store_step(mut):
    c = _store_case()
    assert ((c["dones"] != 0) != (c["touts"] != 0)).any() and (c["dones"] == 2).any()
    out, states = emu_store(c["rew"], c["dones"], c["touts"], c["value"], c["gamma"], c["states"], mut)
    if not mut:
        _check_store_case(c, out, states)
        # time_outs NULL: the reward itself
        out, _ = emu_store(c["rew"], c["dones"], None, c["value"], c["gamma"], [])
        R.check_store(out, c["rew"], c["dones"], None, c["value"], c["gamma"])
        assert R.same_bits(out["st_rewards"], c["rew"])
    else:
        with pytest.raises(AssertionError):
            _check_store_case(c, out, states)


def emu_permutation(n, seed, mut=""):
    b = 2
    while (1 << b) < n:
        b += 1
    a = b // 2
    c = a if mut == "both_halves_b_over_2" else b - a
    key = R.seed_key(seed)[::-1] if mut == "key_swapped" else R.seed_key(seed)
    rounds = 3 if mut == "three_rounds" else 4
    out = np.zeros(n, np.int64)
    for i in range(n):
        x = i
        for _ in range(1 << (a + c)):
            Hh, L = (x >> c) & ((1 << a) - 1), x & ((1 << c) - 1)
            for r in range(rounds):
                if r % 2 == 0:
                    Hh ^= int(emu_philox((L, r, 0x9e11, 0x7e37), key)[0]) & ((1 << a) - 1)
                else:
                    L ^= int(emu_philox((Hh, r, 0x9e11, 0x7e37), key)[0]) & ((1 << c) - 1)
            x = (Hh << c) | L
            if x < n or mut == "no_cycle_walk":
                break
        out[i] = x
    return out


@pytest.mark.parametrize("mut", ["", "three_rounds", "both_halves_b_over_2", "no_cycle_walk", "key_swapped"])
def test_the_checks_reject_a_wrong_permutation(mut):
    n, seed = 300, 0xFEDCBA9800000007          # b = 9: odd, and a domain of 512 to walk in
    got = emu_permutation(n, seed, mut)
    if not mut:
        R.check_permutation(got, n, seed)
    else:
        with pytest.raises(AssertionError):
            R.check_permutation(got, n, seed)
        if mut == "three_rounds":               # still a bijection: only the comparison tells
            assert np.array_equal(np.sort(got), np.arange(n))
