"""tests/gemm_ref.py checked on the CPU: the exactness claim its bitwise comparisons rest on,
the conditions of its inputs, and that the checks bite -- a torch emulation of the kernels
(fp32 matmul, expm1, bf16 rounding) passes and each of a list of plausible kernel bugs fails."""
import pytest
import torch

import gemm_ref as R

CPU = "cpu"


def _trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (the bug: no round-to-nearest)."""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(R.BF16)


def _emu_hidden(a, w, b, store=lambda v: v.to(R.BF16)):
    v = a.float() @ w.float().t() + b[None, :]
    return store(torch.where(v > 0, v, torch.expm1(v)))


def _emu_out(a, w, b):
    return a.float() @ w.float().t() + b[None, :]


def _emu_bwd(dz, wt, y, store=lambda v: v.to(R.BF16)):
    acc = dz.float() @ wt.float().t()
    yf = y.float()
    return store(torch.where(yf > 0, acc, acc * (yf + 1.0)))


def _fwd_case(K, seed, M=70, N=72):
    g = R.gen(seed, CPU)
    return R.grid_act((M, K), g, CPU), R.grid_weight((N, K), K, g, CPU), R.grid_bias(N, g, CPU)


def _fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.mark.parametrize("K", R.ALL_K)
def test_fp32_accumulation_is_exact_in_any_order(K):
    """The fp32 product accumulated in forward and in reversed k order and the fp64 product are
    bitwise equal: every partial sum of the grid inputs is an fp32 number."""
    g = R.gen(K, CPU)
    M, N = 24, 40
    a = R.grid_act((M, K), g, CPU, torch.float32)
    w = R.grid_weight((N, K), K, g, CPU, torch.float32)
    b = R.grid_bias(N, g, CPU)
    assert torch.equal(a, a.to(R.BF16).float()) and torch.equal(w, w.to(R.BF16).float())
    assert torch.equal(b, b.to(R.BF16).float())
    assert 256 * K + 8 * R.grid_scale(K) < 2 ** 24
    fwd = torch.zeros(M, N)
    rev = torch.zeros(M, N)
    for k in range(K):
        fwd += a[:, k, None] * w[None, :, k]
        rev += a[:, K - 1 - k, None] * w[None, :, K - 1 - k]
    fwd += b
    rev = b + rev
    ref = R.preact(a, w, b)
    assert torch.equal(fwd, rev)
    assert torch.equal(fwd.double(), ref)
    assert torch.equal((a @ w.t() + b).double(), ref)  # (whatever order the BLAS takes)
    # the BWD_DX factor keeps the product an fp32 number
    y = R.grid_yprev((M, N), g, CPU)
    assert torch.equal(y.float(), y.float().to(R.BF16).float())
    r = R.bwd_dx_ref(a, w, y)
    R.assert_fp32_exact(r, "BWD_DX")
    assert torch.equal((fwd - b).mul(torch.where(y.float() > 0, torch.ones(M, N), y.float() + 1)).double(), r)


@pytest.mark.parametrize("K", R.ALL_K)
def test_input_conditions_hold_and_the_emulation_is_accepted(K):
    a, w, b = _fwd_case(K, 100 + K)
    v = R.preact(a, w, b)
    assert 0.6 < float(v.std()) < 0.9, float(v.std())
    cond = R.Conditions()
    R.check_fwd_hidden(_emu_hidden(a, w, b), a, w, b, cond)  # (5040 outputs: asserts its own conditions too)
    cond.assert_ok()
    R.check_fwd_out(_emu_out(a, w, b), a, w, b)
    g = R.gen(K, CPU)
    y = R.grid_yprev((a.shape[0], w.shape[0]), g, CPU)
    R.check_bwd_dx(_emu_bwd(a, w, y), a, w, y)


def test_round_bf16_is_round_to_nearest_even_from_fp64():
    bits = lambda h: torch.tensor([h], dtype=torch.int32).view(torch.float32).double()  # noqa: E731
    x = torch.cat([bits(0x3F808000), bits(0x3F818000), bits(0x3F808001), -bits(0x3F818000), bits(0x3FFF8000),
                   torch.tensor([0.0, 1.0, -0.75])])
    want = torch.cat([bits(0x3F800000), bits(0x3F820000), bits(0x3F810000), -bits(0x3F820000), bits(0x40000000),
                      torch.tensor([0.0, 1.0, -0.75])])
    assert torch.equal(R.round_bf16(x), want)
    assert torch.equal(x.float().to(R.BF16).double(), want)  # torch's fp32 -> bf16 cast is the same rounding
    # one rounding from fp64: just above a tie that the detour through fp32 would round to even
    t = bits(0x3F808000) + 2.0 ** -40
    assert R.round_bf16(t).item() == bits(0x3F810000).item() and t.float().to(R.BF16).double().item() == 1.0
    r = torch.randn(4096, dtype=torch.float64)
    assert torch.equal(R.round_bf16(r.float().double()), r.float().to(R.BF16).double())
    o = R.bf16_ordinal(torch.tensor([-1.0, -0.0, 0.0, 1.0, 1.0078125], dtype=torch.float64))
    assert o[1] == o[2] and o[0] < o[1] < o[3] and o[4] - o[3] == 1


def _move_one_ulp(t, idx):
    m = t.clone()
    m.view(torch.int16)[idx] += 1
    return m


@pytest.mark.parametrize("K", [48, 72, 256])
def test_forward_mutations_are_rejected(K):
    a, w, b = _fwd_case(K, 7 + K)
    good = _emu_hidden(a, w, b)
    R.check_fwd_hidden(good, a, w, b)
    lo, hi = R.elu_bounds(R.preact(a, w, b), R.E_ELU)
    # one non-ambiguous element (one acceptable bf16 value) moved by one bf16 ulp, either way,
    # on both branches
    v = R.preact(a, w, b)
    for sel in ((lo == hi) & (v > 0), (lo == hi) & (v < 0)):
        idx = tuple(int(i) for i in sel.nonzero()[len(sel.nonzero()) // 2])
        up = _move_one_ulp(good, idx)
        down = good.clone()
        down.view(torch.int16)[idx] -= 1
        assert abs(float(up[idx]) - float(good[idx])) > 0 and abs(float(down[idx]) - float(good[idx])) > 0
        _fails(R.check_fwd_hidden, up, a, w, b)
        _fails(R.check_fwd_hidden, down, a, w, b)
    # the last 8 k dropped (a ragged last k-tile read short)
    _fails(R.check_fwd_hidden, _emu_hidden(a[:, :K - 8], w[:, :K - 8], b), a, w, b)
    _fails(R.check_fwd_out, _emu_out(a[:, :K - 8], w[:, :K - 8], b), a, w, b)
    # the neighbouring column's bias
    _fails(R.check_fwd_hidden, _emu_hidden(a, w, b.roll(1)), a, w, b)
    _fails(R.check_fwd_out, _emu_out(a, w, b.roll(1)), a, w, b)
    # truncation instead of round-to-nearest in the bf16 store
    _fails(R.check_fwd_hidden, _emu_hidden(a, w, b, store=_trunc_bf16), a, w, b)
    # two output rows swapped
    sw = good.clone()
    sw[[3, 4]] = sw[[4, 3]]
    _fails(R.check_fwd_hidden, sw, a, w, b)
    o = _emu_out(a, w, b)
    o[[3, 4]] = o[[4, 3]]
    _fails(R.check_fwd_out, o, a, w, b)
    # the transposed output: correct, then with one 32 x 32 tile left untransposed
    ct = good.t().contiguous()
    R.check_ct(ct, good)
    ct[32:64, 32:64] = good[32:64, 32:64]
    _fails(R.check_ct, ct, good)
    # a NaN or an untouched sentinel is not accepted anywhere
    for bad in (float("nan"), R.SENTINEL):
        m = good.clone()
        m[5, 6] = bad
        _fails(R.check_fwd_hidden, m, a, w, b)


@pytest.mark.parametrize("K", [16, 64, 200])
def test_input_gradient_mutations_are_rejected(K):
    g = R.gen(31 + K, CPU)
    M, N = 70, 72
    dz, wt, y = R.grid_act((M, K), g, CPU), R.grid_weight((N, K), K, g, CPU), R.grid_yprev((M, N), g, CPU)
    good = _emu_bwd(dz, wt, y)
    R.check_bwd_dx(good, dz, wt, y)
    nz = (good.float() != 0).nonzero()
    _fails(R.check_bwd_dx, _move_one_ulp(good, tuple(int(i) for i in nz[len(nz) // 2])), dz, wt, y)
    _fails(R.check_bwd_dx, _emu_bwd(dz[:, :K - 8], wt[:, :K - 8], y), dz, wt, y)
    _fails(R.check_bwd_dx, _emu_bwd(dz, wt, y.roll(1, 0)), dz, wt, y)  # the neighbouring row's yprev
    _fails(R.check_bwd_dx, _emu_bwd(dz, wt, y, store=_trunc_bf16), dz, wt, y)
    sw = good.clone()
    sw[[3, 4]] = sw[[4, 3]]
    _fails(R.check_bwd_dx, sw, dz, wt, y)
    # ELU' taken from y >= 0 instead of y > 0 (y = 0 is on the negative branch: factor 1 either
    # way) is the same function; from y > -1 + ... it is not: the factor at y = -1 is 0
    _fails(R.check_bwd_dx, _emu_bwd(dz, wt, torch.where(y.float() == -1, torch.ones(()), y.float()).to(R.BF16)),
           dz, wt, y)


@pytest.mark.parametrize("K,ks", R.PARTIAL_KS)
def test_partial_slabs_are_checked_one_by_one(K, ks):
    g = R.gen(K, CPU)
    M, N = 12, 40
    a, b = R.grid_act((K, M), g, CPU), R.grid_weight((K, N), ks, g, CPU)
    S = (K + ks - 1) // ks
    slabs = torch.stack([a[s * ks:(s + 1) * ks].float().t() @ b[s * ks:(s + 1) * ks].float() for s in range(S)])
    sums = torch.stack([a[s * ks:(s + 1) * ks].float().sum(0) for s in range(S)])
    R.check_partial(slabs, a, b, ks, sums)
    # two slabs exchanged: their sum is unchanged, the slabs are not
    sw = slabs.clone()
    sw[[0, S - 1]] = sw[[S - 1, 0]]
    _fails(R.check_partial, sw, a, b, ks)
    # a slab that ran 8 k into the next one / stopped 8 k short
    over = slabs.clone()
    over[0] += a[ks:ks + 8].float().t() @ b[ks:ks + 8].float()
    _fails(R.check_partial, over, a, b, ks)
    short = slabs.clone()
    short[S - 1] -= a[K - 8:].float().t() @ b[K - 8:].float()
    _fails(R.check_partial, short, a, b, ks)
    _fails(R.check_partial, slabs, a, b, ks, sums.roll(1, 1))


def test_random_normal_class_bounds_accept_fp32_and_reject_operand_truncation():
    g = R.gen(5, CPU)
    M, N, K = 64, 72, 200
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g).to(R.BF16)
    b = torch.randn(N, generator=g)
    a = x.to(R.BF16)
    R.check_fwd_out_bound(_emu_out(a, w, b), a, w, b)
    R.check_fwd_hidden_bound(_emu_hidden(a, w, b), a, w, b)
    at = _trunc_bf16(x)  # the rows truncated instead of rounded on load
    assert not torch.equal(at, a)
    _fails(R.check_fwd_out_bound, _emu_out(at, w, b), a, w, b)
    _fails(R.check_fwd_out_bound, _emu_out(a[:, :K - 8], w[:, :K - 8], b), a, w, b)
    _fails(R.check_fwd_hidden_bound, _emu_hidden(a, w, b.roll(1)), a, w, b)


def test_guarded_output_notices_a_stray_write():
    for dtype in (torch.float32, R.BF16):
        G = R.Guarded(5, 7, 12, dtype, CPU, slabs=2)
        assert G.t.shape == (2, 5, 12) and G.mat.stride(0) == 12
        G.t[:, :, :7] = 1.0
        G.t[:, :, 9] = 2.0
        G.assert_untouched("ok", extra_cols=(9,))
        _fails(G.assert_untouched, "col 9")
        for off in (0, G.guard - 1, G.guard + 7, G.guard + 60, -1):  # band, column 7, the row past the last
            H = R.Guarded(5, 7, 12, dtype, CPU)
            H.flat[off] = 0.0
            _fails(H.assert_untouched, "stray")
    a = torch.tensor([0.0, float("nan")])
    assert R.same_bits(a, a.clone()) and not R.same_bits(a, torch.tensor([-0.0, float("nan")]))


def test_tile_config_table_reaches_every_configuration():
    """The sweep's shapes against pmlp_gemm's selection: each configuration is reached."""
    H, O, D = 0, 1, 2
    assert {R.tile_config(H, m, n, 64, 1) for m in (1, 12, 32) for n in (136, 128)} == {(32, 128, 1, 4)}
    assert {R.tile_config(D, m, n, 64, 1) for m in (37, 200) for n in (1, 12, 32)} == {(128, 32, 4, 1)}
    assert {R.tile_config(O, m, n, 64, 1) for m in (37, 200) for n in (40, 64)} == {(128, 64, 4, 1)}
    assert {R.tile_config(H, m, n, 320, 1) for m in (100, 129) for n in (136, 264, 128)} == {(64, 64, 2, 2)}
    assert R.tile_config(H, 4000, 512, 200, 4) == (128, 128, 2, 4)
    assert R.tile_config(O, 4000, 512, 320, 4) == R.tile_config(D, 4000, 512, 320, 4) == (128, 128, 2, 4)
    assert R.tile_config(H, 4000, 512, 256, 4) == R.tile_config(H, 4000, 512, 320, 4) == (128, 128, 2, 2)
    assert R.tile_config(H, 3968, 512, 256, 4) == (64, 64, 2, 2)
    assert R.tile_config(4, 128, 264, 1000, 1) == (128, 128, 2, 4)
