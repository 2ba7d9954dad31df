"""tests/distill_ref.py held to itself on the host: the references against a literal torch
statement, the comparison functions against deliberately wrong outputs, and the input conditions
of every GPU case of tests/test_gpu_distill_reference.py."""
import numpy as np
import pytest
import torch

import distill_ref as dr

TYPES = (dr.MSE, dr.HUBER)


def _bf16_bits(x):
    """float64/32 array -> bf16 bit patterns (round to nearest even), as the kernel's store."""
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _outputs(mu, target, loss_type, scale, Ap):
    """A faithful float32 emulation of the kernel's outputs (the roundings the bounds count)."""
    f = np.float32
    d = (mu - target).astype(f)
    if loss_type == dr.MSE:
        g, term = (f(2.0) * d) * f(scale), d * d
    else:
        inside = np.abs(d) <= 1
        g = np.where(inside, d * f(scale), np.copysign(f(scale), d)).astype(f)
        term = np.where(inside, (f(0.5) * d) * d, np.abs(d) - f(0.5)).astype(f)
    M, A = d.shape
    bits = np.zeros((M, Ap), np.uint16)
    bits[:, :A] = _bf16_bits(g)
    partial = np.array([t.astype(f).sum(dtype=f) for t in dr._groups(term)], f)
    stats = np.zeros(4, f)
    stats[0] = partial.sum(dtype=f) * f(scale)
    return bits, g.astype(f), partial, stats


@pytest.mark.parametrize("loss_type", TYPES)
def test_reference_is_torchs_loss_and_gradient(loss_type):
    """G steps of N rows: the sum of torch's per-step mean losses, and its autograd gradient."""
    N, A, G = 8, 3, 2
    mu, target = dr.loss_case(G * N, A, loss_type)
    m = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(target, dtype=torch.float64)
    fn = torch.nn.functional.mse_loss if loss_type == dr.MSE else \
        (lambda a, b: torch.nn.functional.huber_loss(a, b, delta=1.0))
    loss = sum(fn(m[s * N:(s + 1) * N], t[s * N:(s + 1) * N]) for s in range(G))
    loss.backward()
    scale = 1.0 / (N * A)  # (fp64 here: the reference takes the scale it is given)
    term, _ = dr.terms_ref(mu, target, loss_type)
    np.testing.assert_allclose(term.sum() * scale, loss.item(), rtol=1e-13)
    d = dr._d(mu, target)
    g = 2.0 * d * scale if loss_type == dr.MSE else np.where(np.abs(d) > 1, np.sign(d), d) * scale
    np.testing.assert_allclose(g, m.grad.numpy(), rtol=1e-13, atol=0)
    s32 = dr.entry_scale(N, A)
    np.testing.assert_allclose(dr.grad_ref(mu, target, loss_type, s32), g, rtol=2e-7)


@pytest.mark.parametrize("loss_type", TYPES)
@pytest.mark.parametrize("A,Ap", dr.WIDTHS)
@pytest.mark.parametrize("M", dr.ROWS)
def test_case_conditions_and_faithful_outputs_pass(M, A, Ap, loss_type):
    c = dr.case_conditions(M, A, loss_type)
    assert c["exact"]
    assert Ap % 8 == 0 and A <= Ap <= 32
    if loss_type == dr.HUBER:
        assert c["at"], "a huber case without |d| == 1"
        if c["entries"] >= 4:
            assert c["inside"] and c["outside"]
    mu, target = dr.loss_case(M, A, loss_type)
    scale = dr.entry_scale(dr.ENVS, A)
    bits, gf, partial, stats = _outputs(mu, target, loss_type, scale, Ap)
    fr = dr.check_grad(bits, gf, mu, target, loss_type, scale)
    fr.update(dr.check_loss(partial, stats, mu, target, loss_type, scale))
    assert all(v <= 1.0 for v in fr.values()), fr
    assert partial.shape == (dr.num_partials(M),)


def test_huber_branches_agree_at_one():
    mu = np.array([[1.0, -1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20]], np.float32)
    target = np.zeros_like(mu)
    term, lin = dr.terms_ref(mu, target, dr.HUBER)
    g = dr.grad_ref(mu, target, dr.HUBER, 1.0)
    assert term[0, 0] == 0.5 and term[0, 1] == 0.5 and not lin[0, 0] and not lin[0, 1]
    assert g[0, 0] == 1.0 and g[0, 1] == -1.0
    # both branches' values at |d| = 1, written out
    assert 0.5 * 1.0 * 1.0 == abs(1.0) - 0.5
    assert abs(term[0, 2] - term[0, 3]) < 2.0 ** -18


CASE = (65, 12, 16)


@pytest.mark.parametrize("loss_type", TYPES)
def test_rejects_a_gradient_scaled_by_rows_instead_of_envs(loss_type):
    M, A, Ap = CASE
    mu, target = dr.loss_case(M, A, loss_type)
    scale = dr.entry_scale(dr.ENVS, A)
    wrong = np.float32(1.0 / (M * A))  # the mean over the block's rows: not the steps' means
    bits, gf, _, _ = _outputs(mu, target, loss_type, wrong, Ap)
    with pytest.raises(AssertionError):
        dr.check_grad(bits, None, mu, target, loss_type, scale)
    with pytest.raises(AssertionError):
        good_bits, _, _, _ = _outputs(mu, target, loss_type, scale, Ap)
        dr.check_grad(good_bits, gf, mu, target, loss_type, scale)


def test_rejects_an_unclamped_huber_gradient():
    M, A, Ap = CASE
    mu, target = dr.loss_case(M, A, dr.HUBER)
    scale = dr.entry_scale(dr.ENVS, A)
    g = ((mu - target) * scale).astype(np.float32)  # d * scale everywhere: no clamp beyond delta
    bits = np.zeros((M, Ap), np.uint16)
    bits[:, :A] = _bf16_bits(g)
    with pytest.raises(AssertionError):
        dr.check_grad(bits, None, mu, target, dr.HUBER, scale)
    good, _, _, _ = _outputs(mu, target, dr.HUBER, scale, Ap)
    with pytest.raises(AssertionError):
        dr.check_grad(good, g, mu, target, dr.HUBER, scale)


@pytest.mark.parametrize("loss_type", TYPES)
def test_rejects_a_nonzero_padded_column(loss_type):
    M, A, Ap = CASE
    mu, target = dr.loss_case(M, A, loss_type)
    scale = dr.entry_scale(dr.ENVS, A)
    bits, gf, _, _ = _outputs(mu, target, loss_type, scale, Ap)
    dr.check_grad(bits, gf, mu, target, loss_type, scale)
    for v in (0x8000, 0x0001, 0x3f80):  # -0, the smallest subnormal, 1.0
        bad = bits.copy()
        bad[M - 1, Ap - 1] = v
        with pytest.raises(AssertionError):
            dr.check_grad(bad, gf, mu, target, loss_type, scale)


@pytest.mark.parametrize("loss_type", TYPES)
def test_rejects_wrong_partials_and_loss(loss_type):
    M, A, Ap = CASE
    mu, target = dr.loss_case(M, A, loss_type)
    scale = dr.entry_scale(dr.ENVS, A)
    _, _, partial, stats = _outputs(mu, target, loss_type, scale, Ap)
    dr.check_loss(partial, stats, mu, target, loss_type, scale)
    bad = partial.copy()
    bad[1] = np.nextafter(bad[1], np.float32(np.inf)) * np.float32(1.0 + 2.0 ** -12)
    with pytest.raises(AssertionError):
        dr.check_loss(bad, stats, mu, target, loss_type, scale)
    bad = stats.copy()
    bad[0] *= np.float32(M / dr.ENVS)  # a loss averaged over the wrong count
    with pytest.raises(AssertionError):
        dr.check_loss(partial, bad, mu, target, loss_type, scale)
    bad = stats.copy()
    bad[2] = 1.0
    with pytest.raises(AssertionError):
        dr.check_loss(partial, bad, mu, target, loss_type, scale)
    if loss_type == dr.HUBER:  # the mse's terms in the huber's place
        _, _, p2, s2 = _outputs(mu, target, dr.MSE, scale, Ap)
        with pytest.raises(AssertionError):
            dr.check_loss(p2, s2, mu, target, dr.HUBER, scale)


def test_bf16_bound_is_half_an_ulp_of_eight_bits():
    # 1 + 2^-8 lies half-way between the bf16 neighbours 1 and 1 + 2^-7: the worst case of the store
    g = np.array([1.0, 1.0 + 2.0 ** -8, 1.99, 3.0, 0.0])
    np.testing.assert_array_equal(dr.half_ulp_bf16(g), [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0])
    b = dr.grad_bound(g, bf16=True)
    assert np.all(b >= 2.0 ** -9 * np.abs(g)) and np.all(b <= 2.0 ** -8 * np.abs(g) * 1.001)
    got = dr.bf16_to_f64(_bf16_bits(g))
    assert np.all(np.abs(got - g) <= dr.half_ulp_bf16(g))
