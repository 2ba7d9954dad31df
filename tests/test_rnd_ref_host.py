"""tests/rnd_ref.py held to itself (no GPU): the kernel's arithmetic in numpy float32, in the
kernel's order, sits inside every bound, and a perturbation of a few ulps outside a bound is
caught."""
import numpy as np
import pytest

import distill_ref as dr
import rnd_ref as rr
from act_ref import U
from rsl_rl.modules import rnd  # noqa: F401  (the feature these references belong to)


@pytest.mark.parametrize("E", rr.WIDTHS)
@pytest.mark.parametrize("T,N", rr.SHAPES)
def test_fp32_evaluation_is_inside_the_reward_bounds(T, N, E):
    pred, tgt, w, rew0 = rr.reward_case(T, N, E)
    assert w[1] == 0 and len(set(w.tolist())) == T and (rew0 != 0).all()
    rew, bonus, partial, stats = rr.reward_f32(pred, tgt, w, rew0, N)
    assert partial.shape == (2 * rr.num_partials(T * N),)
    fr = rr.check_reward(rew, bonus, partial, stats, pred, tgt, w, rew0, N)
    assert max(fr.values()) <= 0.5  # the bounds are doubled counts
    # the rows of the zero weight: no bonus, rewards untouched
    assert (bonus[N:2 * N] == 0).all() and np.array_equal(rew[N:2 * N], rew0[N:2 * N])


@pytest.mark.parametrize("what", ["rewards", "bonus", "partial", "stats"])
def test_a_few_ulps_outside_the_reward_bound_is_caught(what):
    T, N, E = 25, 8, 12
    pred, tgt, w, rew0 = rr.reward_case(T, N, E)
    ref = rr.reward_ref(pred, tgt, w, rew0, N)
    out = dict(zip(("rewards", "bonus", "partial", "stats"), rr.reward_f32(pred, tgt, w, rew0, N)))
    key = dict(rewards=("rewards", "b_rew"), bonus=("bonus", "b_bonus"), partial=("partial", "b_partial"),
               stats=("stats", "b_stats"))[what]
    i = out[what].shape[0] - 1  # (the last row's weight is not the zero one)
    want, bound = ref[key[0]][i], ref[key[1]][i]
    assert bound > 0
    # the bound is below (E + 8) U |value| per entry for the rows; the sums' are a few hundred U
    assert bound <= (400 if what in ("partial", "stats") else E + 10) * U * max(abs(want), abs(float(rew0[-1])))
    out[what] = out[what].copy()
    out[what][i] = np.float32(want + bound + 4 * np.spacing(np.float32(abs(want))))
    with pytest.raises(AssertionError):
        rr.check_reward(out["rewards"], out["bonus"], out["partial"], out["stats"], pred, tgt, w, rew0, N)


def test_reward_reference_is_the_definition():
    pred, tgt, w, rew0 = rr.reward_case(3, 8, 8)
    ref = rr.reward_ref(pred, tgt, w, rew0, 8)
    d = tgt.astype(np.float64) - pred.astype(np.float64)
    for m in (0, 9, 23):
        r = np.linalg.norm(d[m])
        assert abs(ref["r"][m] - r) <= 1e-15 * r
        assert abs(ref["rewards"][m] - (float(rew0[m]) + float(w[m // 8]) * r)) <= 1e-14
    assert abs(ref["stats"][1] - ref["r"].sum() * float(rr.inv_rows(24))) <= 1e-14


@pytest.mark.parametrize("M", rr.LOSS_ROWS)
@pytest.mark.parametrize("E", rr.WIDTHS)
def test_loss_case_and_fp32_evaluation(M, E):
    mu, tgt_all, idx = rr.loss_case(M, E)
    assert tgt_all.shape == (rr.LOSS_SOURCE_ROWS, E) and idx.shape == (M,)
    assert len(set(idx.tolist())) < M and (np.diff(idx) < 0).any()  # repeats, out of order
    assert idx.min() == 0 and idx.max() == rr.LOSS_SOURCE_ROWS - 1
    f = np.float32
    scale = rr.loss_scale(M, E)
    for Ap in rr.LOSS_PADS[E]:
        assert Ap % 8 == 0 and E <= Ap <= 32
        d = (mu - tgt_all[idx]).astype(f)
        g = ((f(2) * d).astype(f) * scale).astype(f)
        bits = np.zeros((M, Ap), np.uint16)
        u = g.view(np.uint32)
        bits[:, :E] = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
        term = (d * d).astype(f)
        partial = np.array([t.astype(np.float64).sum() for t in dr._groups(term)], f)
        stats = np.zeros(4, f)
        stats[0] = f(partial.astype(np.float64).sum()) * scale
        fr = rr.check_loss_step(bits, g, partial, stats, mu, tgt_all, idx, scale)
        assert max(fr.values()) <= 1.0
        bad = g.copy()
        bad[-1, -1] = f(bad[-1, -1] * (1 + 16 * U)) if bad[-1, -1] != 0 else f(1e-6)
        with pytest.raises(AssertionError):
            rr.check_loss_step(bits, bad, partial, stats, mu, tgt_all, idx, scale)
        # the target really goes through the index: the identity index fails on a gathered case
        with pytest.raises(AssertionError):
            rr.check_loss_step(bits, g, partial, stats, mu, tgt_all, np.arange(M) % rr.LOSS_SOURCE_ROWS, scale)
