"""The two kernels of csrc/distill.hip against their references, with the bounds derived in
tests/distill_ref.py and tests/act_ref.py (never fitted to what a kernel returns).
tests/test_distill_ref_host.py applies the same comparison functions to deliberately wrong outputs
and asserts the input conditions of every loss case below.

Every output sits in a sentinel-prefilled buffer with a band before and after it; nothing outside
the stated extent may change.  Tests print their worst error as a fraction of its bound (pytest -s
shows them; DESIGN.md section 4 records them).

Arms reached:
  pmlp_distill_loss_step  M = 1, 37, 64, 65, 257 (one lane of one wave; a ragged wave; a whole
                          wave; a wave and a row; a workgroup and a row) x (A, Ap) = (12, 16),
                          (16, 16), (4, 8), (10, 16), (1, 8), (20, 24) x mse, huber x dmu_f given and
                          not; two launches bitwise; the refusals
  pmlp_distill_act        N = 1, 37, 64, 65 x A = 12, 16 (four lanes per row) and 10 (one lane per
                          row), O = 5 (scalar copies) and 8 (float4 copies), both parities
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

import act_ref as AR  # noqa: E402
import distill_ref as DR  # noqa: E402
from gemm_ref import SENTINEL  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
P = mm._p


class Band:
    """n elements in a sentinel-prefilled allocation with 64 elements in front and behind (the
    view .v starts 16-byte aligned): what a kernel is given, and the check that nothing around it
    changed."""

    def __init__(self, n, dtype=F32):
        self.lo, self.n = 64, n
        fill = SENTINEL if dtype.is_floating_point else int(SENTINEL)
        self.flat = torch.full((64 + n + 64,), fill, dtype=dtype, device=DEV)
        self.v = self.flat[64:64 + n]
        self.sentinel = torch.tensor(fill, dtype=dtype, device=DEV)

    def untouched(self, what):
        m = torch.ones_like(self.flat, dtype=torch.bool)
        m[self.lo:self.lo + self.n] = False
        bad = m & (self.flat != self.sentinel)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the buffer were written"

    def all_sentinel(self):
        return bool((self.flat == self.sentinel).all())

    def none_sentinel(self):
        return not bool((self.v == self.sentinel).any())


def _show(what, fr):
    print(f"[distill-ref] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fr.items())))


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------- pmlp_distill_loss_step --
def _loss_launch(mu, target, loss_type, scale, Ap, with_f):
    M, A = mu.shape
    L = mm.load()
    assert L.pmlp_distill_loss_parts(M) == DR.num_partials(M)
    g = dict(partial=Band(DR.num_partials(M)), stats=Band(4), dmu_b=Band(M * Ap, BF), dmu_f=Band(M * A))
    mm.distill_loss_step(mu, target, loss_type, scale, g["partial"].v, g["stats"].v, g["dmu_b"].v.view(M, Ap),
                         g["dmu_f"].v.view(M, A) if with_f else None)
    torch.cuda.synchronize()
    for k, b in g.items():
        b.untouched(k)
    assert g["partial"].none_sentinel() and g["stats"].none_sentinel(), "partials / stats not all written"
    if not with_f:
        assert g["dmu_f"].all_sentinel(), "dmu_f written with NULL given"
    return dict(partial=g["partial"].v.cpu().numpy(), stats=g["stats"].v.cpu().numpy(),
                bits=_bits(g["dmu_b"].v.view(M, Ap)),
                dmu_f=g["dmu_f"].v.view(M, A).cpu().numpy() if with_f else None)


@pytest.mark.parametrize("loss_type", [DR.MSE, DR.HUBER])
@pytest.mark.parametrize("A,Ap", DR.WIDTHS)
def test_loss_step_matches_fp64(A, Ap, loss_type):
    worst = {}
    for M in DR.ROWS:
        mu_h, tg_h = DR.loss_case(M, A, loss_type)
        mu, tg = torch.from_numpy(mu_h).to(DEV), torch.from_numpy(tg_h).to(DEV)
        scale = DR.entry_scale(DR.ENVS, A)
        outs = []
        for with_f in (True, False, True):
            o = _loss_launch(mu, tg, loss_type, scale, Ap, with_f)
            fr = DR.check_grad(o["bits"], o["dmu_f"], mu_h, tg_h, loss_type, scale)
            fr.update(DR.check_loss(o["partial"], o["stats"], mu_h, tg_h, loss_type, scale))
            for k, v in fr.items():
                worst[k] = max(worst.get(k, 0.0), v)
            outs.append(o)
        # launches on the same inputs: the same bits (with and without dmu_f, and again)
        for o in outs[1:]:
            for k in ("partial", "stats", "bits"):
                AR.check_equal(o[k], outs[0][k], f"{k} of a second launch, M={M}")
        AR.check_equal(outs[2]["dmu_f"], outs[0]["dmu_f"], f"dmu_f of a second launch, M={M}")
        # the bf16 operand is the fp32 gradient rounded to nearest even
        want = _bits(torch.from_numpy(outs[0]["dmu_f"]).to(BF))
        AR.check_equal(outs[0]["bits"][:, :A], want, f"dmu_b vs round(dmu_f), M={M}")
    _show(f"loss_step A={A} Ap={Ap} {loss_type}", worst)


def test_loss_step_refusals():
    L = mm.load()
    M, A = 8, 12
    mu, tg = torch.zeros(M, A, device=DEV), torch.zeros(M, A, device=DEV)
    part, stats = torch.zeros(1, device=DEV), torch.zeros(4, device=DEV)
    g16 = Band(M * 16, BF)
    st = mm._stream()

    def call(A_=A, Ap=16, lt=0, dmu=None, mu_=mu):
        dmu = g16.v if dmu is None else dmu
        return L.pmlp_distill_loss_step(P(mu_), P(tg), M, A_, lt, 1.0, P(part), P(stats), P(dmu), None, Ap, st)
    assert call() == 0
    assert call(lt=2) == -1 and b"loss_type" in L.pmlp_last_error()
    assert call(A_=33, Ap=40) == -3
    assert call(Ap=12) == -4 and call(Ap=8) == -4 and call(Ap=40) == -4
    assert call(dmu=g16.v[1:]) == -5
    assert L.pmlp_distill_loss_step(None, P(tg), M, A, 0, 1.0, P(part), P(stats), P(g16.v), None, 16, st) == -1
    torch.cuda.synchronize()
    g16.untouched("dmu_b")


# ------------------------------------------------------------- pmlp_distill_act --
def _act_case(N, A, O, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    return dict(mu=rng.normal(0, 1, (N, A)).astype(f), mu_t=rng.normal(0, 1, (N, A)).astype(f),
                std=rng.uniform(0.05, 1.5, A).astype(f), obs=rng.normal(0, 1, (N, O)).astype(f))


@pytest.mark.parametrize("A", [12, 16, 10])
@pytest.mark.parametrize("N", [1, 37, 64, 65])
def test_act_matches_pmlp_act_and_fp64(N, A):
    L = mm.load()
    worst = 0.0
    seed = 0xC0FFEE1234567 + N
    for O, parity, draw0 in ((5, 0, 7), (8, 1, (1 << 32) + 3)):
        c = {k: torch.from_numpy(v).to(DEV) for k, v in _act_case(N, A, O, 100 * N + A + O).items()}
        g = dict(actions=Band(N * A), st_obs=Band(N * O), st_teacher=Band(N * A), draw=Band(2, torch.int64))
        g["draw"].v[parity] = draw0
        g["draw"].v[parity ^ 1] = -5
        mm.distill_act(c["mu"], c["mu_t"], c["std"], c["obs"], g["draw"].v, parity, seed, g["actions"].v.view(N, A),
                       g["st_obs"].v.view(N, O), g["st_teacher"].v.view(N, A))
        torch.cuda.synchronize()
        for k, b in g.items():
            b.untouched(k)
        # the draw counter: this act read draw[parity], the next one reads draw[parity ^ 1]
        assert g["draw"].v.tolist() == ([draw0, draw0 + 1] if parity == 0 else [draw0 + 1, draw0])
        # the storage rows are bitwise copies
        AR.check_equal(g["st_obs"].v.view(N, O).cpu().numpy(), c["obs"].cpu().numpy(), "st_obs")
        AR.check_equal(g["st_teacher"].v.view(N, A).cpu().numpy(), c["mu_t"].cpu().numpy(), "st_teacher_actions")
        # bitwise pmlp_act's actions for the same (seed, draw, mu, std)
        draw = torch.tensor([draw0], dtype=torch.int64, device=DEV)
        z = lambda *s: torch.empty(*s, device=DEV)  # noqa: E731
        ref_act = z(N, A)
        mm._ok(L.pmlp_act(P(c["mu"]), P(c["std"]), P(z(N).zero_()), P(c["obs"]), None, N, A, O, 0, P(draw), seed,
                          P(ref_act), P(z(N, A)), P(z(N)), P(z(N, A)), P(z(N, A)), P(z(N)), P(z(N, O)), None,
                          mm._stream()), "pmlp_act")
        torch.cuda.synchronize()
        act = g["actions"].v.view(N, A).cpu().numpy()
        AR.check_equal(act, ref_act.cpu().numpy(), "actions vs pmlp_act")
        # and within act_ref's bound of mu + sigma z in fp64 (the draw word: the low 32 bits)
        zz, rad = AR.noise_parts(seed, draw0, N, A)
        m64, s64 = c["mu"].cpu().numpy().astype(np.float64), c["std"].cpu().numpy().astype(np.float64)
        worst = max(worst, AR.check_close(act, m64 + s64 * zz, AR.act_bound(m64, s64, zz, rad), "actions"))
    _show(f"act N={N} A={A}", dict(act=worst))


def test_act_alternates_the_draw_counter_and_draws_fresh_noise():
    """Four acts in a row as DistillRollout issues them: parity k % 2, draws 0, 1, 2, 3."""
    N, A, O = 64, 12, 8
    c = {k: torch.from_numpy(v).to(DEV) for k, v in _act_case(N, A, O, 5).items()}
    draw = torch.zeros(2, dtype=torch.int64, device=DEV)
    acts = []
    for k in range(4):
        out, so, stt = (torch.empty(N, A, device=DEV), torch.empty(N, O, device=DEV), torch.empty(N, A, device=DEV))
        mm.distill_act(c["mu"], c["mu_t"], c["std"], c["obs"], draw, k % 2, 11, out, so, stt)
        torch.cuda.synchronize()
        assert int(draw[(k + 1) % 2]) == k + 1 and int(draw[k % 2]) == k
        acts.append(out.cpu().numpy())
        z, rad = AR.noise_parts(11, k, N, A)
        m64, s64 = c["mu"].cpu().numpy().astype(np.float64), c["std"].cpu().numpy().astype(np.float64)
        AR.check_close(acts[-1], m64 + s64 * z, AR.act_bound(m64, s64, z, rad), f"actions of draw {k}")
    assert all(not np.array_equal(acts[i], acts[j]) for i in range(4) for j in range(i))


def test_act_refusals():
    L = mm.load()
    N, O = 8, 8
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    draw = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = mm._stream()

    def call(A=12, parity=0, mu=True):
        return L.pmlp_distill_act(P(z(N, A)) if mu else None, P(z(N, A)), P(z(A) + 1), P(z(N, O)), N, A, O, P(draw),
                                  parity, 1, P(z(N, A)), P(z(N, O)), P(z(N, A)), st)
    assert call() == 0
    assert call(A=17) == -3 and call(A=20) == -3
    assert call(parity=2) == -1 and call(mu=False) == -1
    torch.cuda.synchronize()
