"""The recurrent kernels (csrc/lstm_seq.hip, gru_seq.hip, heads.hip) against the fp64 references
of tests/seq_ref.py, one step at a time from the kernels' own saved operands, at every arm of
the host's selection ("The recurrent anchor").  Every output is allocated NaN-filled
inside sentinel guard bands: a store outside a tensor, a row never written, a write past B or
past I fails the test.  The bounds are derived in seq_ref.py's docstring; each test prints the
worst measured fraction of each bound."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seq_ref as R  # noqa: E402
from rsl_rl.modules import gru_seq, lstm_seq  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

H = R.MH
SENT, GUARD = 1234.5, 64
P = mm._p
no_tile_override = pytest.mark.skipif("PMLP_LSTM_STEP_TILES" in os.environ,
                                      reason="the tile count under test is overridden")


class Out:
    """An fp32 output of the given shape, NaN-filled, between two bands of the sentinel; `init`
    (an array) fills it instead: a buffer the kernel reads and overwrites in place."""

    def __init__(self, *shape, init=None):
        n = int(np.prod(shape))
        self.flat = torch.full((n + 2 * GUARD,), SENT, device="cuda")
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).view(*shape))

    def get(self):
        g = torch.cat([self.flat[:GUARD], self.flat[-GUARD:]])
        assert bool((g == SENT).all()), "a store outside the tensor (guard band overwritten)"
        return self.t.cpu().numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ins(c, keys):
    return {k: dev(c.get(k)) for k in keys}


def got(outs):
    torch.cuda.synchronize()
    return {k: (o.get() if isinstance(o, Out) else o) for k, o in outs.items() if o is not None}


W = ("x", "w_ih", "b_ih", "b_hh", "w_hh", "h0", "c0")


# ------------------------------------------------------------------- launchers --
def lstm_fwd(cases):
    """pmlp_lstm_fwd_mfma_jobs on 1..2 cases over the same [T, B] and reset."""
    T, B = cases[0]["T"], cases[0]["B"]
    reset = dev(cases[0]["reset"])
    jobs, keep, outs = (lstm_seq.LstmJob * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, W)
        o = dict(h_out=Out(T, B, H), c_out=Out(T, B, H), gact=Out(T, B, 4 * H), xh=Out(T, B, c["I"] + H + 1))
        jobs[n] = lstm_seq.LstmJob(c["I"], *(P(i[k]) for k in W), P(o["h_out"].t), P(o["c_out"].t), P(o["gact"].t),
                                   P(o["xh"].t))
        keep.append(i)
        outs.append(o)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_fwd_mfma_jobs(len(cases), jobs, T, B, H, P(reset), mm._stream()), "fwd")
    return [got(o) for o in outs]


def lstm_step(cases, save):
    """pmlp_lstm_step_mfma_jobs in place; returns the outputs in the forward's shapes."""
    B = cases[0]["B"]
    jobs, keep, outs = (lstm_seq.LstmJob * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, W[:5])
        o = dict(h_out=Out(1, B, H, init=c["h0"]), c_out=Out(1, B, H, init=c["c0"]),
                 h_save=Out(B, H) if save else None, c_save=Out(B, H) if save else None)
        jobs[n] = lstm_seq.LstmJob(c["I"], *(P(i[k]) for k in W[:5]), None, None, P(o["h_out"].t), P(o["c_out"].t),
                                   None, None, None, None, P(o["h_save"].t) if save else None,
                                   P(o["c_save"].t) if save else None)
        keep.append(i)
        outs.append(o)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_step_mfma_jobs(len(cases), jobs, B, H, mm._stream()), "step")
    return [got(o) for o in outs]


def lstm_bwd(c, fwd):
    """pmlp_lstm_bwd_mfma: dgx."""
    T, B = c["T"], c["B"]
    i = ins(c, ("w_hh", "c0", "reset", "dh_out"))
    f = {k: dev(fwd[k]) for k in ("c_out", "gact")}
    o = Out(T, B, 4 * H)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_bwd_mfma(T, B, H, P(i["w_hh"]), P(i["c0"]), P(i["reset"]), P(f["c_out"]),
                                                    P(f["gact"]), P(i["dh_out"]), P(o.t), mm._stream()), "bwd_mfma")
    return got(dict(dgx=o))["dgx"]


def lstm_bwd_dw(pairs):
    """pmlp_lstm_bwd_dw_mfma_jobs on 1..2 (case, forward arrays) over the same [T, B] and reset:
    the slabs [nblk, 256 (I + 65)]."""
    c0 = pairs[0][0]
    T, B = c0["T"], c0["B"]
    reset = dev(c0["reset"])
    L = lstm_seq._lib()
    nblk = L.pmlp_lstm_bwd_dw_blocks(B)
    assert nblk == (B + R.ME - 1) // R.ME
    jobs, keep, outs = (lstm_seq.LstmJob * len(pairs))(), [], []
    for n, (c, fwd) in enumerate(pairs):
        i = ins(c, ("w_hh", "c0", "dh_out"))
        f = {k: dev(fwd[k]) for k in ("c_out", "gact", "xh")}
        o = Out(nblk, 4 * H * (c["I"] + H + 1))
        jobs[n] = lstm_seq.LstmJob(c["I"], None, None, None, None, P(i["w_hh"]), None, P(i["c0"]), None, P(f["c_out"]),
                                   P(f["gact"]), P(f["xh"]), P(i["dh_out"]), P(o.t))
        keep += [i, f]
        outs.append(o)
    lstm_seq._ok(L.pmlp_lstm_bwd_dw_mfma_jobs(len(pairs), jobs, T, B, H, P(reset), mm._stream()), "bwd_dw")
    return [got(dict(s=o))["s"] for o in outs]


WJ = lstm_seq.LstmWideJob


def wide_fwd(cases):
    T, B = cases[0]["T"], cases[0]["B"]
    reset = dev(cases[0]["reset"])
    jobs, keep, outs = (WJ * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, W)
        o = dict(h_out=Out(T, B, H), c_out=Out(T, B, H), gact=Out(T, B, 4 * H), gx=Out(T, B, 4 * H), hp=Out(T, B, H + 1))
        jobs[n] = WJ(c["I"], *(P(i[k]) for k in W), *(P(o[k].t) for k in ("h_out", "c_out", "gact", "gx", "hp")))
        keep.append(i)
        outs.append(o)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_fwd_wide_jobs(len(cases), jobs, T, B, H, P(reset), mm._stream()), "fwd_wide")
    return [got(o) for o in outs]


def wide_bwd(pairs):
    c0 = pairs[0][0]
    T, B = c0["T"], c0["B"]
    reset = dev(c0["reset"])
    L = lstm_seq._lib()
    nblk, nch = L.pmlp_lstm_bwd_dw_blocks(B), L.pmlp_lstm_wide_dw_blocks(T, B)
    assert nch == (T * B + R.WDR - 1) // R.WDR
    jobs, keep, outs = (WJ * len(pairs))(), [], []
    for n, (c, fwd) in enumerate(pairs):
        i = ins(c, ("x", "w_hh", "c0", "dh_out"))
        f = {k: dev(fwd[k]) for k in ("c_out", "gact", "hp")}
        o = dict(dgx=Out(T, B, 4 * H), slab=Out(nblk, 4 * H * (H + 1)), slab_ih=Out(nch, 4 * H * c["I"]))
        jobs[n] = WJ(c["I"], P(i["x"]), None, None, None, P(i["w_hh"]), None, P(i["c0"]), None, P(f["c_out"]),
                     P(f["gact"]), None, P(f["hp"]), P(i["dh_out"]), P(o["dgx"].t), P(o["slab"].t), P(o["slab_ih"].t))
        keep += [i, f]
        outs.append(o)
    lstm_seq._ok(L.pmlp_lstm_bwd_wide_jobs(len(pairs), jobs, T, B, H, P(reset), mm._stream()), "bwd_wide")
    return [got(o) for o in outs]


def wide_step(cases, save):
    B = cases[0]["B"]
    jobs, keep, outs = (WJ * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, W[:5])
        o = dict(h_out=Out(1, B, H, init=c["h0"]), c_out=Out(1, B, H, init=c["c0"]), gx=Out(1, B, 4 * H),
                 h_save=Out(B, H) if save else None, c_save=Out(B, H) if save else None)
        jobs[n] = WJ(c["I"], *(P(i[k]) for k in W[:5]), None, None, P(o["h_out"].t), P(o["c_out"].t), None, P(o["gx"].t),
                     None, None, None, None, None, P(o["h_save"].t) if save else None, P(o["c_save"].t) if save else None)
        keep.append(i)
        outs.append(o)
    lstm_seq._ok(lstm_seq._lib().pmlp_lstm_step_wide_jobs(len(cases), jobs, B, H, mm._stream()), "step_wide")
    return [got(o) for o in outs]


GJ = gru_seq.GruJob
GW = ("x", "w_ih", "b_ih", "b_hh", "w_hh", "h0")


def gru_fwd(cases, gact=True, xh=True, save=True):
    T, B = cases[0]["T"], cases[0]["B"]
    reset = dev(cases[0]["reset"])
    jobs, keep, outs = (GJ * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, GW)
        o = dict(h_out=Out(T, B, H), gact=Out(T, B, 4 * H) if gact else None,
                 xh=Out(T, B, c["I"] + H + 1) if xh else None, h_save=Out(B, H) if save else None)
        q = lambda k: P(o[k].t) if o[k] is not None else None  # noqa: E731
        jobs[n] = GJ(c["I"], *(P(i[k]) for k in GW), q("h_out"), q("gact"), q("xh"), None, None, q("h_save"))
        keep.append(i)
        outs.append(o)
    gru_seq._ok(gru_seq._lib().pmlp_gru_fwd_jobs(len(cases), jobs, T, B, H, P(reset), mm._stream()), "gru_fwd")
    return [got(o) for o in outs]


def gru_bwd(pairs):
    c0 = pairs[0][0]
    T, B = c0["T"], c0["B"]
    reset = dev(c0["reset"])
    jobs, keep, outs = (GJ * len(pairs))(), [], []
    for n, (c, fwd) in enumerate(pairs):
        i = ins(c, ("w_hh", "dh_out"))
        f = {k: dev(fwd[k]) for k in ("gact", "xh")}
        o = Out(T, B, 4 * H)
        jobs[n] = GJ(c["I"], None, None, None, None, P(i["w_hh"]), None, None, P(f["gact"]), P(f["xh"]), P(i["dh_out"]),
                     P(o.t), None)
        keep += [i, f]
        outs.append(o)
    gru_seq._ok(gru_seq._lib().pmlp_gru_bwd_jobs(len(pairs), jobs, T, B, H, P(reset), mm._stream()), "gru_bwd")
    return [got(dict(d=o))["d"] for o in outs]


def gru_step(cases, save):
    B = cases[0]["B"]
    jobs, keep, outs = (GJ * len(cases))(), [], []
    for n, c in enumerate(cases):
        i = ins(c, GW[:5])
        o = dict(h_out=Out(1, B, H, init=c["h0"]), h_save=Out(B, H) if save else None)
        jobs[n] = GJ(c["I"], *(P(i[k]) for k in GW[:5]), None, P(o["h_out"].t), None, None, None, None,
                     P(o["h_save"].t) if save else None)
        keep.append(i)
        outs.append(o)
    gru_seq._ok(gru_seq._lib().pmlp_gru_step_jobs(len(cases), jobs, B, H, mm._stream()), "gru_step")
    return [got(o) for o in outs]


# --------------------------------------------------- matrix-core LSTM, narrow inputs --
@pytest.mark.parametrize("I", R.MF_I)
def test_lstm_forward_step_by_step(I):
    """pmlp_lstm_fwd_mfma_jobs over T = 1, 2, 3, 4, 7 (the two-step prefetch past the end, both
    LDS buffers) x B = 1, 15, 16, 17, 37 (tail envs, three workgroups), h0 / c0 / reset each
    present and NULL, every reset pattern."""
    st = R.Stats()
    for c in R.sweep(I, R.MF_T, R.MF_B, I):
        out, = lstm_fwd([c])
        R.lstm_fwd_check(c, out, "x", st, f"T={c['T']} B={c['B']} I={I}")
    print(st.line(f"lstm fwd I={I}"))


@pytest.mark.parametrize("pattern", R.RESET_PATTERNS)
def test_lstm_reset_patterns_forward_and_backward(pattern):
    """Every reset pattern at T = 7, B = 21 (a tail env in the second workgroup) through the
    forward, the gate-gradient backward and, at T = 4 on test-built arrays, the slab backward."""
    st = R.Stats()
    c, (n, fw), _ = R.pattern_cases(pattern)
    out, = lstm_fwd([c])
    R.lstm_fwd_check(c, out, "x", st, pattern)
    R.lstm_bwd_check(c, out, lstm_bwd(c, out), stats=st, what=pattern)
    R.narrow_slab_condition(n, fw)
    R.narrow_slab_check(n, fw, lstm_bwd_dw([(n, fw)])[0], st, pattern)
    print(st.line(f"lstm reset pattern {pattern}"))


def test_lstm_two_jobs_of_different_width_in_one_launch():
    """Two memories in one launch, forward (I = 3, 64) and slab backward (I = 1, 63): each job's
    outputs satisfy its own checks (one job's tiles are not confused with the other's)."""
    st = R.Stats()
    a, b = R.lstm_pair_cases()
    for c, out in zip((a, b), lstm_fwd([a, b])):
        R.lstm_fwd_check(c, out, "x", st, f"I={c['I']}")
    (n1, f1), (n2, f2) = R.narrow_pair_cases()
    R.narrow_slab_condition(n1, f1), R.narrow_slab_condition(n2, f2)
    for (c, fw), slab in zip(((n1, f1), (n2, f2)), lstm_bwd_dw([(n1, f1), (n2, f2)])):
        R.narrow_slab_check(c, fw, slab, st, f"I={c['I']}")
    print(st.line("lstm two jobs"))


@no_tile_override
@pytest.mark.parametrize("B", [37, 4117])
@pytest.mark.parametrize("save", [True, False])
def test_lstm_step_in_place(B, save):
    """pmlp_lstm_step_mfma_jobs: B = 37 is one tile, 4117 two tiles per workgroup with the last
    workgroup's second tile partly empty; two jobs (I = 47, 4); h_save / c_save present and
    absent.  No gates are saved: their bounds are multiplied through to c and h."""
    st = R.Stats()
    cs = R.step_cases(B)
    for c, out in zip(cs, lstm_step(cs, save)):
        assert ("h_save" in out) == save
        R.lstm_fwd_check(c, out, "x", st, f"step B={B} I={c['I']}")
    print(st.line(f"lstm step B={B}"))


@pytest.mark.parametrize("T", R.BWD_T)
def test_lstm_backward_gate_gradients_step_by_step(T):
    """pmlp_lstm_bwd_mfma at B = 1, 16, 17, 37, c0 NULL and given, fed the forward's outputs."""
    st = R.Stats()
    for c in R.bwd_cases(T):
        out, = lstm_fwd([c])
        R.lstm_bwd_check(c, out, lstm_bwd(c, out), stats=st, what=f"T={T} B={c['B']} c0={c['c0'] is not None}")
    print(st.line(f"lstm bwd T={T}"))


@pytest.mark.parametrize("I", R.DW_I)
def test_lstm_backward_slabs_row_by_row(I):
    """pmlp_lstm_bwd_dw_mfma_jobs: I = 1, 31 (three column tiles), 32 (four), 63 (the full 128
    columns) x B = 1, 15, 17, 37 x T = 1..4 on test-built arrays; every slab row against the
    free-running fp64 backward.  The condition of the check is asserted per case."""
    st = R.Stats()
    for c, fw in R.narrow_cases(I):
        R.narrow_slab_condition(c, fw)
        R.narrow_slab_check(c, fw, lstm_bwd_dw([(c, fw)])[0], st, f"T={c['T']} B={c['B']} I={I}")
    print(st.line(f"lstm bwd_dw I={I}"))


# ----------------------------------------------------------- exact grids, T = 1 --
@pytest.mark.parametrize("I", R.MF_I)
def test_lstm_and_gru_on_the_exact_grid(I):
    """Exact pre-activations: the gates within the activation budget alone (an index or staging
    error moves them by whole products), gh_n of the GRU exactly."""
    st, es, et = R.Stats(), 0.0, 0.0
    for B in R.MF_B:
        c = R.grid_case(I * 10 + B, B, I, reset0=(B == 37))
        lo, = lstm_fwd([c])
        R.grid_lstm_check(c, lo, st, f"lstm grid B={B} I={I}")
        a, b = R.grid_act_errors(c, lo)
        es, et = max(es, a), max(et, b)
        g = R.grid_case(I * 10 + B, B, I, gates=3, reset0=(B == 37))
        out, = gru_fwd([g])
        R.grid_gru_check(g, out, st, f"gru grid B={B} I={I}")
        hp = R.h_prev_expected(g, out["h_out"])
        ghn = R.d(hp[0]) @ R.d(g["w_hh"][2 * H:]).T + R.d(g["b_hh"][2 * H:])
        R.equal("ghn", out["gact"][0][:, 3 * H:], ghn.astype(np.float32), f"gru grid gh_n B={B} I={I}")
    print(st.line(f"exact grid I={I} (activation budget alone)") + f"; max |fsig error| {es:.2f} u, |ftanh error| {et:.2f} u")


@pytest.mark.parametrize("I", [1, 47, 64])
def test_all_ones_mantissas_split_exactly(I):
    """Operands whose round-to-nearest split is exact and whose truncating split is 1.5 times
    outside the bound (seq_ref.ones_case)."""
    st = R.Stats()
    c = R.ones_case(I, 17, I)
    R.lstm_fwd_check(c, lstm_fwd([c])[0], "x", st, f"ones I={I}")
    g = R.ones_case(I, 17, I, gates=3)
    R.gru_fwd_check(g, gru_fwd([g])[0], st, f"gru ones I={I}")
    print(st.line(f"all-ones mantissas I={I}"))


# ------------------------------------------------------------------ wide inputs --
@pytest.mark.parametrize("n", range(len(R.WIDE)))
def test_wide_lstm_forward_backward_and_slabs(n):
    """pmlp_lstm_fwd_wide_jobs / _bwd_wide_jobs: T B = 1, 511, 512, 513 rows (k_lstm_dwih_wide's
    512-row chunks), one, two and three 128-column groups, x rows aligned to 4 (65, 237), 8
    (234) and 16 bytes (384); every reset pattern once over the cases (reset == NULL at T = 7,
    every env at one step at T = 3), h0 and c0 each present and NULL; dgx step by step, both slabs
    row by row from the kernel's dgx."""
    st = R.Stats()
    c = list(R.wide_cases())[n]
    I, T, B = R.WIDE[n]
    out, = wide_fwd([c])
    R.check_wide_gx(c, out["gx"], f"I={I}", st)
    R.lstm_fwd_check(c, out, "gx", st, f"wide I={I} T={T} B={B}")
    b, = wide_bwd([(c, out)])
    R.lstm_bwd_check(c, out, b["dgx"], stats=st, what=f"wide I={I}")
    R.wide_slab_check(c, out["hp"], b["dgx"], b["slab"], b["slab_ih"], st, f"wide I={I} T={T} B={B}")
    print(st.line(f"wide I={I} T={T} B={B} reset {R.WIDE_RESETS[n]}"))


@pytest.mark.parametrize("pair", ["all", "null"])
def test_wide_two_jobs_of_different_width(pair):
    """Two wide jobs (I = 65, 300) in one launch: every env reset at one step, and reset == NULL;
    h0 / c0 NULL in one job each."""
    st = R.Stats()
    a, b = R.wide_pair_cases() if pair == "all" else R.wide_pair_null_cases()
    outs = wide_fwd([a, b])
    for c, out, bw in zip((a, b), outs, wide_bwd(list(zip((a, b), outs)))):
        R.check_wide_gx(c, out["gx"], f"wide pair I={c['I']}", st)
        R.lstm_fwd_check(c, out, "gx", st, f"wide pair I={c['I']}")
        R.lstm_bwd_check(c, out, bw["dgx"], stats=st)
        R.wide_slab_check(c, out["hp"], bw["dgx"], bw["slab"], bw["slab_ih"], st, f"wide pair I={c['I']}")
    print(st.line(f"wide two jobs, reset {pair}"))


@no_tile_override
@pytest.mark.parametrize("B", [37, 4117])
@pytest.mark.parametrize("save", [True, False])
def test_wide_step_in_place(B, save):
    st = R.Stats()
    c = R.wide_step_case(B)
    out, = wide_step([c], save)
    R.check_wide_gx(c, out["gx"], "step", st)
    R.lstm_fwd_check(c, out, "gx", st, f"wide step B={B}")
    print(st.line(f"wide step B={B}"))


# ---------------------------------------------------------------------------- GRU --
@pytest.mark.parametrize("I", R.GRU_I)
def test_gru_forward_and_backward_step_by_step(I):
    """pmlp_gru_fwd_jobs / _bwd_jobs over the LSTM's T x B sweep; the n_x / n_h column split
    through gh_n and n separately."""
    st = R.Stats()
    for c in R.sweep(300 + I, R.MF_T, R.MF_B, I, gates=3):
        out, = gru_fwd([c])
        R.gru_fwd_check(c, out, st, f"gru T={c['T']} B={c['B']} I={I}")
        R.gru_bwd_check(c, out, gru_bwd([(c, out)])[0], st, f"gru T={c['T']} B={c['B']} I={I}")
    print(st.line(f"gru I={I}"))


@pytest.mark.parametrize("pattern", R.RESET_PATTERNS)
def test_gru_reset_patterns_and_optional_outputs(pattern):
    """Every reset pattern; two jobs (I = 3, 64) in one launch; with gact / xh / h_save absent
    h_out holds the same bits."""
    st = R.Stats()
    a, b = R.pattern_cases(pattern)[2]
    outs = gru_fwd([a, b])
    bare = gru_fwd([a, b], gact=False, xh=False, save=False)
    for c, out, dg, o2 in zip((a, b), outs, gru_bwd(list(zip((a, b), outs))), bare):
        R.gru_fwd_check(c, out, st, f"gru {pattern} I={c['I']}")
        R.gru_bwd_check(c, out, dg, st, f"gru {pattern} I={c['I']}")
        assert set(o2) == {"h_out"}
        R.equal("out", o2["h_out"], out["h_out"], "h_out without the optional outputs")
    print(st.line(f"gru reset pattern {pattern}"))


@no_tile_override
@pytest.mark.parametrize("B", [37, 4117])
@pytest.mark.parametrize("save", [True, False])
def test_gru_step_in_place(B, save):
    st = R.Stats()
    cs = R.step_cases(B, gates=3)
    for c, out in zip(cs, gru_step(cs, save)):
        R.gru_fwd_check(c, out, st, f"gru step B={B} I={c['I']}")
    print(st.line(f"gru step B={B}"))


# ------------------------------------------------------------- fp32 VALU kernels --
def valu_run(c, form, xh=True):
    T, B, Hh, I = c["T"], c["B"], c["H"], c["I"]
    L = lstm_seq._lib()
    i = ins(c, W + ("gx", "reset", "dh_out"))
    o = dict(h_out=Out(T, B, Hh), c_out=Out(T, B, Hh), gact=Out(T, B, 4 * Hh), h_last=Out(B, Hh), c_last=Out(B, Hh))
    q = lambda k: P(o[k].t)  # noqa: E731
    if form == "valu_gx":
        lstm_seq._ok(L.pmlp_lstm_fwd(T, B, Hh, P(i["gx"]), P(i["w_hh"]), P(i["h0"]), P(i["c0"]), P(i["reset"]), q("h_out"),
                                     q("c_out"), q("gact"), q("h_last"), q("c_last"), mm._stream()), "lstm_fwd")
    else:
        if xh:
            o["xh"] = Out(T, B, I + Hh + 1)
        lstm_seq._ok(L.pmlp_lstm_fwd_x(T, B, Hh, I, P(i["x"]), P(i["w_ih"]), P(i["b_ih"]), P(i["b_hh"]), P(i["w_hh"]),
                                       P(i["h0"]), P(i["c0"]), P(i["reset"]), q("h_out"), q("c_out"), q("gact"),
                                       q("h_last"), q("c_last"), q("xh") if xh else None, mm._stream()), "lstm_fwd_x")
    out = got(o)
    d = Out(T, B, 4 * Hh)
    f = {k: dev(out[k]) for k in ("c_out", "gact")}
    lstm_seq._ok(L.pmlp_lstm_bwd(T, B, Hh, P(i["w_hh"]), P(i["c0"]), P(i["reset"]), P(f["c_out"]), P(f["gact"]),
                                 P(i["dh_out"]), P(d.t), mm._stream()), "lstm_bwd")
    out["dgx"] = got(dict(d=d))["d"]
    return out


def valu_check(c, out, form, st, what):
    R.equal("last", out.pop("h_last"), out["h_out"][-1], f"{what}: h_last")
    R.equal("last", out.pop("c_last"), out["c_out"][-1], f"{what}: c_last")
    R.lstm_fwd_check(c, out, form, st, what)
    R.lstm_bwd_check(c, out, out["dgx"], "valu", st, what)


@pytest.mark.parametrize("Hh", R.VALU_H)
def test_valu_lstm_forward_and_backward_step_by_step(Hh):
    """pmlp_lstm_fwd (gx-fed), pmlp_lstm_fwd_x at I = 1, 32, 33, 48, 49, 64 (the IP arms 32 / 48 /
    64 at both ends) and pmlp_lstm_bwd at B = 1, 4, 5, T = 3; xh present and absent; the reset
    patterns rotate so that over the three hidden sizes every form meets every one."""
    st = R.Stats()
    for c, form, xh in R.valu_cases(Hh):
        out = valu_run(c, form, xh=xh)
        assert ("xh" in out) == (form == "valu_x" and xh)
        valu_check(c, out, form, st, f"valu H={Hh} {form} I={c['I']} B={c['B']}")
    print(st.line(f"lstm VALU H={Hh}"))


@pytest.mark.parametrize("B", [4088, 4089])
def test_valu_lstm_at_the_env_block_switch(B):
    """T = 2 at B = 4088 (4 envs per workgroup) and 4089 (8): H = 64, I = 33 and gx-fed, with
    every env reset at one step, one env on both steps, and reset == NULL."""
    st = R.Stats()
    for c, form in R.valu_switch_cases(B):
        valu_check(c, valu_run(c, form), form, st, f"valu B={B} {form}")
    print(st.line(f"lstm VALU B={B}"))


@pytest.mark.parametrize("Hh", R.VALU_H)
def test_valu_lstm_step_in_place(Hh):
    """pmlp_lstm_step: one step in place from gx, h_save / c_save present and absent."""
    st = R.Stats()
    for save in (True, False):
        c, form = R.valu_step_case(Hh)
        i = ins(c, ("gx", "w_hh"))
        o = dict(h_out=Out(1, 37, Hh, init=c["h0"]), c_out=Out(1, 37, Hh, init=c["c0"]),
                 h_save=Out(37, Hh) if save else None, c_save=Out(37, Hh) if save else None)
        lstm_seq._ok(lstm_seq._lib().pmlp_lstm_step(37, Hh, P(i["gx"]), P(i["w_hh"]), P(o["h_out"].t), P(o["c_out"].t),
                                                    P(o["h_save"].t) if save else None,
                                                    P(o["c_save"].t) if save else None, mm._stream()), "lstm_step")
        R.lstm_fwd_check(c, got(o), form, st, f"valu step H={Hh}")
    print(st.line(f"lstm VALU step H={Hh}"))


# -------------------------------------------------------------------------- heads --
@pytest.mark.parametrize("M", R.HEADS_M)
def test_heads_on_the_exact_grid(M):
    """pmlp_heads_forward / _backward, two jobs of different N0 / N1 per launch at H = 32, 64,
    128: y0 on the positive branch, out on the rows whose y0 is positive, dh and every slab row
    [dW0 | db0 | dW1 | db1] are EQUAL to the fp64 values, block by block (padding rows past M
    contribute exactly nothing); the ELU's negative branch within its derived bound.  M = 16383
    is the VALU forward, 16421 the matrix-core forward."""
    st = R.Stats()
    L = mm.load()
    nblk = L.pmlp_heads_blocks(M)
    assert nblk == (M + R.HEAD_ROWS - 1) // R.HEAD_ROWS
    for Hh, cs in R.heads_cases(M):
        jobs, keep, outs = (mm.HeadJob * 2)(), [], []
        for k, c in enumerate(cs):
            i = ins(c, ("h", "W0", "b0", "W1", "b1", "dout", "y0b"))
            o = dict(y0=Out(M, c["N0"]), out=Out(M, c["N1"]), dh=Out(M, Hh),
                     slab=Out(nblk, c["N0"] * Hh + c["N0"] + c["N1"] * c["N0"] + c["N1"]))
            jobs[k] = mm.HeadJob(P(i["h"]), P(i["W0"]), P(i["b0"]), P(i["W1"]), P(i["b1"]), P(o["y0"].t), P(o["out"].t),
                                 P(i["dout"]), P(o["dh"].t), P(o["slab"].t), c["N0"], c["N1"])
            keep.append(i)
            outs.append(o)
        lstm_seq._ok(L.pmlp_heads_forward(2, jobs, M, Hh, mm._stream()), "heads_forward")
        fw = [got(dict(y0=o["y0"], out=o["out"])) for o in outs]
        for k in range(2):  # the backward reads the test-built y0
            jobs[k].y0 = P(keep[k]["y0b"])
        lstm_seq._ok(L.pmlp_heads_backward(2, jobs, M, Hh, mm._stream()), "heads_backward")
        for c, f, o in zip(cs, fw, outs):
            b = got(dict(dh=o["dh"], slab=o["slab"]))
            what = f"heads M={M} H={Hh} N0={c['N0']} N1={c['N1']}"
            R.heads_fwd_check(c, f["y0"], f["out"], st, what)
            R.heads_bwd_check(c, b["dh"], b["slab"], what)
    print(st.line(f"heads M={M}"))
