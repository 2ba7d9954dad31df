"""The checks of tests/seq_ref.py are themselves tested (CPU): a float32 emulation of each
kernel form -- the matrix-core forms as the split with torch's round-to-nearest bf16, three
products, fp32 accumulation from the bias and activations rounded operation by operation; the
VALU forms in plain fp32 -- passes every comparison function that
tests/test_gpu_seq_reference.py applies to the kernels, on the GPU cases' own inputs, and
deliberately wrong emulations are rejected by the check meant for each.  The grid builders'
exactness assertions and the narrow slab's condition run here for every GPU case's inputs: both
files draw their cases from the generators of seq_ref.py (sweep, wide_cases, bwd_cases,
narrow_cases, pattern_cases, the pair, step, VALU and heads generators), so the inputs are the
same arrays."""
import numpy as np
import pytest
import torch

import seq_ref as R

f = np.float32
H = R.MH
LOG2E = f(1.4426950408889634)


# ------------------------------------------------------------------ emulations --
def bf(v, trunc=False):
    v = np.ascontiguousarray(v, dtype=f)
    if trunc:
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(f)
    return torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()


def split(v, trunc=False):
    hi = bf(v, trunc)
    return hi, bf(f(v) - hi, trunc)


def prod3(a, w, start, mut=""):
    """start + a w^T as hi.hi + hi.lo + lo.hi in fp32 (a [M, K], w [N, K], start [N] or [M, N])."""
    ah, al = split(a, mut == "trunc")
    wh, wl = split(w, mut == "trunc")
    acc = (np.zeros((a.shape[0], w.shape[0]), f) + f(start)).astype(f)
    acc = acc + ah @ wh.T
    if mut != "drop_cross":
        acc = acc + ah @ wl.T
        acc = acc + al @ wh.T
    return acc.astype(f)


def fsig(x):
    with np.errstate(over="ignore"):
        return (f(1) / (f(1) + np.exp2((-f(x)) * LOG2E, dtype=f))).astype(f)


def ftanh(x):
    with np.errstate(over="ignore"):
        return (f(2) * (f(1) / (f(1) + np.exp2((f(-2) * f(x)) * LOG2E, dtype=f))) - f(1)).astype(f)


def vsig(x):
    with np.errstate(over="ignore"):
        return (f(1) / (f(1) + np.exp(-f(x), dtype=f))).astype(f)


def vtanh(x):
    return np.tanh(f(x), dtype=f)


def lstm_emu(c, form="x", mut=""):
    """The LSTM forward in float32 as the kernels write it.  form as seq_ref.lstm_preact."""
    T, B, I, Hh = c["T"], c["B"], c["I"], c["H"]
    valu = form.startswith("valu")
    sg, th = (vsig, vtanh) if valu else (fsig, ftanh)
    z = lambda: np.zeros((B, Hh), f)  # noqa: E731
    h = z() if c["h0"] is None else c["h0"].copy()
    cc = z() if c["c0"] is None else c["c0"].copy()
    rs = c["reset"]
    out = dict(h_out=np.zeros((T, B, Hh), f), c_out=np.zeros((T, B, Hh), f), gact=np.zeros((T, B, 4 * Hh), f))
    if form in ("x", "valu_x"):
        out["xh"] = np.zeros((T, B, I + Hh + 1), f)
    if form == "gx":
        out["hp"] = np.zeros((T, B, Hh + 1), f)
        out["gx"] = np.stack([prod3(c["x"][t], c["w_ih"], c["b_ih"] + c["b_hh"], mut if mut == "trunc" else "")
                              for t in range(T)])
    bias = c["b_ih"] if mut == "bias_once" else (c["b_ih"] + c["b_hh"]).astype(f)
    for t in range(T):
        if rs is not None:
            tr = t - 1 if mut == "reset_late" else t
            if tr >= 0 and not (mut == "h0_despite_reset" and t == 0):
                m = rs[tr] != 0
                h[m] = 0
                if mut != "reset_h_only":
                    cc[m] = 0
        if t == 0:
            out["h_save"], out["c_save"] = h.copy(), cc.copy()
        x = c["x"][t].copy() if form != "valu_gx" else None
        if form in ("x", "valu_x"):
            out["xh"][t, :, :I], out["xh"][t, :, I:I + Hh] = x, h
            out["xh"][t, :, I + Hh] = 0 if mut == "no_ones" else 1
        if form == "gx":
            out["hp"][t, :, :Hh], out["hp"][t, :, Hh] = h, 1
        if mut == "clamped_x" and I > 1:
            x[:, I - 1] = x[:, I - 2]
        if form == "x":
            a = prod3(np.concatenate([x, h], 1), np.concatenate([c["w_ih"], c["w_hh"]], 1), bias, mut)
        elif form == "gx":
            a = prod3(h, c["w_hh"], out["gx"][t], mut)
        elif form == "valu_x":
            a = (bias + x @ c["w_ih"].T + h @ c["w_hh"].T).astype(f)
        else:
            a = (c["gx"][t] + h @ c["w_hh"].T).astype(f)
        q = [a[:, k * Hh:(k + 1) * Hh] for k in range(4)]
        if mut == "gate_order":
            q[1], q[2] = q[2], q[1]
        ig, fg, gg, og = sg(q[0]), sg(q[1]), th(q[2]), sg(q[3])
        cc = (fg * cc + ig * gg).astype(f)
        hn = (og * th(cc)).astype(f)
        out["gact"][t] = np.concatenate([ig, fg, gg, og], 1)
        out["c_out"][t], out["h_out"][t] = cc, hn
        if mut == "xh_holds_h_out" and "xh" in out:
            out["xh"][t, :, I:I + Hh] = hn
        h = hn.copy()
    return out


def lstm_bwd_emu(c, fwd, mut="", valu=False):
    """dgx [T, B, 4H] in float32 as k_lstm_bwd_mfma / k_lstm_bwd write it."""
    T, B, Hh = c["T"], c["B"], c["H"]
    th = vtanh if valu else ftanh
    rs = c["reset"]
    cp_all = R.c_prev_expected(c, fwd["c_out"])
    dg = np.zeros((T, B, 4 * Hh), f)
    dhn, dcn = np.zeros((B, Hh), f), np.zeros((B, Hh), f)
    for t in range(T - 1, -1, -1):
        ig, fg, gg, og = (fwd["gact"][t][:, k * Hh:(k + 1) * Hh] for k in range(4))
        dh = c["dh_out"][t] + dhn
        tc = th(fwd["c_out"][t])
        dc = (dcn + dh * og * (f(1) - tc * tc)).astype(f)
        if mut == "no_dc":
            dc = (dh * og * (f(1) - tc * tc)).astype(f)
        dg[t] = np.concatenate([dc * gg * ig * (f(1) - ig), dc * cp_all[t] * fg * (f(1) - fg),
                                dc * ig * (f(1) - gg * gg), dh * tc * og * (f(1) - og)], 1)
        keep = np.ones((B, 1), bool) if (rs is None or mut == "carry_across_reset") else (rs[t] == 0)[:, None]
        dcn = np.where(keep, dc * fg, 0).astype(f)
        mat = (dg[t] @ c["w_hh"]).astype(f) if valu else prod3(dg[t], c["w_hh"].T.copy(), 0.0, mut)
        dhn = np.where(keep, mat, 0).astype(f)
    return dg


def slab_emu(dg, rows, B, I, mut=""):
    """The per-workgroup slab rows of dG^T rows in float32 split products."""
    nblk = (B + R.ME - 1) // R.ME
    s = np.zeros((nblk, dg.shape[-1], rows.shape[-1]), f)
    for b in range(nblk):
        e1 = min(B, (b + 1) * R.ME)
        if mut == "skip_tail_env" and b == nblk - 1:
            e1 -= 1
        g = dg[:, b * R.ME:e1].reshape(-1, dg.shape[-1])
        r = rows[:, b * R.ME:e1].reshape(-1, rows.shape[-1])
        if mut == "stale_neighbour" and b == nblk - 1 and B % R.ME:
            g = np.concatenate([g, dg[:, B - 1]])
            r = np.concatenate([r, rows[:, B - 1]])
        s[b] = prod3(g.T.copy(), r.T.copy(), 0.0, mut) if g.size else 0
    if mut == "permuted":  # the kernel's gate-row order left in place: units 16w..16w+15 of gate q at 64w + 16q
        tr = np.array([((gp >> 4) & 3) * H + 16 * (gp >> 6) + (gp & 15) for gp in range(4 * H)])
        s = s[:, tr]
    return R.slab_layout(s, I).astype(f)


def gru_emu(c, mut=""):
    T, B, I = c["T"], c["B"], c["I"]
    h = np.zeros((B, H), f) if c["h0"] is None else c["h0"].copy()
    rs = c["reset"]
    out = dict(h_out=np.zeros((T, B, H), f), gact=np.zeros((T, B, 4 * H), f), xh=np.zeros((T, B, I + H + 1), f))
    wi, wh, bi, bh = c["w_ih"], c["w_hh"], c["b_ih"], c["b_hh"]
    for t in range(T):
        if rs is not None:
            tr = t - 1 if mut == "reset_late" else t
            if tr >= 0 and not (mut == "h0_despite_reset" and t == 0):
                h[rs[tr] != 0] = 0
        if t == 0:
            out["h_save"] = h.copy()
        x = c["x"][t]
        out["xh"][t, :, :I], out["xh"][t, :, I:I + H], out["xh"][t, :, I + H] = x, h, 1
        xhr = np.concatenate([x, h], 1)
        rz = prod3(xhr, np.concatenate([wi[:2 * H], wh[:2 * H]], 1), (bi[:2 * H] + bh[:2 * H]).astype(f), mut)
        r, z = fsig(rz[:, :H]), fsig(rz[:, H:])
        gin = prod3(x, wi[2 * H:], bi[2 * H:], mut)
        if mut == "bhn_outside":
            ghn = prod3(h, wh[2 * H:], 0.0, mut)
            n = ftanh((gin + r * ghn).astype(f) + bh[2 * H:])
        else:
            ghn = prod3(h, wh[2 * H:], bh[2 * H:], mut)
            n = ftanh((gin + r * ghn).astype(f))
        hn = ((f(1) - z) * n + z * h).astype(f)
        out["gact"][t] = np.concatenate([r, z, n, ghn], 1)
        out["h_out"][t] = hn
        h = hn.copy()
    return out


def gru_bwd_emu(c, fwd, mut=""):
    T, B, I = c["T"], c["B"], c["I"]
    rs = c["reset"]
    dg = np.zeros((T, B, 4 * H), f)
    dhn = np.zeros((B, H), f)
    cols = np.r_[0:2 * H, 3 * H:4 * H]
    for t in range(T - 1, -1, -1):
        r, z, n, ghn = (fwd["gact"][t][:, k * H:(k + 1) * H] for k in range(4))
        hp = fwd["xh"][t][:, I:I + H]
        dh = (c["dh_out"][t] + dhn).astype(f)
        dn = dh * (f(1) - z)
        dz = dh * (hp - n)
        da_n = dn * (f(1) - n * n)
        dg[t] = np.concatenate([da_n * ghn * r * (f(1) - r), dz * z * (f(1) - z), da_n, da_n * r], 1)
        keep = np.ones((B, 1), bool) if (rs is None or mut == "carry_across_reset") else (rs[t] == 0)[:, None]
        mat = prod3(dg[t][:, cols], c["w_hh"].T.copy(), 0.0, mut)
        dhn = np.where(keep, dh * z + mat, 0).astype(f)
    return dg


def heads_emu(c, mut=""):
    M = c["M"]
    z0 = (c["h"] @ c["W0"].T + c["b0"]).astype(f)
    y0 = np.where(z0 > 0, z0, np.expm1(np.minimum(z0, 0), dtype=f)).astype(f)
    out = (y0 @ c["W1"].T + c["b1"]).astype(f)
    y0b = c["y0b"]
    fac = np.where(y0b > 0, f(1), np.exp(y0b, dtype=f) if mut == "elu_from_input" else y0b + f(1)).astype(f)
    dz0 = ((c["dout"] @ c["W1"]) * fac).astype(f)
    dh = (dz0 @ c["W0"]).astype(f)
    rows = []
    for b in range(0, M, R.HEAD_ROWS):
        s = slice(b, min(M, b + R.HEAD_ROWS))
        dz, hh, do, yy = dz0[s], c["h"][s], c["dout"][s], y0b[s]
        if mut == "pad_row_counted" and s.stop == M and M % R.HEAD_ROWS:
            dz, hh = np.concatenate([dz, dz[-1:]]), np.concatenate([hh, hh[-1:]])
            do, yy = np.concatenate([do, do[-1:]]), np.concatenate([yy, yy[-1:]])
        rows.append(np.concatenate([(dz.T @ hh).reshape(-1), dz.sum(0), (do.T @ yy).reshape(-1), do.sum(0)]))
    return dict(y0=y0, out=out, dh=dh, slab=np.stack(rows).astype(f))


def rejected(check, fn):
    with pytest.raises(R.CheckFailed) as e:
        fn()
    names = (check,) if isinstance(check, str) else check
    assert e.value.check in names, (e.value.check, names, str(e.value)[:300])


# ---------------------------------------------------------------- the activations --
def test_activation_budgets_clear_the_correctly_rounded_floor():
    """A float32 emulation of fsig / ftanh with every operation correctly rounded stays within
    1.6u / 3.1u absolute on [-20, 20]; the budgets lie above that floor everywhere and the
    emulation inside them."""
    x = np.linspace(-20, 20, 400001).astype(f)
    x64 = x.astype(np.float64)
    es, et = np.abs(fsig(x) - R.sig(x64)), np.abs(ftanh(x) - np.tanh(x64))
    print(f"fsig emulation: max |err| {es.max() / R.U:.2f} u, worst fraction of the budget {(es / R.b_fsig(x64)).max():.3f}")
    print(f"ftanh emulation: max |err| {et.max() / R.U:.2f} u, worst fraction of the budget {(et / R.b_ftanh(x64)).max():.3f}")
    assert es.max() <= 1.6 * R.U and et.max() <= 3.1 * R.U
    assert (es <= R.b_fsig(x64)).all() and (et <= R.b_ftanh(x64)).all()
    assert R.b_fsig(0.0) == 4 * R.U and R.b_ftanh(0.0) == 8 * R.U
    assert R.b_fsig(x64).min() > 0 and (R.b_ftanh(x64) >= 2 * R.U * np.abs(np.tanh(x64))).all()
    ev, ew = np.abs(vsig(x) - R.sig(x64)), np.abs(vtanh(x) - np.tanh(x64))
    assert (ev <= R.b_vsig(x64)).all() and (ew <= R.b_vtanh(x64)).all()


# ------------------------------------------------------------------ LSTM forward --
@pytest.mark.parametrize("I", R.MF_I)
def test_matrix_core_lstm_emulation_passes_the_forward_checks(I):
    st = R.Stats()
    for c in R.sweep(I, R.MF_T, R.MF_B, I):
        R.lstm_fwd_check(c, lstm_emu(c), "x", st)
    print(st.line(f"lstm x-fed emulation I={I}"))


def wide_emu_check(c, st):
    """The wide emulation of one case through every wide check; returns what the slab mutants need."""
    T, B, I = c["T"], c["B"], c["I"]
    out = lstm_emu(c, "gx")
    R.check_wide_gx(c, out["gx"], "emu", st)
    R.lstm_fwd_check(c, out, "gx", st)
    dg = lstm_bwd_emu(c, out)
    R.lstm_bwd_check(c, out, dg, stats=st)
    slab = slab_emu(dg, out["hp"], B, 0)
    g, x = dg.reshape(T * B, -1), c["x"].reshape(T * B, I)
    nch = (T * B + R.WDR - 1) // R.WDR
    sih = np.stack([prod3(g[k * R.WDR:(k + 1) * R.WDR].T.copy(), x[k * R.WDR:(k + 1) * R.WDR].T.copy(), 0.0)
                    for k in range(nch)]).reshape(nch, -1)
    R.wide_slab_check(c, out["hp"], dg, slab, sih, st)
    return out, dg, sih


@pytest.mark.parametrize("n", range(len(R.WIDE)))
def test_wide_lstm_emulation_passes_the_checks(n):
    st = R.Stats()
    c = list(R.wide_cases())[n]
    B = c["B"]
    assert (c["reset"] is None) == (R.WIDE_RESETS[n] == "none")
    out, dg, sih = wide_emu_check(c, st)
    print(st.line(f"wide emulation I={c['I']} T={c['T']} B={B} reset {R.WIDE_RESETS[n]}"))
    if B > 1:
        for mut, chk in (("skip_tail_env", "slab"), ("permuted", "slab"), ("drop_cross", "slab")):
            rejected(chk, lambda: R.wide_slab_check(c, out["hp"], dg, slab_emu(dg, out["hp"], B, 0, mut), sih))
        if B % R.ME:
            rejected("slab", lambda: R.wide_slab_check(c, out["hp"], dg, slab_emu(dg, out["hp"], B, 0, "stale_neighbour"), sih))


def test_the_wide_cases_cover_every_reset_pattern_and_null_inputs():
    cs = list(R.wide_cases())
    assert sorted(R.WIDE_RESETS) == sorted(R.RESET_PATTERNS)
    assert any(c["reset"] is None and c["T"] > 1 for c in cs)
    assert any(c["reset"] is not None and c["reset"].all(axis=1).any() and c["T"] > 1 for c in cs)
    for k in ("h0", "c0"):
        assert any(c[k] is None for c in cs) and any(c[k] is not None for c in cs)


def test_pair_cases_emulations_pass():
    """The two-job cases of the GPU file, narrow and wide."""
    st = R.Stats()
    for c in R.lstm_pair_cases():
        R.lstm_fwd_check(c, lstm_emu(c), "x", st)
    for c in R.wide_pair_cases() + R.wide_pair_null_cases():
        wide_emu_check(c, st)
    a, b = R.wide_pair_cases()
    assert a["reset"].all(axis=1).any() and a["h0"] is None and b["c0"] is None
    assert all(c["reset"] is None for c in R.wide_pair_null_cases())
    print(st.line("pair emulations"))


@pytest.mark.parametrize("Hh", R.VALU_H)
def test_valu_lstm_emulation_passes_the_checks(Hh):
    st = R.Stats()
    for c, form, _ in R.valu_cases(Hh):
        valu_emu_check(c, form, st)
    c, form = R.valu_step_case(Hh)
    o = lstm_emu(c, form)
    R.lstm_fwd_check(c, {k: o[k] for k in ("h_out", "c_out", "h_save", "c_save")}, form, st)
    print(st.line(f"lstm VALU emulation H={Hh}"))


def valu_emu_check(c, form, st):
    out = lstm_emu(c, form)
    del out["h_save"], out["c_save"]  # (only pmlp_lstm_step writes them, and it takes no reset)
    R.lstm_fwd_check(c, out, form, st)
    R.lstm_bwd_check(c, out, lstm_bwd_emu(c, out, valu=True), "valu", st)


@pytest.mark.parametrize("B", [4088, 4089])
def test_valu_lstm_emulation_at_the_env_block_switch(B):
    st = R.Stats()
    for c, form in R.valu_switch_cases(B):
        valu_emu_check(c, form, st)
    print(st.line(f"lstm VALU emulation B={B}"))


def test_every_valu_form_meets_every_reset_pattern():
    seen = {}
    for Hh in R.VALU_H:
        n, hidx = 0, R.VALU_H.index(Hh)
        for I in R.VALU_I:
            for B in R.VALU_B:
                seen.setdefault(I, set()).add(R.RESET_PATTERNS[(3 * hidx + n) % 7])
                n += 1
    assert all(v == set(R.RESET_PATTERNS) for v in seen.values()), seen


@pytest.mark.parametrize("pattern", R.RESET_PATTERNS)
def test_emulations_pass_on_every_reset_pattern(pattern):
    """The reset-pattern cases of the GPU file, LSTM and GRU, forward and backward."""
    st = R.Stats()
    c, _, grus = R.pattern_cases(pattern)
    out = lstm_emu(c)
    R.lstm_fwd_check(c, out, "x", st)
    R.lstm_bwd_check(c, out, lstm_bwd_emu(c, out), stats=st)
    for g in grus:
        o = gru_emu(g)
        R.gru_fwd_check(g, o, st)
        R.gru_bwd_check(g, o, gru_bwd_emu(g, o), st)
    print(st.line(f"emulations, reset pattern {pattern}"))


def test_an_unwritten_or_non_finite_element_is_rejected():
    """The GPU outputs start NaN-filled: a row the kernel never wrote must fail every kind of
    comparison, a zero bound included."""
    c = R.seq_case(1, 2, 5, 3)
    out = lstm_emu(c)
    for k, check in (("gact", "gate"), ("c_out", "cell"), ("h_out", ("chain", "out")), ("xh", "chain")):
        bad = dict(out)
        bad[k] = out[k].copy()
        bad[k][1, 4, -1] = np.nan
        rejected(check, lambda: R.lstm_fwd_check(c, bad, "x"))
    rejected("x", lambda: R.equal("x", np.array([np.inf], f), np.array([np.inf], f), "inf"))
    rejected("x", lambda: R.within("x", np.array([np.nan]), np.array([0.0]), np.array([1.0]), "nan"))


MUT_CASE = dict(T=4, B=21, I=47)


def _mut_case(**kw):
    p = dict(MUT_CASE)
    p.update(kw)
    return R.seq_case(11, p.pop("T"), p.pop("B"), p.pop("I"), **p)


@pytest.mark.parametrize("mut,check", [
    ("drop_cross", "gate"), ("bias_once", "gate"), ("gate_order", "gate"),
    ("reset_late", ("chain", "gate", "cell")), ("reset_h_only", ("cell", "save")), ("h0_despite_reset", ("chain", "save")),
    ("xh_holds_h_out", "chain"), ("clamped_x", "gate"), ("no_ones", "chain")])
def test_wrong_lstm_forwards_are_rejected(mut, check):
    c = _mut_case()
    R.lstm_fwd_check(c, lstm_emu(c), "x")
    rejected(check, lambda: R.lstm_fwd_check(c, lstm_emu(c, "x", mut), "x"))


@pytest.mark.parametrize("I", [1, 47, 64])
def test_truncating_split_is_rejected_on_the_all_ones_mantissas(I):
    """Random operands cannot tell a truncating split from a rounding one inside 2^-15 sum|a||w|
    (its residuals cancel); the all-ones case makes them add up: 1.5 times the bound."""
    c = R.ones_case(I, 17, I)
    R.lstm_fwd_check(c, lstm_emu(c), "x")
    rejected("gate", lambda: R.lstm_fwd_check(c, lstm_emu(c, "x", "trunc"), "x"))
    g = R.ones_case(I, 17, I, gates=3)
    R.gru_fwd_check(g, gru_emu(g))
    rejected(("gate", "ghn"), lambda: R.gru_fwd_check(g, gru_emu(g, "trunc")))


def test_dropped_cross_term_leaves_the_bound_on_most_elements():
    """The forward product without hi.lo and lo.hi is outside 2^-15 sum|a||w| on most elements."""
    for I in (1, 47, 64):
        c = R.seq_case(I, 1, 37, I, reset="none")
        hp = R.h_prev_expected(c, None)
        z, ez = R.lstm_preact(c, hp, "x")
        row = np.concatenate([c["x"][0], hp[0]], 1)
        w = np.concatenate([c["w_ih"], c["w_hh"]], 1)
        b = (c["b_ih"] + c["b_hh"]).astype(f)
        good = np.abs(prod3(row, w, b) - z[0]) / ez[0]
        bad = np.abs(prod3(row, w, b, "drop_cross") - z[0]) / ez[0]
        print(f"I={I}: split product worst {good.max():.3f} of the bound; without the cross terms "
              f"{(bad > 1).mean() * 100:.0f} % of the elements are outside")
        assert good.max() < 0.25 and (bad > 1).mean() > 0.5


# ----------------------------------------------------------------- LSTM backward --
def test_matrix_core_lstm_backward_emulation_passes_and_wrong_ones_are_rejected():
    st = R.Stats()
    for T in R.BWD_T:
        for c in R.bwd_cases(T):
            fwd = lstm_emu(c)
            R.lstm_bwd_check(c, fwd, lstm_bwd_emu(c, fwd), stats=st)
    print(st.line("lstm bwd emulation"))
    c = _mut_case()
    fwd = lstm_emu(c)
    for mut in ("drop_cross", "carry_across_reset", "no_dc"):
        rejected("dgx", lambda: R.lstm_bwd_check(c, fwd, lstm_bwd_emu(c, fwd, mut)))


def _narrow(seed, T, B, I, n):
    p = R.presence(n)
    return R.narrow_bwd_case(seed, T, B, I, c0=p["c0"], reset=p["reset"])


@pytest.mark.parametrize("I", R.DW_I)
def test_narrow_slab_condition_and_emulation(I):
    """For every case of the GPU file: the reference's own bound stays below a quarter of a
    dropped cross term on every slab element, and the emulation passes."""
    st, worst = R.Stats(), 0.0
    for c, fwd in R.narrow_cases(I):
        worst = max(worst, R.narrow_slab_condition(c, fwd))
        R.narrow_slab_check(c, fwd, slab_emu(lstm_bwd_emu(c, fwd), fwd["xh"], c["B"], I), st)
    print(st.line(f"narrow slab emulation I={I}") + f"; bound / cross term <= {worst:.3f}")


def test_narrow_slab_condition_of_the_pattern_and_pair_cases():
    """The other narrow-slab cases of the GPU file: every reset pattern, and the two-job launch."""
    st = R.Stats()
    cases = [R.pattern_cases(p)[1] for p in R.RESET_PATTERNS] + list(R.narrow_pair_cases())
    for c, fwd in cases:
        R.narrow_slab_condition(c, fwd)
        R.narrow_slab_check(c, fwd, slab_emu(lstm_bwd_emu(c, fwd), fwd["xh"], c["B"], c["I"]), st)
    print(st.line("narrow slab emulation, pattern and pair cases"))


@pytest.mark.parametrize("B", [37, 4117])
def test_step_emulations_pass_with_the_bounds_multiplied_through(B):
    """The in-place steps save no gates: the LSTM's and the GRU's T = 1 emulation without gact."""
    st = R.Stats()
    for c, g in zip(R.step_cases(B), R.step_cases(B, gates=3)):
        o = lstm_emu(c)
        R.lstm_fwd_check(c, {k: o[k] for k in ("h_out", "c_out", "h_save", "c_save")}, "x", st)
        o = gru_emu(g)
        R.gru_fwd_check(g, {k: o[k] for k in ("h_out", "h_save")}, st)
    c = R.wide_step_case(B)
    o = lstm_emu(c, "gx")
    R.lstm_fwd_check(c, {k: o[k] for k in ("h_out", "c_out", "gx", "h_save", "c_save")}, "gx", st)
    print(st.line(f"step emulations B={B}"))


@pytest.mark.parametrize("mut", ["drop_cross", "skip_tail_env", "stale_neighbour", "permuted"])
def test_wrong_narrow_slabs_are_rejected(mut):
    c, fwd = _narrow(5, 3, 21, 31, 3)
    dg = lstm_bwd_emu(c, fwd)
    R.narrow_slab_check(c, fwd, slab_emu(dg, fwd["xh"], 21, 31))
    rejected("slab", lambda: R.narrow_slab_check(c, fwd, slab_emu(dg, fwd["xh"], 21, 31, mut)))


@pytest.mark.parametrize("mut", ["carry_across_reset", "no_dc", "drop_cross"])
def test_wrong_backward_inside_the_narrow_slab_is_rejected(mut):
    c, fwd = _narrow(5, 4, 21, 31, 5)
    rejected("slab", lambda: R.narrow_slab_check(c, fwd, slab_emu(lstm_bwd_emu(c, fwd, mut), fwd["xh"], 21, 31)))


# ---------------------------------------------------------------------------- GRU --
@pytest.mark.parametrize("I", R.GRU_I)
def test_gru_emulation_passes_the_checks(I):
    st = R.Stats()
    for c in R.sweep(300 + I, R.MF_T, R.MF_B, I, gates=3):
        out = gru_emu(c)
        R.gru_fwd_check(c, out, st)
        R.gru_bwd_check(c, out, gru_bwd_emu(c, out), st)
        if c["T"] == 1:
            R.gru_fwd_check(c, dict(h_out=out["h_out"], h_save=out["h_save"]), st)
    print(st.line(f"gru emulation I={I}"))


@pytest.mark.parametrize("mut,check", [
    ("drop_cross", ("gate", "ghn", "n")), ("bhn_outside", "ghn"),
    ("reset_late", ("chain", "gate")), ("h0_despite_reset", ("chain", "save"))])
def test_wrong_gru_forwards_are_rejected(mut, check):
    c = R.seq_case(12, 4, 21, 47, gates=3)
    rejected(check, lambda: R.gru_fwd_check(c, gru_emu(c, mut)))


@pytest.mark.parametrize("mut", ["drop_cross", "carry_across_reset"])
def test_wrong_gru_backwards_are_rejected(mut):
    c = R.seq_case(12, 4, 21, 47, gates=3)
    fwd = gru_emu(c)
    rejected("dg", lambda: R.gru_bwd_check(c, fwd, gru_bwd_emu(c, fwd, mut)))


# -------------------------------------------------------------------- exact grids --
@pytest.mark.parametrize("gates", [4, 3])
def test_grid_cases_are_exact_and_leave_the_activation_budget_alone(gates):
    """The builder asserts the exactness; on the grid the emulation's pre-activation error is
    zero, so the gate check's bound is the activation budget (e_z scaled to nothing)."""
    st = R.Stats()
    for I in R.MF_I:
        for B in R.MF_B:
            c = R.grid_case(I * 10 + B, B, I, gates=gates, reset0=(B == 37))
            if gates == 4:
                R.grid_lstm_check(c, lstm_emu(c), st)
            else:
                R.grid_gru_check(c, gru_emu(c), st)
    print(st.line(f"grid emulation gates={gates}"))


def test_grid_check_rejects_an_index_error_a_random_bound_would_pass():
    """One x column taken from its neighbour: on the grid the gates move by whole products."""
    c = R.grid_case(3, 17, 47)
    rejected("gate", lambda: R.grid_lstm_check(c, lstm_emu(c, "x", "clamped_x")))


# -------------------------------------------------------------------------- heads --
@pytest.mark.parametrize("M", R.HEADS_M)
def test_heads_grid_is_exact_and_the_emulation_is_equal(M):
    """Both jobs of every launch of the GPU file (the builder asserts the exactness)."""
    st = R.Stats()
    for Hh, cs in R.heads_cases(M):
        for c in cs:
            e = heads_emu(c)
            R.heads_fwd_check(c, e["y0"], e["out"], st)
            R.heads_bwd_check(c, e["dh"], e["slab"])
    print(st.line(f"heads emulation M={M}"))


@pytest.mark.parametrize("mut,check", [("elu_from_input", ("dh", "slab")), ("pad_row_counted", "slab")])
def test_wrong_heads_backwards_are_rejected(mut, check):
    c = R.heads_case(1, 129, 64, 32, 12)
    e = heads_emu(c, mut)
    rejected(check, lambda: R.heads_bwd_check(c, e["dh"], e["slab"]))
