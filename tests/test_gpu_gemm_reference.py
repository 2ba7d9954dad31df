"""The bf16 GEMM family of csrc/ppo_mlp.hip (pmlp_gemm, pmlp_gemm_pair) and its helper
kernels (pmlp_convert, pmlp_rowsum, pmlp_reduce_slabs) against the fp64 references of
tests/gemm_ref.py, element by element, at every arm of the host's selection: the six tile
configurations, the LDS-DMA / register / short-k loops, the bf16 / fp32-gather / [K,N] operand
forms and the five epilogues.  Exact-grid inputs make the linear part exact in fp32 in any
order, so the comparisons carry no tolerance beyond the ELU margin derived in gemm_ref.

Every output sits in a guarded buffer prefilled with a sentinel: nothing outside [M, N] may be
written.  Every case runs under each operand-staging mode (pmlp_set_gemm_staging); the modes
must agree bit for bit and the reference is then checked once.

Arms reached (tile configuration x k-loop x operand form), to tick against launch<>() and
pmlp_gemm's selection in csrc/ppo_mlp.hip:
  FWD_HIDDEN  32x128, 128x32, 128x64, 64x64: LDS-DMA (bf16 A, K 64 / 128 / 256 / 320); register
              staging (bf16 A: K 16 / 32 / 72 / 200, and every K under staging 0; the fp32 gather:
              every K but 40 / 48); the short-k loop NKS = 3 (K 40 / 48, bf16 A and the gather).
              128x128 eight waves: NKS = 3 both forms (48), LDS-DMA (64), register gather (72),
              register bf16 (200).  128x128 four waves: LDS-DMA, register bf16 (staging 0) and
              register gather at K 256 / 320.
  FWD_OUT     the four small configurations and 128x128 eight waves: LDS-DMA (bf16 A), register
              (bf16 A with a ragged last k-tile; the gather).
  BWD_DX      B [N,K]: LDS-DMA, register, NKS = 1 (K 16) on all five configurations.  B [K,N]:
              LDS-DMA on 32x128 (N 128), 128x64 (N 64), 64x64 (N 128, 512) and 128x128 (N 512),
              register elsewhere (128x32 always), NKS = 1.  yprev by 16-byte loads and by element.
  PARTIAL     register staging (its only loop) on 32x128, 128x32, 128x64, 128x128 eight waves.
  PARTIAL_TN  register on the same four; LDS-DMA with two buffers (staging 1) and the four-buffer
              ring (staging 2, 3) on 128x64 (256 x 64) and 128x128 (256 x 512, 128 x 256); sum_col
              on all of them.
  pmlp_gemm_pair  both paired instantiations (32x128 PARTIAL_TN + 64x64 NKS = 1 BWD_DX; 128x128
              LDS-DMA PARTIAL_TN + BWD_DX) and the unpaired fall-through.
Not reached, because the selection never picks them: 64x64 tiles for the split-K epilogues,
128x128 four waves for anything but FWD_HIDDEN, LDS-DMA with the gather form or with PARTIAL;
nor what is compiled out (the PMLP_NBUF = 2 loop, the PMLP_DIAG_* builds, PMLP_EXACT_ELU)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from rsl_rl.modules import mfma_mlp  # noqa: E402

import gemm_ref as R  # noqa: E402

DEV = "cuda"
H, O, D, P, PT = (mfma_mlp.EPI_FWD_HIDDEN, mfma_mlp.EPI_FWD_OUT, mfma_mlp.EPI_BWD_DX, mfma_mlp.EPI_PARTIAL,
                  mfma_mlp.EPI_PARTIAL_TN)
F32, BF = torch.float32, torch.bfloat16


def _c(n, m):
    return (n + m - 1) // m * m


def _off(n, m):
    """The smallest leading dimension > n + 1 that is NOT a multiple of m."""
    ld = n + 2
    return ld if ld % m else ld + 1


def _padded(t, ld, fill=1.0):
    """t [r, c] as a view of a [r, ld] buffer whose other columns hold `fill` (never to be read)."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    v = buf[:, :t.shape[1]]
    assert v.stride(0) == ld
    return v


def _staged(modes, run):
    """run() (-> a list of Guarded outputs, launched on the current stream) under each staging
    mode; the outputs, guard bands included, must be bitwise equal.  The previous mode is
    restored: the setting is process-global."""
    lib = mfma_mlp.load()
    prev = lib.pmlp_set_gemm_staging(modes[0])
    try:
        res = []
        for m in modes:
            lib.pmlp_set_gemm_staging(m)
            res.append(run())
            torch.cuda.synchronize()
    finally:
        lib.pmlp_set_gemm_staging(prev)
    for m, r in zip(modes[1:], res[1:]):
        for a, b in zip(res[0], r):
            assert R.same_bits(a.flat, b.flat), f"staging mode {m} differs from mode {modes[0]}"
    return res[0]


# ---------------------------------------------------------------- forward --
def _fwd_spec(M, N, K, form, v, g, kaf=None):
    """One forward job on exact-grid inputs.  v: layout variant (odd: padded operand rows and
    leading dimensions off the vector paths; 2: cb only; 3: ct only)."""
    odd = v & 1
    w, bias = R.grid_weight((N, K), K, g, DEV), R.grid_bias(N, g, DEV)
    job = dict(B=_padded(w, K + 8 * odd), M=M, N=N, K=K, bias=bias)
    if form == "af":
        kaf = K - 3 if kaf is None else kaf
        nrows = M + 5
        x = R.grid_act((nrows, kaf), g, DEV, F32)
        rows = None if v == 1 else torch.randperm(nrows, generator=g, device=DEV)[:M]
        a = torch.zeros(M, K, dtype=BF, device=DEV)
        a[:, :kaf] = (x[:M] if rows is None else x[rows]).to(BF)
        job.update(af=_padded(x, _c(kaf, 4) + 4 + 4 * odd), rows=rows)
        assert job["af"].stride(0) > kaf
    else:
        a = R.grid_act((M, K), g, DEV)
        job["A"] = _padded(a, K + 8 * odd)
    return dict(job=job, a=a, w=w, bias=bias, M=M, N=N, K=K, v=v, af=form == "af")


def _fwd_outs(epi, s):
    M, N, K, v, odd = s["M"], s["N"], s["K"], s["v"], s["v"] & 1
    o = {}
    if epi == O:
        o["cf"] = R.Guarded(M, N, _off(N, 4) if odd else _c(N, 4) + 4, F32, DEV)
    else:
        if v != 3:
            o["cb"] = R.Guarded(M, N, _off(N, 8) if odd else _c(N, 8) + 8, BF, DEV)
        if v != 2:  # ldct > M: a multiple of 8 (16-byte stores) or of 4 only (by element)
            o["ct"] = R.Guarded(N, M, _c(M, 8) + (4 if odd else 8), BF, DEV)
    if s["af"]:
        o["xa"] = R.Guarded(M, K, K + 8, BF, DEV)
    return o


def _fwd_check(epi, s, o, cond, what):
    a, w, bias = s["a"], s["w"], s["bias"]
    for k, G in o.items():
        G.assert_untouched(f"{what} {k}")
    if epi == O:
        R.check_fwd_out(o["cf"].got(), a, w, bias, what)
    else:
        if "cb" in o:
            R.check_fwd_hidden(o["cb"].got(), a, w, bias, cond, what + " cb")
            if "ct" in o:
                R.check_ct(o["ct"].got(), o["cb"].got(), what)
        else:
            R.check_fwd_hidden(o["ct"].got().t(), a, w, bias, cond, what + " ct")
    if "xa" in o:  # the converted rows, zeros at the padded columns
        assert R.same_bits(o["xa"].got().contiguous(), a.contiguous()), what + " xa"


def _run_fwd(epi, shapes, K, form, v, seed, cond=None, modes=(0, 1), kaf=None):
    g = R.gen(seed, DEV)
    specs = [_fwd_spec(M, N, K, form, v, g, kaf) for M, N in shapes]
    outs = []

    def run():
        outs.append([_fwd_outs(epi, s) for s in specs])
        mfma_mlp._gemm(epi, [dict(s["job"], **{k: G.mat for k, G in o.items()}) for s, o in zip(specs, outs[-1])])
        return [G for o in outs[-1] for G in o.values()]

    _staged(modes, run)
    for i, (s, o) in enumerate(zip(specs, outs[0])):
        _fwd_check(epi, s, o, cond, f"epi {epi} job {i} M={s['M']} N={s['N']} K={K} {form} v{v}")


# ---------------------------------------------------------- input gradient --
def _bwd_spec(M, N, K, form, v, g):
    odd = v & 1
    dz, wt, y = R.grid_act((M, K), g, DEV), R.grid_weight((N, K), K, g, DEV), R.grid_yprev((M, N), g, DEV)
    # N % 8 != 0 or ldyp % 8 != 0: yprev by element; else 16-byte loads
    job = dict(A=_padded(dz, K + 8 * odd), M=M, N=N, K=K, yprev=_padded(y, _c(N, 8) + 4 * odd, 0.5))
    if form == "kn":  # B = W[out, in] = [K, N], n contiguous
        job.update(B=_padded(wt.t().contiguous(), _c(N, 8) + 8 * odd), b_kn=1)
    else:
        job["B"] = _padded(wt, K + 8 * odd)
    return dict(job=job, dz=dz, wt=wt, y=y, M=M, N=N, K=K, v=v, af=False)


def _bwd_check(s, o, what):
    for k, G in o.items():
        G.assert_untouched(f"{what} {k}")
    if "cb" in o:
        R.check_bwd_dx(o["cb"].got(), s["dz"], s["wt"], s["y"], what + " cb")
        if "ct" in o:
            R.check_ct(o["ct"].got(), o["cb"].got(), what)
    else:
        R.check_bwd_dx(o["ct"].got().t(), s["dz"], s["wt"], s["y"], what + " ct")


def _run_bwd(shapes, K, form, v, seed, modes=(0, 1, 2, 3)):
    g = R.gen(seed, DEV)
    specs = [_bwd_spec(M, N, K, form, v, g) for M, N in shapes]
    outs = []

    def run():
        outs.append([_fwd_outs(D, s) for s in specs])
        mfma_mlp._gemm(D, [dict(s["job"], **{k: G.mat for k, G in o.items()}) for s, o in zip(specs, outs[-1])])
        return [G for o in outs[-1] for G in o.values()]

    _staged(modes, run)
    for i, (s, o) in enumerate(zip(specs, outs[0])):
        _bwd_check(s, o, f"BWD_DX job {i} M={s['M']} N={s['N']} K={K} {form} v{v}")


# ------------------------------------------------------------------ sweeps --
# (M, N) per tile configuration: the smallest shapes that reach it (gemm_ref.tile_config)
SMALL = {
    "32x128": [(1, 136), (12, 136), (32, 136), (1, 128), (12, 128), (32, 128)],
    "128x32": [(37, 1), (200, 1), (37, 12), (200, 12), (37, 32), (200, 32)],
    "128x64": [(37, 40), (200, 40), (37, 64), (200, 64)],
    "64x64": [(100, 136), (129, 136), (100, 264), (129, 264), (100, 128), (129, 128)],
}
# N % 8 != 0 beside them for the input gradient (yprev by element, ragged [K,N] rows)
SMALL_BWD = {"32x128": [(12, 100)], "128x32": [], "128x64": [(37, 52)], "64x64": [(100, 132)]}
CFG = {"32x128": (32, 128, 1, 4), "128x32": (128, 32, 4, 1), "128x64": (128, 64, 4, 1), "64x64": (64, 64, 2, 2)}


def _variants(K):
    return (0, 1, 2, 3) if K in (48, 64) else (0, 1)


@pytest.mark.parametrize("epi", [H, O], ids=["hidden", "out"])
@pytest.mark.parametrize("cfg", list(SMALL))
def test_forward_small_tiles(cfg, epi):
    """FWD_HIDDEN / FWD_OUT on one of the four small tile configurations: every K class (the
    short-k form at 40 and 48, LDS-DMA at 64 / 128 / 256 / 320, register staging with a ragged
    last k-tile at 72 and 200), bf16 A and the fp32 gather form with xa."""
    cond = R.Conditions()
    seed = 0
    for M, N in SMALL[cfg]:
        for K in R.K_CLASSES:
            assert R.tile_config(epi, M, N, K, 1) == CFG[cfg]
            for form in ("bf16", "af"):
                for v in (_variants(K) if epi == H else (0, 1)):
                    seed += 1
                    _run_fwd(epi, [(M, N)], K, form, v, 1000 * epi + seed, cond)
    if epi == H:
        cond.assert_ok()


@pytest.mark.parametrize("cfg", list(SMALL))
def test_input_gradient_small_tiles(cfg):
    """BWD_DX on the small tile configurations: B as [N,K] and as [K,N] (LDS-DMA where N is a
    whole number of tiles and K of k-tiles, register staging elsewhere), the one-step k loop
    at K = 16, yprev by 16-byte loads and by element, staging modes 0..3."""
    seed = 0
    for M, N in SMALL[cfg] + SMALL_BWD[cfg]:
        for K in R.K_CLASSES:
            assert R.tile_config(D, M, N, K, 1) == CFG[cfg]
            for form in ("nk", "kn"):
                for v in _variants(K):
                    seed += 1
                    _run_bwd([(M, N)], K, form, v, 5000 + seed)


BIG = [(4000, 512)] * 4  # 32 x 4 x 4 = 512 tiles of 128 x 128: the threshold


@pytest.mark.parametrize("K,form", [(48, "bf16"), (48, "af"), (64, "bf16"), (72, "af"), (200, "bf16")])
def test_forward_hidden_128x128_eight_waves(K, form):
    assert R.tile_config(H, 4000, 512, K, 4) == (128, 128, 2, 4)
    cond = R.Conditions()
    _run_fwd(H, BIG, K, form, 0, 21000 + K, cond)
    cond.assert_ok()


@pytest.mark.parametrize("K,form", [(256, "bf16"), (256, "af"), (320, "bf16"), (320, "af")])
def test_forward_hidden_128x128_four_waves(K, form):
    assert R.tile_config(H, 4000, 512, K, 4) == (128, 128, 2, 2)
    cond = R.Conditions()
    _run_fwd(H, BIG, K, form, 1 if form == "af" else 0, 22000 + K, cond)
    cond.assert_ok()


@pytest.mark.parametrize("K,form", [(64, "bf16"), (72, "af"), (200, "bf16"), (256, "bf16"), (320, "af")])
def test_forward_out_128x128(K, form):
    assert R.tile_config(O, 4000, 512, K, 4) == (128, 128, 2, 4)
    _run_fwd(O, BIG, K, form, 0, 23000 + K)


@pytest.mark.parametrize("K,form", [(16, "kn"), (16, "nk"), (64, "kn"), (72, "kn"), (256, "nk"), (320, "kn")])
def test_input_gradient_128x128(K, form):
    assert R.tile_config(D, 4000, 512, K, 4) == (128, 128, 2, 4)
    _run_bwd(BIG, K, form, 0, 24000 + K)


@pytest.mark.parametrize("epi,K,form", [(H, 64, "bf16"), (H, 256, "af"), (O, 72, "bf16"), (D, 64, "kn"),
                                        (D, 200, "nk")])
def test_just_under_the_tile_threshold_runs_64x64(epi, K, form):
    """31 x 4 x 4 = 496 tiles of 128 x 128 < 512: the same batch on 64 x 64 tiles."""
    shapes = [(3968, 512)] * 4
    assert R.tile_config(epi, 3968, 512, K, 4) == (64, 64, 2, 2)
    if epi == D:
        _run_bwd(shapes, K, form, 0, 25000 + K)
    else:
        _run_fwd(epi, shapes, K, form, 0, 25000 + K + epi)


@pytest.mark.parametrize("shapes", [[(100, 136), (37, 40)], [(37, 12), (200, 1)]], ids=["64x64", "128x32"])
def test_unequal_jobs_in_one_launch(shapes):
    """The grid is sized by the largest job: the smaller job's surplus tiles write nothing
    (guard bands) and its own tiles are not confused with the other job's."""
    seed = 30000
    for order in (shapes, shapes[::-1]):
        for K in (48, 64, 72):
            for v in (0, 1):
                seed += 1
                for form in ("bf16", "af"):
                    _run_fwd(H, order, K, form, v, seed)
                    _run_fwd(O, order, K, form, v, seed + 500)
                for form in ("nk", "kn"):
                    _run_bwd(order, K, form, v, seed + 1000)
        _run_bwd(order, 16, "kn", 0, seed + 2000)


# ---------------------------------------------------------- weight gradient --
def _partial_spec(epi, M, N, K, ks, sum_col, v, g):
    odd = v & 1
    a, b = R.grid_act((K, M), g, DEV), R.grid_weight((K, N), ks, g, DEV)
    if epi == PT:
        job = dict(A=_padded(a, _c(M, 8) + 8 * odd), B=_padded(b, _c(N, 8) + 8 * odd), M=M, N=N, K=K)
        if sum_col:
            job["sum_col"] = N
    else:
        job = dict(A=_padded(a.t().contiguous(), K + 8 * odd), B=_padded(b.t().contiguous(), K + 8 * odd), M=M, N=N,
                   K=K)
    return dict(job=job, a=a, b=b, M=M, N=N, K=K, sum_col=bool(sum_col) and epi == PT, odd=odd)


def _run_partial(epi, shapes_k, ks, sum_col, v, seed, modes):
    g = R.gen(seed, DEV)
    specs = [_partial_spec(epi, M, N, K, ks, sum_col, v, g) for M, N, K in shapes_k]
    outs = []

    def run():
        outs.append([R.Guarded(s["M"], s["N"], _off(s["N"], 4) if s["odd"] else _c(s["N"], 4) + 4, F32, DEV,
                               slabs=(s["K"] + ks - 1) // ks) for s in specs])
        mfma_mlp._gemm(epi, [dict(s["job"], cf=G.t) for s, G in zip(specs, outs[-1])], ksplit=ks)
        return outs[-1]

    _staged(modes, run)
    for i, (s, G) in enumerate(zip(specs, outs[0])):
        what = f"epi {epi} job {i} M={s['M']} N={s['N']} K={s['K']} ks={ks} v{v}"
        G.assert_untouched(what, extra_cols=(s["N"],) if s["sum_col"] else ())
        R.check_partial(G.t[:, :, :s["N"]], s["a"], s["b"], ks, G.t[:, :, s["N"]] if s["sum_col"] else None, what)


# the (M, N) of the sum-of-slabs tests (test_gpu_fused_ppo.py), whole 128 x 64 tiles and 128 x 32 tiles
PARTIAL_MN = [(512, 56), (256, 520), (128, 264), (12, 136), (1, 136), (64, 64),
              (512, 48), (256, 512), (128, 256), (12, 128), (1, 128), (64, 56), (256, 64), (200, 24)]


@pytest.mark.parametrize("K,ks", R.PARTIAL_KS)
@pytest.mark.parametrize("epi", [P, PT], ids=["nt", "tn"])
def test_partial_slab_by_slab(epi, K, ks):
    """Each split-K slab is the fp64 product over its own k range (a 40-row last slab at
    K = 1000), sum_col the column sum of that range; PARTIAL_TN under staging modes 0..3."""
    seed = 40000 + K
    for M, N in PARTIAL_MN:
        for v in (0, 1):
            for sum_col in ((0, 1) if epi == PT else (0,)):
                seed += 1
                _run_partial(epi, [(M, N, K)], ks, sum_col, v, seed, (0, 1, 2, 3) if epi == PT else (0, 1))


@pytest.mark.parametrize("epi", [P, PT], ids=["nt", "tn"])
def test_partial_jobs_of_different_k_and_extent(epi):
    """Jobs of different K (1000 and 1024: four slabs of 256 either way) and different
    extents in one launch."""
    modes = (0, 1, 2, 3) if epi == PT else (0, 1)
    for shapes in ([(128, 264, 1000), (12, 136, 1024)], [(12, 136, 1024), (128, 264, 1000)],
                   [(64, 56, 1024), (512, 48, 1000)], [(256, 512, 1024), (128, 256, 1000), (1, 128, 1024)]):
        for v in (0, 1):
            _run_partial(epi, shapes, 256, 1, v, 41000 + v, modes)


def _pair_case(batch, nw, nx_k, nx_n, ks, njobs, seed):
    """A layer's backward: dW = dz^T y (PARTIAL_TN, sum_col) beside dx = (dz W) ELU'(yprev)."""
    g = R.gen(seed, DEV)
    jw, jx, ref = [], [], []
    for _ in range(njobs):
        dz = R.grid_act((batch, nx_k), g, DEV)                  # [batch, out]
        yin = R.grid_weight((batch, nx_n), ks, g, DEV)          # the layer's input rows [batch, in]
        w = R.grid_weight((nx_k, nx_n), nx_k, g, DEV)           # W[out, in]
        yp = R.grid_yprev((batch, nx_n), g, DEV)
        lda = _c(nw, 8)
        jw.append(dict(A=_padded(dz[:, :nw].contiguous(), lda), B=yin, M=nw, N=nx_n, K=batch, sum_col=nx_n))
        jx.append(dict(A=dz, B=w, b_kn=1, M=batch, N=nx_n, K=nx_k, yprev=yp))
        ref.append((dz, yin, w, yp))
    return jw, jx, ref


@pytest.mark.parametrize("name,batch,nw,kx,nx,ks,njobs", [
    ("32x128+64x64", 1000, 12, 16, 128, 512, 2),       # the output layer's backward
    ("128x128+128x128", 8192, 256, 256, 512, 1024, 2),  # a hidden layer's backward (LDS-DMA both)
    ("unpaired", 1000, 64, 64, 128, 512, 1),            # no paired instantiation: the two launches
])
def test_gemm_pair_against_the_references(name, batch, nw, kx, nx, ks, njobs):
    """pmlp_gemm_pair's two paired instantiations and its unpaired fall-through: both halves
    against their references and bitwise the two separate launches."""
    jw, jx, ref = _pair_case(batch, nw, kx, nx, ks, njobs, 42000 + batch)
    S = (batch + ks - 1) // ks
    res = {}
    for paired in (True, False):
        cf = [R.Guarded(nw, nx, nx + 4, F32, DEV, slabs=S) for _ in range(njobs)]
        cb = [R.Guarded(batch, nx, nx + 8, BF, DEV) for _ in range(njobs)]
        ct = [R.Guarded(nx, batch, batch + 8, BF, DEV) for _ in range(njobs)]
        w = [dict(j, cf=c.t) for j, c in zip(jw, cf)]
        x = [dict(j, cb=b.mat, ct=t.mat) for j, b, t in zip(jx, cb, ct)]
        if paired:
            mfma_mlp._gemm_pair(w, ks, x)
        else:
            mfma_mlp._gemm(PT, w, ksplit=ks)
            mfma_mlp._gemm(D, x)
        torch.cuda.synchronize()
        res[paired] = cf + cb + ct
    for a, b in zip(res[True], res[False]):
        assert R.same_bits(a.flat, b.flat)
    cf, cb, ct = res[True][:njobs], res[True][njobs:2 * njobs], res[True][2 * njobs:]
    for i, (dz, yin, w, yp) in enumerate(ref):
        cf[i].assert_untouched(f"{name} slab {i}", extra_cols=(nx,))
        cb[i].assert_untouched(f"{name} cb {i}")
        ct[i].assert_untouched(f"{name} ct {i}")
        R.check_partial(cf[i].t[:, :, :nx], dz[:, :nw], yin, ks, cf[i].t[:, :, nx], f"{name} dW {i}")
        R.check_bwd_dx(cb[i].got(), dz, w.t(), yp, f"{name} dx {i}")
        R.check_ct(ct[i].got(), cb[i].got(), f"{name} dx {i}")


# ------------------------------------------------------ the PPO layer shapes --
@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("K0,kx", [(48, 48), (64, 64), (256, 240), (448, 448)])
def test_layer_shapes_on_the_exact_grid(K0, kx, M):
    """Every layer shape of the actor and the critic (K0 -> 512 -> 256 -> 128 -> 12 / 1, both
    nets in one launch) on exact-grid inputs: the per-layer forward that the fused forward is
    bitwise equal to now ends in a reference."""
    cond = R.Conditions()
    for v in (0, 1):
        _run_fwd(H, [(M, 512)] * 2, K0, "af", v, 50000 + K0 + v, cond, kaf=kx)
        _run_fwd(H, [(M, 256)] * 2, 512, "bf16", v, 51000 + v, cond)
        _run_fwd(H, [(M, 128)] * 2, 256, "bf16", v, 52000 + v, cond)
        _run_fwd(O, [(M, 12), (M, 1)], 128, "bf16", v, 53000 + v)
    cond.assert_ok()


@pytest.mark.parametrize("M", [37, 200])
@pytest.mark.parametrize("K0,kx", [(48, 48), (64, 64), (256, 240), (448, 448)])
def test_layer_chain_and_fused_forward(K0, kx, M):
    """The 4-layer forward of both nets, layer by layer, each layer fed the bf16 output the
    previous kernel layer produced: layer 0 (exact-grid rows and weights) against the exact
    reference; the later layers, whose inputs are ELU outputs off the grid, against the fp64
    product of those very inputs within e_acc (gemm_ref: the any-order fp32 summation bound),
    so errors do not compound.  pmlp_mlp_forward on the same inputs is bitwise the chain."""
    g = R.gen(60000 + K0 + M, DEV)
    widths = [[512, 256, 128, 12], [512, 256, 128, 1]]
    nrows = M + 5
    x = _padded(R.grid_act((nrows, kx), g, DEV, F32), _c(kx, 4) + 4)
    rows = torch.randperm(nrows, generator=g, device=DEV)[:M]
    a0 = torch.zeros(M, K0, dtype=BF, device=DEV)
    a0[:, :kx] = x[rows].to(BF)
    nets = []
    for ns in widths:
        ks = [K0] + ns[:-1]
        nets.append(dict(W=[R.grid_weight((n, k), k, g, DEV) for n, k in zip(ns, ks)],
                         b=[R.grid_bias(n, g, DEV) for n in ns], N=ns))
    # layer by layer
    ys = [[] for _ in nets]
    xa = torch.empty(M, K0, dtype=BF, device=DEV)
    for l in range(3):
        gj = []
        for n, net in enumerate(nets):
            y = torch.empty(M, net["N"][l], dtype=BF, device=DEV)
            src = dict(af=x, rows=rows, xa=xa if n == 0 else None) if l == 0 else dict(A=ys[n][-1])
            gj.append(dict(B=net["W"][l], bias=net["b"][l], M=M, N=net["N"][l], K=K0 if l == 0 else net["N"][l - 1],
                           cb=y, **src))
            ys[n].append(y)
        mfma_mlp._gemm(H, gj)
    outs = [torch.empty(M, net["N"][3], device=DEV) for net in nets]
    mfma_mlp._gemm(O, [dict(A=ys[n][2], B=net["W"][3], bias=net["b"][3], M=M, N=net["N"][3], K=net["N"][2],
                            cf=outs[n]) for n, net in enumerate(nets)])
    torch.cuda.synchronize()
    assert R.same_bits(xa, a0)
    cond = R.Conditions()
    for n, net in enumerate(nets):
        R.check_fwd_hidden(ys[n][0], a0, net["W"][0], net["b"][0], cond, f"net {n} layer 0")
        for l in (1, 2):
            R.check_fwd_hidden_bound(ys[n][l], ys[n][l - 1], net["W"][l], net["b"][l], f"net {n} layer {l}")
        R.check_fwd_out_bound(outs[n], ys[n][2], net["W"][3], net["b"][3], f"net {n} output")
    cond.assert_ok()
    # the fused forward
    fy = [[torch.full_like(y, float("nan")) for y in ys[n]] for n in range(2)]
    fo = [torch.full_like(o, float("nan")) for o in outs]
    fxa = torch.full_like(xa, float("nan"))
    mfma_mlp.mlp_forward([dict(x=x, kx=kx, rows=rows, xa=fxa if n == 0 else None, K0=K0, W=net["W"], b=net["b"],
                               N=net["N"], y=fy[n], out=fo[n]) for n, net in enumerate(nets)], M)
    torch.cuda.synchronize()
    assert R.same_bits(fxa, xa)
    for n in range(2):
        for l in range(3):
            assert R.same_bits(fy[n][l], ys[n][l]), (n, l)
        assert R.same_bits(fo[n], outs[n]), n


# ------------------------------------------------------ random-normal class --
@pytest.mark.parametrize("M,N", [(12, 136), (37, 12), (200, 64), (129, 264)])
def test_random_normal_rows_through_the_gather_form(M, N):
    """Full-mantissa fp32 rows through the af form: xa is bitwise x.to(bfloat16) (round to
    nearest even, not truncation) with zeros at the padded columns; the outputs lie within
    e_acc of the fp64 product of the bf16-rounded operands."""
    for K in (40, 72, 128, 320):
        g = R.gen(70000 + K + M, DEV)
        kaf, nrows = K - 3, M + 7
        x = 2.0 * torch.randn(nrows, kaf, generator=g, device=DEV)
        x.view(torch.int32)[::3, ::2] |= 0x8000  # ties and near-ties among them
        x.view(torch.int32)[::3, ::4] &= -32768
        rows = torch.randperm(nrows, generator=g, device=DEV)[:M]
        w = (torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(BF)
        bias = torch.randn(N, generator=g, device=DEV)
        a = torch.zeros(M, K, dtype=BF, device=DEV)
        a[:, :kaf] = x[rows].cpu().to(BF).to(DEV)
        job = dict(af=_padded(x, _c(kaf, 4) + 4, 7.0), rows=rows, B=w, bias=bias, M=M, N=N, K=K)

        def run(epi):
            o = dict(xa=R.Guarded(M, K, K + 8, BF, DEV))
            if epi == H:
                o.update(cb=R.Guarded(M, N, _c(N, 8) + 8, BF, DEV), ct=R.Guarded(N, M, _c(M, 8) + 4, BF, DEV))
            else:
                o["cf"] = R.Guarded(M, N, N + 3, F32, DEV)
            mfma_mlp._gemm(epi, [dict(job, **{k: G.mat for k, G in o.items()})])
            return o

        for epi in (H, O):
            o = {}

            def go():
                o.clear()
                o.update(run(epi))
                return list(o.values())

            _staged((0, 1), go)
            what = f"randn epi {epi} M={M} N={N} K={K}"
            for k, G in o.items():
                G.assert_untouched(f"{what} {k}")
            assert R.same_bits(o["xa"].got().contiguous(), a), what + " xa"
            if epi == H:
                R.check_fwd_hidden_bound(o["cb"].got(), a, w, bias, what)
                R.check_ct(o["ct"].got(), o["cb"].got(), what)
            else:
                R.check_fwd_out_bound(o["cf"].got(), a, w, bias, what)


# ------------------------------------------------------------ helper kernels --
def _full_mantissa(shape, g):
    """fp32 values with full mantissas; a quarter exactly halfway between two bf16 numbers
    (ties go to even), some a bit to either side of halfway."""
    x = torch.randn(shape, generator=g, device=DEV) * 3.0
    b = x.view(torch.int32)
    sel = torch.randint(0, 8, shape, generator=g, device=DEV)
    b[sel < 2] = (b[sel < 2] & -65536) | 0x8000
    b[sel == 2] = (b[sel == 2] & -65536) | 0x8001
    b[sel == 3] = (b[sel == 3] & -65536) | 0x7FFF
    return x


CONVERT_MK = [(M, K) for M in (1, 63, 64, 65, 200) for K in (1, 47, 64, 65)]


def _convert_job(M, K, i, g):
    var = i % 6
    use_rows = var in (0, 3, 4)
    nrows = M + 3 if use_rows else M
    x = _padded(_full_mantissa((nrows, K), g), K + i % 3, 9.0)
    rows = torch.randperm(nrows, generator=g, device=DEV)[:M] if use_rows else None
    Kp = (K, _c(K, 8) + 8, _c(K, 8), K + 5, _c(K, 8) + 8, K)[var]
    one_col = (0, K, 0, Kp - 1, 0, 0)[var]
    want_y, want_yt = var != 2, var in (0, 2, 4)
    ldyt = (M, 0, _c(M, 8) + 8, 0, M + 3, 0)[var]
    xs = (x if rows is None else x[rows])[:M].cpu().to(BF)  # the reference rounding, on the CPU
    ey = torch.zeros(M, Kp, dtype=BF)
    ey[:, :K] = xs
    if one_col:
        ey[:, one_col] = 1.0
    eyt = torch.zeros(Kp, ldyt, dtype=BF)
    if want_yt:
        eyt[:K, :M] = xs.t()
    y = R.Guarded(M, Kp, Kp, BF, DEV) if want_y else None
    yt = R.Guarded(Kp, ldyt, ldyt, BF, DEV) if want_yt else None
    job = (x, Kp, y.mat if y else None, yt.mat if yt else None, rows, one_col)
    return job, (y, ey, yt, eyt, f"convert M={M} K={K} variant {var}")


@pytest.mark.parametrize("first", [0, 4])
def test_convert_against_torch_rounding(first):
    """pmlp_convert, 16 jobs of different shapes in one call: bitwise x.to(bfloat16) with the
    rows gather, zero columns K..Kp-1, the ones column at K and at Kp-1, the transposed copy
    with ldyt > M (zero columns M..ldyt-1, zero rows K..Kp-1); y only, yt only and both."""
    g = R.gen(80000 + first, DEV)
    made = [_convert_job(M, K, first + i, g) for i, (M, K) in enumerate(CONVERT_MK[first:first + 16])]
    assert len(made) == 16
    mfma_mlp._convert([j for j, _ in made])
    torch.cuda.synchronize()
    for _, (y, ey, yt, eyt, what) in made:
        if y is not None:
            y.assert_untouched(what + " y")
            assert R.same_bits(y.got().contiguous().cpu(), ey), what + " y"
        if yt is not None:
            yt.assert_untouched(what + " yt")
            assert R.same_bits(yt.got().contiguous().cpu(), eyt), what + " yt"


def test_rowsum_against_fp64():
    """pmlp_rowsum: exact-grid bf16 rows, ld > cols, jobs of different row counts in one grid."""
    g = R.gen(81000, DEV)
    jobs, chk = [], []
    for i, cols in enumerate((1, 7, 8, 9, 2047, 2048, 2056, 4100)):
        rows = (5, 1, 12, 3, 7, 2, 9, 4)[i]
        buf = R.grid_act((rows + 2, _c(cols, 8) + 8), g, DEV)  # (the columns past cols are not zero)
        x = buf[:, :cols]
        out = R.Guarded(1, rows, rows, F32, DEV)
        jobs.append((x, out.t, rows))
        chk.append((out, x[:rows].double().sum(1), f"rowsum cols={cols} rows={rows}"))
    mfma_mlp._rowsum(jobs)
    torch.cuda.synchronize()
    for out, want, what in chk:
        out.assert_untouched(what)
        R.assert_equal(out.got()[0], want, what)


def _reduce(jobs):
    arr = (mfma_mlp.ReduceJob * len(jobs))(*jobs)
    mfma_mlp._ok(mfma_mlp.load().pmlp_reduce_slabs(len(jobs), arr, torch.cuda.current_stream().cuda_stream),
                 "pmlp_reduce_slabs")


NSLABS = (1, 8, 9, 16, 17, 128, 129, 300)  # the edges of reduce_pack's group counts (8 slabs per thread)


@pytest.mark.parametrize("layout", ["vector", "stride", "base"])
def test_reduce_slabs_against_fp64(layout):
    """pmlp_reduce_slabs, eight jobs (one per slab-count edge) in one call, n % 4 != 0: 16-byte
    loads; a stride that is no multiple of 4 and a slab base that is not 16-byte aligned (both
    by element)."""
    g = R.gen(82000, DEV)
    n = 1030
    stride, off = {"vector": (1032, 0), "stride": (1031, 0), "base": (1032, 1)}[layout]
    jobs, chk = [], []
    for ns in NSLABS:
        buf = R.grid_act((off + ns * stride + 8,), g, DEV, F32)
        slab = buf[off:]
        out = R.Guarded(1, n, n, F32, DEV)
        jobs.append(mfma_mlp.ReduceJob(slab.data_ptr(), out.t.data_ptr(), None, stride, n, ns, 0, 0))
        want = slab[:ns * stride].view(ns, stride)[:, :n].double().sum(0)
        chk.append((out, want, f"reduce {layout} nslabs={ns}", buf))
    _reduce(jobs)
    torch.cuda.synchronize()
    for out, want, what, _ in chk:
        out.assert_untouched(what)
        R.assert_equal(out.got()[0], want, what)


def test_reduce_slabs_bias_out_against_fp64():
    """bias_out: slab rows of cols_in columns; columns < cols_out to out [rows, cols_out],
    column cols_out to bias_out, the later ones dropped (quads straddle rows)."""
    g = R.gen(83000, DEV)
    rows = 5
    jobs, chk = [], []
    for i, ci in enumerate((9, 17, 520)):
        for co in (ci - 1, ci - 8):
            ns = (9, 17, 129, 8, 300, 16)[len(jobs)]
            n = rows * ci
            stride = n + (0 if i != 1 else 3)
            buf = R.grid_act((ns * stride + 8,), g, DEV, F32)
            out, bias = R.Guarded(rows, co, co, F32, DEV), R.Guarded(1, rows, rows, F32, DEV)
            jobs.append(mfma_mlp.ReduceJob(buf.data_ptr(), out.t.data_ptr(), bias.t.data_ptr(), stride, n, ns, ci, co))
            s = buf[:ns * stride].view(ns, stride)[:, :n].double().sum(0).view(rows, ci)
            chk.append((out, bias, s, co, f"reduce bias_out cols_in={ci} cols_out={co} nslabs={ns}", buf))
    _reduce(jobs)
    torch.cuda.synchronize()
    for out, bias, s, co, what, _ in chk:
        out.assert_untouched(what)
        bias.assert_untouched(what + " bias")
        R.assert_equal(out.got(), s[:, :co], what)
        R.assert_equal(bias.got()[0], s[:, co], what + " bias")
