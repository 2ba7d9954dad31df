"""Digests and times the PPO loss (csrc/ppo_loss.h in every kernel that holds it) with the
libppomlp.so named by PPOMLP_LIB, for a bitwise and a speed comparison of two builds.
Digests (SHA-256 over every output buffer, inputs of tests/ppo_ref.loss_inputs at fixed seeds,
rows gathered, clipped_value on, transposes on): pmlp_ppo_loss_step at every (A, Ap) of its
three arms and M = 65, 517; pmlp_ppo_loss_step_f32 at A = 12, 10, 20; pmlp_ppo_loss_fwd + _bwd;
the three LOSS forwards at M = 18469; pmlp_reduce_slabs_step's finish at M = 101, A = 12.
Medians (HIP events, `time` as argument): the step's three arms at M = 24,576, fwd + bwd at
A = 12, the LOSS forward at M = 24,576 (K0 48, hidden 512 / 256 / 128), the folded finish.
usage: [PPOMLP_LIB=...] python tools/probes/ppo_loss_digest.py [time]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "unitree-rl-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

import ppo_ref as R  # noqa: E402

dev = "cuda"
F32, BF = torch.float32, torch.bfloat16
L, P = mm.load(), mm._p
VCOEF, ECOEF, VP = 0.5, 0.01, 8
name = os.path.basename(os.environ.get("PPOMLP_LIB", "libppomlp.so"))
QUAD = ((4, 4), (4, 8), (12, 16), (16, 16))
REG = ((10, 16), (1, 8), (3, 8), (12, 24), (8, 32))
GENERIC = ((10, 12), (17, 17), (20, 24))


def z(*s, dtype=F32):
    return torch.zeros(*s, dtype=dtype, device=dev)


def inputs(M, A, **kw):
    inp = R.loss_inputs(M, A, R.loss_seed(M, A), True, **kw)
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}


def largs(d):
    return tuple(P(d[k]) for k in ("mu", "std", "value", "act", "old_logp", "old_mu", "old_sigma", "adv", "ret",
                                   "target", "rows"))


def digest(bufs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for b in bufs:
        h.update(b.view(torch.int16 if b.dtype == BF else b.dtype).cpu().numpy().tobytes())
    return h.hexdigest()


def step_bufs(M, A, Ap):
    return dict(partial=z(L.pmlp_ppo_loss_step_parts(M, A)), stats=z(4), dstd=z(A), dmu=z(M, Ap, dtype=BF),
                dmu_t=z(Ap, M, dtype=BF), dv=z(M, VP, dtype=BF), dv_t=z(VP, M, dtype=BF))


def step(d, M, A, Ap, g, stats=True):
    mm._ok(L.pmlp_ppo_loss_step(*largs(d), M, A, R.CLIP, 1, VCOEF, ECOEF, P(g["partial"]),
                                P(g["stats"]) if stats else None, P(g["dstd"]) if stats else None, P(g["dmu"]),
                                P(g["dmu_t"]), Ap, P(g["dv"]), P(g["dv_t"]), VP, mm._stream()), "pmlp_ppo_loss_step")


def step_f32(d, M, A, g):
    mm._ok(L.pmlp_ppo_loss_step_f32(*largs(d), M, A, R.CLIP, 1, VCOEF, ECOEF, P(g["partial"]), P(g["stats"]),
                                    P(g["dstd"]), P(g["dmu"]), P(g["dv"]), mm._stream()), "pmlp_ppo_loss_step_f32")


def fwd_bwd(d, M, A, g):
    a = largs(d)
    mm._ok(L.pmlp_ppo_loss_fwd(*a, M, A, R.CLIP, 1, VCOEF, ECOEF, P(g["partial"]), P(g["loss"]), P(g["stats"]),
                               mm._stream()), "pmlp_ppo_loss_fwd")
    mm._ok(L.pmlp_ppo_loss_bwd(*a, M, A, R.CLIP, 1, VCOEF, ECOEF, P(g["gout"]), P(g["dmu"]), P(g["dv"]),
                               P(g["pstd"]), P(g["dstd"]), mm._stream()), "pmlp_ppo_loss_bwd")


def fwd_bwd_bufs(M, A):
    nb = L.pmlp_ppo_loss_blocks(M)
    return dict(partial=z(4 * nb), loss=z(1), stats=z(4), dmu=z(M, A), dv=z(M), pstd=z(A * nb), dstd=z(A),
                gout=torch.tensor([0.5], device=dev))


def loss_forward(M, A, Ap, K0, hidden, seed):
    """The two nets and the loss arguments of one pmlp_mlp_forward_ppo_loss launch; mu and value
    of the plain forward stand in the rollout side's construction (as the reference test does)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    rows_cpu = R.loss_inputs(M, A, R.loss_seed(M, A), True)["rows"]
    x = torch.randn(M + R.STORE_EXTRA, K0, generator=gen, device=dev)

    def net(nout):
        ks, ns = [K0] + list(hidden), list(hidden) + [nout]
        W = [(torch.randn(n, k, generator=gen, device=dev) * (1.2 / k ** 0.5)).to(BF).contiguous()
             for n, k in zip(ns, ks)]
        return dict(x=x, kx=K0 - 3, rows=rows_cpu.to(dev), K0=K0, W=W,
                    b=[0.1 * torch.randn(n, generator=gen, device=dev) for n in ns], N=ns, out=z(M, nout))

    jobs = [net(A), net(1)]
    mm.mlp_forward(jobs, M)
    torch.cuda.synchronize()
    d = inputs(M, A, mu=jobs[0]["out"].clone(), value=jobs[1]["out"].clone())
    nparts = L.pmlp_mlp_forward_ppo_loss_parts_k0(M, A, K0)
    g = dict(partial=z(nparts), dmu=z(M, Ap, dtype=BF), dmu_t=z(Ap, M, dtype=BF), dv=z(M, VP, dtype=BF),
             dv_t=z(VP, M, dtype=BF))
    loss = (P(d["std"]), P(d["act"]), P(d["old_logp"]), P(d["old_mu"]), P(d["old_sigma"]), P(d["adv"]), P(d["ret"]),
            P(d["target"]), P(d["rows"]), A, R.CLIP, 1, VCOEF, ECOEF, P(g["partial"]), P(g["dmu"]), P(g["dmu_t"]), Ap,
            P(g["dv"]), P(g["dv_t"]), VP, mm._stream())
    return jobs, d, g, loss


def finish(partial, nb, A, M, std):
    """pmlp_reduce_slabs_step on the step's partials with the optimizer preparation and one slab job."""
    gen = torch.Generator(device=dev).manual_seed(5)
    slab = torch.randint(-16, 17, (3, 37), generator=gen, device=dev).float() / 8
    g = dict(stats=z(4), dstd=z(A), out=z(37), norm=z(8), step=torch.tensor([4.0], device=dev),
             lr=torch.tensor([1e-3], device=dev), acc=torch.tensor([2.0, 3.0], device=dev))
    rs = mm.ReduceStep(P(partial), nb, A, M, ECOEF, P(std), P(g["stats"]), P(g["dstd"]), P(g["norm"]), P(g["step"]),
                       P(g["lr"]), P(g["acc"]), R.DESIRED_KL, 1, 8)
    return g, (lambda: mm._reduce_step([(slab, g["out"], 37, 3)], rs))


def median_us(fn):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 20 * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def show_time(what, fn):
    med, lo, hi = median_us(fn)
    print(f"time {what}: {med:.2f} us (min {lo:.2f}, max {hi:.2f} of 9 x 20)", flush=True)


def digests():
    for arm, cases in (("quad", QUAD), ("reg", REG), ("generic", GENERIC)):
        for A, Ap in cases:
            assert R.loss_arm(A, Ap).startswith(arm), (arm, A, Ap)
            for M in (65, 517):
                d, g = inputs(M, A), step_bufs(M, A, Ap)
                step(d, M, A, Ap, g)
                print(f"digest step {arm} A={A} Ap={Ap} M={M}: {digest(g.values())}", flush=True)
    for A in (12, 10, 20):
        for M in (65, 517):
            d = inputs(M, A)
            g = dict(partial=z(L.pmlp_ppo_loss_step_parts(M, A)), stats=z(4), dstd=z(A), dmu=z(M, A), dv=z(M))
            step_f32(d, M, A, g)
            print(f"digest step_f32 {R.loss_arm(A, 0)} A={A} M={M}: {digest(g.values())}", flush=True)
    for A in (12, 10):
        M = 517
        d, g = inputs(M, A), fwd_bwd_bufs(M, A)
        fwd_bwd(d, M, A, g)
        print(f"digest fwd_bwd A={A} M={M}: {digest(g.values())}", flush=True)
    for K0, form in ((16, "k_mlp_fwd<96, LOSS>"), (80, "k_mlp_fwd<96, LOSS, WIDE>"), (320, "k_mlp_fwd<64, LOSS, WIDER>")):
        jobs, d, g, loss = loss_forward(R.FWD_LOSS_M, 12, 16, K0, (32, 32, 32), K0)
        mm.mlp_forward(jobs, R.FWD_LOSS_M, loss=loss)
        print(f"digest loss forward {form} M={R.FWD_LOSS_M}: {digest([j['out'] for j in jobs] + list(g.values()))}",
              flush=True)
    M, A, Ap = 101, 12, 16
    d, g = inputs(M, A), step_bufs(M, A, Ap)
    step(d, M, A, Ap, g, stats=False)
    gf, run = finish(g["partial"], (M + 63) // 64, A, M, d["std"])
    run()
    print(f"digest reduce_slabs_step finish M={M} A={A}: {digest(gf.values())}", flush=True)


def times():
    M = 24576
    for arm, (A, Ap) in (("quad", (12, 16)), ("reg", (10, 16)), ("generic", (20, 24))):
        d, g = inputs(M, A), step_bufs(M, A, Ap)
        show_time(f"step {arm} A={A} Ap={Ap} M={M}", lambda: step(d, M, A, Ap, g))
    d, g = inputs(M, 12), fwd_bwd_bufs(M, 12)
    show_time(f"fwd_bwd A=12 M={M}", lambda: fwd_bwd(d, M, 12, g))
    jobs, d, g, loss = loss_forward(M, 12, 16, 48, (512, 256, 128), 48)
    show_time(f"loss forward K0=48 512/256/128 M={M}", lambda: mm.mlp_forward(jobs, M, loss=loss))
    gs = step_bufs(M, 12, 16)
    step(d, M, 12, 16, gs, stats=False)
    gf, run = finish(gs["partial"], (M + 63) // 64, 12, M, d["std"])
    show_time(f"reduce_slabs_step finish M={M} A=12", run)


print(f"# {name}", flush=True)
if sys.argv[1:] == ["time"]:
    times()
else:
    digests()
