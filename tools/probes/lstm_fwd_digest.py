"""Digests and times the matrix-core LSTM sequence kernels (csrc/lstm_seq.hip: k_lstm_fwd8 in its
x-fed and gx-fed forms, k_lstm_bwd_mfma) with the libppomlp.so named by PPOMLP_LIB, for a bitwise
and a speed comparison of two builds.  Digests (SHA-256 over every output buffer, fixed seed):
two memories, I = 47 / 50 and 234 / 237, T = 24, B = 100 with resets inside, and one in-place
step at B = 8213 (4 tiles per workgroup, a ragged last one).  Medians: the update's shape
(T = 24, B = 2048 per memory) and the rollout's (T = 1, B = 4096 and 8192).
usage: [PPOMLP_LIB=...] python tools/probes/lstm_fwd_digest.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "unitree-rl-gym_amd"))
import torch  # noqa: E402
from rsl_rl.modules import lstm_seq as ls  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402

H = 64
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
L, P, st = ls._lib(), mm._p, torch.cuda.current_stream().cuda_stream
name = os.path.basename(os.environ.get("PPOMLP_LIB", "libppomlp.so"))


def rn(*s, scale=1.0):
    return scale * torch.randn(*s, device=dev, generator=g)


def z(*s):
    return torch.zeros(*s, device=dev)


def make(Is, T, B):
    """Two memories' inputs, weights and output buffers at (T, B); reset[0, :7] = 1 and 10% inside."""
    reset = (torch.rand(T, B, device=dev, generator=g) < 0.1).to(torch.uint8)
    reset[0, :7] = 1
    ms = []
    for I in Is:
        m = dict(I=I, x=rn(T, B, I), w_ih=rn(4 * H, I, scale=0.1), b_ih=rn(4 * H, scale=0.1), b_hh=rn(4 * H, scale=0.1),
                 w_hh=rn(4 * H, H, scale=0.1), h0=rn(B, H, scale=0.5), c0=rn(B, H, scale=0.5), dh_out=rn(T, B, H),
                 h_out=z(T, B, H), c_out=z(T, B, H), gact=z(T, B, 4 * H), h_save=z(B, H), c_save=z(B, H))
        if I <= 64:
            m.update(xh=z(T, B, I + H + 1), slab=z(L.pmlp_lstm_bwd_dw_blocks(B), 4 * H * (I + H + 1)))
        else:
            m.update(gx=z(T, B, 4 * H), hp=z(T, B, H + 1), dgx=z(T, B, 4 * H),
                     slab=z(L.pmlp_lstm_bwd_dw_blocks(B), 4 * H * (H + 1)),
                     slab_ih=z(L.pmlp_lstm_wide_dw_blocks(T, B), 4 * H * I))
        ms.append(m)
    return reset, ms


def seq_jobs(ms):
    if ms[0]["I"] <= 64:
        return (ls.LstmJob * 2)(*[ls.LstmJob(m["I"], P(m["x"]), P(m["w_ih"]), P(m["b_ih"]), P(m["b_hh"]), P(m["w_hh"]),
                                             P(m["h0"]), P(m["c0"]), P(m["h_out"]), P(m["c_out"]), P(m["gact"]),
                                             P(m["xh"]), P(m["dh_out"]), P(m["slab"]), None, None) for m in ms])
    return (ls.LstmWideJob * 2)(*[ls.LstmWideJob(m["I"], P(m["x"]), P(m["w_ih"]), P(m["b_ih"]), P(m["b_hh"]),
                                                 P(m["w_hh"]), P(m["h0"]), P(m["c0"]), P(m["h_out"]), P(m["c_out"]),
                                                 P(m["gact"]), P(m["gx"]), P(m["hp"]), P(m["dh_out"]), P(m["dgx"]),
                                                 P(m["slab"]), P(m["slab_ih"]), None, None) for m in ms])


def step_jobs(ms):
    """The in-place step on h0 / c0 (T = 1), the state it starts from saved."""
    if ms[0]["I"] <= 64:
        return (ls.LstmJob * 2)(*[ls.LstmJob(m["I"], P(m["x"]), P(m["w_ih"]), P(m["b_ih"]), P(m["b_hh"]), P(m["w_hh"]),
                                             None, None, P(m["h0"]), P(m["c0"]), None, None, None, None,
                                             P(m["h_save"]), P(m["c_save"])) for m in ms])
    return (ls.LstmWideJob * 2)(*[ls.LstmWideJob(m["I"], P(m["x"]), P(m["w_ih"]), P(m["b_ih"]), P(m["b_hh"]),
                                                 P(m["w_hh"]), None, None, P(m["h0"]), P(m["c0"]), None, P(m["gx"]),
                                                 None, None, None, None, None, P(m["h_save"]), P(m["c_save"]))
                                  for m in ms])


def calls(wide):
    fwd, bwd, step = ((L.pmlp_lstm_fwd_wide_jobs, L.pmlp_lstm_bwd_wide_jobs, L.pmlp_lstm_step_wide_jobs) if wide else
                      (L.pmlp_lstm_fwd_mfma_jobs, L.pmlp_lstm_bwd_dw_mfma_jobs, L.pmlp_lstm_step_mfma_jobs))
    tag = "wide" if wide else "mfma"
    return tag, fwd, bwd, step


def digest(ms, keys):
    torch.cuda.synchronize()
    d = hashlib.sha256()
    for m in ms:
        for k in keys:
            d.update(m[k].cpu().numpy().tobytes())
    return d.hexdigest()


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
    return ts[len(ts) // 2]


print(f"# {name}", flush=True)
for wide, Is in ((False, (47, 50)), (True, (234, 237))):
    tag, fwd, bwd, step = calls(wide)
    T, B = 24, 100
    reset, ms = make(Is, T, B)
    jobs = seq_jobs(ms)
    ls._ok(fwd(2, jobs, T, B, H, P(reset), st), "fwd")
    print(f"digest fwd_{tag}_jobs T={T} B={B}: "
          f"{digest(ms, ('h_out', 'c_out', 'gact') + (('gx', 'hp') if wide else ('xh',)))}", flush=True)
    ls._ok(bwd(2, jobs, T, B, H, P(reset), st), "bwd")
    print(f"digest bwd_{tag}_jobs T={T} B={B}: {digest(ms, ('dgx', 'slab', 'slab_ih') if wide else ('slab',))}",
          flush=True)
    B = 8213
    _, ms = make(Is, 1, B)
    ls._ok(step(2, step_jobs(ms), B, H, st), "step")
    print(f"digest step_{tag}_jobs B={B}: "
          f"{digest(ms, ('h0', 'c0', 'h_save', 'c_save') + (('gx',) if wide else ()))}", flush=True)

for wide, Is in ((False, (47, 50)), (True, (234, 237))):
    tag, fwd, bwd, step = calls(wide)
    T, B = 24, 2048
    reset, ms = make(Is, T, B)
    jobs = seq_jobs(ms)
    tf = median_us(lambda: ls._ok(fwd(2, jobs, T, B, H, P(reset), st), "fwd"))
    tb = median_us(lambda: ls._ok(bwd(2, jobs, T, B, H, P(reset), st), "bwd"))
    print(f"time fwd_{tag}_jobs T={T} B={B}: {tf:.1f} us", flush=True)
    print(f"time bwd_{tag}_jobs T={T} B={B}: {tb:.1f} us", flush=True)
    for B in (4096, 8192):
        _, ms = make(Is, 1, B)
        sj = step_jobs(ms)
        ts = median_us(lambda: ls._ok(step(2, sj, B, H, st), "step"))
        print(f"time step_{tag}_jobs B={B}: {ts:.1f} us", flush=True)
