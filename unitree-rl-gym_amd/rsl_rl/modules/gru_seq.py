"""The GRU memory of ActorCriticRecurrent(rnn_type="gru") on hand-written HIP sequence
kernels (csrc/gru_seq.hip through include/ppo_mlp.h, "recurrent memory: GRU"): the sibling
of lstm_seq.py, in the same dense form -- every env's T steps run in order and h is zeroed
before step t when the env was done at t-1, which is the zero state a padded trajectory that
starts there begins from.

``gru_dense`` is differentiable w.r.t. the four GRU parameters (an autograd Function around
pmlp_gru_fwd_jobs / pmlp_gru_bwd_jobs plus one row-chunked product for the parameter
gradients); ``gru_dense_reference`` is the same recurrence in plain torch ops (any device):
the statement the kernels are checked against, and what a CPU policy runs.
"""
import ctypes as C

import torch

from . import lstm_seq
from . import mfma_mlp as mm

_bound = False


class GruJob(C.Structure):
    """include/ppo_mlp.h pmlp_gru_job: one memory's sequence in a launch of 1..2."""
    _fields_ = [("I", C.c_int32)] + [(n, C.c_void_p) for n in (
        "x", "w_ih", "b_ih", "b_hh", "w_hh", "h0", "h_out", "gact", "xh", "dh_out", "dg", "h_save")]


def _lib():
    global _bound
    L = mm.load()
    if not _bound:
        vp, i32 = C.c_void_p, C.c_int32
        L.pmlp_gru_supported.argtypes = [i32, i32]
        L.pmlp_gru_fwd_jobs.argtypes = [i32, C.POINTER(GruJob), i32, i32, i32, vp, vp]
        L.pmlp_gru_bwd_jobs.argtypes = [i32, C.POINTER(GruJob), i32, i32, i32, vp, vp]
        L.pmlp_gru_step_jobs.argtypes = [i32, C.POINTER(GruJob), i32, i32, vp]
        _bound = True
    return L


_ok = lstm_seq._ok  # (one error text for the LSTM, the GRU and the heads: pmlp_lstm_last_error)


HIDDEN, MAX_INPUT = 64, 64  # pmlp_gru_supported


def usable(rnn, x):
    """The kernels cover a one-layer GRU with bias, hidden 64 and inputs <= 64 on a GPU, fp32."""
    return (x.is_cuda and isinstance(rnn, torch.nn.GRU) and rnn.num_layers == 1 and rnn.bias
            and x.dtype == torch.float32 and rnn.hidden_size == HIDDEN and rnn.input_size <= MAX_INPUT
            and not rnn.batch_first)


class _GRUDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h0, reset, w_ih, w_hh, b_ih, b_hh):
        T, B, I = x.shape
        H = w_hh.shape[1]
        whh = w_hh.detach().contiguous()
        h_out = torch.empty(T, B, H, device=x.device)
        gact = torch.empty(T, B, 4 * H, device=x.device)  # r, z, n, gh_n
        xh = torch.empty(T, B, I + H + 1, device=x.device)  # [x | h_prev | 1]
        p = mm._p
        job = GruJob(I, p(x), p(w_ih.detach().contiguous()), p(b_ih.detach()), p(b_hh.detach()), p(whh), p(h0),
                     p(h_out), p(gact), p(xh))
        _ok(_lib().pmlp_gru_fwd_jobs(1, C.byref(job), T, B, H, p(reset), mm._stream()), "pmlp_gru_fwd_jobs")
        ctx.save_for_backward(xh, reset, whh, gact)
        ctx.I = I
        return h_out

    @staticmethod
    def backward(ctx, dh_out):
        xh, reset, whh, gact = ctx.saved_tensors
        I, p = ctx.I, mm._p
        T, B, _ = xh.shape
        H = whh.shape[1]
        dg = torch.empty(T, B, 4 * H, device=xh.device)  # da_r, da_z, da_n, da_hn
        job = GruJob(I, None, None, None, None, p(whh), None, None, p(gact), p(xh), p(dh_out.contiguous()), p(dg))
        _ok(_lib().pmlp_gru_bwd_jobs(1, C.byref(job), T, B, H, p(reset), mm._stream()), "pmlp_gru_bwd_jobs")
        # all four parameter gradients from ONE product dg^T [x | h_prev | 1] over the T*B rows
        # (fp32, split over the rows): the input side takes the rows of da_r, da_z, da_n, the
        # hidden side those of da_r, da_z, da_hn
        dw = lstm_seq._rows_tn(dg.view(T * B, 4 * H), xh.view(T * B, I + H + 1))
        hid = torch.cat((dw[:2 * H], dw[3 * H:]))
        return (None, None, None, dw[:3 * H, :I].contiguous(), hid[:, I:I + H].contiguous(),
                dw[:3 * H, I + H].contiguous(), hid[:, I + H].contiguous())


def _state(h0, B):
    if h0 is None:
        return None
    if isinstance(h0, (tuple, list)):  # (the storage hands every memory's states as a tuple)
        h0 = h0[0]
    h0 = h0.detach().reshape(B, -1)
    return h0.clone() if h0.is_inference() else h0.contiguous()


def gru_dense(rnn, x, h0, reset):
    """[T,B,I] -> [T,B,H] through rnn (nn.GRU, one layer, usable()) with resets before step t
    where reset[t] != 0; h0 [B,H] (detached: the saved rollout state) or None."""
    reset = None if reset is None else reset.to(torch.uint8).contiguous()
    return _GRUDense.apply(x.contiguous(), _state(h0, x.shape[1]), reset, rnn.weight_ih_l0, rnn.weight_hh_l0,
                           rnn.bias_ih_l0, rnn.bias_hh_l0)


def gru_dense_reference(rnn, x, h0, reset):
    """The same recurrence in torch ops (any device), torch's gate order r, z, n: the n gate
    keeps its hidden part, with b_hn, inside r * (.)."""
    T, B, _ = x.shape
    H = rnn.hidden_size
    h = x.new_zeros(B, H) if h0 is None else _state(h0, B)
    gi = torch.addmm(rnn.bias_ih_l0, x.reshape(T * B, -1), rnn.weight_ih_l0.t()).view(T, B, 3 * H)
    out = []
    for t in range(T):
        if reset is not None:
            h = h * (reset[t] == 0).to(x.dtype).unsqueeze(-1)
        gh = torch.addmm(rnn.bias_hh_l0, h, rnn.weight_hh_l0.t())
        i_r, i_z, i_n = gi[t].chunk(3, dim=-1)
        h_r, h_z, h_n = gh.chunk(3, dim=-1)
        r = torch.sigmoid(i_r + h_r)
        z = torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = (1.0 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


def gru_step_pair_(steps):
    """The memories' rollout step in ONE launch (pmlp_gru_step_jobs: the dense forward's
    kernel at T = 1, so its numbers are the ones the update recomputes).  steps:
    [(rnn, x, h, save)] x 1..2, same batch size; h [1,B,H] static buffers, read and overwritten
    in place (capturable); save (or None) receives the state the step starts from.  Returns
    the h buffers."""
    p = mm._p
    B = steps[0][1].shape[0]
    jobs = (GruJob * len(steps))()
    for n, (rnn, x, h, save) in enumerate(steps):
        jobs[n] = GruJob(x.shape[1], p(x), p(rnn.weight_ih_l0), p(rnn.bias_ih_l0), p(rnn.bias_hh_l0),
                         p(rnn.weight_hh_l0), None, p(h), None, None, None, None, p(save))
    with torch.no_grad():
        _ok(_lib().pmlp_gru_step_jobs(len(steps), jobs, B, steps[0][0].hidden_size, mm._stream()),
            "pmlp_gru_step_jobs")
    return [st[2] for st in steps]
