"""Empirical observation normalisation (rsl_rl's EmpiricalNormalization): running mean and
variance of the observation rows, applied before the policy and the critic see them.

The state is kept in fp64 and the rows are normalised through two fp32 tables,
    mean32 = (float) mean,  inv32 = (float) (1 / (sqrt(var) + eps)),  y = (x - mean32) * inv32,
which is rsl_rl's (x - mean) / (std + eps) with the division replaced by a table.  The update
merges each batch's moments (fp64 sums of d = x - x[0] and d^2) into the state before the rows
are normalised, as rsl_rl does; the arithmetic is stated in include/ppo_mlp.h
(pmlp_obs_norm_step) and restated in torch below.

On a CUDA tensor with the native library `forward` is one pmlp_obs_norm_step call (two
launches; one when frozen) writing into static per-parity output buffers: a captured rollout
replays the calls, and the runner's graph identity test and the policy kernels see fixed
addresses.  Elsewhere (the CPU path) it runs the torch restatement.
"""
import torch
import torch.nn as nn

from . import mfma_mlp


def tables(mean, var, eps):
    """(mean32, inv32) of a state, the fp64 arithmetic of the kernel."""
    return mean.to(torch.float32), (1.0 / (torch.sqrt(var) + eps)).to(torch.float32)


def merge(count, mean, var, x):
    """The state after the rows x [N, D] (fp32): (count', mean', var'), fp64, the kernel's merge."""
    n = float(x.shape[0])
    s = x[0].to(torch.float64)
    d = x.to(torch.float64) - s
    s1, s2 = d.sum(0), (d * d).sum(0)
    mean_x = s + s1 / n
    m2 = torch.clamp(s2 - s1 * s1 / n, min=0.0)
    c = float(count)
    nn_ = c + n
    r = n / nn_
    delta = mean_x - mean
    return int(count) + x.shape[0], mean + delta * r, (var * c + m2 + delta * delta * c * r) / nn_


def apply_rows(x, mean32, inv32):
    """y = (x - mean32) * inv32 in fp32 (two roundings: the kernel's rows bit for bit)."""
    return (x - mean32) * inv32


def _native(x):
    """The kernel path: fp32 CUDA rows (a missing library is an error there, not a fall-back)."""
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1


class EmpiricalNormalization(nn.Module):
    """Normalise rows [N, D] with the running mean and variance of the rows seen so far.
    train() / eval() switch the update on and off; `until`: no update once `count` has
    reached it.  Buffers carry rsl_rl's names, so a plain state_dict round-trips."""

    def __init__(self, shape, eps=1e-2, until=None):
        super().__init__()
        D = int(shape[0] if isinstance(shape, (tuple, list, torch.Size)) else shape)
        self.D, self.eps, self.until = D, float(eps), until
        self.register_buffer("_mean", torch.zeros(1, D, dtype=torch.float64))
        self.register_buffer("_var", torch.ones(1, D, dtype=torch.float64))
        self.register_buffer("_std", torch.ones(1, D, dtype=torch.float32))
        self.register_buffer("count", torch.zeros((), dtype=torch.int64))
        self.register_buffer("mean32", torch.zeros(D, dtype=torch.float32), persistent=False)
        self.register_buffer("inv32", torch.ones(D, dtype=torch.float32), persistent=False)
        self._scratch = None
        self._out, self._parity = None, 0
        self._frozen_out = None

    @property
    def mean(self):
        return self._mean.squeeze(0).clone()

    @property
    def std(self):
        return torch.sqrt(self._var).to(torch.float32).squeeze(0)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        with torch.no_grad():  # _std is derived: the kernels keep _var alone
            self._std.copy_(torch.sqrt(self._var).to(torch.float32))
        super()._save_to_state_dict(destination, prefix, keep_vars)

    # ---- native path ----
    def _static(self, x):
        """The static outputs (one per parity, and one for frozen rows) and the kernel's scratch."""
        N = x.shape[0]
        if self._out is None or self._out[0].shape[0] != N or self._out[0].device != x.device:
            with torch.inference_mode(False):
                self._out = [torch.empty(N, self.D, device=x.device) for _ in range(2)]
                self._frozen_out = torch.empty(N, self.D, device=x.device)
                nbytes = mfma_mlp.load().pmlp_obs_norm_scratch_bytes(self.D)
                if nbytes <= 0:
                    raise RuntimeError(f"EmpiricalNormalization: width {self.D} is past what pmlp_obs_norm_step "
                                       f"is built for ({mfma_mlp.load().pmlp_obs_norm_max_width()})")
                self._scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
            self._parity = 0

    def _job(self, x, frozen):
        if x.shape[1] != self.D:
            raise ValueError(f"EmpiricalNormalization: rows of width {x.shape[1]}, built for {self.D}")
        self._static(x)
        if frozen:
            y = self._frozen_out
        else:
            y = self._out[self._parity]
            self._parity ^= 1
        return dict(x=x, y=y, D=self.D, count=self.count, mean=self._mean, var=self._var, mean32=self.mean32,
                    inv32=self.inv32, scratch=self._scratch)

    # ---- torch restatement ----
    def _torch(self, x, update):
        with torch.no_grad():
            if update and (self.until is None or int(self.count) < self.until):
                count, mean, var = merge(int(self.count), self._mean[0], self._var[0], x)
                self.count.fill_(count)
                self._mean[0].copy_(mean)
                self._var[0].copy_(var)
            m32, i32 = tables(self._mean[0], self._var[0], self.eps)
            self.mean32.copy_(m32)
            self.inv32.copy_(i32)
            return apply_rows(x, self.mean32, self.inv32)

    def forward(self, x):
        """Update (in training mode) and normalise x [N, D]."""
        if _native(x):
            j = self._job(x, frozen=not self.training)
            mfma_mlp.obs_norm_step([j], x.shape[0], self.training, self.until, self.eps)
            return j["y"]
        return self._torch(x, self.training)

    def frozen(self, x):
        """Normalise x with the state as it stands, whatever the mode (inference, and the
        first rows of a learn() call)."""
        if _native(x):
            j = self._job(x, frozen=True)
            mfma_mlp.obs_norm_step([j], x.shape[0], False, self.until, self.eps)
            return j["y"]
        return self._torch(x, False)


def normalize_pair(norm_a, x_a, norm_c, x_c, frozen=False):
    """Actor and privileged rows through their normalisers: ONE native call for both where the
    kernel path applies.  norm_c is norm_a (and x_c is x_a) when the critic reads the actor's
    rows: one job, and the same tensor comes back twice."""
    if norm_c is norm_a:
        y = norm_a.frozen(x_a) if frozen else norm_a(x_a)
        return y, y
    if _native(x_a) and _native(x_c) and x_a.shape[0] == x_c.shape[0] and norm_a.training == norm_c.training \
            and norm_a.until == norm_c.until and norm_a.eps == norm_c.eps:
        frozen = frozen or not norm_a.training
        ja, jc = norm_a._job(x_a, frozen), norm_c._job(x_c, frozen)
        mfma_mlp.obs_norm_step([ja, jc], x_a.shape[0], not frozen, norm_a.until, norm_a.eps)
        return ja["y"], jc["y"]
    if frozen:
        return norm_a.frozen(x_a), norm_c.frozen(x_c)
    return norm_a(x_a), norm_c(x_c)
