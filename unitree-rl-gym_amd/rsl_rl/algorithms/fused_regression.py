"""What the fused optimizer steps of two regressions of one Linear/ELU MLP onto per-row targets
share: teacher-student distillation's (distillation.FusedDistillStep) and
random network distillation's (rnd_step.FusedRndStep).

FusedRegressionStep: flat parameter, gradient and Adam-moment buffers over one MLP, its bf16
weight copies (mirror jobs of the Adam launch), the buffers of the one-job pmlp_mlp_forward with
xa / y stores, and everything after the loss kernel has written the output gradient: the paired
weight / input-gradient GEMMs, the slab combine, pmlp_opt_prepare and pmlp_adam_mirror_n.  A
subclass supplies the forward's rows and the loss launch.
"""
import torch
import torch.nn as nn

from rsl_rl.modules import mfma_mlp as mm


def _ceil8(n):
    return (n + 7) // 8 * 8


def _lins(seq):
    return [m for m in seq if isinstance(m, nn.Linear)]


class FusedRegressionStep:
    """One optimizer step of the MLP `net` (its Linear layers `lins`) on M rows.  `optimizer` is
    the torch Adam that holds exactly the net's parameters (its state is pointed at the flat
    moments); `what` names the step in refusals."""

    def __init__(self, net, optimizer, k0p, block_rows, max_out, what):
        if not mm.supported(net):
            raise ValueError(f"{what}: the net must be a Linear/ELU MLP")
        self.lins = _lins(net)
        L = self.L = len(self.lins)
        if L > mm.PMLP_MAX_MIRROR:
            raise ValueError(f"{what}: at most {mm.PMLP_MAX_MIRROR} Linear layers")
        self.A = A = self.lins[-1].out_features
        if A > max_out:
            raise ValueError(f"{what}: at most {max_out} outputs")
        self.k0p = k0p
        if not mm.mlp_forward_supported(self.lins, self.k0p):
            raise ValueError(f"{what}: the fused forward does not take the net's shape")
        params = [p for lin in self.lins for p in (lin.weight, lin.bias)]
        opt_params = [p for g in optimizer.param_groups for p in g["params"]]
        if sorted(map(id, params)) != sorted(map(id, opt_params)):
            raise ValueError(f"{what}: the optimizer must hold the net's parameters alone")
        self.optimizer, self.M = optimizer, int(block_rows)
        if self.M % 8:
            raise ValueError(f"{what}: the block must be a multiple of 8 rows")
        dev = self.dev = params[0].device
        n = self.n = sum(p.numel() for p in params)
        self.flat = torch.empty(n, device=dev)
        self.grad = torch.zeros(n + 4, device=dev)  # tail: [loss of the step, 0, 0, 0]
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        self.step_t = torch.zeros((), device=dev)
        self.params = params
        self._gview, self._mview, self._vview, self._offset = {}, {}, {}, {}
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                v = self.flat[off:off + k].view_as(p)
                v.copy_(p.data)
                p.data = v
                p.grad = self.grad[off:off + k].view_as(p)
                self._gview[id(p)] = p.grad
                self._mview[id(p)] = self.exp_avg[off:off + k].view_as(p)
                self._vview[id(p)] = self.exp_avg_sq[off:off + k].view_as(p)
                self._offset[id(p)] = off
                off += k
        self.stats = self.grad[n:n + 4]
        # the bf16 weight copies lag the fp32 weights (construction, a load): reconverted before use
        self.weights_changed = True
        self.sync_optimizer_state(optimizer)
        self._alloc()

    def _loss_parts(self):
        """The loss kernel's partials for M rows."""
        raise NotImplementedError

    def _alloc(self):
        M, dev, bf, L, lins = self.M, self.dev, torch.bfloat16, self.L, self.lins
        kin = [self.k0p] + [lin.in_features for lin in lins[1:]]  # padded input width per layer
        self.xb = torch.empty(M, self.k0p, dtype=bf, device=dev)
        # W[out, in] in bf16 (the last layer's rows padded to 8 with zeros: the input gradient's K)
        self.wb = [torch.zeros(_ceil8(lin.out_features) if l == L - 1 else lin.out_features, kin[l], dtype=bf,
                               device=dev) for l, lin in enumerate(lins)]
        self.wf = [torch.zeros(-(-w.shape[0] // 32) * 32 * w.shape[1], dtype=bf, device=dev) for w in self.wb]
        self.mirror = (mm.MirrorJob * L)(*[
            mm.MirrorJob(self._offset[id(lin.weight)], lin.out_features, lin.in_features, self.wb[l].shape[1],
                         self.wb[l].data_ptr(), self.wf[l].data_ptr()) for l, lin in enumerate(lins)])
        self.y = [torch.empty(M, lin.out_features, dtype=bf, device=dev) for lin in lins[:-1]]
        self.out = torch.empty(M, self.A, device=dev)
        self.dz_out = torch.empty(M, _ceil8(self.A), dtype=bf, device=dev)
        self.dz = [torch.empty(M, lin.in_features, dtype=bf, device=dev) if l > 0 else None
                   for l, lin in enumerate(lins)]
        self.loss_partial = torch.empty(self._loss_parts(), device=dev)
        self.opt_partial = torch.empty(mm.load().pmlp_opt_parts(), device=dev)
        # split-K weight-gradient slabs (the bias gradient in column kin of each); a first layer
        # padded past the parameter's width combines into a staging buffer
        self.ks, self.slab, self.red, self.copies = [], [], [], []
        for l, lin in enumerate(lins):
            ks = mm._ksplit(M, mm._tiles(lin.out_features, kin[l]), slab_bytes=4 * lin.out_features * (kin[l] + 8))
            self.ks.append(ks)
            self.slab.append(torch.empty((M + ks - 1) // ks, lin.out_features, kin[l] + 8, device=dev))
        for l in range(L - 1, -1, -1):
            lin, slab = lins[l], self.slab[l]
            dw = self._gview[id(lin.weight)]
            if kin[l] != lin.in_features:
                stage = torch.empty(lin.out_features, kin[l], device=dev)
                self.copies.append((dw, stage[:, :lin.in_features]))
                dw = stage
            self.red.append((slab, dw, lin.out_features * (kin[l] + 8), slab.shape[0], self._gview[id(lin.bias)],
                             kin[l] + 8, kin[l]))

    def sync_optimizer_state(self, opt):
        """Point the torch Adam's per-parameter state at the flat moments (after construction or
        an optimizer.load_state_dict, copying loaded values in)."""
        with torch.no_grad():
            for p in self.params:
                st = opt.state.get(p)
                m, v = self._mview[id(p)], self._vview[id(p)]
                if st and st.get("exp_avg") is not None and st["exp_avg"].data_ptr() == m.data_ptr():
                    continue
                if st and "exp_avg" in st:
                    m.copy_(st["exp_avg"])
                    v.copy_(st["exp_avg_sq"])
                    self.step_t.fill_(float(st["step"]))
                opt.state[p] = {"step": self.step_t, "exp_avg": m, "exp_avg_sq": v}
            for p in self.params:  # gradients must alias the flat buffer
                if p.grad is None or p.grad.data_ptr() != self._gview[id(p)].data_ptr():
                    p.grad = self._gview[id(p)]

    def ensure_weights(self):
        """Refresh the net's bf16 weight copies when they lag the fp32 weights (outside any
        captured graph: the captured steps keep them current through the Adam mirror)."""
        if not self.weights_changed:
            return
        mm._convert([(lin.weight.detach(), self.wb[l].shape[1], self.wb[l][:lin.out_features], None)
                     for l, lin in enumerate(self.lins)])
        for wb, wf in zip(self.wb, self.wf):
            wf.copy_(mm.frag_pack(wb, wf.numel() // wb.shape[1]))
        self.weights_changed = False

    def net_job(self, x, **extra):
        """The net's pmlp_mlp_forward job on rows x."""
        lins = self.lins
        return dict(x=x, kx=lins[0].in_features, K0=self.k0p, W=self.wb, Wf=self.wf,
                    b=[lin.bias.detach() for lin in lins], N=[lin.out_features for lin in lins], **extra)

    def forward(self, x, rows=None):
        """One launch, one job; the bf16 input rows and hidden activations are stored for the
        weight gradients.  rows (int64 [M]): the forward gathers x[rows]."""
        extra = {} if rows is None else dict(rows=rows)
        mm.mlp_forward([self.net_job(x, xa=self.xb, y=self.y, out=self.out, **extra)], self.M)

    def backward_and_step(self, lr, acc, max_norm):
        """Everything after the loss kernel has written dz_out and stats: the backward GEMMs, the
        slab combine, the optimizer bookkeeping (acc[1] += stats[0]) and Adam with the bf16
        copies written on the way.  lr: the device learning-rate tensor."""
        M, L, lins = self.M, self.L, self.lins
        lib, P, st = mm.load(), mm._p, mm._stream()
        # backward: a layer's weight gradient (split-K slabs) and input gradient in one launch
        # where their tiles pair
        dz = self.dz_out
        for l in range(L - 1, -1, -1):
            lin = lins[l]
            kp = self.k0p if l == 0 else lin.in_features
            B = self.xb if l == 0 else self.y[l - 1]
            gw = [dict(A=dz, B=B, M=lin.out_features, N=kp, K=M, cf=self.slab[l], sum_col=kp)]
            if l == 0:
                mm._gemm(mm.EPI_PARTIAL_TN, gw, ksplit=self.ks[l])
            else:
                gx = [dict(A=dz, B=self.wb[l], b_kn=1, M=M, N=lin.in_features, K=dz.shape[1], yprev=self.y[l - 1],
                           cb=self.dz[l])]
                mm._gemm_pair(gw, self.ks[l], gx)
                dz = self.dz[l]
        # slab combine + bias sums into the flat gradient
        mm._reduce(self.red)
        for dst, src in self.copies:
            dst.copy_(src)
        # grad-norm partials, Adam's step count and the loss accumulation (stats laid out for
        # this bookkeeping, adaptive off), then Adam with the bf16 copies written on the way
        grp = self.optimizer.param_groups[0]
        b1, b2 = grp.get("betas", (0.9, 0.999))
        eps = grp.get("eps", 1e-8)
        mm._ok(lib.pmlp_opt_prepare(P(self.grad), self.n, 1.0, P(self.opt_partial), P(self.step_t), P(self.stats),
                                    P(lr), P(acc), 0.0, 0, st), "pmlp_opt_prepare")
        mm._ok(lib.pmlp_adam_mirror_n(P(self.flat), P(self.grad), P(self.exp_avg), P(self.exp_avg_sq), self.n, 1.0,
                                      P(self.opt_partial), self.opt_partial.numel(), P(self.step_t), P(lr),
                                      max_norm, float(b1), float(b2), float(eps), len(self.mirror), self.mirror, st),
               "pmlp_adam_mirror_n")
