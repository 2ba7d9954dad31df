"""The fused pieces of random network distillation: the predictor's optimizer step
on a PPO mini-batch's gathered rows (FusedRndStep, a FusedRegressionStep) and the once-per-rollout
reward pass (RndRewardPass).  `supported` is the one test of whether a pair of nets takes them; it
is made before anything is built, because building a step re-points the predictor's parameters
and its optimizer's state at flat buffers.
"""
import numpy as np
import torch

from rsl_rl.algorithms.fused_regression import FusedRegressionStep, _ceil8, _lins
from rsl_rl.algorithms.fused_step import _first_layer_pads
from rsl_rl.modules import mfma_mlp as mm


def rnd_k0(num_states):
    """The padded first-layer width of the two RND nets (one width for both): fused_step's rule
    for nets of one width (87 -> 96, 274 -> 320)."""
    return _first_layer_pads([num_states, num_states])[0]


def supported(rnd, block_rows):
    """None when FusedRndStep and RndRewardPass take the nets of `rnd` at mini-batches of
    block_rows rows, else the reason they do not.  Builds and changes nothing."""
    k0p = rnd_k0(rnd.num_states)
    for name, net in (("predictor", rnd.predictor), ("target", rnd.target)):
        if not mm.supported(net):
            return f"the {name} is not a Linear/ELU MLP with hidden widths in multiples of 8"
        lins = _lins(net)
        if len(lins) > mm.PMLP_MAX_MIRROR:
            return f"the {name} has more than {mm.PMLP_MAX_MIRROR} Linear layers"
        if lins[-1].out_features != rnd.num_outputs or rnd.num_outputs > mm.RND_MAX_E:
            return f"the {name} has more than {mm.RND_MAX_E} outputs"
        if not mm.mlp_forward_supported(lins, k0p):
            return (f"the one-launch forward does not take the {name}'s shape ({rnd.num_states} -> {k0p} inputs, "
                    f"layers {[lin.out_features for lin in lins]}: three hidden layers of at most 512 / 256 / 512 "
                    "in multiples of 32)")
    if int(block_rows) % 8:
        return f"a mini-batch of {block_rows} rows is no multiple of 8"
    return None


class FusedRndStep(FusedRegressionStep):
    """One optimizer step of the RND predictor on the M gathered rows of a PPO mini-batch: the
    launches of FusedDistillStep with a gathered forward and pmlp_rnd_loss_step, whose target is
    the stored target output of the reward pass read through the same index."""

    def __init__(self, rnd, optimizer, lr, block_rows):
        self.rnd, self._lr = rnd, lr
        super().__init__(rnd.predictor, optimizer, rnd_k0(rnd.num_states), block_rows, mm.RND_MAX_E,
                         "fused RND step")
        self.entry_scale = float(np.float32(1.0 / (self.M * self.A)))

    def _loss_parts(self):
        return mm.load().pmlp_rnd_parts(self.M)

    def run(self, idx, state_src, tgt_all, acc):
        """One optimizer step on the rows state_src[idx] (state_src: the flat storage [R, S], idx
        int64 [M]) against tgt_all[idx]; acc[1] += the step's mean squared error."""
        self.ensure_weights()
        self.forward(state_src, rows=idx)
        mm.rnd_loss_step(self.out, tgt_all, idx, self.entry_scale, self.loss_partial, self.stats, self.dz_out)
        self.backward_and_step(self._lr, acc, 0.0)


class RndRewardPass:
    """The bonus of every row of a finished rollout in three launches: ONE pmlp_mlp_forward of two
    jobs (predictor, target) over the T x N flat storage rows, then pmlp_rnd_reward's two.  The
    target's bf16 copies live here: converted once, and again after a load (target_changed); the
    predictor's are the step's, kept current by its Adam launch.  tgt_all stays for the update."""

    def __init__(self, step: FusedRndStep, T, N):
        self.f, self.T, self.N = step, int(T), int(N)
        rnd = step.rnd
        dev, bf = step.dev, torch.bfloat16
        self.tlins = _lins(rnd.target)
        self.k0p = step.k0p
        E = step.A
        if not mm.supported(rnd.target) or self.tlins[-1].out_features != E or \
                not mm.mlp_forward_supported(self.tlins, self.k0p):
            raise ValueError("RND reward pass: the fused forward does not take the target's shape")
        L = len(self.tlins)
        self.twb = [torch.zeros(_ceil8(lin.out_features) if l == L - 1 else lin.out_features,
                                self.k0p if l == 0 else lin.in_features, dtype=bf, device=dev)
                    for l, lin in enumerate(self.tlins)]
        self.twf = [torch.zeros(-(-w.shape[0] // 32) * 32 * w.shape[1], dtype=bf, device=dev) for w in self.twb]
        self.target_changed = True
        R = self.T * self.N
        self.pred = torch.empty(R, E, device=dev)
        self.tgt_all = torch.empty(R, E, device=dev)
        self.w = torch.zeros(self.T, device=dev)
        self._w_host = None
        self.intrinsic = None  # (a caller that wants the per-row bonus allocates it)
        self.partial = torch.empty(2 * mm.load().pmlp_rnd_parts(R), device=dev)
        self.stats = torch.zeros(2, device=dev)

    def ensure_target(self):
        if not self.target_changed:
            return
        mm._convert([(lin.weight.detach(), self.twb[l].shape[1], self.twb[l][:lin.out_features], None)
                     for l, lin in enumerate(self.tlins)])
        for wb, wf in zip(self.twb, self.twf):
            wf.copy_(mm.frag_pack(wb, wf.numel() // wb.shape[1]))
        self.target_changed = False

    def set_weights(self, weights):
        """The per-step weights w[T] of this iteration (a constant schedule uploads once)."""
        weights = [float(x) for x in weights]
        if weights != self._w_host:
            self.w.copy_(torch.tensor(weights, dtype=torch.float32), non_blocking=False)
            self._w_host = weights

    def run(self, states, rewards):
        """states: the flat storage rows [T N, S]; rewards: the storage's rewards [T, N, 1], added
        to in place."""
        self.f.ensure_weights()
        self.ensure_target()
        t = self.tlins
        R = self.T * self.N
        mm.mlp_forward([self.f.net_job(states, out=self.pred),
                        dict(x=states, kx=t[0].in_features, K0=self.k0p, W=self.twb, Wf=self.twf,
                             b=[lin.bias.detach() for lin in t], N=[lin.out_features for lin in t],
                             out=self.tgt_all)], R)
        mm.rnd_reward(self.pred, self.tgt_all, self.w, self.T, self.N, rewards, self.intrinsic, self.partial,
                      self.stats)
