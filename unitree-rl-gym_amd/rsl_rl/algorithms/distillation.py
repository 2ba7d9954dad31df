"""Teacher-student distillation (rsl_rl 2.x `Distillation`, feed-forward student).

A frozen teacher that reads the privileged row labels every rollout step with its action; the
student, which reads only the policy row, is regressed onto those labels (behaviour cloning):

    act(obs, teacher_obs):  store (obs_t, teacher(teacher_obs_t)); return a sample of N(student(obs_t), std)
    update():               per epoch, over the steps in time order: loss_t = mse | huber(delta=1) of
                            student(obs_t) against the stored teacher actions (a mean over N x A entries);
                            the losses of `gradient_length` consecutive steps are summed, backpropagated
                            and stepped with Adam (clipped only when max_grad_norm is set)

One optimizer step is therefore one contiguous block of gradient_length x N storage rows, every
entry scaled by 1 / (N A): no permutation, no gather.

Two statements of the update:
* the plain path (`_update_plain`): the loop above in fp32 torch autograd, on any device.  It is
  the reference, as PPO._reference_loss is for PPO.
* the fused path (`FusedDistillStep`, with `DistillRollout` for acting): the library's bf16
  matrix-core kernels with one job per launch and the two kernels of csrc/distill.hip, captured
  as one HIP graph of T / gradient_length x epochs optimizer steps.  It needs T % gradient_length
  == 0 (a block never straddles an epoch boundary) and a student the fused forward takes; else
  the plain path runs.
"""
import warnings

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from rsl_rl.algorithms.fused_step import noise_seed
from rsl_rl.modules import mfma_mlp as mm
from rsl_rl.storage import DistillationStorage
from rsl_rl.utils import capture_without_gc

LOSS_TYPES = ("mse", "huber")


def _ceil8(n):
    return (n + 7) // 8 * 8


def _lins(seq):
    return [m for m in seq if isinstance(m, nn.Linear)]


def _net_widths(policy):
    """The padded first-layer widths of (student, teacher): one rule for the update's one-job
    forward and the rollout's two-job forward, so both read the same bf16 weight copies."""
    return mm._pad_k0_nets([_lins(policy.student)[0].in_features, _lins(policy.teacher)[0].in_features])


class FusedDistillStep:
    """One optimizer step of the student on M = gradient_length x N contiguous storage rows: the
    launches of FusedPPOStep with one job instead of two and the behaviour loss in place of PPO's.
    Flat parameter, gradient and Adam-moment buffers over the student alone (std and the teacher
    are not trained); every weight's bf16 copies are mirror jobs of the Adam launch."""

    def __init__(self, alg, block_rows):
        pol = alg.actor_critic
        if not (mm.supported(pol.student) and mm.supported(pol.teacher)):
            raise ValueError("fused distillation step: student and teacher must be Linear/ELU MLPs")
        self.lins = _lins(pol.student)
        L = self.L = len(self.lins)
        if L > mm.PMLP_MAX_MIRROR:
            raise ValueError(f"fused distillation step: at most {mm.PMLP_MAX_MIRROR} Linear layers")
        self.A = A = self.lins[-1].out_features
        if A > mm.DISTILL_LOSS_MAX_A:
            raise ValueError(f"fused distillation step: at most {mm.DISTILL_LOSS_MAX_A} actions")
        self.k0p = _net_widths(pol)[0]
        if not mm.mlp_forward_supported(self.lins, self.k0p):
            raise ValueError("fused distillation step: the fused forward does not take the student's shape")
        params = [p for lin in self.lins for p in (lin.weight, lin.bias)]
        opt_params = [p for g in alg.optimizer.param_groups for p in g["params"]]
        if sorted(map(id, params)) != sorted(map(id, opt_params)):
            raise ValueError("fused distillation step: the optimizer must hold the student's parameters alone")
        self.alg, self.pol, self.M = alg, pol, int(block_rows)
        if self.M % 8:
            raise ValueError("fused distillation step: the block must be a multiple of 8 rows")
        dev = self.dev = pol.std.device
        n = self.n = sum(p.numel() for p in params)
        self.flat = torch.empty(n, device=dev)
        self.grad = torch.zeros(n + 4, device=dev)  # tail: [behaviour loss of the step, 0, 0, 0]
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
        self.rollout = None  # the DistillRollout built on this step, if any
        self.sync_optimizer_state(alg.optimizer)
        self._alloc()

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
        self.loss_partial = torch.empty(mm.load().pmlp_distill_loss_parts(M), device=dev)
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
        """Refresh the student's bf16 weight copies when they lag the fp32 weights (outside any
        captured graph: the captured steps keep them current through the Adam mirror)."""
        if self.rollout is not None:  # (the teacher's copies: the runner refreshes through this step)
            self.rollout.ensure_teacher()
        if not self.weights_changed:
            return
        mm._convert([(lin.weight.detach(), self.wb[l].shape[1], self.wb[l][:lin.out_features], None)
                     for l, lin in enumerate(self.lins)])
        for wb, wf in zip(self.wb, self.wf):
            wf.copy_(mm.frag_pack(wb, wf.numel() // wb.shape[1]))
        self.weights_changed = False

    def net_job(self, x, **extra):
        """The student's pmlp_mlp_forward job on rows x."""
        lins = self.lins
        return dict(x=x, kx=lins[0].in_features, K0=self.k0p, W=self.wb, Wf=self.wf,
                    b=[lin.bias.detach() for lin in lins], N=[lin.out_features for lin in lins], **extra)

    def run(self, obs, target, acc):
        """One optimizer step on the contiguous rows obs [M, O] with the teacher's actions target
        [M, A] (views of the flat storage); acc[1] += the step's loss (the sum of its
        gradient_length per-step mean losses)."""
        alg, M, L, lins = self.alg, self.M, self.L, self.lins
        lib, P, st = mm.load(), mm._p, mm._stream()
        self.ensure_weights()
        # 1. forward: one launch, one job; the bf16 input rows and hidden activations are stored
        #    for the weight gradients
        mm.mlp_forward([self.net_job(obs, xa=self.xb, y=self.y, out=self.out)], M)
        # 2. the behaviour loss and its gradient, straight into the backward's bf16 operand
        mm.distill_loss_step(self.out, target, alg.loss_type, alg.entry_scale, self.loss_partial, self.stats,
                             self.dz_out)
        # 3. backward: a layer's weight gradient (split-K slabs) and input gradient in one launch
        #    where their tiles pair
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
        # 4. slab combine + bias sums into the flat gradient
        mm._reduce(self.red)
        for dst, src in self.copies:
            dst.copy_(src)
        # 5. grad-norm partials, Adam's step count and the loss accumulation (stats laid out for
        #    this bookkeeping, adaptive off), then Adam with the bf16 copies written on the way
        grp = alg.optimizer.param_groups[0]
        b1, b2 = grp.get("betas", (0.9, 0.999))
        eps = grp.get("eps", 1e-8)
        mm._ok(lib.pmlp_opt_prepare(P(self.grad), self.n, 1.0, P(self.opt_partial), P(self.step_t), P(self.stats),
                                    P(alg._lr), P(acc), 0.0, 0, st), "pmlp_opt_prepare")
        max_norm = float(alg.max_grad_norm) if alg.max_grad_norm is not None else 0.0
        mm._ok(lib.pmlp_adam_mirror_n(P(self.flat), P(self.grad), P(self.exp_avg), P(self.exp_avg_sq), self.n, 1.0,
                                      P(self.opt_partial), self.opt_partial.numel(), P(self.step_t), P(alg._lr),
                                      max_norm, float(b1), float(b2), float(eps), len(self.mirror), self.mirror, st),
               "pmlp_adam_mirror_n")


class DistillRollout:
    """Distillation.act on the GPU in two launches per env step: ONE pmlp_mlp_forward of two jobs
    (student on the observations, teacher on the privileged row), then pmlp_distill_act (the
    sample, the two storage rows, the draw counter).  The teacher's bf16 weight copies live here:
    converted once, and again after a load (teacher_changed).  Nothing is deferred, so the env
    keeps its own extras launch (runner cfg defer_env_extras = False): one launch more per step
    than PPO's rollout."""

    pending = None  # (the runner's rollout graph restores a deferred store: there is none)

    def __init__(self, step: FusedDistillStep, num_envs):
        self.f = step
        pol = step.pol
        self.N = N = int(num_envs)
        dev, bf = step.dev, torch.bfloat16
        self.tlins = _lins(pol.teacher)
        self.tk0p = _net_widths(pol)[1]
        A = step.A
        if self.tlins[-1].out_features != A or A > mm.DISTILL_ACT_MAX_A:
            raise ValueError(f"distillation rollout: student and teacher share at most {mm.DISTILL_ACT_MAX_A} actions")
        if not mm.mlp_forward_supported(self.tlins, self.tk0p):
            raise ValueError("distillation rollout: the fused forward does not take the teacher's shape")
        L = len(self.tlins)
        self.twb = [torch.zeros(_ceil8(lin.out_features) if l == L - 1 else lin.out_features,
                                self.tk0p if l == 0 else lin.in_features, dtype=bf, device=dev)
                    for l, lin in enumerate(self.tlins)]
        self.twf = [torch.zeros(-(-w.shape[0] // 32) * 32 * w.shape[1], dtype=bf, device=dev) for w in self.twb]
        self.teacher_changed = True
        self.out = [torch.empty(N, A, device=dev) for _ in range(2)]  # student mean, teacher action
        self.actions = torch.empty(N, A, device=dev)
        # the k-th act samples with draw[k % 2] and sets draw[(k + 1) % 2] (FusedRollout's scheme)
        self.draw = torch.zeros(2, dtype=torch.int64, device=dev)
        self.k = 0
        self.seed = noise_seed()
        step.rollout = self

    def ensure_teacher(self):
        if not self.teacher_changed:
            return
        mm._convert([(lin.weight.detach(), self.twb[l].shape[1], self.twb[l][:lin.out_features], None)
                     for l, lin in enumerate(self.tlins)])
        for wb, wf in zip(self.twb, self.twf):
            wf.copy_(mm.frag_pack(wb, wf.numel() // wb.shape[1]))
        self.teacher_changed = False

    def usable(self, obs, tobs, storage):
        ok = lambda t, w: (t is not None and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and  # noqa: E731
                           t.shape == (self.N, w) and t.is_contiguous())
        return ok(obs, self.f.lins[0].in_features) and ok(tobs, self.tlins[0].in_features) and \
            storage.num_envs == self.N

    def teacher_job(self, x, out):
        t = self.tlins
        return dict(x=x, kx=t[0].in_features, K0=self.tk0p, W=self.twb, Wf=self.twf,
                    b=[lin.bias.detach() for lin in t], N=[lin.out_features for lin in t], out=out)

    def act(self, obs, tobs, storage, t):
        self.f.ensure_weights()  # (the student's copies and, through the step, the teacher's)
        par = self.k % 2
        self.k += 1
        mm.mlp_forward([self.f.net_job(obs, out=self.out[0]), self.teacher_job(tobs, self.out[1])], self.N)
        mm.distill_act(self.out[0], self.out[1], self.f.pol.std.detach(), obs, self.draw, par, self.seed,
                       self.actions, storage.observations[t], storage.privileged_actions[t])
        return self.actions

    def flush(self, storage):
        pass  # nothing is deferred


class Distillation:
    def __init__(self, policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None,
                 loss_type="mse", device="cpu", fused=True, symmetry_cfg=None, **kwargs):
        if kwargs:
            print("Distillation.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("Distillation is single-process: a torch.distributed world size above 1 is not supported")
        sym = dict(symmetry_cfg or {})
        if sym.get("use_data_augmentation", False) or sym.get("use_mirror_loss", False):
            raise ValueError("Distillation does not support symmetry_cfg (the mirrored rows belong to PPO's update)")
        if getattr(policy, "is_recurrent", False) or not hasattr(policy, "student") or \
                any(isinstance(m, nn.RNNBase) for m in policy.modules()):
            raise ValueError("Distillation needs a feed-forward StudentTeacher: a recurrent student or teacher is "
                             "not supported")
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"Distillation: unknown loss_type {loss_type!r} (known: {list(LOSS_TYPES)})")
        if int(gradient_length) < 1:
            raise ValueError("Distillation: gradient_length >= 1")
        self.device = device
        self.actor_critic = self.policy = policy
        self.policy.to(self.device)
        self.storage = None
        self.num_learning_epochs = int(num_learning_epochs)
        self.gradient_length = int(gradient_length)
        self.max_grad_norm = max_grad_norm
        self.loss_type = loss_type
        self._loss_fn = F.mse_loss if loss_type == "mse" else (lambda a, b: F.huber_loss(a, b, delta=1.0))
        self._lr = torch.tensor(float(learning_rate), device=self.device)
        on_gpu = str(self.device).startswith("cuda")
        params = list(self.policy.student.parameters())  # std and the teacher are never in the optimizer
        self.optimizer = None
        if on_gpu:
            for kw in (dict(fused=True, capturable=True), dict(foreach=True, capturable=True)):
                try:
                    self.optimizer = optim.Adam(params, lr=self._lr, **kw)
                    break
                except (RuntimeError, TypeError, ValueError):
                    continue
        if self.optimizer is None:
            self.optimizer = optim.Adam(params, lr=float(learning_rate))
        self._lr_is_tensor = torch.is_tensor(self.optimizer.param_groups[0]["lr"])
        self.transition = DistillationStorage.Transition()
        self.world_size = 1
        self.use_graph = on_gpu and self.optimizer.defaults.get("capturable", False)
        self._want_fused = bool(fused) and on_gpu
        self._fused = None    # FusedDistillStep, built with the storage
        self._rollout = None  # DistillRollout
        self._stored_t = None
        self._fgraph = None
        self._facc = None
        self._update_calls = 0
        self.entry_scale = None  # 1 / (N A): a step's loss is the mean over its entries

    @property
    def learning_rate(self):
        return float(self._lr)

    @learning_rate.setter
    def learning_rate(self, v):
        self._lr.fill_(float(v))
        if not self._lr_is_tensor:
            for g in self.optimizer.param_groups:
                g["lr"] = float(v)

    def init_storage(self, num_envs, num_transitions_per_env, obs_shape, teacher_obs_shape, action_shape):
        self.storage = DistillationStorage(num_envs, num_transitions_per_env, obs_shape, action_shape, self.device)
        T, G = num_transitions_per_env, self.gradient_length
        self.entry_scale = 1.0 / (num_envs * action_shape[0])
        self._fused = self._rollout = None
        if self._want_fused and getattr(self.policy, "mixed_precision", False) and T % G == 0:
            try:
                self._fused = FusedDistillStep(self, G * num_envs)
            except ValueError:  # a shape the kernels do not take: the plain path runs
                self._fused = None
        if self._fused is not None and num_envs % 8 == 0:
            try:
                self._rollout = DistillRollout(self._fused, num_envs)
            except ValueError:
                self._rollout = None

    def test_mode(self):
        self.policy.eval()

    def train_mode(self):
        self.policy.train()

    def teacher_loaded(self):
        """After policy.load_state_dict: the rollout's bf16 copies of both nets lag the weights."""
        if self._fused is not None:
            self._fused.weights_changed = True
        if self._rollout is not None:
            self._rollout.teacher_changed = True

    def act(self, obs, teacher_obs):
        ro, st = self._rollout, self.storage
        if ro is not None and ro.usable(obs, teacher_obs, st):
            t = st.step
            if t >= st.num_transitions_per_env:
                raise AssertionError("Rollout buffer overflow")
            self._stored_t = t
            return ro.act(obs, teacher_obs, st, t)
        self.transition.observations = obs
        self.transition.privileged_actions = self.policy.evaluate(teacher_obs).detach()
        return self.policy.act(obs).detach()

    def process_env_step(self, rewards, dones, infos):
        job = infos.get("_deferred_extras") if isinstance(infos, dict) else None
        if job is not None:  # the env left its extras to a consumer: nothing here rides along, so run them
            job.run()
        t, self._stored_t = self._stored_t, None
        if t is not None and t == self.storage.step:  # the fused act wrote the rows itself
            self.storage.step += 1
        else:
            self.transition.dones = dones
            self.storage.add_transitions(self.transition)
        self.transition.clear()
        self.policy.reset(dones)

    def compute_returns(self, last_obs):
        pass  # behaviour cloning has no returns

    def flush_rollout(self):
        pass

    # ------------------------------------------------------------------ update --
    def update(self, host_means=True):
        """The distillation update; returns the mean per-step behaviour loss (a Python float, or
        with host_means=False the device tensor)."""
        if not getattr(self.policy, "loaded_teacher", False):
            raise ValueError("Distillation.update: teacher model parameters not loaded (load a teacher checkpoint "
                             "before training the student)")
        self._update_calls += 1
        T = self.storage.num_transitions_per_env
        if self._fused is not None:
            total = self._update_fused()
        else:
            total = self._update_plain()
        mean = total / float(T * self.num_learning_epochs)
        self.storage.clear()
        return float(mean) if host_means else mean

    def _update_plain(self):
        """rsl_rl's loop, literally, in fp32 autograd (the reference of the fused path)."""
        st = self.storage
        student = self.policy.student
        total = torch.zeros((), device=self.device)
        loss, cnt = 0.0, 0
        for _ in range(self.num_learning_epochs):
            self.policy.reset()
            for t in range(st.num_transitions_per_env):
                actions = student(st.observations[t])
                behavior_loss = self._loss_fn(actions, st.privileged_actions[t])
                loss = loss + behavior_loss
                total += behavior_loss.detach()
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    if self.max_grad_norm:
                        nn.utils.clip_grad_norm_(student.parameters(), self.max_grad_norm)
                    self.optimizer.step()
                    loss = 0.0
        if self._fused is not None:  # (a caller that ran this next to the fused step)
            self._fused.weights_changed = True
        return total

    def _update_fused(self):
        """T / gradient_length x epochs FusedDistillStep.run calls over the storage's contiguous
        blocks, replayed as one HIP graph from the second call on."""
        f, st = self._fused, self.storage
        f.sync_optimizer_state(self.optimizer)
        f.ensure_weights()
        if self._facc is None:
            self._facc = torch.zeros(2, device=self.device)
        obs, tgt = st.observations.flatten(0, 1), st.privileged_actions.flatten(0, 1)
        M = f.M
        blocks = obs.shape[0] // M

        def body():
            self._facc.zero_()
            for _ in range(self.num_learning_epochs):
                for b in range(blocks):
                    f.run(obs[b * M:(b + 1) * M], tgt[b * M:(b + 1) * M], self._facc)

        if not (self.use_graph and self._update_calls >= 2):
            body()
            return self._facc[1]
        if self._fgraph is None:
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            graph = torch.cuda.CUDAGraph()
            try:
                with capture_without_gc(), torch.cuda.graph(graph, stream=side):
                    body()
            except RuntimeError as e:  # nothing inside a failed capture has executed
                warnings.warn(f"Distillation: capturing the update failed ({e}); updating eagerly")
                torch.cuda.synchronize(self.device)
                self.use_graph = False
                body()
                return self._facc[1]
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._fgraph = graph
        self._fgraph.replay()
        return self._facc[1]
