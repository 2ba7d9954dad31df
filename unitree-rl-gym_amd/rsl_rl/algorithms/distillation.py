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
from rsl_rl.algorithms.fused_regression import FusedRegressionStep, _ceil8, _lins
from rsl_rl.modules import mfma_mlp as mm
from rsl_rl.modules.rnd import parse_cfg as parse_rnd_cfg
from rsl_rl.storage import DistillationStorage
from rsl_rl.utils import capture_without_gc

LOSS_TYPES = ("mse", "huber")


def _net_widths(policy):
    """The padded first-layer widths of (student, teacher): one rule for the update's one-job
    forward and the rollout's two-job forward, so both read the same bf16 weight copies."""
    return mm._pad_k0_nets([_lins(policy.student)[0].in_features, _lins(policy.teacher)[0].in_features])


class FusedDistillStep(FusedRegressionStep):
    """One optimizer step of the student on M = gradient_length x N contiguous storage rows: the
    launches of FusedPPOStep with one job instead of two and the behaviour loss in place of PPO's.
    Flat parameter, gradient and Adam-moment buffers over the student alone (std and the teacher
    are not trained); every weight's bf16 copies are mirror jobs of the Adam launch.  The buffers,
    the backward and the optimizer tail are FusedRegressionStep's (fused_regression.py)."""

    def __init__(self, alg, block_rows):
        pol = alg.actor_critic
        if not (mm.supported(pol.student) and mm.supported(pol.teacher)):
            raise ValueError("fused distillation step: student and teacher must be Linear/ELU MLPs")
        self.alg, self.pol = alg, pol
        self.rollout = None  # the DistillRollout built on this step, if any
        super().__init__(pol.student, alg.optimizer, _net_widths(pol)[0], block_rows, mm.DISTILL_LOSS_MAX_A,
                         "fused distillation step")

    def _loss_parts(self):
        return mm.load().pmlp_distill_loss_parts(self.M)

    def ensure_weights(self):
        """Refresh the student's bf16 weight copies when they lag the fp32 weights (outside any
        captured graph: the captured steps keep them current through the Adam mirror)."""
        if self.rollout is not None:  # (the teacher's copies: the runner refreshes through this step)
            self.rollout.ensure_teacher()
        super().ensure_weights()

    def run(self, obs, target, acc):
        """One optimizer step on the contiguous rows obs [M, O] with the teacher's actions target
        [M, A] (views of the flat storage); acc[1] += the step's loss (the sum of its
        gradient_length per-step mean losses)."""
        alg = self.alg
        self.ensure_weights()
        # 1. forward: one launch, one job; the bf16 input rows and hidden activations are stored
        #    for the weight gradients
        self.forward(obs)
        # 2. the behaviour loss and its gradient, straight into the backward's bf16 operand
        mm.distill_loss_step(self.out, target, alg.loss_type, alg.entry_scale, self.loss_partial, self.stats,
                             self.dz_out)
        # 3. backward GEMMs, slab combine, optimizer bookkeeping and Adam with the bf16 copies
        max_norm = float(alg.max_grad_norm) if alg.max_grad_norm is not None else 0.0
        self.backward_and_step(alg._lr, acc, max_norm)


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
                 loss_type="mse", device="cpu", fused=True, symmetry_cfg=None, rnd_cfg=None, **kwargs):
        if parse_rnd_cfg(rnd_cfg) is not None:
            raise ValueError("Distillation does not support rnd_cfg: behaviour cloning reads no rewards, so an "
                             "exploration bonus has nothing to add to")
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
