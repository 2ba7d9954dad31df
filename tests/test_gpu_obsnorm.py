"""Empirical observation normalisation on the device (csrc/obs_norm.hip, pmlp_obs_norm_step):
the kernels against the fp64 reference and bounds of tests/obsnorm_ref.py, and OnPolicyRunner
with `empirical_normalization` on, eager and captured.  The same comparisons run on the host
against the torch restatement, and are shown to reject wrong outputs, in
tests/test_obsnorm_host.py."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import isaacgym  # noqa: F401,E402
from legged_gym.envs import task_registry  # noqa: E402
from legged_gym.utils import get_args  # noqa: E402
from legged_gym.utils.helpers import class_to_dict  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402
import obsnorm_ref as R  # noqa: E402

DEV = "cuda:0"
BAND = 64
SENT = {torch.float32: 12345.0, torch.float64: -54321.0, torch.int64: -77}


class Banded:
    """A tensor inside a sentinel-filled buffer: `view` is what the kernel is given, and
    untouched() tells whether everything outside it still holds what it held."""

    def __init__(self, rows, cols, ld, dtype, fill=None):
        n = (rows - 1) * ld + cols
        self.full = torch.full((n + 2 * BAND + (ld - cols),), SENT[dtype], dtype=dtype, device=DEV)
        self.view = self.full[BAND:BAND + rows * ld].view(rows, ld)[:, :cols]
        if fill is not None:
            self.view.copy_(fill)
        self.mask = torch.ones_like(self.full, dtype=torch.bool)
        idx = (torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]).reshape(-1) + BAND
        self.mask[idx] = False
        self.before = self.full.clone()

    def untouched(self):
        return torch.equal(self.full[self.mask], self.before[self.mask])


class Job:
    """One pmlp_obs_norm_job over banded buffers, from the initial state."""

    def __init__(self, N, D, ldx, ldy=None):
        self.N, self.D, self.ldx = N, D, ldx
        ldy = D + 3 if ldy is None else ldy
        self.x = torch.full((N, ldx), 7.0, device=DEV)  # columns >= D: never read into the result
        self.y = Banded(N, D, ldy, torch.float32)
        self.count = Banded(1, 1, 1, torch.int64, fill=torch.zeros(1, 1, dtype=torch.int64))
        self.mean = Banded(1, D, D, torch.float64, fill=torch.zeros(1, D, dtype=torch.float64))
        self.var = Banded(1, D, D, torch.float64, fill=torch.ones(1, D, dtype=torch.float64))
        self.mean32 = Banded(1, D, D, torch.float32)
        self.inv32 = Banded(1, D, D, torch.float32)
        self.scratch = torch.empty(mm.load().pmlp_obs_norm_scratch_bytes(D) // 8, dtype=torch.float64, device=DEV)

    def job(self, batch):
        self.x[:, :self.D].copy_(torch.from_numpy(batch))
        return dict(x=self.x[:, :self.D], y=self.y.view, D=self.D, count=self.count.view, mean=self.mean.view,
                    var=self.var.view, mean32=self.mean32.view, inv32=self.inv32.view, scratch=self.scratch)

    def result(self):
        torch.cuda.synchronize()
        return (int(self.count.view), self.mean.view[0].cpu().numpy(), self.var.view[0].cpu().numpy(),
                self.mean32.view[0].cpu().numpy(), self.inv32.view[0].cpu().numpy(), self.y.view.cpu().numpy())

    def untouched(self):
        return all(b.untouched() for b in (self.y, self.count, self.mean, self.var, self.mean32, self.inv32))


def run_kernel(jobs_batches, flags=None, until=None):
    """jobs_batches: [(Job, batches)] (1 or 2, the same N); per job, per call, Job.result()."""
    ncalls = len(jobs_batches[0][1])
    out = [[] for _ in jobs_batches]
    for i in range(ncalls):
        upd = True if flags is None else flags[i]
        mm.obs_norm_step([j.job(b[i]) for j, b in jobs_batches], jobs_batches[0][0].N, upd, until, R.EPS)
        for o, (j, _) in zip(out, jobs_batches):
            o.append(j.result())
            assert j.untouched(), "a write outside the extent of y, the tables or the state"
    return out


def check(batches, got, flags=None, until=None):
    ref = R.run(batches, flags, until)
    for x, (count, mean, var, m32, i32, y), (st, tab) in zip(batches, got, ref):
        R.check_state(count, mean, var, st)
        R.check_tables(m32, i32, tab)
        R.check_rows(y, x, m32, i32)


def bitwise_equal(a, b):
    return all(ra[0] == rb[0] and all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(ra[1:], rb[1:]))
               for ra, rb in zip(a, b))


@pytest.mark.parametrize("N", R.NS)
@pytest.mark.parametrize("D,ldx", R.WIDTHS)
def test_four_calls_against_the_reference(N, D, ldx):
    """Four consecutive calls with fresh batches (the merge runs with count > 0): state and
    tables within the reference's bounds, rows bitwise the fp32 restatement with the call's
    own tables, nothing outside the buffers' extents written, two runs bitwise equal."""
    batches = R.make_sequence(1000 * N + D, N, D)
    got = run_kernel([(Job(N, D, ldx), batches)])[0]
    check(batches, got)
    count, mean, var = got[-1][:3]
    assert count == 4 * N
    for k in range(D):  # constant columns: variance exactly 0, mean exactly the constant
        want = {"const100": np.float32(100.0), "const0.1": np.float32(0.1), "zero": np.float32(0.0)}.get(R.KINDS[k % 5])
        if want is not None:
            assert var[k] == 0.0 and mean[k] == float(want), (k, R.KINDS[k % 5])
    again = run_kernel([(Job(N, D, ldx), batches)])[0]
    assert bitwise_equal(got, again)


def test_single_large_mean_column():
    batches = R.make_sequence(3, 257, 1, offset=3)  # D = 1: the mean-100, spread-1e-3 column
    check(batches, run_kernel([(Job(257, 1, 1), batches)])[0])


@pytest.mark.parametrize("N", [65, 4096])
def test_two_jobs_of_different_width_in_one_call(N):
    ba, bc = R.make_sequence(5, N, 46), R.make_sequence(6, N, 235, offset=2)
    ja, jc = Job(N, 46, 46), Job(N, 235, 236)
    ga, gc = run_kernel([(ja, ba), (jc, bc)])
    check(ba, ga)
    ref_c = R.run(bc)
    for x, (count, mean, var, m32, i32, y), (st, tab) in zip(bc, gc, ref_c):
        R.check_state(count, mean, var, st)
        R.check_tables(m32, i32, tab)
        R.check_rows(y, x, m32, i32)
    # the same states as one job per call
    assert bitwise_equal(ga, run_kernel([(Job(N, 46, 46), ba)])[0])
    assert bitwise_equal(gc, run_kernel([(Job(N, 235, 236), bc)])[0])


@pytest.mark.parametrize("N,D,ldx", [(65, 48, 48), (257, 427, 448)])
def test_until_and_update_off(N, D, ldx):
    batches = R.make_sequence(7, N, D)
    until = 2 * N - 1  # reached between the second and the third call (tested on the device)
    got = run_kernel([(Job(N, D, ldx), batches)], until=until)[0]
    check(batches, got, until=until)
    assert [g[0] for g in got] == [N, 2 * N, 2 * N, 2 * N]
    flags = [True, True, False, True]
    got = run_kernel([(Job(N, D, ldx), batches)], flags)[0]
    check(batches, got, flags)
    assert [g[0] for g in got] == [N, 2 * N, 2 * N, 3 * N]
    got = run_kernel([(Job(N, D, ldx), batches)], [False] * 4)[0]  # the tables of the initial state
    check(batches, got, [False] * 4)
    assert got[-1][0] == 0


def test_refusals_return_errors_without_writing():
    N, D = 65, 48
    j = Job(N, D, D)
    batch = R.make_sequence(9, N, D, ncalls=1)[0]
    good = j.job(batch)
    x0 = j.x.clone()

    def refused(**edit):
        with pytest.raises(RuntimeError, match="pmlp_obs_norm_step"):
            mm.obs_norm_step([dict(good, **edit)], N, True, None, R.EPS)
        torch.cuda.synchronize()
        assert j.untouched() and torch.equal(j.x, x0)
        assert torch.equal(j.y.full, j.y.before) and int(j.count.view) == 0
    refused(y=good["x"])                    # y aliases x
    refused(y=j.x[1:, :D])                  # ... or overlaps it
    refused(D=mm.load().pmlp_obs_norm_max_width() + 1)
    refused(D=0)
    refused(count=None)
    refused(mean=None)
    refused(var=None)
    assert mm.load().pmlp_obs_norm_max_width() >= 512


# ---- the runner ----
def _run(task, n, graph, tmp_path, keep_raw):
    args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.env.episode_length_s = 0.5  # resets inside the rollouts
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    cfg = class_to_dict(train_cfg)
    cfg["runner"].update(rollout_graph=graph, empirical_normalization=True, num_steps_per_env=4)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device=DEV)
    norms = [runner.obs_normalizer] + ([runner.critic_obs_normalizer] if env.num_privileged_obs is not None else [])
    raw, tabs = [], []
    if keep_raw:
        step = env.step

        def wrapped(actions):
            # the tables as the previous step's call left them, then this step's raw rows
            tabs.append([(m.mean32.clone(), m.inv32.clone()) for m in norms])
            out = step(actions)
            raw.append([out[0].clone()] + ([out[1].clone()] if len(norms) > 1 else []))
            return out
        env.step = wrapped
    runner.learn(3, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    st = runner.alg.storage
    res = dict(runner=runner, env=env, norms=norms, raw=raw, tabs=tabs, cfg=cfg,
               st_obs=st.observations.clone(),
               st_cobs=None if st.privileged_observations is None else st.privileged_observations.clone(),
               st_act=st.actions.clone(), st_rew=st.rewards.clone(),
               state=[{k: v.clone() for k, v in m.state_dict().items()} for m in norms],
               params=[p.detach().clone() for p in runner.alg.actor_critic.parameters()],
               captured=runner._rollout_graph is not None)
    return res


@pytest.mark.parametrize("task,n", [("go2", 64), ("g1", 32)])
def test_runner_with_normalisation_eager_and_captured(task, n, tmp_path):
    """3 iterations of 4 steps: the captured rollouts (one eager, then replays) leave storage,
    normaliser state and parameters bitwise those of the eager run; the state is the
    reference's over the raw rows env.step returned; every stored row is the restatement of the
    raw row it came from with that call's tables; a saved and reloaded runner's inference
    policy, fed raw rows, is the trained runner's."""
    e = _run(task, n, False, tmp_path, keep_raw=True)
    g = _run(task, n, True, tmp_path, keep_raw=False)
    assert g["captured"] and not e["captured"]
    assert not getattr(g["runner"], "_rollout_graph_failed", False)
    for k in ("st_obs", "st_cobs", "st_act", "st_rew"):
        assert (e[k] is None and g[k] is None) or torch.equal(e[k], g[k]), k
    for se, sg in zip(e["state"], g["state"]):
        for k in se:
            assert torch.equal(se[k], sg[k]), k
    for a, b in zip(e["params"], g["params"]):
        assert torch.equal(a, b)
    T, iters = 4, 3
    assert len(e["raw"]) == T * iters
    for i, norm in enumerate(e["norms"]):
        assert int(norm.count) == iters * T * n
        rows = [r[i].cpu().numpy() for r in e["raw"]]
        ref = R.run(rows)
        R.check_state(int(norm.count), norm._mean[0].cpu().numpy(), norm._var[0].cpu().numpy(), ref[-1][0])
        R.check_tables(norm.mean32.cpu().numpy(), norm.inv32.cpu().numpy(), ref[-1][1])
        # the last iteration's storage rows t = 0..3 came from the raw rows of steps 7..10, each
        # normalised by its own call (whose tables the next step's wrapper recorded)
        stored = (e["st_obs"], e["st_cobs"])[i].cpu().numpy()
        for t in range(T):
            j = (iters - 1) * T - 1 + t
            m32, i32 = (v.cpu().numpy() for v in e["tabs"][j + 1][i])
            R.check_tables(m32, i32, ref[j][1])
            R.check_rows(stored[t], rows[j], m32, i32)
    # save, load into a fresh runner, inference on raw rows
    path = str(tmp_path / "model.pt")
    e["runner"].save(path)
    torch.manual_seed(1)
    fresh = OnPolicyRunner(g["env"], g["cfg"], log_dir=None, device=DEV)
    fresh.load(path)
    raw = e["raw"][-1][0]
    for r in (e["runner"], fresh):
        for name in ("memory_a", "memory_c"):
            if hasattr(r.alg.actor_critic, name):
                getattr(r.alg.actor_critic, name).hidden_states = None
    with torch.no_grad():
        want = e["runner"].get_inference_policy(device=DEV)(raw).clone()
        got = fresh.get_inference_policy(device=DEV)(raw).clone()
    assert torch.isfinite(want).all() and torch.equal(want, got)
    assert int(fresh.obs_normalizer.count) == iters * T * n  # inference does not update
    for r in (e, g):
        r["env"].close()
