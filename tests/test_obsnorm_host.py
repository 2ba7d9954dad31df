"""Empirical observation normalisation on the host: the torch restatement
(rsl_rl/modules/normalizer.py) against the fp64 reference and bounds of tests/obsnorm_ref.py on
the kernel test's cases, the comparison functions against deliberately wrong outputs, and the
Python surface (state dict, eval(), export, runner cfg).  The kernel itself:
tests/test_gpu_obsnorm.py."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import obsnorm_ref as R  # noqa: E402
from fake_env import FakeEnv  # noqa: E402
from rsl_rl.modules.normalizer import EmpiricalNormalization, normalize_pair  # noqa: E402
from rsl_rl.runners import OnPolicyRunner  # noqa: E402


def _restatement(batches, flags=None, until=None):
    """Per call: (count, mean, var, mean32, inv32, y) of the torch restatement."""
    norm = EmpiricalNormalization([batches[0].shape[1]], eps=R.EPS, until=until)
    out = []
    for i, x in enumerate(batches):
        norm.train(True if flags is None else flags[i])
        y = norm(torch.from_numpy(x))
        out.append((int(norm.count), norm._mean[0].numpy().copy(), norm._var[0].numpy().copy(),
                    norm.mean32.numpy().copy(), norm.inv32.numpy().copy(), y.numpy().copy()))
    return out


def _check(batches, got, flags=None, until=None):
    ref = R.run(batches, flags, until)
    for x, (count, mean, var, m32, i32, y), (st, tab) in zip(batches, got, ref):
        R.check_state(count, mean, var, st)
        R.check_tables(m32, i32, tab)
        R.check_rows(y, x, m32, i32)


@pytest.mark.parametrize("N", R.NS)
@pytest.mark.parametrize("D,ldx", R.WIDTHS)
def test_restatement_passes_the_reference_comparison(N, D, ldx):
    batches = R.make_sequence(1000 * N + D, N, D)
    got = _restatement(batches)
    _check(batches, got)
    count, mean, var = got[-1][:3]
    assert count == 4 * N
    for k in range(D):  # constant columns: variance exactly 0, mean exactly the constant
        kind = R.KINDS[k % 5]
        if kind in ("const100", "const0.1", "zero"):
            want = {"const100": np.float32(100.0), "const0.1": np.float32(0.1), "zero": np.float32(0.0)}[kind]
            assert var[k] == 0.0 and mean[k] == float(want), (k, kind)


def test_restatement_until_and_frozen_sequences():
    N, D = 65, 48
    batches = R.make_sequence(7, N, D)
    # `until` reached between the second and the third call
    _check(batches, _restatement(batches, until=2 * N - 1), until=2 * N - 1)
    assert _restatement(batches, until=2 * N - 1)[-1][0] == 2 * N
    # update 0 on the third call, and from a fresh state
    flags = [True, True, False, True]
    _check(batches, _restatement(batches, flags), flags)
    _check(batches, _restatement(batches, [False] * 4), [False] * 4)


def test_single_large_mean_column():
    batches = R.make_sequence(3, 257, 1, offset=3)  # D = 1: the mean-100, spread-1e-3 column
    _check(batches, _restatement(batches))


# ---- the comparison functions reject wrong outputs ----
def _case():
    N, D = 257, 48
    batches = R.make_sequence(11, N, D)
    return batches, _restatement(batches), R.run(batches)


def test_rejects_a_mean_one_fp32_ulp_off():
    batches, got, ref = _case()
    count, mean, var = got[-1][:3]
    k = 1  # the constant-100 column
    bad = mean.copy()
    bad[k] = float(np.nextafter(np.float32(mean[k]), np.float32(np.inf)))
    R.check_state(count, mean, var, ref[-1][0])
    with pytest.raises(AssertionError, match="mean"):
        R.check_state(count, bad, var, ref[-1][0])
    k = 0  # an ordinary column
    bad = mean.copy()
    bad[k] = mean[k] + float(np.spacing(np.float32(mean[k])))
    with pytest.raises(AssertionError, match="mean"):
        R.check_state(count, bad, var, ref[-1][0])


def test_rejects_a_variance_from_unshifted_fp32_sums():
    batches, got, ref = _case()
    x = batches[0]
    k = 3  # mean 100, spread 1e-3
    assert R.KINDS[k % 5] == "mean100"
    s1 = np.float32(0.0)
    s2 = np.float32(0.0)
    for v in x[:, k]:
        s1 = np.float32(s1 + v)
        s2 = np.float32(s2 + np.float32(v * v))
    n = np.float32(len(x))
    naive = max(float(np.float32(s2 / n) - np.float32(np.float32(s1 / n) * np.float32(s1 / n))), 0.0)
    count, mean, var = got[0][:3]
    bad = var.copy()
    bad[k] = naive
    R.check_state(count, mean, var, ref[0][0])
    with pytest.raises(AssertionError, match="var"):
        R.check_state(count, mean, bad, ref[0][0])
    tab = R.tables(ref[0][0])
    with pytest.raises(AssertionError, match="inv32"):
        i32 = got[0][4].copy()
        i32[k] = np.float32(1.0 / (np.sqrt(naive) + R.EPS))
        R.check_tables(got[0][3], i32, tab)


def test_rejects_an_update_after_until():
    N, D = 65, 48
    batches = R.make_sequence(7, N, D)
    wrong = _restatement(batches)  # never frozen
    ref = R.run(batches, until=2 * N - 1)
    R.check_state(*wrong[1][:3], ref[1][0])
    with pytest.raises(AssertionError, match="count"):
        R.check_state(*wrong[2][:3], ref[2][0])


def test_rejects_rows_from_the_pre_update_tables():
    batches, got, ref = _case()
    m32_prev, i32_prev = got[0][3], got[0][4]
    x = batches[1]
    stale = R.rows(x, m32_prev, i32_prev)
    R.check_rows(got[1][5], x, got[1][3], got[1][4])
    with pytest.raises(AssertionError, match="differ"):
        R.check_rows(stale, x, got[1][3], got[1][4])


# ---- module surface ----
def test_state_dict_round_trip_and_names():
    norm = EmpiricalNormalization([6])
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        norm(3.0 + 2.0 * torch.randn(16, 6, generator=g))
    sd = norm.state_dict()
    assert set(sd) == {"_mean", "_var", "_std", "count"}
    assert sd["_mean"].dtype == torch.float64 and sd["_mean"].shape == (1, 6)
    assert sd["_var"].dtype == torch.float64 and sd["_var"].shape == (1, 6)
    assert sd["_std"].dtype == torch.float32 and sd["count"].dtype == torch.int64 and int(sd["count"]) == 48
    assert torch.equal(sd["_std"], torch.sqrt(sd["_var"]).float())
    other = EmpiricalNormalization([6])
    other.load_state_dict(sd)
    x = torch.randn(5, 6, generator=g)
    assert torch.equal(other.eval()(x), norm.eval()(x))
    assert not list(norm.parameters())


def test_eval_freezes_the_state():
    norm = EmpiricalNormalization([4])
    g = torch.Generator().manual_seed(1)
    norm(torch.randn(8, 4, generator=g))
    before = {k: v.clone() for k, v in norm.state_dict().items()}
    norm.eval()
    y = norm(5.0 + torch.randn(8, 4, generator=g))
    for k, v in norm.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert y.mean() > 1.0
    norm.train()
    norm(torch.randn(8, 4, generator=g))
    assert int(norm.count) == 16
    # frozen() never updates, whatever the mode
    norm.frozen(torch.randn(8, 4, generator=g))
    assert int(norm.count) == 16


def test_two_job_helper_matches_single_calls():
    g = torch.Generator().manual_seed(2)
    xa, xc = torch.randn(8, 4, generator=g), torch.randn(8, 7, generator=g)
    a1, c1, a2, c2 = (EmpiricalNormalization([d]) for d in (4, 7, 4, 7))
    ya, yc = normalize_pair(a1, xa, c1, xc)
    assert torch.equal(ya, a2(xa)) and torch.equal(yc, c2(xc))
    ya, yc = normalize_pair(a1, xa, a1, xa)
    assert ya is yc and int(a1.count) == 16


def _cfg(policy="ActorCritic", **runner):
    cfg = {"runner": {"policy_class_name": policy, "algorithm_class_name": "PPO", "num_steps_per_env": 8,
                      "save_interval": 50, **runner},
           "algorithm": {"num_learning_epochs": 1, "num_mini_batches": 2, "learning_rate": 1e-3},
           "policy": {"actor_hidden_dims": [16], "critic_hidden_dims": [16], "activation": "elu", "init_noise_std": 1.0}}
    if policy == "ActorCriticRecurrent":
        cfg["policy"].update(rnn_type="lstm", rnn_hidden_size=8, rnn_num_layers=1)
    return cfg


class _ShiftedEnv(FakeEnv):
    """FakeEnv with observations far from zero mean / unit scale."""

    def step(self, actions):
        out = super().step(actions)
        self.obs_buf = self.obs_buf * 3.0 + 10.0
        return (self.obs_buf,) + tuple(out[1:])


@pytest.mark.parametrize("policy", ["ActorCritic", "ActorCriticRecurrent"])
def test_exported_jit_module_reproduces_act_inference_on_raw_rows(policy, tmp_path):
    import legged_gym.envs  # noqa: F401  (train.py's import order: envs before utils)
    from legged_gym.utils.helpers import export_policy_as_jit
    env = _ShiftedEnv(num_envs=8)
    runner = OnPolicyRunner(env, _cfg(policy, empirical_normalization=True), log_dir=None, device="cpu")
    runner.learn(2)
    ac = runner.alg.actor_critic
    assert int(ac.obs_normalizer.count) == 2 * 8 * 8
    assert float(ac.obs_normalizer._mean.mean()) > 5.0
    pol = runner.get_inference_policy()
    export_policy_as_jit(ac, str(tmp_path))
    name = "policy_1.pt" if policy == "ActorCritic" else "policy_lstm_1.pt"
    mod = torch.jit.load(str(tmp_path / name))
    g = torch.Generator().manual_seed(3)
    if policy == "ActorCritic":
        raw = 10.0 + 3.0 * torch.randn(5, env.num_obs, generator=g)
        with torch.no_grad():
            assert torch.allclose(mod(raw), pol(raw), rtol=0, atol=1e-6)
            unnormalised = ac.actor(raw)
        assert not torch.allclose(unnormalised, pol(raw), atol=1e-3)
    else:
        ac.memory_a.hidden_states = None
        mod.reset_memory()
        for _ in range(3):  # the exported module keeps its own state: one env, step by step
            raw = 10.0 + 3.0 * torch.randn(1, env.num_obs, generator=g)
            with torch.no_grad():
                assert torch.allclose(mod(raw), pol(raw), rtol=0, atol=1e-6)
    assert int(ac.obs_normalizer.count) == 2 * 8 * 8  # inference never updates


def test_runner_option_off_has_no_normalizer_and_the_same_keys(tmp_path):
    env = FakeEnv(num_envs=8)
    off = OnPolicyRunner(env, _cfg(), log_dir=None, device="cpu")
    assert off.obs_normalizer is None and not hasattr(off.alg.actor_critic, "obs_normalizer")
    keys = set(off.alg.actor_critic.state_dict())
    assert keys == {"std", "actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias", "critic.0.weight",
                    "critic.0.bias", "critic.2.weight", "critic.2.bias"}
    on = OnPolicyRunner(env, _cfg(empirical_normalization=True, empirical_normalization_until=100), log_dir=None,
                        device="cpu")
    ac = on.alg.actor_critic
    assert ac.obs_normalizer is ac.critic_obs_normalizer and ac.obs_normalizer.until == 100
    extra = {f"{m}.{b}" for m in ("obs_normalizer", "critic_obs_normalizer") for b in ("_mean", "_var", "_std", "count")}
    assert set(ac.state_dict()) == keys | extra
    assert [id(p) for p in ac.parameters()] == [id(p) for p in on.alg.optimizer.param_groups[0]["params"]]
    on.learn(1)
    on.save(str(tmp_path / "m.pt"))
    with pytest.raises(RuntimeError, match="[Uu]nexpected key"):
        off.load(str(tmp_path / "m.pt"))
    again = OnPolicyRunner(env, _cfg(empirical_normalization=True), log_dir=None, device="cpu")
    again.load(str(tmp_path / "m.pt"))
    assert int(again.obs_normalizer.count) == 64 and torch.equal(again.obs_normalizer._mean, on.obs_normalizer._mean)
    # privileged observations: a module of its own for the critic
    priv = OnPolicyRunner(FakeEnv(num_envs=8, num_privileged_obs=9), _cfg(empirical_normalization=True),
                          log_dir=None, device="cpu")
    assert priv.critic_obs_normalizer is not priv.obs_normalizer and priv.critic_obs_normalizer.D == 9
    priv.learn(1)
    assert int(priv.obs_normalizer.count) == int(priv.critic_obs_normalizer.count) == 64
    # the cfg keys are part of the base train cfg, off by default
    import legged_gym.envs  # noqa: F401
    from legged_gym.envs.base.legged_robot_config import LeggedRobotCfgPPO
    assert LeggedRobotCfgPPO.runner.empirical_normalization is False
    assert LeggedRobotCfgPPO.runner.empirical_normalization_until is None


def test_stored_rows_are_the_normalised_env_rows():
    """The rollout stores, and compute_returns sees, normalised rows: each stored row is the
    restatement of the raw env row it came from, with the tables of that step."""
    env = _ShiftedEnv(num_envs=8)
    runner = OnPolicyRunner(env, _cfg(empirical_normalization=True), log_dir=None, device="cpu")
    raw = []
    step = env.step

    def wrapped(actions):
        out = step(actions)
        raw.append(out[0].numpy().copy())
        return out
    env.step = wrapped
    first = env.get_observations().numpy().copy()
    runner.learn(1)
    st = runner.alg.storage.observations.numpy()
    ref = R.run(raw)
    # row 0: the rows the env held at the start, normalised with the initial state (not counted)
    init = R.State(env.num_obs)
    R.check_rows(st[0], first, *R.tables(init))
    for t in range(1, 8):
        m32, i32 = R.tables(ref[t - 1][0])
        got = st[t]
        want = R.rows(raw[t - 1], m32, i32)
        # the reference's tables may sit 1 fp32 ulp from the module's: |dy| <= ulp(mean32) |inv32| + 2^-23 |y|,
        # plus the two roundings of the row arithmetic
        tol = 2 * np.spacing(np.abs(m32)) * np.abs(i32) + np.abs(want) * 2.0 ** -21
        assert (np.abs(got - want) <= tol).all()
    R.check_state(int(runner.obs_normalizer.count), runner.obs_normalizer._mean[0].numpy(),
                  runner.obs_normalizer._var[0].numpy(), ref[-1][0])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, "..", "unitree-rl-gym_amd"), here]
    from fake_env import FakeEnv as Env
    from rsl_rl.runners import OnPolicyRunner as Runner
    try:
        Runner(Env(num_envs=8), _cfg(empirical_normalization=True), log_dir=None, device="cpu")
        res = "accepted"
    except ValueError as e:
        res = str(e)
    Runner(Env(num_envs=8), _cfg(), log_dir=None, device="cpu")  # the option off: as before
    q.put((rank, res))
    dist.destroy_process_group()


def test_world_size_two_refuses_the_option():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all("world size" in r for _, r in res), res
