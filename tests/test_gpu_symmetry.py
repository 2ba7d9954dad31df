"""PPO's symmetry augmentation on the GPU: pmlp_mirror_rows bit for bit against
numpy and its refusals, the tables against k_step's own symmetry on mirrored pairs of envs
(tests/symmetry_case.py), the fused update on doubled mini-batches against the fp32 autograd
update, the captured update against the eager one on go2_robust_sym, and the scripts."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import symmetry_case as sc  # noqa: E402
from legged_gym.envs import task_registry  # noqa: E402
from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCritic  # noqa: E402
from rsl_rl.modules import mfma_mlp as mm  # noqa: E402
from test_gpu_parity import make  # noqa: E402
from test_gpu_priv_params import _fill_asym  # noqa: E402
from test_symmetry_host import ON, env_like  # noqa: E402
from leggedsim.task import symmetry_tables  # noqa: E402

F = np.float32
SENTINEL = F(-12345.678)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def t2n(t):
    return t.detach().cpu().numpy().copy()


def signed_perm(rng, K):
    return rng.permutation(K).astype(np.int32), rng.choice(np.array([-1.0, 1.0], F), K)


# ------------------------------------------------------------------ kernel ---
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", [1, 12, 48, 87, 240, 427, 448])
def test_mirror_rows_is_bitwise_the_numpy_table_and_writes_nothing_else(K, pad):
    """One launch: a signed permutation, the same permutation with sign +1, and a plain copy of rows
    of another width; ld == K and ld == K + 3; destinations pre-filled with a sentinel, two rows
    longer than R."""
    rng = np.random.default_rng(1000 * K + pad)
    perm, sign = signed_perm(rng, K)
    tab = mm.SignedPermutation(perm, sign, "cuda")
    K2 = 5 if K != 5 else 7
    for R in (1, 63, 64, 65, 1000):
        x = rng.standard_normal((R, K + pad)).astype(F)
        x[rng.random(x.shape) < 0.1] = 0.0   # zeros: a -1 makes them -0
        x2 = rng.standard_normal((R, K2 + pad)).astype(F)
        src, src2 = torch.from_numpy(x).cuda(), torch.from_numpy(x2).cuda()
        dst = [torch.full((R + 2, w + pad), float(SENTINEL), device="cuda") for w in (K, K, K2)]
        mm.mirror_rows([(src[:, :K], dst[0][:, :K], tab), (src[:, :K], dst[1][:, :K], tab.unsigned()),
                        (src2[:, :K2], dst[2][:, :K2], None)], R)
        torch.cuda.synchronize()
        want = [sign * x[:, :K][:, perm], x[:, :K][:, perm], x2[:, :K2]]
        for got, w, width in zip(dst, want, (K, K, K2)):
            got = t2n(got)
            assert np.array_equal(bits(got[:R, :width]), bits(w)), (K, pad, R)
            assert (got[R:] == SENTINEL).all() and (got[:, width:] == SENTINEL).all(), (K, pad, R)
        assert np.array_equal(t2n(src), x)


def test_mirror_rows_refuses_bad_arguments_without_launching():
    lib = mm.load()
    R, K = 16, 12
    src = torch.randn(2 * R, K, device="cuda")
    dst = torch.full((R, K), 7.0, device="cuda")
    tab = mm.SignedPermutation(np.arange(K)[::-1].copy(), np.ones(K, F), "cuda")
    P = mm._p

    def job(src=src, dst=dst, ld=K, K=K, tab=tab):
        return mm.MirrorRowsJob(P(src), P(dst), ld, K, P(tab.perm) if tab else None, P(tab.sign) if tab else None,
                                tab.perm_host if tab else None)

    def status(jobs, rows=R):
        arr = (mm.MirrorRowsJob * len(jobs))(*jobs)
        s = lib.pmlp_mirror_rows(len(jobs), arr, rows, mm._stream())
        return s, lib.pmlp_last_error().decode()

    bad = mm.SignedPermutation(np.array(list(range(K - 1)) + [K], np.int32), np.ones(K, F), "cuda")
    cases = [([job(tab=bad)], -5, f"perm[{K - 1}] = {K} outside 0..{K - 1}"),
             ([job(ld=K - 1)], -4, "ld below K"),
             ([job(dst=src[R // 2:])], -6, "dst overlaps src"),
             ([job(dst=src[R:]), job(dst=src)], -6, "job 1: dst overlaps src"),
             ([job()] * (mm.PMLP_MIRROR_MAX_JOBS + 1), -1, f"1 to {mm.PMLP_MIRROR_MAX_JOBS} jobs"),
             ([job(K=mm.PMLP_MIRROR_MAX_K + 1, ld=mm.PMLP_MIRROR_MAX_K + 1)], -3, "K outside"),
             ([job()], -1, "R < 1")]
    for jobs, code, text in cases:
        s, msg = status(jobs, rows=0 if text == "R < 1" else R)
        assert s == code and "pmlp_mirror_rows" in msg and text in msg, (s, msg)
    no_host = job()
    no_host.perm_host = None
    s, msg = status([no_host])
    assert s == -1 and "host copy" in msg
    torch.cuda.synchronize()
    assert (dst == 7.0).all()                      # nothing was launched
    s, _ = status([job(dst=src[R:])])             # adjacent, not overlapping: accepted
    assert s == 0
    torch.cuda.synchronize()
    assert torch.equal(src[R:], src[:R].flip(1))


# ------------------------------------------------------------ equivariance ---
def test_the_tables_are_k_steps_own_symmetry():
    """The mirrored pairs of tests/symmetry_case.py on the fused env step, placed with
    lgs_set_actor_root_state_indexed / lgs_set_dof_state_indexed, under the host test's bound
    (k_step is bitwise the oracle: no margin of its own).  The privileged row is on (clean frame,
    friction, added mass) and held to the critic row's table."""
    env = make("go2", sc.N, env__privileged_parameters=True, env__num_privileged_obs=50, noise__add_noise=False,
               domain_rand__push_robots=False, domain_rand__randomize_friction=False,
               domain_rand__randomize_base_mass=False, commands__heading_command=False,
               commands__resampling_time=1000.0)
    try:
        env.reset()
        policy, critic, joints = env.symmetry_tables()
        assert len(policy[0]) == 48 and len(critic[0]) == 50
        root, q, qd = sc.initial_state(t2n(env.default_dof_pos), joints, kp=float(env.p_gains[0]),
                                       kd=float(env.d_gains[0]), action_scale=env.cfg.control.action_scale)
        env.root_states.copy_(torch.from_numpy(root))
        env.dof_pos.copy_(torch.from_numpy(q))
        env.dof_vel.copy_(torch.from_numpy(qd))
        ids = torch.arange(sc.N, dtype=torch.int32, device=env.device)
        env.sim.set_root_indexed(env.root_states, ids, sc.N)
        env.sim.set_dof_indexed(env.dof_state, ids, sc.N)
        worst = 0.0
        for step in range(sc.STEPS):
            act, cmd = sc.step_inputs(step, joints, dt=env.dt, action_scale=env.cfg.control.action_scale)
            env.commands.copy_(torch.from_numpy(cmd))
            obs, priv, _, reset, _ = env.step(torch.from_numpy(act).to(env.device))
            torch.cuda.synchronize()
            obs, priv = t2n(obs), t2n(priv)
            assert not reset.any() and (env.root_states[:, 2] > 2.5).all()
            for a in (0, 2):
                assert sc.separation(obs[a], policy) >= sc.SEPARATION, (step, a)
            dev, devp = sc.deviation(obs, policy), sc.deviation(priv, critic)
            print(f"step {step}: max |obs_B - mirror(obs_A)| = {dev:.4e}, privileged {devp:.4e}")
            worst = max(worst, dev, devp)
        print(f"largest deviation {worst:.4e}; bound {sc.BOUND:.4e}")
        assert worst <= sc.BOUND
    finally:
        env.close()


# ------------------------------------------------------------ fused update ---
def _mirror_np(x, tab):
    return x if tab is None else (x[..., tab.perm_np] if tab.sign_np is None else tab.sign_np * x[..., tab.perm_np])


@pytest.mark.parametrize("schedule", ["fixed", "adaptive"])
@pytest.mark.parametrize("O,CO,task", [(48, None, "go2"), (240, 87, "go2_robust_asym")])
def test_fused_update_on_doubled_mini_batches_matches_the_fp32_autograd_update(O, CO, task, schedule):
    """tests/test_gpu_fused_ppo.py's shape (N = 1024, T = 8, 1 epoch x 2 mini-batches) and bars, both
    sides with the augmentation; afterwards the second half of every doubled tensor is the numpy
    mirror image or copy of the first, bitwise."""
    N, T, A = 1024, 8, 12
    tabs = symmetry_tables(env_like(task))
    torch.manual_seed(0)
    ac32 = ActorCritic(O, CO or O, A, [512, 256, 128], [512, 256, 128], mixed_precision=False).cuda()
    acbf = copy.deepcopy(ac32)
    acbf.mixed_precision = True
    kw = dict(num_learning_epochs=1, num_mini_batches=2, learning_rate=1e-3, schedule=schedule, device="cuda")
    plain = PPO(copy.deepcopy(acbf), **kw)
    plain.init_storage(N, T, [O], [CO], [A])
    assert plain._fused.M == N * T // 2 and plain.storage.doubled is None     # off is off
    kw.update(symmetry_cfg=ON, symmetry_tables=tabs)
    ref = PPO(ac32, fused_loss=False, **kw)
    ref.use_graph = False
    fus = PPO(acbf, **kw)
    for alg in (ref, fus):
        alg.init_storage(N, T, [O], [CO], [A])
    assert fus._fused is not None and ref._fused is None and fus._fused.M == N * T
    data = _fill_asym(ref, T, N, O, CO or O, A, seed=1) if CO else None
    if CO is None:
        from test_gpu_fused_ppo import _fill_storage
        data = _fill_storage(ref, T, N, O, A, seed=1)
    for k, v in data.items():
        getattr(fus.storage, k).copy_(v)
    fus.storage.step = T
    p0 = [p.detach().clone() for p in ref.actor_critic.parameters()]
    torch.manual_seed(7)
    l_ref = ref.update()
    torch.manual_seed(7)
    l_fus = fus.update()
    print("losses fused / fp32:", l_fus, l_ref)
    np.testing.assert_allclose(l_fus, l_ref, rtol=2e-2, atol=2e-3)
    assert fus.learning_rate == pytest.approx(ref.learning_rate, rel=1e-6)
    lr = 1e-3
    for a, b, c in zip(ref.actor_critic.parameters(), fus.actor_critic.parameters(), p0):
        da, db = (a.detach() - c), (b.detach() - c)
        assert da.abs().max() > 0
        bad = ((da - db).abs() > 0.2 * lr).float().mean().item()
        assert bad < 0.02, bad
        assert (da - db).abs().max() <= 4 * 3 * lr
    so, scr, sa = fus._sym
    how = dict(observations=so, privileged_observations=scr, actions=sa, mu=sa, sigma=sa.unsigned(), values=None,
               returns=None, advantages=None, actions_log_prob=None)
    st = fus.storage
    assert sorted(st.doubled) == sorted(k for k in how if CO or k != "privileged_observations")
    for name, whole in st.doubled.items():
        first = t2n(getattr(st, name))
        assert getattr(st, name).data_ptr() == whole.data_ptr()
        assert np.array_equal(bits(t2n(whole[:T])), bits(data[name].cpu().numpy())), name   # the rollout's rows
        assert np.array_equal(bits(t2n(whole[T:])), bits(_mirror_np(first, how[name]))), name


def test_captured_autograd_update_with_augmentation_tracks_the_eager_one():
    """fused_loss=False, fp32: the torch statement of the augmented update inside
    _update_graphed's captured graph against the same update eager, on identical rollouts, under
    tests/test_gpu_env.py::test_ppo_graph_tracks_eager_over_many_updates' bound (Adam turns
    rounding-level gradient differences into <= ~lr moves per step)."""
    from test_gpu_fused_ppo import _fill_storage
    N, T, O, A, lr = 256, 8, 48, 12, 1e-3
    tabs = symmetry_tables(env_like("go2"))
    torch.manual_seed(0)
    ac = ActorCritic(O, O, A, [64, 32], [64, 32], mixed_precision=False).cuda()
    algs = []
    for graph in (True, False):
        alg = PPO(copy.deepcopy(ac), num_learning_epochs=2, num_mini_batches=2, learning_rate=lr, schedule="adaptive",
                  device="cuda", fused_loss=False, symmetry_cfg=ON, symmetry_tables=tabs)
        alg.use_graph = graph
        alg.init_storage(N, T, [O], [None], [A])
        assert alg._fused is None and alg.storage.doubled is not None
        algs.append(alg)
    for u in range(4):
        data = _fill_storage(algs[1], T, N, O, A, seed=20 + u)
        for k, v in data.items():
            getattr(algs[0].storage, k).copy_(v)
        algs[0].storage.step = T
        for alg in algs:
            torch.manual_seed(50 + u)
            alg.update()
        pg, pe = (list(a.actor_critic.parameters()) for a in algs)
        assert all(torch.isfinite(p).all() for p in pg)
        d = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(pg, pe))
        assert d < 2 * lr * 4 * (u + 1), f"update {u}: graphed params drifted {d:.3e} from eager"
    assert algs[0]._graph is not None and algs[1]._graph is None
    assert algs[0].learning_rate == pytest.approx(algs[1].learning_rate, rel=1e-6)


# ------------------------------------------------------- captured / eager ----
def _learn(task, graph, iters):
    from legged_gym.utils.helpers import class_to_dict
    from rsl_rl.runners import OnPolicyRunner
    env = make(task, 64, env__episode_length_s=0.3)
    try:
        cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(task)[1]))
        cfg["runner"]["rollout_graph"] = graph
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
        alg = runner.alg
        alg.use_graph = graph
        assert alg._fused is not None and alg._rollout is not None, "native PPO path not active"
        st = alg.storage
        names = ("observations", "privileged_observations", "actions", "values", "rewards", "dones", "returns",
                 "advantages", "actions_log_prob", "mu", "sigma")
        out = []
        for n in iters:
            runner.learn(n)
            env.flush_extras()
            torch.cuda.synchronize()
            out.append(dict(storage=[getattr(st, k).clone() for k in names],
                            params=[p.detach().clone() for p in alg.actor_critic.parameters()]))
        return out, alg
    finally:
        env.close()


def test_go2_robust_sym_captured_equals_eager_and_differs_from_asym_only_in_the_update():
    (g1, g3), alg_g = _learn("go2_robust_sym", True, (1, 2))
    assert alg_g._sym is not None and alg_g._fused.M == 2 * 64 * 24 // 4 and alg_g._fgraph is not None
    (e1, e3), alg_e = _learn("go2_robust_sym", False, (1, 2))
    assert alg_e._fgraph is None
    for got, want in ((g1, e1), (g3, e3)):
        for key in ("storage", "params"):
            assert len(got[key]) == len(want[key])
            for a, b in zip(got[key], want[key]):
                assert torch.equal(a, b), key
    # the rollout does not know about the feature; the update does
    (a1,), alg_a = _learn("go2_robust_asym", True, (1,))
    assert alg_a._sym is None and alg_a._fused.M == 64 * 24 // 4
    for a, b in zip(g1["storage"], a1["storage"]):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(g1["params"], a1["params"]))


# ----------------------------------------------------------------- scripts ---
def test_train_then_play_go2_robust_sym():
    import glob
    import os
    from test_gpu_scripts import run
    exp = "pytest_go2_robust_sym"
    out = run("train.py", "--task", "go2_robust_sym", "--num_envs", "64", "--max_iterations", "3", "--headless",
              "--experiment_name", exp, "--run_name", "cli")
    assert "Learning iteration 2/3" in out
    from legged_gym import LEGGED_GYM_ROOT_DIR
    runs = sorted(glob.glob(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "*_cli")))
    assert runs, "train.py wrote no run directory"
    ck = os.path.join(runs[-1], "model_3.pt")
    assert os.path.exists(ck)
    sd = torch.load(ck, map_location="cpu", weights_only=True)["model_state_dict"]
    assert sd["critic.0.weight"].shape[1] == 87 and sd["actor.0.weight"].shape[1] == 240
    run("play.py", "--task", "go2_robust_sym", "--headless", "--experiment_name", exp, "--load_run",
        os.path.basename(runs[-1]))
    assert os.path.exists(os.path.join(LEGGED_GYM_ROOT_DIR, "logs", exp, "exported", "policies", "policy_1.pt"))
