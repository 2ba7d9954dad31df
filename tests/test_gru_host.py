"""The GRU memory's host side (rsl_rl/modules/gru_seq.py, include/ppo_mlp.h "recurrent memory:
GRU"): the dense statement against torch's nn.GRU, the dense update form against rsl_rl's
padded trajectories, the TorchScript export, the C job struct and argument checks, and the
g1_gru task.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from conftest import ROOT
from fake_env import FakeEnv
from rsl_rl.algorithms import PPO
from rsl_rl.modules import ActorCriticRecurrent, gru_seq

HEADER = os.path.join(ROOT, "include", "ppo_mlp.h")


@pytest.mark.parametrize("I", [17, 47, 64])
def test_reference_is_nn_gru(I):
    """No resets, zero state: gru_dense_reference is nn.GRU (measured: <= 1.5e-7)."""
    torch.manual_seed(I)
    rnn = torch.nn.GRU(I, 64)
    x = torch.randn(7, 37, I)
    with torch.no_grad():
        err = float((gru_seq.gru_dense_reference(rnn, x, None, None) - rnn(x)[0]).abs().max())
    print("reference vs nn.GRU", I, err)
    assert err < 1e-6


def _segments(rnn, x, h0, reset):
    """nn.GRU run segment by segment per env, restarting from zeros at each reset."""
    T, B, _ = x.shape
    out = torch.empty(T, B, rnn.hidden_size)
    for b in range(B):
        h = h0[b].view(1, 1, -1)
        t0 = 0
        cuts = [t for t in range(T) if reset[t, b]] + [T]
        for t1 in cuts:
            if t1 > t0:
                y, h = rnn(x[t0:t1, b:b + 1], h)
                out[t0:t1, b] = y[:, 0]
            h = torch.zeros_like(h)
            t0 = t1
    return out


def test_reference_with_resets_is_nn_gru_by_segments():
    torch.manual_seed(1)
    T, B, I = 7, 5, 11
    rnn = torch.nn.GRU(I, 64)
    x = torch.randn(T, B, I)
    h0 = 0.5 * torch.randn(B, 64)
    reset = torch.zeros(T, B, dtype=torch.uint8)
    reset[2, 0] = reset[3, 0] = 1  # two consecutive steps
    reset[T - 1, 1] = 1
    reset[4, 3] = reset[1, 4] = reset[5, 4] = 1
    with torch.no_grad():
        y = gru_seq.gru_dense_reference(rnn, x, h0, reset)
        torch.testing.assert_close(y, _segments(rnn, x, h0, reset), rtol=0, atol=1e-6)


def test_reset_at_the_first_step_discards_h0():
    torch.manual_seed(2)
    T, B, I = 3, 4, 9
    rnn = torch.nn.GRU(I, 64)
    x = torch.randn(T, B, I)
    h0 = torch.randn(B, 64)
    reset = torch.zeros(T, B, dtype=torch.uint8)
    reset[0, :2] = 1
    with torch.no_grad():
        y = gru_seq.gru_dense_reference(rnn, x, h0, reset)
        y_zero = gru_seq.gru_dense_reference(rnn, x, None, None)
        y_kept = gru_seq.gru_dense_reference(rnn, x, h0, None)
    assert torch.equal(y[:, :2], y_zero[:, :2])
    assert torch.equal(y[:, 2:], y_kept[:, 2:])
    assert not torch.equal(y_kept[:, :2], y_zero[:, :2])


def test_dense_gru_update_equals_padded_trajectories():
    """test_rsl_rl.test_dense_recurrent_update_equals_padded_trajectories for a GRU policy: the
    dense form (forced on: a CPU GRU keeps the padded generator by default) gives the padded
    form's losses and gradients, and Memory.dense runs the reference instead of raising."""
    torch.manual_seed(0)
    env = FakeEnv(num_envs=8, num_privileged_obs=9, ep_len=5)
    ac = ActorCriticRecurrent(6, 9, 3, actor_hidden_dims=[16], critic_hidden_dims=[16], rnn_type="gru",
                              rnn_hidden_size=8, rnn_num_layers=1, init_noise_std=0.8)
    ppo = PPO(ac, num_learning_epochs=1, num_mini_batches=2, device="cpu")
    assert not ppo._dense_recurrent
    ppo.init_storage(8, 12, [6], [9], [3])
    obs, priv = env.reset()
    with torch.inference_mode():
        for it in range(2):  # two rollouts: the second starts from a carried (nonzero) state
            ppo.storage.clear()
            for _ in range(12):
                a = ppo.act(obs, priv)
                obs, priv, r, d, info = env.step(a)
                ppo.process_env_step(r, d, info)
            ppo.compute_returns(priv)
    st = ppo.storage
    assert st.dones.any() and st.saved_hidden_states_a[0][0].abs().sum() > 0
    assert len(st.saved_hidden_states_a) == 1  # a GRU's state is one tensor
    params = list(ac.parameters())
    for (padded, dense) in zip(st.reccurent_mini_batch_generator(2, 1), st.recurrent_dense_mini_batch_generator(2, 1)):
        out = []
        for flag, batch in ((False, padded), (True, dense)):
            ppo._dense_recurrent = flag
            loss, surr, vl = ppo._reference_loss(*batch)
            out.append((loss.detach(), surr.detach(), vl.detach(), torch.autograd.grad(loss, params)))
        (l1, s1, v1, g1), (l2, s2, v2, g2) = out
        torch.testing.assert_close(l2, l1, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(s2, s1, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(v2, v1, rtol=1e-5, atol=1e-6)
        for a, b in zip(g2, g1):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


def test_gru_export(tmp_path):
    import legged_gym.envs  # noqa: F401  (train.py's import order: envs before utils)
    from legged_gym.utils.helpers import export_policy_as_jit
    torch.manual_seed(3)
    ac = ActorCriticRecurrent(47, 50, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_type="gru",
                              rnn_hidden_size=64, rnn_num_layers=1, init_noise_std=0.8)
    export_policy_as_jit(ac, str(tmp_path))
    assert not (tmp_path / "policy_lstm_1.pt").exists()
    m = torch.jit.load(str(tmp_path / "policy_gru_1.pt"))
    m.reset_memory()
    xs = torch.randn(5, 1, 47)
    ac.eval()
    ac.memory_a.hidden_states = None
    with torch.no_grad():
        for x in xs:
            torch.testing.assert_close(m(x), ac.act_inference(x), rtol=1e-5, atol=1e-6)
    assert m.hidden_state.abs().sum() > 0
    m.reset_memory()
    assert m.hidden_state.abs().sum() == 0
    with torch.no_grad():  # and from there it is the first step again
        ac.memory_a.hidden_states = None
        torch.testing.assert_close(m(xs[0]), ac.act_inference(xs[0]), rtol=1e-5, atol=1e-6)


def test_ctypes_gru_job_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ppo_mlp.h"\n'
                   'int main(void){printf("%zu\\n", sizeof(pmlp_gru_job)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    assert int(subprocess.check_output([str(exe)])) == C.sizeof(gru_seq.GruJob)


def _good_job(**kw):
    # non-null pointers that are never dereferenced: the checks fail first
    j = gru_seq.GruJob(47, *([16] * 12))
    for k, v in kw.items():
        setattr(j, k, v)
    return j


@pytest.mark.parametrize("entry,kw,args,msg", [
    ("fwd", dict(), dict(H=128), b"hidden 64"),
    ("fwd", dict(I=0), dict(), b"input 1..64"),
    ("fwd", dict(I=65), dict(), b"input 1..64"),
    ("fwd", dict(), dict(T=0), b"T, B >= 1"),
    ("fwd", dict(), dict(B=0), b"T, B >= 1"),
    ("fwd", dict(), dict(njobs=3), b"1..2 jobs"),
    ("fwd", dict(x=None), dict(), b"null x"),
    ("fwd", dict(w_ih=None), dict(), b"null x"),
    ("fwd", dict(b_hh=None), dict(), b"null x"),
    ("fwd", dict(h_out=None), dict(), b"null x"),
    ("fwd", dict(w_hh=None), dict(), b"null w_hh"),
    ("bwd", dict(), dict(H=32), b"hidden 64"),
    ("bwd", dict(I=65), dict(), b"input 1..64"),
    ("bwd", dict(), dict(T=0), b"T, B >= 1"),
    ("bwd", dict(w_hh=None), dict(), b"null w_hh"),
    ("bwd", dict(gact=None), dict(), b"null gact"),
    ("bwd", dict(xh=None), dict(), b"null gact"),
    ("bwd", dict(dh_out=None), dict(), b"null gact"),
    ("bwd", dict(dg=None), dict(), b"null gact"),
    ("step", dict(), dict(H=128), b"hidden 64"),
    ("step", dict(I=0), dict(), b"input 1..64"),
    ("step", dict(), dict(B=0), b"T, B >= 1"),
    ("step", dict(h_out=None), dict(), b"null x"),
    ("step", dict(b_ih=None), dict(), b"null x"),
])
def test_malformed_gru_jobs_are_refused(entry, kw, args, msg):
    """The entries check their arguments before any HIP call and leave a message."""
    L = gru_seq._lib()
    a = dict(njobs=1, T=3, B=5, H=64)
    a.update(args)
    jobs = (gru_seq.GruJob * 2)(_good_job(**kw), _good_job())
    name = f"pmlp_gru_{entry}_jobs"
    if entry == "step":
        status = L.pmlp_gru_step_jobs(a["njobs"], jobs, a["B"], a["H"], None)
    else:
        status = getattr(L, name)(a["njobs"], jobs, a["T"], a["B"], a["H"], None, None)
    assert status != 0
    err = L.pmlp_lstm_last_error()
    assert name.encode() in err and msg in err, err
    assert L.pmlp_gru_supported(64, 1) and L.pmlp_gru_supported(64, 64)
    assert not L.pmlp_gru_supported(64, 65) and not L.pmlp_gru_supported(128, 47) and not L.pmlp_gru_supported(64, 0)


def test_g1_gru_is_registered():
    import isaacgym  # noqa: F401
    from legged_gym.envs import task_registry
    from legged_gym.utils.helpers import class_to_dict
    assert task_registry.task_classes["g1_gru"] is task_registry.task_classes["g1"]
    env_g, train_g = task_registry.get_cfgs("g1_gru")
    env_l, train_l = task_registry.get_cfgs("g1")
    assert class_to_dict(env_g) == class_to_dict(env_l)
    g, l = class_to_dict(train_g), class_to_dict(train_l)
    assert g["policy"].pop("rnn_type") == "gru" and l["policy"].pop("rnn_type") == "lstm"
    assert g["runner"].pop("experiment_name") == "g1_gru" and l["runner"].pop("experiment_name") == "g1"
    assert g == l
