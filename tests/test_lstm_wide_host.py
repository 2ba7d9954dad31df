"""Host side of the wide-input LSTM path: the `g1_terrain_scan` registration,
the shapes `fused_recurrent.supported()` takes, the C ABI of the wide entries (declared,
exported, the job struct's layout) and their argument checks, which run before any HIP call.
No GPU."""
import ctypes as C
import os
import subprocess

import pytest

import isaacgym  # noqa: F401
import legged_gym.envs  # noqa: F401  (task registration)
from conftest import ROOT
from legged_gym.utils import task_registry

HEADER = os.path.join(ROOT, "include", "ppo_mlp.h")
ENTRIES = ("pmlp_lstm_wide_max_input", "pmlp_lstm_wide_dw_blocks", "pmlp_lstm_fwd_wide_jobs",
           "pmlp_lstm_bwd_wide_jobs", "pmlp_lstm_step_wide_jobs")


def test_g1_terrain_scan_is_registered_with_the_scan_in_its_rows():
    from legged_gym.envs.g1.g1_config import G1RoughCfgPPO, G1TerrainCfg, G1TerrainScanCfg
    from legged_gym.envs.g1.g1_env import G1Robot
    from leggedsim.task import terrain_switches
    assert task_registry.get_task_class("g1_terrain_scan") is G1Robot
    env_cfg, train_cfg = task_registry.get_cfgs("g1_terrain_scan")
    assert isinstance(env_cfg, G1TerrainScanCfg) and isinstance(env_cfg, G1TerrainCfg)
    assert isinstance(train_cfg, G1RoughCfgPPO) and train_cfg.runner.experiment_name == "g1_terrain_scan"
    assert train_cfg.runner.policy_class_name == "ActorCriticRecurrent"
    assert env_cfg.terrain.scan_in_observations and terrain_switches(env_cfg) == (True, True, True)
    assert (env_cfg.env.num_observations, env_cfg.env.num_privileged_obs) == (47 + 187, 50 + 187)
    # g1_terrain keeps its 47 / 50 rows
    plain, plain_train = task_registry.get_cfgs("g1_terrain")
    assert not getattr(plain.terrain, "scan_in_observations", False)
    assert (plain.env.num_observations, plain.env.num_privileged_obs) == (47, 50)
    assert plain_train.runner.experiment_name == "g1"


def test_fused_recurrent_step_takes_wide_memories_at_hidden_64_only():
    from rsl_rl.algorithms import fused_recurrent
    from rsl_rl.modules import ActorCriticRecurrent, lstm_seq

    def ac(obs, priv, hidden):
        return ActorCriticRecurrent(obs, priv, 12, actor_hidden_dims=[32], critic_hidden_dims=[32], rnn_type="lstm",
                                    rnn_hidden_size=hidden, rnn_num_layers=1)

    assert fused_recurrent.supported(ac(234, 237, 64), 64, 4)
    assert fused_recurrent.supported(ac(47, 237, 64), 64, 4)  # a narrow actor next to a wide critic
    assert fused_recurrent.supported(ac(384, 384, 64), 64, 4)
    assert not fused_recurrent.supported(ac(385, 385, 64), 64, 4)
    assert not fused_recurrent.supported(ac(234, 385, 64), 64, 4)
    assert not fused_recurrent.supported(ac(234, 237, 32), 64, 4)
    assert not fused_recurrent.supported(ac(234, 237, 128), 64, 4)
    assert fused_recurrent.supported(ac(47, 50, 32), 64, 4)
    assert lstm_seq._lib().pmlp_lstm_wide_max_input() == lstm_seq.WIDE_MAX_INPUT == 384


def test_header_declares_and_library_exports_the_wide_entries(tmp_path):
    from rsl_rl.modules import lstm_seq
    src = open(HEADER).read()
    L = lstm_seq._lib()
    for name in ENTRIES:
        assert "PMLP_API" in src and f" {name}(" in src, name
        assert hasattr(L, name), name
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include "ppo_mlp.h"\nint main(void){printf("%zu %zu\\n",'
                 ' sizeof(pmlp_lstm_wide_job), sizeof(pmlp_lstm_job)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.dirname(HEADER), "-o", str(exe), str(c)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(lstm_seq.LstmWideJob), C.sizeof(lstm_seq.LstmJob)]
    names = [f[0] for f in lstm_seq.LstmWideJob._fields_]
    assert names == ["I", "x", "w_ih", "b_ih", "b_hh", "w_hh", "h0", "c0", "h_out", "c_out", "gact", "gx", "hp",
                     "dh_out", "dgx", "slab", "slab_ih", "h_save", "c_save"]
    assert L.pmlp_lstm_wide_dw_blocks(24, 1024) == 48 and L.pmlp_lstm_wide_dw_blocks(5, 37) == 1


def _full_job(I):
    """Every buffer non-null and aligned (never dereferenced: the checks fail first)."""
    from rsl_rl.modules import lstm_seq
    j = lstm_seq.LstmWideJob()
    j.I = I
    for name, _ in lstm_seq.LstmWideJob._fields_[1:]:
        setattr(j, name, 64)
    return j


@pytest.mark.parametrize("entry", ["fwd", "bwd", "step"])
def test_wide_entries_refuse_bad_arguments_before_any_launch(entry):
    from rsl_rl.modules import lstm_seq
    L = lstm_seq._lib()

    def call(njobs, jobs, H=64):
        arr = (lstm_seq.LstmWideJob * 3)(*jobs)
        if entry == "step":
            return L.pmlp_lstm_step_wide_jobs(njobs, arr, 37, H, None)
        fn = L.pmlp_lstm_fwd_wide_jobs if entry == "fwd" else L.pmlp_lstm_bwd_wide_jobs
        return fn(njobs, arr, 5, 37, H, None, None)

    def refused(text, *a, **kw):
        assert call(*a, **kw) != 0
        msg = L.pmlp_lstm_last_error()
        assert f"pmlp_lstm_{entry}_wide_jobs".encode() in msg and text in msg, msg

    ok = _full_job(234)
    refused(b"65..384", 1, [_full_job(64)])
    refused(b"65..384", 1, [_full_job(385)])
    refused(b"65..384", 2, [ok, _full_job(47)])
    refused(b"1..2 jobs", 3, [ok, ok, ok])
    refused(b"1..2 jobs", 0, [ok])
    refused(b"hidden 64", 1, [ok], H=32)
    needed = {"fwd": ("x", "w_ih", "b_ih", "b_hh", "w_hh", "h_out", "c_out", "gact", "gx", "hp"),
              "bwd": ("x", "w_hh", "c_out", "gact", "hp", "dh_out", "dgx", "slab", "slab_ih"),
              "step": ("x", "w_ih", "b_ih", "b_hh", "w_hh", "h_out", "c_out", "gx")}[entry]
    for name in needed:
        for bad in (None, 66):  # null, not 4-byte aligned
            j = _full_job(237)
            setattr(j, name, bad)
            refused(b"null or unaligned", 2, [ok, j])
    if entry == "step":
        for lone in ("h_save", "c_save"):
            j = _full_job(234)
            setattr(j, lone, None)
            refused(b"h_save and c_save together", 1, [j])
