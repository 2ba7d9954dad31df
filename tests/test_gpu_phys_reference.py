"""The HIP physics substep (lgs_simulate) and lgs_forward_kinematics against the fp64 reference
(phys_ref.py), directly and not through the CPU oracle.

A bare native.Sim per family: bind, set_env_properties, the family's heightfield / self-collision
proxies, set_dof_actuation_force, ONE simulate(); root_states, dof_state and net_contact_forces
are compared with the reference under each case's own tolerance (phys_ref.MARGIN x the spread
fp32 rounding of the inputs alone causes, floored at 4 ulps), then lgs_forward_kinematics' rows
with the reference's rows of the new state.  The families, their references and the tolerances
are test_phys_ref_host.py's, where the oracle runs through the same comparison without a GPU.
Odd env counts (67, 65, 129) leave the last wave ragged and put one env in a wave; even counts
(64) put two.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import isaacgym  # noqa: F401,E402
import phys_ref as pr  # noqa: E402
from leggedsim import native  # noqa: E402
from test_phys_ref_host import (FAMILIES, check_body_rows, check_counts, compare, dof_state, reference,  # noqa: E402
                                run_oracle, sim_params_for, spec_of, touching_bodies)


def run_kernel(spec, fam):
    """One lgs_simulate of the family on a bare sim, then lgs_forward_kinematics; the new state, the contact
    forces, the body rows and the capacity-drop counts."""
    N, D, B = fam.n, spec.num_dof, spec.num_bodies
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()  # noqa: E731
    root, dofs, tau = dev(fam.root), dev(dof_state(fam)), dev(fam.tau)
    cf, rbs = torch.zeros(N * B, 3, device="cuda"), torch.zeros(N * B, 13, device="cuda")
    sim = native.Sim(fam.model, sim_params_for(spec, fam), N, 0)
    try:
        sim.bind(root, dofs, cf, rbs)
        sim.set_env_properties(fam.friction, fam.added_mass)
        if fam.hf is not None:
            sim.set_heightfield(fam.hf["heights"], fam.hf["hs"], fam.hf["vs"], fam.hf["border"])
        if fam.sc is not None:
            sim.set_self_collision(fam.sc)
        sim.contact_stats(reset=True)
        sim.simulate(tau)
        stats = sim.contact_stats(reset=True)
        sim.forward_kinematics()
        torch.cuda.synchronize()
        d = dofs.cpu().numpy().reshape(N, D, 2)
        return dict(root=root.cpu().numpy(), q=d[:, :, 0].copy(), qd=d[:, :, 1].copy(),
                    cforce=cf.cpu().numpy().reshape(N, B, 3), rbs=rbs.cpu().numpy().reshape(N, B, 13),
                    stats=(stats["bodies"], stats["self"], stats["limits"]))
    finally:
        sim.close()


@pytest.mark.parametrize("task,name", FAMILIES)
def test_substep_matches_the_fp64_reference(task, name, oracle_lib):
    spec = spec_of(task)
    fam, refs, tols, _ = reference(task, name)
    got = run_kernel(spec, fam)
    compare(task, name, got, "HIP kernel", show=True)
    check_counts(task, name, got, "HIP kernel")
    check_body_rows(fam, got, f"{task} {name} HIP kernel")
    # cases next to a branch are left out of the value comparison, but still land on the oracle's bodies
    near = [e for e in range(fam.n) if refs[e]["excluded"]]
    if near:
        orc = run_oracle(oracle_lib, spec, fam, native_chain(spec, fam))
        assert got["stats"] == orc["stats"]
        tb_k, tb_o = touching_bodies(got["cforce"]), touching_bodies(orc["cforce"])
        assert all(tb_k[e] == tb_o[e] for e in near)
    if name == "self":
        for e in range(fam.n):   # in flight only the self contacts act: equal and opposite on the two bodies
            if refs[e]["counts"]["primary"] == 0 and not refs[e]["excluded"]:
                f = got["cforce"][e].astype(np.float64)
                assert np.abs(f.sum(0)).max() <= 8 * pr.EPS32 * np.abs(f).max()


def native_chain(spec, fam):
    sim = native.Sim(fam.model, sim_params_for(spec, fam), fam.n, 0)
    try:
        return sim.factor_chain()
    finally:
        sim.close()


def test_converged_sweeps_meet_the_contact_conditions_on_the_kernels_impulses():
    """Family 7 at 40 sweeps (go2, one candidate per foot, so a foot's net force IS its contact's impulse / dt):
    the kernel's own impulses, put through the reference's fp64 rows, meet the contact conditions as well as
    the reference's 40-sweep solve does, up to what the case's force tolerance moves them by: lam_n >= 0 and
    inside the cone to the impulse tolerance; normal velocity not below its target and complementarity to
    ||A|| x the impulse tolerance beyond the reference's own residual."""
    task, name = "go2", "sweeps40"
    spec = spec_of(task)
    fam, refs, tols, _ = reference(task, name)
    got = run_kernel(spec, fam)
    dt = fam.params["dt"]
    judged = 0
    for e in range(fam.n):
        r = refs[e]
        rows = r["rows"]
        if r["excluded"] or not len(rows["mu"]) or len(rows["tgt"]) != 3 * len(rows["mu"]):
            continue
        assert len({g["b"] for g in rows["slots"]}) == len(rows["slots"])   # one contact per body
        lam = np.concatenate([rows["frames"][c] @ got["cforce"][e][g["b"]].astype(np.float64) * dt
                              for c, g in enumerate(rows["slots"])])
        v = r["vfree"] + r["A"] @ lam
        tol_l = tols[e]["cforce"] * dt
        tol_v = np.abs(r["A"]).sum(1).max() * tol_l
        mine, ref = pr.lcp_residuals(rows, lam, v, r["A"]), pr.lcp_residuals(rows, r["lam"], r["v"], r["A"])
        assert mine["neg"] <= tol_l and mine["cone"] <= ref["cone"] + 2 * tol_l, (e, mine, ref)
        assert mine["below"] <= ref["below"] + tol_v, (e, mine, ref)
        assert mine["compl"] <= ref["compl"] + tol_v * np.abs(lam).max() + tol_l * np.abs(v - rows["tgt"]).max(), (e, mine, ref)
        judged += bool((r["lam"][rows["kind"] == 0] > 0).any())   # envs whose feet carry load
    assert judged >= fam.n // 2
