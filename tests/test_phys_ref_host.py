"""The fp64 physics reference (phys_ref.py) against physics, and the CPU oracle against the reference.

The reference is first pinned to physics without the oracle: its mass matrix against the kinetic
energy of finite-differenced body motions, its accelerations against the momentum and energy
balances, its converged contact solve against the conditions of the contact problem.  Then every
case family runs through oracle/lgs_oracle.c (orc_simulate, orc_body_states_env) under the
tolerances the GPU test (test_gpu_phys_reference.py) uses, and single-term mutations of the
reference show that those tolerances would notice a wrong term.
"""
import ctypes as C
import dataclasses
import functools
import os

import numpy as np
import pytest

import bridge
import phys_ref as pr
from hostspec import make_spec
from leggedsim import cabi

ROBOTS = ("go2", "h1", "g1", "h1_2")
CHAIN = {"go2": 3, "h1": 5, "g1": 6, "h1_2": 6}   # the level order the HIP kernels eliminate in (lgs_get_factor_chain)

GENERATORS = {
    "flight0": lambda s: pr.flight(s, 0),
    "flight1": lambda s: pr.flight(s, 1),
    "limits": pr.joint_limits,
    "limits_over": lambda s: pr.joint_limits(s, rows=3),
    "plane": lambda s: pr.plane_contacts(s, N=129 if s.model.name == "go2" else 65),
    "overcap": pr.over_capacity,
    "heightfield": pr.heightfield,
    "self": pr.self_contacts,
    "sweeps1": lambda s: pr.plane_contacts(s, sweeps=1, feet_only=True, N=64),
    "sweeps40": lambda s: pr.plane_contacts(s, sweeps=40, feet_only=True, N=64),
}
FAMILIES = [(t, f) for f in ("flight0", "flight1", "limits", "plane", "overcap", "heightfield") for t in ROBOTS] + \
    [(t, "self") for t in ("h1", "g1", "h1_2")] + [("go2", "sweeps1"), ("go2", "sweeps40"), ("go2", "limits_over")]
MAX_EXCLUDED = 0.10


@functools.lru_cache(maxsize=None)
def spec_of(task):
    return make_spec(task)


@functools.lru_cache(maxsize=None)
def family(task, name):
    return GENERATORS[name](spec_of(task))


SPREADS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phys_ref_spreads.npz")


@functools.lru_cache(maxsize=None)
def stored_spreads():
    """phys_ref.sensitivity (k = 32) of every case, recorded by tools/phys_ref_report.py: 33 evaluations per
    case are most of the cost of a family, so the suite reads them and test_stored_spreads_* re-measures a
    sample of every family."""
    if not os.path.exists(SPREADS):
        return {}
    with np.load(SPREADS) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def reference(task, name):
    """(family, reference results, tolerances, spreads) of a family: computed once, shared, never changed."""
    fam = family(task, name)
    refs = pr.step_all(fam)
    st = stored_spreads().get(f"{task}/{name}")
    if st is not None and st.shape == (fam.n, len(pr.GROUPS)):
        spreads = [dict(zip(pr.GROUPS, (float(x) for x in row))) for row in st]
    else:
        spreads = [pr.sensitivity(fam, e) for e in range(fam.n)]
    tols = [pr.tolerance_of(spreads[e], refs[e]) for e in range(fam.n)]
    return fam, refs, tols, spreads


def sim_params_for(spec, fam):
    sp = cabi.SimParams.from_buffer_copy(spec.sim_params)
    for k, v in fam.meta["over"].items():
        if k == "gravity":
            sp.gravity[:] = tuple(v)
        else:
            setattr(sp, k, v)
    return sp


def dof_state(fam):
    return np.ascontiguousarray(np.stack([fam.q, fam.qd], -1).reshape(-1, 2), dtype=np.float32)


def run_oracle(lib, spec, fam, chain=0):
    """One orc_simulate of the family; returns root, q, qd, cforce [N,B,3], rigid_body_states [N,B,13] of the
    new state and the capacity-drop counts."""
    N, D, B = fam.n, spec.num_dof, spec.num_bodies
    sp = sim_params_for(spec, fam)
    mh = cabi.ModelHandle(fam.model)
    root, dofs, tau = fam.root.copy(), dof_state(fam), np.ascontiguousarray(fam.tau)
    cf, rbs = np.zeros((N * B, 3), np.float32), np.zeros((N * B, 13), np.float32)
    stats = np.zeros(3, np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    hf = fam.hf
    try:
        if hf is not None:
            h16 = np.ascontiguousarray(hf["heights"], np.int16)
            lib.orc_set_heightfield(p(h16), h16.shape[0], h16.shape[1], hf["hs"], hf["vs"], hf["border"])
        bridge.set_self_collision(lib, fam.sc)
        lib.orc_set_factor_chain(chain)
        lib.orc_contact_stats(p(stats), 1)
        lib.orc_simulate(C.byref(mh.desc), C.byref(sp), N, p(root), p(dofs), p(tau), p(cf), p(rbs),
                         p(np.ascontiguousarray(fam.added_mass)), p(np.ascontiguousarray(fam.friction)))
        lib.orc_contact_stats(p(stats), 1)
    finally:
        lib.orc_set_heightfield(None, 0, 0, 0.0, 0.0, 0.0)
        bridge.set_self_collision(lib, None)
        lib.orc_set_factor_chain(0)
    d = dofs.reshape(N, D, 2)
    return dict(root=root, q=d[:, :, 0].copy(), qd=d[:, :, 1].copy(), cforce=cf.reshape(N, B, 3),
                rbs=rbs.reshape(N, B, 13), stats=tuple(int(x) for x in stats))


def compare(task, name, got, what, show=False):
    """Every env's new state and contact forces against the reference, under the case's own tolerances.
    Returns the worst deviation / tolerance per quantity group (excluded cases left out) and the number of
    excluded cases; excluded cases must still be finite."""
    fam, refs, tols, _ = reference(task, name)
    excluded = [e for e in range(fam.n) if refs[e]["excluded"]]
    assert len(excluded) <= MAX_EXCLUDED * fam.n, f"{task} {name}: {len(excluded)} of {fam.n} cases near a branch"
    worst = {g: (0.0, -1, 0.0, 0.0) for g in pr.GROUPS}
    for e in range(fam.n):
        g_e = dict(root=got["root"][e], q=got["q"][e], qd=got["qd"][e], cforce=got["cforce"][e])
        assert all(np.isfinite(v).all() for v in g_e.values()), f"{task} {name} env {e}: not finite ({what})"
        if e in excluded:
            continue
        dev = pr.deviation(refs[e], g_e)
        for g in pr.GROUPS:
            r = dev[g] / tols[e][g] if tols[e][g] > 0 else (0.0 if dev[g] == 0 else np.inf)
            if r > worst[g][0]:
                worst[g] = (float(r), e, float(dev[g]), float(tols[e][g]))
    if show:
        print(f"{task} {name} {what}: " + " ".join(f"{g}={worst[g][0]:.3f}" for g in pr.GROUPS) + f" excluded={len(excluded)}")
    bad = {g: w for g, w in worst.items() if w[0] > 1.0}
    assert not bad, f"{task} {name} ({what}): deviation / tolerance, env, deviation, tolerance: {bad}"
    return worst, len(excluded)


def touching_bodies(cforce):
    return [tuple(np.nonzero(np.abs(f).max(-1) > 0)[0]) for f in cforce]


def count_bounds(refs):
    """What lgs_get_contact_stats must read for a family, from the reference alone: per counter (bodies, self
    contacts, limits without a slot) the sum of the reference's drops, widened for every activation
    decision the reference reports within its exclusion threshold (a ground candidate or a self pair within
    1e-5 m of contact_offset, a predicted joint position within 1e-6 rad of a limit), each of which may fall
    either way in fp32 and move its env's count by one.  Without such a decision the bounds coincide."""
    lo, hi = [0, 0, 0], [0, 0, 0]
    for r in refs:
        d, near = r["counts"]["dropped"], r["rows"]["near"]
        # a ground candidate switching changes the contact slots in use, hence also the slots left to the
        # self contacts and the rows left to the limits
        slack = (near[0], near[0] + near[1], 3 * (near[0] + near[1]) + near[2])
        for k in range(3):
            lo[k] += max(d[k] - slack[k], 0)
            hi[k] += d[k] + slack[k]
    return tuple(lo), tuple(hi)


def check_counts(task, name, got, what):
    """The capacity drops reported for the family (every env, the excluded ones included) lie within the
    reference's count_bounds, and per compared env the bodies that carry a contact force are the ones the
    documented slot order selects: none without a slot, and every body whose reference force exceeds the
    case's force tolerance has one."""
    fam, refs, tols, _ = reference(task, name)
    lo, hi = count_bounds(refs)
    assert all(lo[k] <= got["stats"][k] <= hi[k] for k in range(3)), \
        f"{task} {name} ({what}): capacity drops {got['stats']} outside the reference's {lo} .. {hi}"
    tb = touching_bodies(got["cforce"])
    for e in range(fam.n):
        if refs[e]["excluded"]:
            continue
        slotted = {g["b"] for g in refs[e]["rows"]["slots"]} | {g["b2"] for g in refs[e]["rows"]["slots"] if g["b2"] >= 0}
        assert set(tb[e]) <= slotted, f"{task} {name} env {e} ({what}): force on {set(tb[e]) - slotted}, no slot there"
        loaded = set(np.nonzero(np.abs(refs[e]["cforce"]).max(-1) > tols[e]["cforce"])[0])
        assert loaded <= set(tb[e]), f"{task} {name} env {e} ({what}): no force on {loaded - set(tb[e])}"


# ---------------------------------------------------------------- the reference against physics --
def _fd_body_velocities(model, root, q, qd, m_added, h=1e-5):
    """COM velocity and angular velocity of every body from finite differences of fk alone."""
    r = np.asarray(root, np.float64)
    R0 = pr.quat_to_mat(r[3:7])
    w = r[10:13]
    vO = r[7:10] - np.cross(w, R0 @ np.asarray(model.com[0], np.float64))
    out = []
    for sg in (h, -h):
        Rs = pr.expmap(sg * w) @ R0
        Rb, _, _, cw = pr.fk(model, r[0:3] + sg * vO, pr.mat_to_quat(Rs), np.asarray(q, np.float64) + sg * np.asarray(qd, np.float64))
        out.append((Rb, cw))
    v = (out[0][1] - out[1][1]) / (2 * h)
    S = out[0][0] @ np.swapaxes(out[1][0], -1, -2)      # exp(2h [w_b]x)
    S = 0.5 * (S - np.swapaxes(S, -1, -2))
    wb = np.stack([S[:, 2, 1], S[:, 0, 2], S[:, 1, 0]], -1) / (2 * h)
    return v, wb


@pytest.mark.parametrize("task", ROBOTS)
def test_mass_matrix_is_the_kinetic_energy_of_the_moving_bodies(task):
    """1/2 u^T M u == sum_b 1/2 m |v_c|^2 + 1/2 w_b^T I w_b with the body velocities taken from central
    differences of fk positions and rotations (h = 1e-5 s), no Jacobian in the check; added base mass
    scales the root's mass and inertia; the armature is exactly M's extra joint diagonal.  Bound 1e-8
    relative; the finite differences leave 2.2e-10 (go2), 4.5e-10 (h1), 2.0e-9 (g1), 9.5e-10 (h1_2) at worst
    over the family's 67 states (measured here, CPU)."""
    fam = dataclasses.replace(family(task, "flight0"))
    fam.root = fam.root.astype(np.float64)
    fam.root[:, 0:3] *= 0.1  # near the origin: less cancellation in the differences
    fam.root[:, 3:7] /= np.linalg.norm(fam.root[:, 3:7], axis=1, keepdims=True)  # unit in fp64: R0 is a rotation
    dyn = pr.dynamics(fam)
    m = fam.model
    worst = 0.0
    for e in range(fam.n):
        v, wb = _fd_body_velocities(m, fam.root[e], fam.q[e], fam.qd[e], fam.added_mass[e])
        Rb = pr.fk(m, fam.root[e, 0:3], fam.root[e, 3:7], fam.q[e])[0]
        mass = np.asarray(m.mass, np.float64).copy()
        I6 = np.asarray(m.inertia, np.float64)
        Ib = np.stack([np.array([[a[0], a[3], a[4]], [a[3], a[1], a[5]], [a[4], a[5], a[2]]]) for a in I6])
        dm = float(fam.added_mass[e])
        if dm != 0:
            Ib[0] *= (mass[0] + dm) / mass[0]
            mass[0] += dm
        Iw = Rb @ Ib @ np.swapaxes(Rb, -1, -2)
        ke = 0.5 * np.sum(mass * np.sum(v * v, -1)) + 0.5 * np.einsum("bi,bij,bj->", wb, Iw, wb)
        u = dyn["u"][e]
        worst = max(worst, abs(0.5 * u @ dyn["M"][e] @ u - ke) / ke)
    print(f"{task}: kinetic energy, worst relative difference {worst:.2e}")
    assert worst < 1e-8
    f1 = family(task, "flight1")
    with_arm = pr.dynamics(f1)["M"]
    without = pr.dynamics(f1, mut=("no_armature",))["M"]
    D = f1.q.shape[1]
    np.testing.assert_allclose(with_arm - without, np.diag([0.0] * 6 + [f1.params["armature"]] * D)[None] + 0 * with_arm,
                               atol=1e-15)


def _moments(fam):
    """Linear momentum, angular momentum about the system COM, kinetic (with the armature's 1/2 a qd^2) and
    potential energy of every env, from M and the Jacobians the kinetic-energy test anchors."""
    d = pr.dynamics(fam)
    u, m, Iw, g = d["u"], d["m"], d["Iw"], fam.params["gravity"]
    v, wb = pr.mv(d["JV"], u[:, None, :]), pr.mv(d["JW"], u[:, None, :])
    mt = m.sum(1)
    c = (m[..., None] * d["K"]["cw"]).sum(1) / mt[:, None]
    p = (m[..., None] * v).sum(1)
    L = (np.cross(d["K"]["cw"] - c[:, None, :], m[..., None] * v) + pr.mv(Iw, wb)).sum(1)
    ke = 0.5 * np.einsum("ni,nij,nj->n", u, d["M"], u)
    pe = -(m[..., None] * d["K"]["cw"] * g).sum((1, 2))
    return d, p, L, ke, pe, mt


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("task", ROBOTS)
def test_flight_accelerations_obey_the_balance_laws(task, variant):
    """In flight with random torques, moving every env along the reference's own accelerations for +-h
    (h = 2e-6 s: configuration along the velocities, velocities along the accelerations) changes the total
    linear momentum at the rate m_total g, leaves the angular momentum about the system COM alone, and
    changes KE + PE at the rate tau . qd.  The momenta and energies come from M and the Jacobians at the two
    displaced states, so the velocity-product bias (the differenced Jacobians inside the accelerations) is
    checked by a path that does not contain it.  All four robots, added base mass of both signs, armature 0
    and 0.01, straight and tilted gravity.  Bound 1e-8 of the sum of the magnitudes of each balance's terms;
    the central differences (this test's and the reference's own, phys_ref.FD_STEP = 2e-6 s) leave at most
    3.3e-9 (linear), 7.5e-9 (angular), 6.6e-9 (energy) over the eight runs, the largest on the runs with
    joints above their velocity limit (measured here, CPU).  With FD_STEP = 1e-5 s the same runs left 4e-8
    to 2e-7, which is why the reference's step is the smaller one."""
    fam = dataclasses.replace(family(task, f"flight{variant}"))
    fam.root = fam.root.astype(np.float64)
    fam.root[:, 0:3] *= 0.1
    fam.root[:, 3:7] /= np.linalg.norm(fam.root[:, 3:7], axis=1, keepdims=True)
    d, p0, L0, ke0, pe0, mt = _moments(fam)
    acc, u, g = d["acc"], d["u"], fam.params["gravity"]
    R0 = pr.quat_to_mat(fam.root[:, 3:7])
    com0 = np.asarray(fam.model.com[0], np.float64)
    h, side = 2e-6, []
    for sg in (h, -h):
        f2 = dataclasses.replace(fam)
        un = u + sg * acc
        Rs = pr.expmap(sg * u[:, 0:3]) @ R0
        f2.root = fam.root.copy()
        f2.root[:, 0:3] += sg * u[:, 3:6]
        f2.root[:, 3:7] = np.stack([pr.mat_to_quat(R) for R in Rs])
        f2.root[:, 10:13] = un[:, 0:3]
        f2.root[:, 7:10] = un[:, 3:6] + np.cross(un[:, 0:3], pr.mv(Rs, com0))
        f2.q = np.asarray(fam.q, np.float64) + sg * u[:, 6:]
        f2.qd = un[:, 6:]
        side.append(_moments(f2))
    dp, dL = (side[0][1] - side[1][1]) / (2 * h), (side[0][2] - side[1][2]) / (2 * h)
    dE = (side[0][3] + side[0][4] - side[1][3] - side[1][4]) / (2 * h)
    power = (np.asarray(fam.tau, np.float64) * u[:, 6:]).sum(1)
    m = d["m"]
    a = pr.mv(d["JV"], acc[:, None, :]) + d["adv"]
    f_scale = np.abs(m[..., None] * a).sum((1, 2)) + mt * np.linalg.norm(g)
    c = (m[..., None] * d["K"]["cw"]).sum(1) / mt[:, None]
    t_scale = np.abs(np.cross(d["K"]["cw"] - c[:, None, :], m[..., None] * a)).sum((1, 2))
    v = pr.mv(d["JV"], u[:, None, :])
    p_scale = np.abs(m[..., None] * v * a).sum((1, 2)) + np.abs(np.asarray(fam.tau, np.float64) * u[:, 6:]).sum(1)
    res = ((np.abs(dp - mt[:, None] * g).max(1) / f_scale).max(), (np.abs(dL).max(1) / t_scale).max(),
           (np.abs(dE - power) / p_scale).max())
    print(f"{task} flight{variant}: balance residuals linear {res[0]:.2e} angular {res[1]:.2e} energy {res[2]:.2e}")
    assert max(res) < 1e-8


CONVERGED = {"go2": ("plane", "heightfield"), "h1": ("plane", "heightfield", "self"),
             "g1": ("plane", "heightfield", "self"), "h1_2": ("plane", "heightfield", "self")}


@pytest.mark.parametrize("task", ROBOTS)
def test_converged_solve_meets_the_contact_conditions(task):
    """The reference's Gauss-Seidel at 500 sweeps, checked in fp64 against the contact problem itself and not
    against a sweep-by-sweep copy: lam_n >= 0 exactly; the normal velocity not below its target and
    complementary to the impulse; friction inside the cone; pairs inside the cone at rest, pairs on it
    opposing their sliding velocity (in the metric of the pair's diagonal, phys_ref.lcp_residuals).
    On the envs of the plane, heightfield and self-contact families whose rows are independent
    (cond(A) <= 1e4): a sweep then contracts the error by a factor bounded away from 1 and 500 sweeps reach
    rounding, so the bound is 1e-12 (m/s; relative for the cone and the direction), a few thousand fp64
    ulps of the 20 m/s these cases reach.  Every 2nd env for go2, every env for the humanoids.  The
    several sole points of a flat humanoid foot make A singular; such envs stop anywhere between 1e-3 and
    1e-17 m/s after 500 sweeps, in v as well as in lam, and are not judged.  So that the humanoids' ground
    contacts are judged all the same, their plane family runs once more with two contact slots (one per
    foot); at least 8 judged envs per robot carry a loaded ground contact.  Worst measured over the judged envs (CPU): 2e-15."""
    worst = dict(below=0.0, compl=0.0, cone=0.0, stick=0.0, oppose=0.0)
    used = ground = sliding = sticking = 0
    fams = [family(task, name) for name in CONVERGED[task]]
    if task != "go2":
        # the humanoids' ground contacts: the plane family with two contact slots, which the slot order gives to
        # the first touching candidate of each foot, so the rows are independent and the solve can be judged
        two = dataclasses.replace(family(task, "plane"))
        two.params = dict(two.params, max_contacts=2, max_rows=14)
        fams.append(two)
    for fam in fams:
        for e in range(0, fam.n, 2 if task == "go2" else 1):
            r = pr.step(fam, e, sweeps=500)
            if not len(r["lam"]) or np.linalg.cond(r["A"]) > 1e4:
                continue
            used += 1
            ground += bool(r["counts"]["primary"]) and bool((r["lam"][r["rows"]["kind"] == 0] > 0).any())
            res = pr.lcp_residuals(r["rows"], r["lam"], r["v"], r["A"])
            lmax = max(np.abs(r["lam"]).max(), 1e-12)
            assert res["neg"] == 0.0
            for k, scale in (("below", 1.0), ("compl", lmax), ("cone", lmax), ("stick", 1.0), ("oppose", 1.0)):
                worst[k] = max(worst[k], res[k] / scale)
            sliding += res["oppose"] > 0
            sticking += res["stick"] > 0
    print(f"{task}: {used} envs ({sliding} sliding, {sticking} sticking), converged residuals "
          + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    print(f"{task}: {ground} of them with a loaded ground contact")
    assert used >= 8 and ground >= 8 and sliding >= 2 and sticking >= 2
    assert max(worst.values()) < 1e-12


MUTATION_FAMILY = {"no_gyro": ("go2", "flight0"), "ixy_sign": ("go2", "flight0"), "no_armature": ("go2", "flight1"),
                   "mass_no_inertia": ("go2", "flight0"), "mu_not_averaged": ("go2", "plane"),
                   "no_baumgarte_clamp": ("go2", "plane"), "limit_sign": ("go2", "limits"),
                   "tangent_no_orth": ("go2", "heightfield"), "self_no_second": ("h1", "self")}


@pytest.mark.parametrize("mut", pr.MUTATIONS)
def test_tolerances_notice_a_single_wrong_term(mut):
    """One term of the reference removed or altered at a time: at least one case of the matching family moves
    by more than 10x that case's own tolerance, so a kernel with that error would fail the comparison."""
    assert set(MUTATION_FAMILY) == set(pr.MUTATIONS)
    task, name = MUTATION_FAMILY[mut]
    fam, refs, tols, _ = reference(task, name)
    wrong = pr.step_all(fam, mut=(mut,))
    best = 0.0
    for e in range(fam.n):
        if refs[e]["excluded"]:
            continue
        dev = pr.deviation(refs[e], dict(root=np.concatenate([wrong[e]["pos"], wrong[e]["quat"], wrong[e]["vlin"],
                                                              wrong[e]["vang"]]),
                                         q=wrong[e]["q"], qd=wrong[e]["qd"], cforce=wrong[e]["cforce"]))
        best = max(best, max(dev[g] / tols[e][g] for g in pr.GROUPS if tols[e][g] > 0))
    print(f"{mut} on {task} {name}: moves a case by {best:.1f} tolerances")
    assert best > 10.0


@pytest.mark.parametrize("task,name", FAMILIES)
def test_stored_spreads_are_what_the_reference_measures(task, name):
    """tests/golden/phys_ref_spreads.npz holds every family, and every 8th case re-measured here gives the
    stored spread (1e-3 relative: the same perturbations, up to the rounding of another LAPACK build)."""
    fam = family(task, name)
    st = stored_spreads().get(f"{task}/{name}")
    assert st is not None and st.shape == (fam.n, len(pr.GROUPS)), "run tools/phys_ref_report.py --store"
    for e in range(0, fam.n, 8):
        sp = pr.sensitivity(fam, e)
        np.testing.assert_allclose([sp[g] for g in pr.GROUPS], st[e], rtol=1e-3, atol=1e-300)


# ---------------------------------------------------------------- the oracle against the reference --
@pytest.mark.parametrize("task,name", FAMILIES)
def test_oracle_matches_the_reference(task, name, oracle_lib):
    """orc_simulate on every family under the GPU test's tolerances (index-order factorisation and, for the
    chain-structured robots, the level order the HIP kernels use), and orc_body_states_env's rows."""
    spec = spec_of(task)
    fam, refs, _, _ = reference(task, name)
    for chain in sorted({0, CHAIN[task]}):
        got = run_oracle(oracle_lib, spec, fam, chain)
        compare(task, name, got, f"oracle, factor chain {chain}", show=True)
        check_counts(task, name, got, f"oracle, factor chain {chain}")
        check_body_rows(fam, got, f"{task} {name} oracle")
    check_family_covers(task, name)


def check_body_rows(fam, got, what, every=1):
    """rigid_body_states rows of the new state against the reference's rows of that same state (quaternions up
    to sign), every env (the ragged last ones included): tolerance MARGIN x the rows' own spread, floored at 4 ulps of the largest
    entry."""
    for e in range(0, fam.n, every):
        want = pr.body_states(fam.model, got["root"][e], got["q"][e], got["qd"][e])
        sp = pr.body_states_spread(fam.model, got["root"][e], got["q"][e], got["qd"][e])
        rows = np.asarray(got["rbs"][e], np.float64)
        sign = np.sign(np.sum(rows[:, 3:7] * want[:, 3:7], -1))[:, None]
        for sl, spread, nm in ((slice(0, 3), sp[0], "origin"), (slice(3, 7), sp[1], "quaternion"),
                               (slice(7, 10), sp[2], "COM velocity"), (slice(10, 13), sp[3], "angular velocity")):
            a = rows[:, sl] * (sign if nm == "quaternion" else 1.0)
            tol = max(pr.MARGIN * spread, 4 * pr.EPS32 * np.abs(want[:, sl]).max())
            assert np.abs(a - want[:, sl]).max() <= tol, f"{what} env {e}: body rows {nm} off by " \
                f"{np.abs(a - want[:, sl]).max():.3e} (tolerance {tol:.3e})"


def check_family_covers(task, name):
    """What each family is there to exercise really occurs in it (from the reference alone)."""
    fam, refs, _, _ = reference(task, name)
    cnt = [r["counts"] for r in refs]
    if name == "limits":
        mode = fam.meta["mode"]
        assert all(sum(c["dropped"]) == 0 for c in cnt) and all(c["limits"] >= 1 for c in cnt)
        assert sum(c["limits"] for c in cnt) >= 2 * fam.n
        assert all((mode == k).any() for k in (1, 2, 3, 4))
        # rows of both signs and both target branches
        signs = {(float(r["rows"]["J"][i, 6:].sum()), bool(r["rows"]["tgt"][i] > 0)) for r in refs
                 for i in range(len(r["rows"]["tgt"]))}
        assert signs == {(1.0, False), (1.0, True), (-1.0, False), (-1.0, True)}
    if name == "plane":
        inside = on = 0
        for r in refs:
            for c, mu in enumerate(r["rows"]["mu"]):
                ln, lt = r["lam"][3 * c], np.linalg.norm(r["lam"][3 * c + 1:3 * c + 3])
                if ln > 0:
                    inside += lt < mu * ln * (1 - 1e-9)
                    on += lt >= mu * ln * (1 - 1e-9)
        assert inside >= 0.25 * (inside + on) and on >= 0.25 * (inside + on), (inside, on)
        assert any(c["secondary"] > 0 for c in cnt) and any(c["primary"] > 1 for c in cnt)
        feet = set(spec_of(task).feet_indices)
        assert any({g["b"] for g in r["rows"]["slots"]} - feet for r in refs), "no link but the feet touches"
        assert any(r["rows"]["tgt"][0] == fam.params["max_depenetration_velocity"] for r in refs if len(r["rows"]["tgt"]))
    if name == "overcap":
        over = sum(c["candidates"] > fam.params["max_contacts"] for c in cnt)
        assert over >= fam.n // 2 and all(c["primary"] + c["secondary"] == fam.params["max_contacts"]
                                           for c in cnt if c["candidates"] > fam.params["max_contacts"])
        if task == "go2":   # the body counter is compared on a non-zero value
            assert over == fam.n and count_bounds(refs)[0][0] > 0.9 * sum(c["dropped"][0] for c in cnt) > 0
    if name == "heightfield":
        assert min(r["margins"]["terrain"] for r in refs) > pr.TERRAIN_MARGIN
        nz = [g["n"][2] for r in refs for g in r["rows"]["slots"]]
        assert min(nz) < 0.9 and any(abs(z - 1 / np.sqrt(1.09)) < 1e-6 for z in nz)   # the step and the 0.3 slope
        assert fam.root[0, 0] < -fam.hf["border"] and len(refs[0]["rows"]["slots"]) > 0    # env 0: outside the map
        assert any(len({tuple(np.round(g["n"], 6)) for g in r["rows"]["slots"]}) > 1 for r in refs)  # two triangles
    if name == "limits_over":   # the limit counter is compared on a non-zero value
        assert count_bounds(refs)[0][2] > 0 and any(c["limits"] == 3 and c["dropped"][2] > 0 for c in cnt)
    if name in ("plane", "heightfield", "sweeps1", "sweeps40"):   # most envs carry a contact force
        assert sum(bool((r["lam"][r["rows"]["kind"] == 0] > 0).any()) for r in refs if len(r["lam"])) >= 0.6 * fam.n
    if name == "self":
        assert {c["self"] for c in cnt} >= {1} and max(c["self"] for c in cnt) >= 2
        if task in ("h1", "g1"):   # three pairs touch, two slots: the self counter is compared on a non-zero value
            assert count_bounds(refs)[0][1] > 0
        assert any(c["self"] > 0 and c["primary"] > 0 for c in cnt) and any(c["self"] > 0 and c["primary"] == 0 for c in cnt)
        for r in refs:   # equal and opposite: the self contacts alone sum to zero over the bodies
            if r["counts"]["primary"] == 0:
                assert np.abs(r["cforce"].sum(0)).max() <= 1e-9 * max(np.abs(r["cforce"]).max(), 1.0)
