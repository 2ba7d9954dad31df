"""An fp64 reference of one physics substep (lgs_simulate), independent of the kernel's algorithm.

The HIP kernel and oracle/lgs_oracle.c share one algorithm (spatial-vector RNEA bias, composite
inertias, a leaves-first Cholesky, Y = L^-1 J^T) in one fp32 operation order, so their bit parity
says nothing about a term both have wrong.  This module computes the same substep from the
textbook definitions instead, in plain numpy fp64:

* per-body Jacobians of the COM velocity and the angular velocity in u = [w, v_O, qd]
  (v_O: the classical velocity of the root origin),
* M = sum_b m Jv^T Jv + Jw^T I Jw (+ armature), bias = sum_b Jv^T m (Jv' u - g) + Jw^T (I Jw' u + w_b x I w_b)
  with J' u from central differences of the Jacobians along the motion,
* a dense np.linalg.solve, A = J M^-1 J^T, and the projected Gauss-Seidel that include/leggedsim.h documents.

It reads a leggedsim.model.Model and nothing else of the project.  Every activation decision is
reported with its margin, `sensitivity` measures how far fp32 rounding of the inputs alone moves
the true answer of a case (the tolerance of every comparison comes from there), and `MUTATIONS`
switches single terms off so a test can show that the tolerance would notice them.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

# tolerance = MARGIN x sensitivity(case), floored at 4 fp32 ulps of the quantity's own magnitude.
# The spread holds cond(M) * 2^-23 for the rounding of the inputs; the kernel adds the rounding of
# a solve in 16-18 unknowns, of up to 32 constraint rows and of the sweeps.  The work started at 64;
# the CPU oracle and the HIP kernel both need at most 14.5 (h1_2 in flight; every other family 0.7
# to 10.5), so the margin is the next power of two, 16.  profiles/phys_ref/README.md has every
# measured spread and deviation and what the tolerance comes to per family.
MARGIN = 16.0
EPS32 = 2.0 ** -23
FD_STEP = 2e-6  # the central-difference step of J' u, in seconds along the motion

# exclusion thresholds: a case is left out of a value comparison only when a branch margin is below these
ACT_MARGIN = 1e-5    # m, |sep - contact_offset| of a ground candidate or a self pair
LIMIT_MARGIN = 1e-6  # rad, predicted joint position to a limit
CONE_MARGIN = 1e-4   # relative, |l|^2 to (mu ln)^2 in the last sweep
TERRAIN_MARGIN = 1e-4  # cell units to a triangle's edge; the generators keep every case above it (asserted)

MUTATIONS = ("no_gyro", "ixy_sign", "no_armature", "mass_no_inertia", "mu_not_averaged", "no_baumgarte_clamp",
             "limit_sign", "tangent_no_orth", "self_no_second")

GROUPS = ("pos", "quat", "vlin", "vang", "q", "qd", "cforce")


# ------------------------------------------------------------------ small algebra (batched) --
def skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1),
                     np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def quat_to_mat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def mat_to_quat(R):
    """xyzw of a rotation matrix: the eigenvector of the largest eigenvalue of Bar-Itzhack's K matrix
    (no branch on the trace), sign chosen with w >= 0."""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, V = np.linalg.eigh(K)
    q = V[:, -1]
    return q if q[3] >= 0 else -q


def rot_axis(a, ang):
    """Rodrigues: cos I + sin [a]x + (1 - cos) a a^T (a as the model gives it)."""
    c, s = np.cos(ang)[..., None, None], np.sin(ang)[..., None, None]
    return c * np.eye(3) + s * skew(a) + (1 - c) * a[..., :, None] * a[..., None, :]


def expmap(w):
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    safe = np.where(th > 0, th, 1.0)
    A = np.where(th > 0, np.sin(safe) / safe, 1.0)
    Bc = np.where(th > 0, 2 * np.sin(0.5 * safe) ** 2 / safe ** 2, 0.5)
    Kx = skew(w)
    return np.eye(3) + A * Kx + Bc * (Kx @ Kx)


def mv(A, v):
    return (A @ v[..., None])[..., 0]


# ------------------------------------------------------------------ model, parameters, cases --
@dataclass
class Topo:
    B: int
    D: int
    parent: np.ndarray
    dof: np.ndarray
    dof_body: np.ndarray
    anc: np.ndarray      # [B, D] joint j lies between the root and body b
    pt_body: np.ndarray


def topo_of(model):
    B, D = model.num_bodies, model.num_dofs
    parent = np.asarray(model.parent, dtype=np.int64)
    dof = np.asarray(model.dof, dtype=np.int64)
    anc = np.zeros((B, D), bool)
    dof_body = np.zeros(D, np.int64)
    for b in range(1, B):
        anc[b] = anc[parent[b]]
        if dof[b] >= 0:
            anc[b, dof[b]] = True
            dof_body[dof[b]] = b
    return Topo(B, D, parent, dof, dof_body, anc, np.asarray(model.pt_body, dtype=np.int64))


CONST_KEYS = ("joint_rot", "joint_pos", "axis", "mass", "com", "inertia", "dof_lower", "dof_upper", "dof_velocity",
              "pt_pos", "pt_radius")


def consts_of(model):
    C = {k: np.asarray(getattr(model, k), dtype=np.float64).copy() for k in CONST_KEYS}
    C["joint_rot"] = C["joint_rot"].reshape(-1, 3, 3)
    return C


PARAM_FLOATS = ("dt", "contact_offset", "rest_offset", "max_depenetration_velocity", "baumgarte", "ground_friction",
                "armature")
PARAM_INTS = ("solver_iterations", "clamp_joint_velocity", "max_contacts", "max_rows")


def params_of(sp, **over):
    """A plain dict of an lgs_sim_params-like object (attribute access), fp32 values as fp64."""
    P = {k: float(np.float32(getattr(sp, k))) for k in PARAM_FLOATS}
    P.update({k: int(getattr(sp, k)) for k in PARAM_INTS})
    P["gravity"] = np.array([float(np.float32(x)) for x in sp.gravity])
    for k, v in over.items():
        P[k] = np.array([float(np.float32(x)) for x in v]) if k == "gravity" else \
            (int(v) if k in PARAM_INTS else float(np.float32(v)))
    return P


@dataclass
class Family:
    """The cases of one launch: N envs that share the model, the sim parameters and the ground."""
    name: str
    model: object
    params: dict
    root: np.ndarray        # [N, 13] float32
    q: np.ndarray           # [N, D] float32
    qd: np.ndarray          # [N, D]
    tau: np.ndarray         # [N, D]
    friction: np.ndarray    # [N]
    added_mass: np.ndarray  # [N]
    hf: dict = None         # heights int16 [rows, cols], hs, vs, border
    sc: object = None       # proxy_body, capsules, pairs, max_self_contacts
    meta: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.root.shape[0]


def _inputs(fam, e):
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    r = f(fam.root[e])
    return dict(pos=r[0:3], quat=r[3:7], vcom=r[7:10], w=r[10:13], q=f(fam.q[e]), qd=f(fam.qd[e]), tau=f(fam.tau[e]),
                friction=f(fam.friction[e]), added_mass=f(fam.added_mass[e]))


# ------------------------------------------------------------------ kinematics --
def _kin(T, C, pos, R0, q):
    """Body rotations R [..,B,3,3], origins p [..,B,3], world joint axes by DOF aw [..,D,3], the joints'
    origins pj [..,D,3] and the COMs cw [..,B,3].  child = parent . joint_rot . Rot(axis, q)."""
    R, p, aw = [None] * T.B, [None] * T.B, [None] * T.D
    R[0], p[0] = R0, pos
    for b in range(1, T.B):
        a = T.parent[b]
        Rj = R[a] @ C["joint_rot"][..., b, :, :]
        p[b] = p[a] + mv(R[a], C["joint_pos"][..., b, :])
        j = T.dof[b]
        if j >= 0:
            ax = C["axis"][..., b, :]
            aw[j] = mv(Rj, ax)
            R[b] = Rj @ rot_axis(ax, q[..., j])
        else:
            R[b] = Rj
    bs = np.broadcast_shapes(*[x.shape[:-2] for x in R])
    R = np.stack([np.broadcast_to(x, bs + (3, 3)) for x in R], -3)
    p = np.stack([np.broadcast_to(x, bs + (3,)) for x in p], -2)
    aw = np.stack([np.broadcast_to(x, bs + (3,)) for x in aw], -2)
    cw = p + mv(R, C["com"])
    return dict(R=R, p=p, aw=aw, pj=p[..., T.dof_body, :], cw=cw)


def _jac(T, K, pts=None):
    """Jw [..,B,3,n] and Jv [..,B,3,n] of the points pts [..,B,3] (one per body; default the COMs)."""
    pts = K["cw"] if pts is None else pts
    bs, n = pts.shape[:-2], 6 + T.D
    JW, JV = np.zeros(bs + (T.B, 3, n)), np.zeros(bs + (T.B, 3, n))
    JW[..., 0:3] = np.eye(3)
    JV[..., 3:6] = np.eye(3)
    JV[..., 0:3] = -skew(pts - K["p"][..., 0:1, :])
    anc = T.anc[:, :, None]
    awb = K["aw"][..., None, :, :]
    JW[..., 6:] = np.swapaxes(awb * anc, -1, -2)
    JV[..., 6:] = np.swapaxes(np.cross(awb, pts[..., :, None, :] - K["pj"][..., None, :, :]) * anc, -1, -2)
    return JW, JV


def _point_jac(T, K, b, pt):
    """[3, n] Jacobian of the velocity of the world point pt moving with body b (unbatched)."""
    J = np.zeros((3, 6 + T.D))
    J[:, 0:3] = -skew(pt - K["p"][0])
    J[:, 3:6] = np.eye(3)
    for j in np.nonzero(T.anc[b])[0]:
        J[:, 6 + j] = np.cross(K["aw"][j], pt - K["pj"][j])
    return J


def fk(model, root_pos, quat_xyzw, q):
    """Body rotations, origins, world joint axes (by body, zero without a joint) and COMs."""
    T, C = topo_of(model), consts_of(model)
    K = _kin(T, C, np.asarray(root_pos, np.float64), quat_to_mat(np.asarray(quat_xyzw, np.float64)),
             np.asarray(q, np.float64))
    axes = np.zeros((T.B, 3))
    axes[T.dof_body] = K["aw"]
    return K["R"], K["p"], axes, K["cw"]


def _body_rows(T, C, s):
    K = _kin(T, C, s["pos"], quat_to_mat(s["quat"]), s["q"])
    vO = s["vcom"] - np.cross(s["w"], mv(K["R"][..., 0, :, :], C["com"][..., 0, :]))
    u = np.concatenate([s["w"], vO, s["qd"]], -1)
    JW, JV = _jac(T, K)
    return K, mv(JV, u[..., None, :]), mv(JW, u[..., None, :])


def body_states(model, root13, q, qd):
    """The rigid_body_states rows [B, 13]: origin, quaternion xyzw, COM linear velocity, angular velocity."""
    T, C = topo_of(model), consts_of(model)
    r = np.asarray(root13, np.float64)
    s = dict(pos=r[0:3], quat=r[3:7], vcom=r[7:10], w=r[10:13], q=np.asarray(q, np.float64), qd=np.asarray(qd, np.float64))
    K, v, w = _body_rows(T, C, s)
    quat = np.stack([mat_to_quat(K["R"][b]) for b in range(T.B)])
    return np.concatenate([K["p"], quat, v, w], -1)


def body_states_spread(model, root13, q, qd, k=32, seed=0):
    """max - min of the rows' positions / velocities (and of the rotation matrices' entries) over k
    evaluations with every input and constant perturbed by a relative 2^-23: (pos, rot, vel, ang)."""
    T, C = topo_of(model), consts_of(model)
    rng = np.random.default_rng(seed)
    pert = lambda a: np.asarray(a, np.float64) * (1 + EPS32 * rng.uniform(-1, 1, (k,) + np.shape(a)))  # noqa: E731
    r = np.asarray(root13, np.float64)
    s = dict(pos=pert(r[0:3]), quat=pert(r[3:7]), vcom=pert(r[7:10]), w=pert(r[10:13]), q=pert(q), qd=pert(qd))
    K, v, w = _body_rows(T, {key: pert(val) for key, val in C.items()}, s)
    sp = lambda a: float((a.max(0) - a.min(0)).max())  # noqa: E731
    return sp(K["p"]), sp(K["R"]), sp(v), sp(w)


# ------------------------------------------------------------------ dynamics (batched) --
def _inertia3(I6, mut):
    ixy = -I6[..., 3] if "ixy_sign" in mut else I6[..., 3]
    return np.stack([np.stack([I6[..., 0], ixy, I6[..., 4]], -1),
                     np.stack([ixy, I6[..., 1], I6[..., 5]], -1),
                     np.stack([I6[..., 4], I6[..., 5], I6[..., 2]], -1)], -2)


def _mass_inertia(C, added_mass, mut):
    """Per-body mass and body-frame inertia; added base mass scales the root's mass and its inertia
    by (m + d) / m (lgs_set_env_properties)."""
    m = C["mass"] * np.ones(np.shape(added_mass) + (1,))
    Ib = _inertia3(C["inertia"], mut) * np.ones(np.shape(added_mass) + (1, 1, 1))
    m0 = m[..., 0]
    on = (np.asarray(added_mass) != 0) & (m0 > 0)
    scale = np.where(on, (m0 + added_mass) / np.where(m0 > 0, m0, 1.0), 1.0)
    m[..., 0] = np.where(on, m0 + added_mass, m0)
    if "mass_no_inertia" not in mut:
        Ib[..., 0, :, :] = Ib[..., 0, :, :] * scale[..., None, None]
    return m, Ib


def _dynamics(T, C, P, s, mut=()):
    """Mass matrix, bias and free velocity u_f = u + dt M^-1 (tau_gen - bias); every array may carry
    leading batch axes."""
    R0 = quat_to_mat(s["quat"])
    K = _kin(T, C, s["pos"], R0, s["q"])
    vO = s["vcom"] - np.cross(s["w"], mv(R0, C["com"][..., 0, :]))
    u = np.concatenate([s["w"], vO, s["qd"]], -1)
    JW, JV = _jac(T, K)
    m, Ib = _mass_inertia(C, s["added_mass"], mut)
    Iw = K["R"] @ Ib @ np.swapaxes(K["R"], -1, -2)
    M = np.einsum("...b,...bin,...bim->...nm", m, JV, JV) + np.einsum("...bin,...bij,...bjm->...nm", JW, Iw, JW)
    if "no_armature" not in mut:
        idx = np.arange(6, 6 + T.D)
        M[..., idx, idx] += np.asarray(P["armature"])[..., None]
    # J' u by central differences along the motion
    h = FD_STEP
    vel = []
    for sg in (h, -h):
        Ks = _kin(T, C, s["pos"] + sg * vO, expmap(sg * s["w"]) @ R0, s["q"] + sg * s["qd"])
        JWs, JVs = _jac(T, Ks)
        vel.append((mv(JVs, u[..., None, :]), mv(JWs, u[..., None, :])))
    adv = (vel[0][0] - vel[1][0]) / (2 * h)
    adw = (vel[0][1] - vel[1][1]) / (2 * h)
    wb = mv(JW, u[..., None, :])
    gyro = 0.0 if "no_gyro" in mut else np.cross(wb, mv(Iw, wb))
    f = m[..., None] * (adv - np.asarray(P["gravity"])[..., None, :])
    nb = mv(Iw, adw) + gyro
    bias = np.einsum("...bin,...bi->...n", JV, f) + np.einsum("...bin,...bi->...n", JW, nb)
    rhs = -bias
    rhs[..., 6:] += s["tau"]
    acc = np.linalg.solve(M, rhs[..., None])[..., 0]
    uf = u + np.asarray(P["dt"])[..., None] * acc
    return dict(K=K, M=M, u=u, uf=uf, acc=acc, bias=bias, m=m, Iw=Iw, JW=JW, JV=JV, adv=adv, adw=adw)


# ------------------------------------------------------------------ ground and self contacts --
def terrain(hf, x, y):
    """Ground height under the points (x, y) [K], the unit normals [K, 3] of the triangles there and each
    point's distance (cell units) to the nearest edge of its triangle across which the normal jumps.
    lgs_set_heightfield: sample (i, j) at x = i hs - border, y = j hs - border, z = heights vs; cell
    (i, j) split along its (i,j)-(i+1,j+1) diagonal; outside the map the coordinates are clamped to its edge."""
    x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
    if hf is None:
        return np.zeros_like(x), np.tile([0.0, 0.0, 1.0], (len(x), 1)), np.full(len(x), np.inf)
    H, hs, vs, border = hf["heights"].astype(np.float64), hf["hs"], hf["vs"], hf["border"]
    rows, cols = H.shape
    u0, v0 = (x + border) / hs, (y + border) / hs
    u, v = np.clip(u0, 0.0, rows - 1.0), np.clip(v0, 0.0, cols - 1.0)
    i, j = np.minimum(np.floor(u).astype(int), rows - 2), np.minimum(np.floor(v).astype(int), cols - 2)
    fu, fv = u - i, v - j
    low = fu >= fv  # the triangle (i,j), (i+1,j), (i+1,j+1); else (i,j), (i+1,j+1), (i,j+1)
    vert = lambda a, b: np.stack([a * hs - border, b * hs - border, H[a, b] * vs], -1)  # noqa: E731
    p00, p11 = vert(i, j), vert(i + 1, j + 1)
    third = np.where(low[:, None], vert(i + 1, j), vert(i, j + 1))
    nrm = np.where(low[:, None], np.cross(third - p00, p11 - p00), np.cross(p11 - p00, third - p00))
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    xc, yc = u * hs - border, v * hs - border
    h = p00[:, 2] - (nrm[:, 0] * (xc - p00[:, 0]) + nrm[:, 1] * (yc - p00[:, 1])) / nrm[:, 2]
    inf = np.full(len(x), np.inf)
    edge = np.minimum.reduce([np.abs(fu - fv),
                              np.where((u0 == u) & (i > 0), fu, inf), np.where((u0 == u) & (i < rows - 2), 1 - fu, inf),
                              np.where((v0 == v) & (j > 0), fv, inf), np.where((v0 == v) & (j < cols - 2), 1 - fv, inf)])
    return h, nrm, edge


def ground_frame(n, mut=()):
    """n, t1 = normalise(e_x - n_x n), t2 = n x t1."""
    t1 = np.array([1.0, 0.0, 0.0])
    if "tangent_no_orth" not in mut:
        t1 = t1 - n[0] * n
        t1 = t1 / np.linalg.norm(t1)
    return np.stack([n, t1, np.cross(n, t1)])


def self_frame(n):
    """A self contact's friction frame: as the ground's with e = x, or e = y when n is within
    acos(0.57735) of the x axis (lgs_self_collision_desc)."""
    e = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.57735 else np.array([0.0, 1.0, 0.0])
    t1 = e - (e @ n) * n
    t1 = t1 / np.linalg.norm(t1)
    return np.stack([n, t1, np.cross(n, t1)])


def segment_closest(p1, q1, p2, q2):
    """Closest points of two segments: the unconstrained minimum of |p1 + s d1 - p2 - t d2|^2 when it lies
    in the unit square, else the best of the four edges of the square (each a point-segment problem)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, b, c, f = d1 @ d1, d2 @ d2, d1 @ d2, d1 @ r, d2 @ r
    cands = []
    den = a * e - b * b
    if den > 1e-14 * a * e and a > 0 and e > 0:
        s, t = (b * f - c * e) / den, (a * f - b * c) / den
        if 0 <= s <= 1 and 0 <= t <= 1:
            cands.append((s, t))
    if not cands:
        for t in (0.0, 1.0):   # s free on [0, 1]
            cands.append((min(max((b * t - c) / a, 0.0), 1.0) if a > 0 else 0.0, t))
        for s in (0.0, 1.0):   # t free on [0, 1]
            cands.append((s, min(max((b * s + f) / e, 0.0), 1.0) if e > 0 else 0.0))
    s, t = min(cands, key=lambda st: np.sum((r + st[0] * d1 - st[1] * d2) ** 2))
    return p1 + s * d1, p2 + t * d2


def _target(sep, P, mut=()):
    if sep >= 0:
        return -sep / P["dt"]
    t = -P["baumgarte"] * sep / P["dt"]
    return t if "no_baumgarte_clamp" in mut else min(t, P["max_depenetration_velocity"])


def _rows(T, C, P, K, uf, q, friction, hf, sc, mut=()):
    """The substep's constraint rows in solve order (contact slots of include/leggedsim.h, then the joint
    limits in DOF order) with every activation margin and the counts per slot class."""
    maxc = P["max_contacts"]
    R, p = K["R"], K["p"]
    act_margin, terr_margin = [], [np.inf]
    # ground candidates
    prim, sec, seen = [], [], set()
    cen = p[T.pt_body] + mv(R[T.pt_body], C["pt_pos"])
    hgt, nrms, edges = terrain(hf, cen[:, 0], cen[:, 1])
    seps = (cen[:, 2] - hgt) * nrms[:, 2] - C["pt_radius"] - P["rest_offset"]
    act_margin += list(np.abs(seps - P["contact_offset"]))
    terr_margin += list(edges[seps < 2 * P["contact_offset"] + 0.01])
    for k in np.nonzero(seps < P["contact_offset"])[0]:
        b, n = int(T.pt_body[k]), nrms[k]
        g = dict(b=b, b2=-1, pt=cen[k] - C["pt_radius"][k] * n, sep=seps[k], n=n, kind="ground", cand=int(k))
        if b not in seen:
            seen.add(b)
            prim.append(g)
        else:
            sec.append(g)
    # self contacts
    selfc = []
    if sc is not None:
        caps = np.asarray(sc["capsules"], np.float64)
        for (i, k) in sc["pairs"]:
            a, b = int(sc["proxy_body"][i]), int(sc["proxy_body"][k])
            c1, c2 = segment_closest(p[a] + R[a] @ caps[i, 0:3], p[a] + R[a] @ caps[i, 3:6],
                                     p[b] + R[b] @ caps[k, 0:3], p[b] + R[b] @ caps[k, 3:6])
            dist = np.linalg.norm(c1 - c2)
            n = (c1 - c2) / dist if dist > 1e-9 else np.array([0.0, 0.0, 1.0])
            sep = dist - caps[i, 6] - caps[k, 6] - P["rest_offset"]
            act_margin.append(abs(sep - P["contact_offset"]))
            if sep < P["contact_offset"]:
                selfc.append(dict(b=a, b2=b, pt=0.5 * ((c1 - caps[i, 6] * n) + (c2 + caps[k, 6] * n)), sep=sep, n=n,
                                  kind="self"))
    npg = min(len(prim), maxc)
    nsc = min(len(selfc), sc["max_self_contacts"] if sc is not None else 0, maxc - npg)
    nsu = min(len(sec), maxc - npg - nsc)
    slots = prim[:npg] + sec[:nsu] + selfc[:nsc]  # solve order: the ground contacts, then the self contacts
    mu_ground = friction if "mu_not_averaged" in mut else 0.5 * (P["ground_friction"] + friction)
    J, tgt, kind, mu, frames = [], [], [], [], []
    for g in slots:
        if g["kind"] == "ground":
            fr = ground_frame(g["n"], mut)
            Jp = _point_jac(T, K, g["b"], g["pt"])
            mu.append(mu_ground)
        else:
            fr = self_frame(g["n"])
            Jp = _point_jac(T, K, g["b"], g["pt"])
            if "self_no_second" not in mut:
                Jp = Jp - _point_jac(T, K, g["b2"], g["pt"])
            mu.append(friction)
        J += [fr[0] @ Jp, fr[1] @ Jp, fr[2] @ Jp]
        tgt += [_target(g["sep"], P, mut), 0.0, 0.0]
        kind += [0, 1, 2]
        frames.append(fr)
    # joint limits on the predicted position
    cap = P["max_rows"] - 3 * maxc + 3 * (maxc - len(slots))
    nl, lim_margin = 0, []
    for j in range(T.D):
        lo, hi = C["dof_lower"][j], C["dof_upper"][j]
        qn = q[j] + P["dt"] * uf[6 + j]
        lim_margin.append(min(abs(qn - lo), abs(qn - hi)))
        if not qn < lo and not qn > hi:
            continue
        nl += 1
        if nl > cap:
            continue
        row = np.zeros(6 + T.D)
        lower = qn < lo
        row[6 + j] = (1.0 if lower else -1.0) * (-1.0 if "limit_sign" in mut else 1.0)
        gap = q[j] - lo if lower else hi - q[j]
        J.append(row)
        tgt.append(-gap / P["dt"] if gap >= 0 else -P["baumgarte"] * gap / P["dt"])
        kind.append(0)
    counts = dict(primary=npg, secondary=nsu, self=nsc, limits=min(nl, cap), candidates=len(prim) + len(sec),
                  dropped=(len(prim) - npg, len(selfc) - nsc, max(nl - cap, 0)))
    return dict(J=np.array(J).reshape(-1, 6 + T.D), tgt=np.array(tgt), kind=np.array(kind, int), mu=np.array(mu),
                slots=slots, frames=frames, counts=counts, act_margin=np.array(act_margin),
                near=(int(np.sum(np.array(act_margin[:len(T.pt_body)]) < ACT_MARGIN)),
                      int(np.sum(np.array(act_margin[len(T.pt_body):]) < ACT_MARGIN)),
                      int(np.sum(np.array(lim_margin) < LIMIT_MARGIN))),
                lim_margin=np.array(lim_margin), terr_margin=min(terr_margin))


def pgs(A, vfree, tgt, kind, mu, sweeps):
    """Projected Gauss-Seidel in row order on v = vfree + A lam: unilateral rows lam >= 0 towards v = tgt;
    every friction pair moved together by its rows' diagonals (+1e-9) and projected onto the disc of
    radius mu lam_n.  Returns lam, v and each pair's relative cone margin in the last sweep."""
    nr = len(tgt)
    lam, v = np.zeros(nr), vfree.copy()
    inv = 1.0 / (np.diag(A) + 1e-9) if nr else np.zeros(0)
    cone = np.ones(len(mu))
    for _ in range(sweeps):
        for r in range(nr):
            if kind[r] == 0:
                ln = max(0.0, lam[r] + (tgt[r] - v[r]) * inv[r])
                v += A[:, r] * (ln - lam[r])
                lam[r] = ln
            elif kind[r] == 1:
                lim = mu[r // 3] * lam[r - 1]
                l = np.array([lam[r] - v[r] * inv[r], lam[r + 1] - v[r + 1] * inv[r + 1]])
                n2 = l @ l
                cone[r // 3] = abs(n2 - lim * lim) / max(n2, lim * lim, 1e-300) if max(n2, lim * lim) > 0 else 1.0
                if n2 > lim * lim:
                    l = l * (lim / np.sqrt(n2))
                v += A[:, r] * (l[0] - lam[r]) + A[:, r + 1] * (l[1] - lam[r + 1])
                lam[r:r + 2] = l
    return lam, v, cone


def lcp_residuals(rows, lam, v, A):
    """How far (lam, v = vfree + A lam) is from the contact problem's conditions.  Velocities in m/s (rad/s),
    impulses in N s: negative impulse, normal velocity below its target, complementarity lam (v - tgt),
    friction outside the cone, the tangential velocity of pairs inside it, and for pairs on the cone the part
    of the friction impulse that does not oppose the sliding velocity (relative).  The documented projection
    moves the two rows of a pair by their own diagonals d1, d2, so its fixed point opposes (v1/d1, v2/d2):
    the sliding direction in the metric of the pair's diagonal, exact when d1 == d2."""
    dg = np.diag(A) + 1e-9
    kind, tgt, mu = rows["kind"], rows["tgt"], rows["mu"]
    out = dict(neg=0.0, below=0.0, compl=0.0, cone=0.0, oppose=0.0, stick=0.0)
    for r in np.nonzero(kind == 0)[0]:
        out["neg"] = max(out["neg"], -lam[r])
        out["below"] = max(out["below"], tgt[r] - v[r])
        out["compl"] = max(out["compl"], abs(lam[r] * (v[r] - tgt[r])))
    for r in np.nonzero(kind == 1)[0]:
        lim, l, vt = mu[r // 3] * lam[r - 1], lam[r:r + 2], v[r:r + 2]
        nl, nv = np.linalg.norm(l), np.linalg.norm(vt / dg[r:r + 2])
        out["cone"] = max(out["cone"], nl - lim)
        if nl < lim * (1 - 1e-6):      # inside the cone: sticking
            out["stick"] = max(out["stick"], np.linalg.norm(vt))
        elif nl > 0 and np.linalg.norm(vt) > 1e-7:   # on it: the impulse opposes the sliding velocity
            out["oppose"] = max(out["oppose"], np.linalg.norm(l / nl + vt / dg[r:r + 2] / nv))
    return out


# ------------------------------------------------------------------ one substep --
def _finish(T, C, P, s, dyn, hf, sc, mut=(), sweeps=None):
    """Rows, solve and integration of one (unbatched) case after its dynamics."""
    K, M, uf = dyn["K"], dyn["M"], dyn["uf"]
    dt = P["dt"]
    rows = _rows(T, C, P, K, uf, s["q"], float(s["friction"]), hf, sc, mut)
    J = rows["J"]
    MiJt = np.linalg.solve(M, J.T) if len(J) else np.zeros((6 + T.D, 0))
    A = J @ MiJt
    vfree = J @ uf
    lam, v, cone = pgs(A, vfree, rows["tgt"], rows["kind"], rows["mu"], P["solver_iterations"] if sweeps is None else sweeps)
    un = uf + MiJt @ lam
    if P["clamp_joint_velocity"]:
        lim = C["dof_velocity"]
        un[6:] = np.where(lim > 0, np.clip(un[6:], -lim, lim), un[6:])
    cforce = np.zeros((T.B, 3))
    for c, g in enumerate(rows["slots"]):
        F = (lam[3 * c:3 * c + 3] @ rows["frames"][c]) / dt
        cforce[g["b"]] += F
        if g["b2"] >= 0:
            cforce[g["b2"]] -= F
    # semi-implicit Euler
    w, vO = un[0:3], un[3:6]
    pos = s["pos"] + dt * vO
    x, y, z, qw = s["quat"]
    quat = s["quat"] + 0.5 * dt * np.array([qw * w[0] + w[1] * z - w[2] * y, qw * w[1] + w[2] * x - w[0] * z,
                                             qw * w[2] + w[0] * y - w[1] * x, -(w[0] * x + w[1] * y + w[2] * z)])
    quat = quat / np.linalg.norm(quat)
    vcom = vO + np.cross(w, quat_to_mat(quat) @ C["com"][0])
    out = dict(pos=pos, quat=quat, vlin=vcom, vang=w, q=s["q"] + dt * un[6:], qd=un[6:].copy(), cforce=cforce,
               u=un, uf=uf, lam=lam, v=v, A=A, vfree=vfree, rows=rows, cone_margin=cone, counts=rows["counts"],
               M=M)
    out["margins"] = dict(act=float(rows["act_margin"].min()) if len(rows["act_margin"]) else np.inf,
                          limit=float(rows["lim_margin"].min()),
                          cone=float(cone.min()) if len(cone) else np.inf, terrain=float(rows["terr_margin"]))
    out["excluded"] = bool(out["margins"]["act"] < ACT_MARGIN or out["margins"]["limit"] < LIMIT_MARGIN
                           or out["margins"]["cone"] < CONE_MARGIN)
    return out


def _sc_dict(sc):
    if sc is None or len(sc.pairs) == 0:
        return None
    return dict(proxy_body=np.asarray(sc.proxy_body), capsules=np.asarray(sc.capsules, np.float64),
                pairs=[(int(i), int(k)) for i, k in np.asarray(sc.pairs)], max_self_contacts=int(sc.max_self_contacts))


def _hf_dict(hf):
    if hf is None:
        return None
    return dict(heights=np.asarray(hf["heights"], np.int16), hs=float(np.float32(hf["hs"])),
                vs=float(np.float32(hf["vs"])), border=float(np.float32(hf["border"])))


def step(fam, e, mut=(), sweeps=None):
    """The reference substep of env e of a family."""
    T, C = topo_of(fam.model), consts_of(fam.model)
    s = _inputs(fam, e)
    dyn = _dynamics(T, C, fam.params, s, mut)
    return _finish(T, C, fam.params, s, dyn, _hf_dict(fam.hf), _sc_dict(fam.sc), mut, sweeps)


def _batch_inputs(fam):
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    r = f(fam.root)
    return dict(pos=r[:, 0:3], quat=r[:, 3:7], vcom=r[:, 7:10], w=r[:, 10:13], q=f(fam.q), qd=f(fam.qd), tau=f(fam.tau),
                friction=f(fam.friction), added_mass=f(fam.added_mass))


def dynamics(fam, mut=()):
    """M, u, the acceleration acc = M^-1 (tau_gen - bias), the Jacobians JV / JW [N,B,3,n] and J' u (adv, adw)
    of every env of a family."""
    return _dynamics(topo_of(fam.model), consts_of(fam.model), fam.params, _batch_inputs(fam), mut)


def step_all(fam, mut=(), sweeps=None):
    """step for every env (the dynamics of the whole family in one batch)."""
    T, C = topo_of(fam.model), consts_of(fam.model)
    s = _batch_inputs(fam)
    dyn = _dynamics(T, C, fam.params, s, mut)
    hf, sc = _hf_dict(fam.hf), _sc_dict(fam.sc)
    out = []
    for e in range(fam.n):
        de = {k: (v[e] if k != "K" else {kk: vv[e] for kk, vv in v.items()}) for k, v in dyn.items()}
        out.append(_finish(T, C, fam.params, {k: v[e] for k, v in s.items()}, de, hf, sc, mut, sweeps))
    return out


def sensitivity(fam, e, k=32, seed=0):
    """How far fp32 rounding of the inputs alone moves the true answer: the case is evaluated k times with
    the state, tau, the env's properties, the sim parameters and every model constant each perturbed by an
    independent random relative error of at most 2^-23; returns max - min per quantity group (the largest
    over the group's entries)."""
    T, C = topo_of(fam.model), consts_of(fam.model)
    rng = np.random.default_rng([seed, e])
    pert = lambda a: np.asarray(a, np.float64) * (1 + EPS32 * rng.uniform(-1, 1, (k,) + np.shape(a)))  # noqa: E731
    s = {key: pert(v) for key, v in _inputs(fam, e).items()}
    Ck = {key: pert(v) for key, v in C.items()}
    Pk = dict(fam.params)
    for key in PARAM_FLOATS + ("gravity",):
        Pk[key] = pert(fam.params[key])
    dyn = _dynamics(T, Ck, Pk, s)
    hf, sc = _hf_dict(fam.hf), _sc_dict(fam.sc)
    outs = []
    for i in range(k):
        Pi = dict(fam.params)
        Pi.update({key: (Pk[key][i] if key == "gravity" else float(Pk[key][i])) for key in PARAM_FLOATS + ("gravity",)})
        hfi = None if hf is None else dict(hf, hs=hf["hs"] * (1 + EPS32 * rng.uniform(-1, 1)),
                                           vs=hf["vs"] * (1 + EPS32 * rng.uniform(-1, 1)),
                                           border=hf["border"] * (1 + EPS32 * rng.uniform(-1, 1)))
        sci = None if sc is None else dict(sc, capsules=sc["capsules"] * (1 + EPS32 * rng.uniform(-1, 1, sc["capsules"].shape)))
        de = {key: (v[i] if key != "K" else {kk: vv[i] for kk, vv in v.items()}) for key, v in dyn.items()}
        outs.append(_finish(T, {key: v[i] for key, v in Ck.items()}, Pi, {key: v[i] for key, v in s.items()}, de, hfi, sci))
    spread = {}
    for g in GROUPS:
        a = np.stack([o[g] for o in outs])
        if g == "quat":
            a = a * np.sign(a @ a[0])[:, None]
        spread[g] = float((a.max(0) - a.min(0)).max())
    return spread


def tolerance_of(spread, ref, margin=None):
    """Per quantity group: margin x spread, floored at 4 fp32 ulps of the group's largest magnitude."""
    margin = MARGIN if margin is None else margin
    return {g: max(margin * spread[g], 4 * EPS32 * float(np.abs(ref[g]).max())) for g in GROUPS}


def tolerances(fam, e, ref, k=32, margin=None):
    sp = sensitivity(fam, e, k)
    return tolerance_of(sp, ref, margin), sp


def deviation(ref, got):
    """max |got - ref| per quantity group; got: dict with root [13], q, qd, cforce [B,3]."""
    d = {}
    root = np.asarray(got["root"], np.float64)
    qg = root[3:7] * (1.0 if root[3:7] @ ref["quat"] >= 0 else -1.0)
    d["pos"] = np.abs(root[0:3] - ref["pos"]).max()
    d["quat"] = np.abs(qg - ref["quat"]).max()
    d["vlin"] = np.abs(root[7:10] - ref["vlin"]).max()
    d["vang"] = np.abs(root[10:13] - ref["vang"]).max()
    d["q"] = np.abs(np.asarray(got["q"], np.float64) - ref["q"]).max()
    d["qd"] = np.abs(np.asarray(got["qd"], np.float64) - ref["qd"]).max()
    d["cforce"] = np.abs(np.asarray(got["cforce"], np.float64) - ref["cforce"]).max()
    return d


# ------------------------------------------------------------------ case generators --
# Deterministic seeds; the same float32 arrays go to the oracle, to the HIP kernel and (as fp64) to the
# reference.  `spec` is a host env spec (hostspec.make_spec): its model, default pose and lgs_sim_params.
def quat_rpy(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), \
        np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


def touchdown_z(model, quat, q, gap, hf=None, xy=(0.0, 0.0)):
    """The root height at which the lowest contact candidate of the posed robot has separation `gap`."""
    T, C = topo_of(model), consts_of(model)
    K = _kin(T, C, np.array([xy[0], xy[1], 0.0]), quat_to_mat(np.asarray(quat, np.float64)), np.asarray(q, np.float64))
    cen = K["p"][T.pt_body] + mv(K["R"][T.pt_body], C["pt_pos"])
    h, n, _ = terrain(_hf_dict(hf), cen[:, 0], cen[:, 1])
    sep0 = (cen[:, 2] - h) * n[:, 2] - C["pt_radius"]   # at root z = 0; moves by n_z per unit of z
    return float(np.max((gap - sep0) / n[:, 2]))


def _family(name, spec, N, over, rng):
    D = spec.num_dof
    fam = Family(name, spec.model, params_of(spec.sim_params, **over), np.zeros((N, 13), np.float32),
                 np.tile(np.asarray(spec.default_dof_pos, np.float32).reshape(1, D), (N, 1)),
                 np.zeros((N, D), np.float32), np.zeros((N, D), np.float32), np.ones(N, np.float32),
                 np.zeros(N, np.float32))
    fam.root[:, 6] = 1.0
    fam.root[:, 2] = 5.0
    fam.meta["over"] = dict(over)
    return fam


def _added_mass(fam, rng):
    """A third of the envs each: none, heavier, lighter."""
    N = fam.n
    dm = np.where(np.arange(N) % 3 == 1, rng.uniform(0.5, 3.0, N), np.where(np.arange(N) % 3 == 2, -rng.uniform(0.2, 1.0, N), 0.0))
    fam.added_mass[:] = dm


def flight(spec, variant):
    """Family 1.  variant 0: gravity (0,0,-9.81), armature 0, no velocity clamp, 67 envs; variant 1: gravity
    (1,-2,-9), armature 0.01, clamp on with two joints per env above their velocity limit, 64 envs."""
    over = [dict(armature=0.0, clamp_joint_velocity=0, gravity=(0.0, 0.0, -9.81)),
            dict(armature=0.01, clamp_joint_velocity=1, gravity=(1.0, -2.0, -9.0))][variant]
    N = (67, 64)[variant]
    rng = np.random.default_rng(100 + variant)
    fam = _family(f"flight{variant}", spec, N, over, rng)
    m, D = spec.model, spec.num_dof
    qt = rng.normal(size=(N, 4))
    fam.root[:, 3:7] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
    fam.root[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    fam.root[:, 7:13] = rng.uniform(-3, 3, (N, 6))
    fam.q[:] = m.dof_lower + rng.uniform(0.2, 0.8, (N, D)) * (m.dof_upper - m.dof_lower)
    fam.qd[:] = rng.uniform(-3, 3, (N, D))
    if variant == 1:
        for e in range(N):
            for j in rng.choice(D, 2, replace=False):
                fam.qd[e, j] = rng.choice([-1.0, 1.0]) * m.dof_velocity[j] * rng.uniform(1.02, 1.2)
    fam.tau[:] = rng.uniform(-0.5, 0.5, (N, D)) * m.dof_effort
    _added_mass(fam, rng)
    return fam


def parent_child_dofs(model):
    return [(int(model.dof[model.parent[b]]), int(model.dof[b])) for b in range(1, model.num_bodies)
            if model.dof[b] >= 0 and model.dof[model.parent[b]] >= 0]


def joint_limits(spec, rows=None):
    """Family 2, in flight, 65 envs (with `rows`: the same cases with one contact slot and `rows` constraint
    rows, so that in flight `rows` limits fit and an env with more drops the rest: the limit counter).  Two to four joints per env, each in one of four states: about to cross
    its lower / upper limit from inside, or already beyond it (the Baumgarte branch); every fourth env has
    a parent-child pair among them.  meta["mode"][e, j]: 0 free, 1 lower cross, 2 upper cross, 3 lower
    beyond, 4 upper beyond."""
    N = 65
    rng = np.random.default_rng(200)
    over = dict(clamp_joint_velocity=0) if rows is None else dict(clamp_joint_velocity=0, max_contacts=1, max_rows=rows)
    fam = _family("limits" if rows is None else "limits_over", spec, N, over, rng)
    m, D, dt = spec.model, spec.num_dof, fam.params["dt"]
    qt = rng.normal(size=(N, 4))
    fam.root[:, 3:7] = qt / np.linalg.norm(qt, axis=1, keepdims=True)
    fam.root[:, 7:13] = rng.uniform(-1, 1, (N, 6))
    fam.q[:] = m.dof_lower + rng.uniform(0.3, 0.7, (N, D)) * (m.dof_upper - m.dof_lower)
    fam.qd[:] = rng.uniform(-1, 1, (N, D))
    fam.tau[:] = rng.uniform(-0.03, 0.03, (N, D)) * m.dof_effort
    pairs = parent_child_dofs(m)
    mode = np.zeros((N, D), int)
    for e in range(N):
        js = list(pairs[rng.integers(len(pairs))]) if e % 4 == 0 else []
        while len(js) < 2 + e % 3:
            j = int(rng.integers(D))
            if j not in js:
                js.append(j)
        for j in js:
            md = int(rng.integers(1, 5))
            mode[e, j] = md
            lo, hi = m.dof_lower[j], m.dof_upper[j]
            if md == 1:
                fam.q[e, j], fam.qd[e, j] = lo + 0.2 * 0.02 * dt / 0.005, -4.0 * rng.uniform(0.8, 1.2)
            elif md == 2:
                fam.q[e, j], fam.qd[e, j] = hi - 0.2 * 0.02 * dt / 0.005, 4.0 * rng.uniform(0.8, 1.2)
            elif md == 3:
                fam.q[e, j], fam.qd[e, j] = lo - rng.uniform(0.003, 0.02), rng.uniform(-1, 1)
            else:
                fam.q[e, j], fam.qd[e, j] = hi + rng.uniform(0.003, 0.02), rng.uniform(-1, 1)
    fam.meta["mode"] = mode
    return fam


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _stance(fam, spec, rng, e, hf=None, xy=(0.0, 0.0), tilt=0.01, gap=None, q=None, roll0=0.0, align=False):
    """Env e: the pose q (default: the default pose) with a small tilt (about the ground's normal under the
    root with `align`), lowered until its lowest candidate sits between 2 mm of penetration and 8 mm of
    gap (or at `gap`)."""
    quat = quat_rpy(roll0 + rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-np.pi, np.pi))
    if align:
        n = terrain(_hf_dict(hf), xy[0], xy[1])[1][0]
        ax = np.cross([0.0, 0.0, 1.0], n)
        sn = np.linalg.norm(ax)
        if sn > 0:
            half = 0.5 * np.arctan2(sn, n[2])
            quat = quat_mul(np.append(ax / sn * np.sin(half), np.cos(half)), quat)
    if q is not None:
        fam.q[e] = q
    fam.root[e, 3:7] = quat
    fam.root[e, 0:2] = xy
    g = rng.uniform(-0.002, 0.008) if gap is None else gap
    fam.root[e, 2] = touchdown_z(fam.model, fam.root[e, 3:7], fam.q[e], g, hf, fam.root[e, 0:2])
    return g


def _terrain_margin(fam, e):
    T, C = topo_of(fam.model), consts_of(fam.model)
    r = np.asarray(fam.root[e], np.float64)
    K = _kin(T, C, r[0:3], quat_to_mat(r[3:7]), np.asarray(fam.q[e], np.float64))
    cen = K["p"][T.pt_body] + mv(K["R"][T.pt_body], C["pt_pos"])
    h, n, edge = terrain(_hf_dict(fam.hf), cen[:, 0], cen[:, 1])
    near = (cen[:, 2] - h) * n[:, 2] - C["pt_radius"] < 0.05
    return float(edge[near].min()) if near.any() else np.inf


def plane_contacts(spec, sweeps=None, feet_only=False, N=129):
    """Family 3 (and 7 with `sweeps`, feet only).  Default pose on the plane, feet between 2 mm of penetration
    and 8 mm of gap, root tangential velocity 0 for 2 envs in 8 and up to 2 m/s for the others, friction
    0.3 / 1.0 / 1.5 per env; every 8th env penetrates 30-45 mm (the depenetration clamp), and (not
    feet_only) every 5th env is crouched so that links other than the feet touch as well."""
    rng = np.random.default_rng(300)
    over = {} if sweeps is None else dict(solver_iterations=sweeps)
    fam = _family("plane" if sweeps is None else f"sweeps{sweeps}", spec, N, over, rng)
    m, D = spec.model, spec.num_dof
    crouch = fam.meta["crouch"] = np.zeros(N, bool)
    for e in range(N):
        deep = e % 8 == 5
        if not feet_only and e % 5 == 4:
            crouch[e] = True
            w = rng.uniform(0.85, 1.0, D)
            qc = np.where(rng.random(D) < 0.5, m.dof_lower, m.dof_upper) * w + fam.q[e] * (1 - w)
            g = _stance(fam, spec, rng, e, tilt=0.3, q=qc, gap=rng.uniform(-0.002, 0.002))
        else:
            g = _stance(fam, spec, rng, e, gap=-rng.uniform(0.03, 0.045) if deep else None)
        still = e % 8 < 2
        vt = 0.0 if still else rng.uniform(0.05, 2.0)
        ang = rng.uniform(0, 2 * np.pi)
        fam.root[e, 7:10] = [vt * np.cos(ang), vt * np.sin(ang), -(max(g, 0.0) / fam.params["dt"] + rng.uniform(0.05, 0.4))]  # the lowest candidate closes its gap and loads
        fam.root[e, 10:13] = rng.uniform(-0.3, 0.3, 3) * (0.0 if still else 1.0)
        fam.qd[e] = rng.uniform(-0.5, 0.5, D) * (0.0 if still else 1.0)
        fam.friction[e] = (0.3, 1.0, 1.5)[e % 3]
    fam.tau[:] = rng.uniform(-0.1, 0.1, (N, D)) * m.dof_effort
    if not feet_only:
        _added_mass(fam, rng)
    return fam


def over_capacity(spec):
    """Family 4, 64 envs: the robot on its side (roll +-90 degrees), pressed 3-6 mm into the plane (a robot whose
    soles have several candidates: every other env standing with both soles pressed in flat), so more
    candidates touch than the 4 contact slots (max_rows 20) this family runs with can take."""
    N = 64
    rng = np.random.default_rng(400)
    fam = _family("overcap", spec, N, dict(max_contacts=4, max_rows=20), rng)
    D = spec.num_dof
    flat_soles = int(np.sum(spec.model.pt_body == spec.feet_indices[0])) > 1
    for e in range(N):
        if flat_soles and e % 2:   # several candidates per sole: standing with both soles pressed in flat
            _stance(fam, spec, rng, e, tilt=0.002, gap=-rng.uniform(0.003, 0.006))
        else:
            _stance(fam, spec, rng, e, tilt=0.01, gap=-rng.uniform(0.003, 0.006), roll0=(np.pi / 2) * (1 if e % 4 < 2 else -1))
        fam.root[e, 7:13] = rng.uniform(-0.3, 0.3, 6)
        fam.qd[e] = rng.uniform(-0.5, 0.5, D)
        fam.friction[e] = (0.3, 1.0, 1.5)[e % 3]
    fam.tau[:] = rng.uniform(-0.1, 0.1, (N, D)) * spec.model.dof_effort
    return fam


def small_heightfield():
    """14 x 12 int16 samples, 0.25 m apart, 5 mm units, 1 m border: a slope of 0.3 in x over the first rows
    (15 units per sample), a 0.1 m step down, then a cross slope of 0.2 in y."""
    H = np.zeros((14, 12), np.int16)
    for i in range(14):
        for j in range(12):
            H[i, j] = 15 * min(i, 7) - (20 if i >= 8 else 0) + (10 * j if i >= 10 else 0)
    return dict(heights=H, hs=0.25, vs=0.005, border=1.0)


def heightfield(spec):
    """Family 5, 67 envs: the default pose set down at random places of small_heightfield (random yaw, so the
    feet fall on both triangles of a cell, on neighbouring cells and across the step); env 0 stands outside
    the map, where the edge samples continue."""
    N = 67
    rng = np.random.default_rng(500)
    fam = _family("heightfield", spec, N, {}, rng)
    fam.hf = small_heightfield()
    D = spec.num_dof
    for e in range(N):
        while True:  # redrawn until no candidate near the ground is within 1e-3 cells of a triangle's edge
            xy = (-2.5, 0.4) if e == 0 else (rng.uniform(-0.6, 1.9), rng.uniform(-0.6, 1.4))
            g = _stance(fam, spec, rng, e, hf=fam.hf, xy=xy, tilt=0.01 if e % 2 else 0.1, align=True)
            if _terrain_margin(fam, e) > 1e-3:
                break
        vt = 0.0 if e % 8 < 3 else rng.uniform(0.05, 1.0)
        ang = rng.uniform(0, 2 * np.pi)
        fam.root[e, 7:10] = [vt * np.cos(ang), vt * np.sin(ang), -(max(g, 0.0) / fam.params["dt"] + rng.uniform(0.05, 0.4))]
        fam.qd[e] = rng.uniform(-0.5, 0.5, D) * (0.0 if e % 8 < 3 else 1.0)
        fam.friction[e] = (0.3, 1.0, 1.5)[e % 3]
    fam.tau[:] = rng.uniform(-0.1, 0.1, (N, D)) * spec.model.dof_effort
    return fam


def self_separations(model, sc, q):
    """Surface distance of every tested proxy pair at joint angles q (root frame)."""
    T, C = topo_of(model), consts_of(model)
    K = _kin(T, C, np.zeros(3), np.eye(3), np.asarray(q, np.float64))
    R, p, caps = K["R"], K["p"], np.asarray(sc.capsules, np.float64)
    out = []
    for i, k in np.asarray(sc.pairs):
        a, b = int(sc.proxy_body[i]), int(sc.proxy_body[k])
        c1, c2 = segment_closest(p[a] + R[a] @ caps[i, 0:3], p[a] + R[a] @ caps[i, 3:6],
                                 p[b] + R[b] @ caps[k, 0:3], p[b] + R[b] @ caps[k, 3:6])
        out.append(np.linalg.norm(c1 - c2) - caps[i, 6] - caps[k, 6])
    return np.array(out)


def crossed_poses(spec, want=4, seed=600, tries=3000):
    """Joint vectors near the default pose in which one to three tested pairs touch (5-30 mm deep at most)."""
    m, sc = spec.model, spec.self_collision
    rng = np.random.default_rng(seed)
    q0 = np.asarray(spec.default_dof_pos, np.float64).reshape(-1)
    found = []
    for _ in range(tries):
        q = np.clip(q0 + rng.normal(0, 0.4, m.num_dofs), m.dof_lower + 0.05, m.dof_upper - 0.05)
        seps = self_separations(m, sc, q)
        hit = seps < 0.008
        if 1 <= hit.sum() <= 3 and -0.03 < seps.min() < -0.005 and not np.any((seps > 0.008) & (seps < 0.012)):
            found.append((q.astype(np.float32), int(hit.sum())))
            if len(found) == want:
                break
    assert len(found) == want, f"{m.name}: only {len(found)} crossed poses"
    return found


def self_contacts(spec):
    """Family 6, 64 envs: crossed-leg poses (+- 3 mrad per joint) in which one to three proxy pairs touch; even
    envs in flight, odd envs set down on the plane (so the self contacts take the slots after one per
    touching ground body)."""
    N = 64
    rng = np.random.default_rng(601)
    fam = _family("self", spec, N, dict(clamp_joint_velocity=0), rng)
    fam.sc = replace(spec.self_collision, max_self_contacts=2)   # three touching pairs: one goes without a slot
    D = spec.num_dof
    poses = crossed_poses(spec)
    fam.meta["pairs_touching"] = [c for _, c in poses]
    for e in range(N):
        q = poses[e % len(poses)][0] + rng.uniform(-0.003, 0.003, D).astype(np.float32)
        if e % 2:
            _stance(fam, spec, rng, e, q=q, tilt=0.05, gap=rng.uniform(-0.002, 0.004))
        else:
            fam.q[e] = q
            qt = rng.normal(size=4)
            fam.root[e, 3:7] = qt / np.linalg.norm(qt)
        fam.root[e, 7:13] = rng.uniform(-0.3, 0.3, 6)
        fam.qd[e] = rng.uniform(-1, 1, D)
        fam.friction[e] = (0.3, 1.0, 1.5)[e % 3]
    fam.tau[:] = rng.uniform(-0.1, 0.1, (N, D)) * spec.model.dof_effort
    return fam
