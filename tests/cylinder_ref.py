"""Test-side restatement of the sphere-cylinder rule of include/idto_model.h, and the models the oracle can evaluate
in a cylinder's place.

`sphere_cylinder` is the closed form as the header states it, in numpy, with no reduction: it is what the host and GPU
tests compare phi, n, Ca and Cb with.

The oracle knows no cylinders.  `frozen_model` builds, for one configuration, the model whose pair k holds, in a
cylinder's place, the primitive that equals the cylinder in the region of the sphere's centre there:
  * side (outside beside the cylinder, or inside with R - r <= H - |c.z| and r > 0): a sphere of radius R on the axis;
  * cap (above or below a cap with r <= R, inside nearer to a cap, and r == 0 inside): a box of half extents (R, R, H);
  * rim (r > R and |c.z| > H): a sphere of radius 0 at the rim point.
It is frozen again at every perturbed configuration (`frozen_expectation`), as capsule_ref.frozen_sphere_model is.
The oracle and Model.validate accept a sphere of radius 0 (tests/test_model_cylinder.py evaluates one), so rim states
are held by all three yardsticks."""
import copy

import numpy as np

from capsule_ref import geom_world, without_geometry
from idto_amd.model import GEOM_TYPES
from oracle_lib import Oracle

SPHERE, BOX, CYLINDER = GEOM_TYPES["sphere"], GEOM_TYPES["box"], GEOM_TYPES["cylinder"]


def sphere_cylinder(x, rho, p, RX, R, H, sphere_is_A=True):
    """dict(phi, n, Ca, Cb, region) of a sphere (centre x, radius rho) against the cylinder (centre p, rotation RX, radius R,
    half length H): include/idto_model.h, term by term"""
    x, p, RX = np.asarray(x, float), np.asarray(p, float), np.asarray(RX, float)
    c = RX.T @ (x - p)
    r = float(np.sqrt(c[0] * c[0] + c[1] * c[1]))
    e = np.array([c[0], c[1], 0.0]) / r if r != 0 else np.array([1.0, 0.0, 0.0])
    z = np.array([0.0, 0.0, 1.0])
    if r > R or abs(c[2]) > H:
        rn, zn = min(r, R), min(max(c[2], -H), H)
        dv = np.array([r - rn, c[2] - zn])
        dist = float(np.sqrt(dv @ dv))
        g2 = dv / dist
        phi = dist - rho
        region = "rim" if (r > R and abs(c[2]) > H) else ("side" if r > R else "cap")
    else:
        dr, dz = R - r, H - abs(c[2])
        if dr <= dz:
            g2, rn, zn, phi, region = np.array([1.0, 0.0]), R, c[2], -dr - rho, "inside-side"
        else:
            s = 1.0 if c[2] >= 0 else -1.0
            g2, rn, zn, phi, region = np.array([0.0, s]), r, s * H, -dz - rho, "inside-cap"
    gW = RX @ (e * g2[0] + z * g2[1])
    on_cyl = p + RX @ (e * rn + z * zn)
    on_sph = x - gW * rho
    if sphere_is_A:
        return dict(phi=phi, n=-gW, Ca=on_sph, Cb=on_cyl, region=region)
    return dict(phi=phi, n=gW, Ca=on_cyl, Cb=on_sph, region=region)


def substitute(x, p, RX, R, H):
    """(type, world centre, size) of the primitive that stands for the cylinder with the sphere's centre at x"""
    c = RX.T @ (x - p)
    r, az = float(np.sqrt(c[0] * c[0] + c[1] * c[1])), abs(c[2])
    if az > H:
        if r <= R:
            return BOX, p, np.array([R, R, H])
        return SPHERE, p + RX @ np.array([c[0] * (R / r), c[1] * (R / r), H if c[2] >= 0 else -H]), np.zeros(3)
    if r <= R and not (R - r <= H - az and r > 0):
        return BOX, p, np.array([R, R, H])
    return SPHERE, p + RX @ np.array([0.0, 0.0, c[2]]), np.array([R, 0.0, 0.0])


def frozen_model(model, X_body):
    """The model with one geometry per (pair, side), pair k = (2k, 2k + 1) in the same order and path: a cylinder side is
    its region's substitute for the body poses X_body [nb, 12], in its body's frame (a box keeps the cylinder's frame);
    every other side is copied."""
    m = copy.deepcopy(model)
    gb, gt, gs, gx = [], [], [], []
    for k in range(model.npairs):
        pair = (int(model.pair_a[k]), int(model.pair_b[k]))
        for g, other in zip(pair, pair[::-1]):
            b, t = int(model.geom_body[g]), int(model.geom_type[g])
            x, size = np.array(model.geom_X[g], float), np.array(model.geom_size[g], float)
            if t == CYLINDER:
                assert int(model.geom_type[other]) == SPHERE
                RX, p = geom_world(model, X_body, g)
                t, c, size = substitute(geom_world(model, X_body, other)[1], p, RX, size[0], size[1])
                if t == SPHERE:
                    if b >= 0:
                        Rb, pb = X_body[b][:9].reshape(3, 3), X_body[b][9:]
                        c = Rb.T @ (c - pb)
                    x = np.concatenate([np.eye(3).ravel(), c])
            gb.append(b); gt.append(t); gs.append(size); gx.append(x)
    m.geom_body, m.geom_type, m.geom_size, m.geom_X = gb, gt, gs, gx
    m.pair_a = np.arange(0, 2 * model.npairs, 2)
    m.pair_b = m.pair_a + 1
    m.pair_path = np.array(model.pair_path)
    return m.normalize()


def without_cylinder_pairs(model):
    """the model without the pairs that have a cylinder side"""
    m = copy.deepcopy(model)
    keep = [k for k in range(model.npairs)
            if CYLINDER not in (int(model.geom_type[int(model.pair_a[k])]), int(model.geom_type[int(model.pair_b[k])]))]
    m.pair_a, m.pair_b, m.pair_path = m.pair_a[keep], m.pair_b[keep], m.pair_path[keep]
    gkeep = [g for g in range(model.ngeoms) if int(model.geom_type[g]) != CYLINDER]
    renum = {g: i for i, g in enumerate(gkeep)}
    m.geom_body, m.geom_type = m.geom_body[gkeep], m.geom_type[gkeep]
    m.geom_size, m.geom_X = m.geom_size[gkeep], m.geom_X[gkeep]
    m.pair_a = np.array([renum[int(g)] for g in m.pair_a], dtype=np.int32)
    m.pair_b = np.array([renum[int(g)] for g in m.pair_b], dtype=np.int32)
    return m.normalize()


class Frozen:
    """inverse dynamics by the oracle on the model frozen at the configuration being evaluated"""

    def __init__(self, model, prob, sp):
        self.model, self.prob, self.sp = model, prob, sp
        self.base = Oracle(without_geometry(model), prob, sp)
        self.cache = {}

    def tau(self, q, v, a):
        key = np.asarray(q).tobytes()
        if key not in self.cache:
            self.cache[key] = Oracle(frozen_model(self.model, self.base.body_poses(q)), self.prob, self.sp)
        return self.cache[key].inverse_dynamics(q, v, a)


def frozen_expectation(model, prob, sp, q):
    """v, a, tau, tau without the cylinder pairs, and the three dtau/dq blocks of forward differences (oracle/traj_opt.h)
    with every inverse dynamics evaluated by the oracle on the model frozen at that evaluation's configuration"""
    N, nq, dt = prob.num_steps, model.nq, prob.time_step
    fr = Frozen(model, prob, sp)
    base = fr.base
    v, a, _, _ = base.eval_traj(q)
    tau_no_cyl = Oracle(without_cylinder_pairs(model), prob, sp).eval_traj(q)[2]
    tau = np.array([fr.tau(q[t + 1], v[t + 1], a[t]) for t in range(N)])
    P = base.eval_partials(q)   # (dtau_dqm: the mass matrix, no contact)
    dqp, dqt = np.zeros_like(P["dtau_dqp"]), np.zeros_like(P["dtau_dqt"])
    Np = [base.nplus(q[t]) for t in range(N + 1)]
    eps = np.sqrt(np.finfo(float).eps)
    for t in range(1, N + 1):
        for i in range(nq):
            qi = q[t, i]
            dq = eps * max(1.0, abs(qi))
            dq = (qi + dq) - qi
            dv = dq / dt
            da = dv / dt
            qe = q[t].copy()
            qe[i] = qi + dq
            dqp[t - 1][:, i] = (fr.tau(qe, v[t] + dv * Np[t][:, i], a[t - 1] + da * Np[t][:, i]) - tau[t - 1]) / dq
            if t < N:
                vp = v[t + 1] - dv * Np[t + 1][:, i]
                ap = a[t] - da * (Np[t + 1][:, i] + Np[t][:, i])
                dqt[t][:, i] = (fr.tau(q[t + 1], vp, ap) - tau[t]) / dq
    return v, a, tau, tau_no_cyl, dict(dtau_dqp=dqp, dtau_dqt=dqt, dtau_dqm=P["dtau_dqm"])
