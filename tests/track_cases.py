"""Shared by tests/test_track_body_host.py and tests/test_gpu_plant_track.py: the inputs of a tracked rollout (a nominal from
tests/lin_cases.py's states, random gains of size 1, initial states offset in tangent coordinates) and the composition that
idto_hip_plant_track replaces - per control step tests/lin_cases.py's host `control`, then HipPath.plant_step in hold mode for the
step's substeps on a twin context.  Everything is a pure function of its arguments and a fixed seed."""
import numpy as np

import lin_cases as lc

FLOATING = 3


def actuated(name):
    model = lc.case(name)[0]
    act = np.flatnonzero(np.asarray(model.actuated))
    return act if len(act) else np.arange(model.nv)   # (pendulum and free_body name no actuator: every dof)


def tangent_add(model, x, d):
    """x (+) d for d = [dtheta (nv); dv (nv)] in csrc/plant_tangent.h's convention: a floating joint's quaternion moves by
    q + 1/2 [0, omega] q with omega in the world frame and is divided by its norm, everything else adds"""
    nq, nv = model.nq, model.nv
    x, d = np.array(x, dtype=float), np.asarray(d, dtype=float)
    q = x[:nq]
    for b in range(model.nbodies):
        qs, vs = int(model.qstart[b]), int(model.vstart[b])
        if int(model.jtype[b]) == FLOATING:
            w, v = q[qs], q[qs + 1:qs + 4].copy()
            om = d[vs:vs + 3]
            q[qs] = w - 0.5 * om.dot(v)
            q[qs + 1:qs + 4] = v + 0.5 * (w * om + np.cross(om, v))
            q[qs:qs + 4] /= np.linalg.norm(q[qs:qs + 4])
            q[qs + 4:qs + 7] += d[vs + 3:vs + 6]
        else:
            nvj = (int(model.vstart[b + 1]) if b + 1 < model.nbodies else nv) - vs
            q[qs:qs + nvj] += d[vs:vs + nvj]
    x[nq:] += d[nv:]
    return x


def inputs(name, S, R, seed=0, delta=1e-2):
    """-> (x_nom [S + 1, nq + nv], tau_nom [S, nv], K [S, nu, n] as [row, col] with entries within 1, x0 [R, nq + nv], actuated).
    The nominal's rows are the case's states in turn (row 0 is states()[0]: an active contact where the model has pairs);
    x0 is x_nom[0] (+) offsets within delta."""
    model, states = lc.case(name)[0], lc.case(name)[5]
    act = actuated(name)
    nv, nu = model.nv, len(act)
    rng = np.random.default_rng(4100 + 17 * seed + len(name))
    x_nom = np.array([np.concatenate(states[t % 3][:2]) for t in range(S + 1)])
    tau_nom = np.array([states[t % 3][2] for t in range(S)])
    K = rng.uniform(-1.0, 1.0, (S, nu, 2 * nv))
    x0 = np.array([tangent_add(model, x_nom[0], rng.uniform(-delta, delta, 2 * nv)) for _ in range(R)])
    return x_nom, tau_nom, K, x0, act


def composition(twin, name, x_nom, tau_nom, K, x0, act, m):
    """One rollout by the existing pieces on `twin`, a HipPath of one problem with plant_begin(h) done: per step the host's
    tvlqr_control (lin_cases.control), the torque tau_nom with u on the actuated dofs, m substeps of plant_step in hold mode.
    The law's deviation is the same program's: with K = I_n and u_nom = 0 its row i is 0 - (0 dx_0 + ... + 1 dx_i + ... + 0 dx_n-1),
    -dx_i exactly.  -> (x [S, nq + nv], u [S, nu], dx [S + 1, n])"""
    model = lc.case(name)[0]
    S = len(tau_nom)
    n = 2 * model.nv
    deviation = lambda x_ref, x: -lc.control(lc.built(), model, np.eye(n), x_ref, np.zeros(n), x)
    x, xs, us, dxs = np.array(x0, dtype=float), [], [], []
    twin.plant_set_state(0.0, x)
    for t in range(S):
        u = lc.control(lc.built(), model, K[t], x_nom[t], tau_nom[t][act], x)
        dxs.append(deviation(x_nom[t], x))
        tau = np.array(tau_nom[t], dtype=float)
        tau[act] = u
        rec, status = twin.plant_step(m, tau, record_every=m)
        assert status.tolist() == [[0, m]], status
        x = rec[0, 0]
        xs.append(x.copy())
        us.append(u)
    dxs.append(deviation(x_nom[S], x))
    return np.array(xs), np.array(us), np.array(dxs)


def weights(nv, nu, seed):
    """symmetric positive definite Q [n, n] (block diagonal, as TrajectoryOptimizer.track builds it), R [nu, nu], Qf [n, n] (dense)"""
    rng = np.random.default_rng(seed)

    def spd(m, scale):
        M = rng.uniform(-1, 1, (m, m))
        return scale * (M @ M.T / m + np.eye(m))
    Q = np.zeros((2 * nv, 2 * nv))
    Q[:nv, :nv], Q[nv:, nv:] = spd(nv, 10.0), spd(nv, 1.0)
    return Q, spd(nu, 0.1), spd(2 * nv, 100.0)
