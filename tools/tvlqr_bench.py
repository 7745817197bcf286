#!/usr/bin/env python3
"""Writes profiles/tvlqr.txt: what the time-varying LQR gains about a trajectory cost on the device, beside the host composition
of the same thing.  Recorded, not gated.

  (d) HipPath.plant_tvlqr: the perturbation, the S * P rollouts (one plant_kernel launch), the difference and the Riccati
      recursion enqueued at once and waited for once; A, B, K and P come back.
  (h) the host composition: the S * P perturbed states built with numpy, rolled out through HipPath.plant_step on a batch
      context of S * P plants (one launch, one wait) and read back with plant_get_state, the central difference and the
      Riccati recursion (numpy.linalg.solve) in numpy.

hopper at N = 50 and mini_cheetah at N = 40, S = N states, substeps = time_step / sim_time_step of the example YAMLs (50).  The
states are a synthetic trajectory near q_init (velocities zero, small held torques): every rollout ends with status 0, which is
asserted.  WALL time of the calls - the Python binding, the uploads, the launches, the kernels and the copies back -, each
sample the mean over a window of at least WINDOW seconds of calls (at least 3; the count is set from a warm-up sample and
printed), the two legs in turn, median of REPEATS samples with (max - min) / 2 as the spread.  The two legs' A, B and K are compared (they agree to the round-off of numpy's differently ordered sums, printed).
A run without a GPU measures nothing and says so.

usage: tvlqr_bench.py [--out profiles/tvlqr.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from idto_amd.model import load_model  # noqa: E402
from idto_amd.problem import load_config, make_problem, synthetic_trajectory  # noqa: E402

REPEATS, WINDOW = 5, 0.25
EPS = 6.0554544523933395e-06
FLOATING = 3


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def columns(model, x, tau, eps):
    """the P = 1 + 6 nv perturbed copies of (x, tau), csrc/plant_tangent.h's layout, in numpy -> ([P, nq + nv], [P, nv])"""
    nq, nv = model.nq, model.nv
    P = 1 + 6 * nv
    xs, ts = np.tile(x, (P, 1)), np.tile(tau, (P, 1))
    for k in range(3 * nv):
        kind, comp = divmod(k, nv)
        for sgn, e in ((0, eps), (1, -eps)):
            c = 1 + 2 * k + sgn
            if kind == 1:
                xs[c, nq + comp] += e
            elif kind == 2:
                ts[c, comp] += e
            else:
                b = max(i for i in range(model.nbodies) if int(model.vstart[i]) <= comp)
                qs, off = int(model.qstart[b]), comp - int(model.vstart[b])
                if int(model.jtype[b]) == FLOATING and off < 3:
                    w = np.zeros(4)
                    w[1 + off] = 0.5 * e
                    qn = xs[c, qs:qs + 4] + _qmul(w, xs[c, qs:qs + 4])
                    xs[c, qs:qs + 4] = qn / np.linalg.norm(qn)
                else:
                    xs[c, qs + off + (1 if int(model.jtype[b]) == FLOATING else 0)] += e
    return xs, ts


def difference(model, finals, eps):
    """finals [P, nq + nv] -> (A [n, n], B [n, nv])"""
    nq, nv = model.nq, model.nv
    n = 2 * nv
    M = np.zeros((n, 3 * nv))
    for k in range(3 * nv):
        xp, xm = finals[1 + 2 * k], finals[2 + 2 * k]
        for b in range(model.nbodies):
            qs, vs = int(model.qstart[b]), int(model.vstart[b])
            if int(model.jtype[b]) == FLOATING:
                d = _qmul(xp[qs:qs + 4], xm[qs:qs + 4] * np.array([1.0, -1, -1, -1]))
                M[vs:vs + 3, k] = (2.0 if d[0] >= 0 else -2.0) * d[1:]
                M[vs + 3:vs + 6, k] = xp[qs + 4:qs + 7] - xm[qs + 4:qs + 7]
            else:
                nj = 3 if int(model.jtype[b]) == 2 else 1
                M[vs:vs + nj, k] = xp[qs:qs + nj] - xm[qs:qs + nj]
        M[nv:, k] = xp[nq:] - xm[nq:]
    M /= 2.0 * eps
    return M[:, :n], M[:, n:]


def riccati(A, B, act, Q, R, Qf):
    S, n = A.shape[0], A.shape[1]
    K, P = np.zeros((S, len(act), n)), np.zeros((S + 1, n, n))
    P[S] = Qf
    for t in range(S - 1, -1, -1):
        Bu = B[t][:, act]
        K[t] = np.linalg.solve(R + Bu.T @ P[t + 1] @ Bu, Bu.T @ P[t + 1] @ A[t])
        Acl = A[t] - Bu @ K[t]
        P[t] = Q + K[t].T @ R @ K[t] + Acl.T @ P[t + 1] @ Acl
    return K, P


def case(name, N, out):
    from idto_amd import hip
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=3)
    h = float(cfg["sim_time_step"])
    substeps = int(round(float(cfg["time_step"]) / h))
    nq, nv, n = model.nq, model.nv, 2 * model.nv
    P = 1 + 6 * nv
    q = synthetic_trajectory(cfg, model, N, seed=0)[:N]
    x = np.hstack([q, np.zeros((N, nv))])
    act = np.flatnonzero(np.asarray(model.actuated))
    tau = np.zeros((N, nv))
    tau[:, act] = 0.1 * np.random.default_rng(1).uniform(-1, 1, (N, len(act)))
    Q, R, Qf = np.diag([10.0] * nv + [1.0] * nv), 0.1 * np.eye(len(act)), np.diag([100.0] * nv + [10.0] * nv)

    dev = hip.HipPath(model, prob, sp)
    plants = hip.HipPath(model, [prob] * (N * P), sp)
    plants.plant_begin(h)

    def leg_d():
        return dev.plant_tvlqr(x, tau, h, substeps, act, Q, R, Qf)

    def leg_h():
        cols = [columns(model, x[s], tau[s], EPS) for s in range(N)]
        plants.plant_set_state(0.0, np.concatenate([c[0] for c in cols]))
        _, status = plants.plant_step(substeps, np.concatenate([c[1] for c in cols]))
        assert status[:, 0].max() == 0, status
        finals = plants.plant_get_state()[1].reshape(N, P, nq + nv)
        AB = [difference(model, finals[s], EPS) for s in range(N)]
        A, B = np.array([a for a, _ in AB]), np.array([b for _, b in AB])
        return (A, B) + riccati(A, B, act, Q, R, Qf)

    samples, calls = {"d": [], "h": []}, {"d": 3, "h": 3}
    for run in range(REPEATS + 1):   # (run 0: the warm-up, which also sizes the window)
        for leg, fn in (("d", leg_d), ("h", leg_h)):
            t = time.perf_counter()
            for _ in range(calls[leg]):
                res = fn()
            per_call = (time.perf_counter() - t) / calls[leg]
            if run:
                samples[leg].append(per_call * 1e3)
            else:
                calls[leg] = int(min(500, max(3, np.ceil(WINDOW / per_call))))
            if leg == "d":
                r = res
            else:
                Ah, Bh, Kh, Ph = res
    assert r.status.tolist() == [0] and not r.lin_status.any(), (r.status, r.lin_status)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dev.close()
    plants.close()
    fmt = lambda s: f"{np.median(s):9.3f} ({(max(s) - min(s)) / 2:.3f})"
    out.append(f"  {name}: {calls['d']} calls per sample of (d), {calls['h']} of (h)")
    out.append(f"  {name:13s} N = {N}, nv = {nv}, nu = {len(act)}, {N * P} rollouts of {substeps} substeps:  (d) {fmt(samples['d'])} ms   (h) {fmt(samples['h'])} ms"
               f"   |A_d - A_h| {rel(r.A, Ah):.1e}  |B_d - B_h| {rel(r.B, Bh):.1e}  |K_d - K_h| {rel(r.K, Kh):.1e} (relative to the largest entry)")


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "tvlqr.txt")
    lines = ["time-varying LQR gains about a trajectory (csrc/plant_lin.h, csrc/tvlqr_step.h) - tools/tvlqr_bench.py", "",
             f"ms per call (wall, one wait per device call), median of {REPEATS} samples of at least {WINDOW} s of calls after a warm-up sample, the legs in turn (spread = (max - min) / 2):",
             "(d) HipPath.plant_tvlqr | (h) numpy columns + plant_step on S * P plants + plant_get_state + numpy difference and Riccati"]
    import torch
    if not torch.cuda.is_available():
        lines.append("no GPU: not measured in this run")
    else:
        for name, N in (("hopper", 50), ("mini_cheetah", 40)):
            case(name, N, lines)
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
