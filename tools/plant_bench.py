#!/usr/bin/env python3
"""Writes profiles/plant.txt: what the plants on the device (csrc/plant.h) cost and how accurate their solve is.

  1. (CPU) forward dynamics' residual |ID(q, v, a) - tau|_inf of idto_plant_solve_host's a against numpy.linalg.solve's on
     the same M and c, for the states of tests/plant_cases.py - the figures tests/test_plant_step.py bounds.
  2. (GPU, skipped without one) microseconds per substep in hold mode, S = 17 substeps in one launch, for hopper and
     mini_cheetah at B = 1, 8, 64: the WALL time of HipPath.plant_step with its status fetched (one wait) - the Python
     binding, the torque's upload, the launch, the kernel and the copy back, not the kernel alone -, median of 5 after a
     warm-up call, the legs in turn, (max - min) / 2 as the spread.
  3. (GPU) milliseconds per closed-loop tick at B = 8, N = 20, one iteration, 17 substeps, wall time as above, the three legs
     in turn: (t) idto_hip_mpc_batch_tick_plants, (u) idto_hip_mpc_batch_replan alone from a fixed state, (h) the host
     composition plant_step -> plant_get_state -> idto_hip_mpc_batch_replan.

The states and the host restatement are tests/plant_cases.py's, so that the figures are of the states the tests bound.

usage: plant_bench.py [--out profiles/plant.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plant_cases as pc  # noqa: E402

S, REPEATS, H = 17, 5, 1e-3


def residuals(out):
    out.append("forward dynamics' residual |ID(q, v, a) - tau|_inf: the un-pivoted LDL^T of csrc/plant_step.h | numpy.linalg.solve | "
               "eps (|M|_2 |a|_2 + |c|_inf + |tau|_inf)")
    eps = np.finfo(float).eps
    for name in pc.MODELS:
        orc = pc.oracle(name)
        for k, (q, v, tau) in enumerate(pc.states(name)):
            a, M, c = pc.host_fd(orc, q, v, tau)
            a_np = np.linalg.solve(M, tau - c)
            r = np.abs(orc.inverse_dynamics(q, v, a) - tau).max()
            r_np = np.abs(orc.inverse_dynamics(q, v, a_np) - tau).max()
            floor = eps * (np.linalg.norm(M, 2) * np.linalg.norm(a) + np.abs(c).max() + np.abs(tau).max())
            out.append(f"  {name:14s} state {k}{' (contact)' if k == 0 and orc.model.npairs else '':10s} {r:.3e} | {r_np:.3e} | {floor:.3e}")


def timings(out):
    import torch
    if not torch.cuda.is_available():
        out.append("no GPU: the timings were not measured in this run")
        return
    from idto_amd import hip
    out.append(f"hold mode, {S} substeps in one launch, one wait: microseconds per substep, median of {REPEATS} (spread = (max - min) / 2)")
    legs = []
    for name in ("hopper", "mini_cheetah"):
        model = pc.case(name)[0]
        prob, sp = pc.problem(name)
        q, v, tau = pc.states(name)[1]
        for B in (1, 8, 64):
            dev = hip.HipPath(model, [prob] * B if B > 1 else prob, sp)
            dev.plant_begin(H)
            x, taus = np.tile(np.concatenate([q, v]), (B, 1)), np.tile(0.1 * tau, (B, 1))
            dev.plant_set_state(0.0, x)
            dev.plant_step(S, taus)
            legs.append((name, B, dev, x, taus, []))
    for _ in range(REPEATS):   # the legs in turn
        for name, B, dev, x, taus, samples in legs:
            dev.plant_set_state(0.0, x)
            t = time.perf_counter()
            _, status = dev.plant_step(S, taus)
            samples.append((time.perf_counter() - t) * 1e6 / S)
            assert status[:, 0].max() == 0, (name, B, status)
    for name, B, dev, x, taus, samples in legs:
        dev.close()
        out.append(f"  {name:14s} B = {B:3d}   {np.median(samples):8.2f} ({(max(samples) - min(samples)) / 2:.2f})")
    ticks(out)


def ticks(out):
    from idto_amd import hip
    from idto_amd.problem import synthetic_trajectory
    B, N, TICKS = 8, 20, 8
    out.append("")
    out.append(f"closed-loop tick, B = {B}, N = {N}, 1 iteration, {S} substeps: ms per tick (wall), median of {REPEATS} runs of {TICKS} ticks "
               "(spread = (max - min) / 2): (t) tick_plants | (u) replan alone | (h) plant_step + get_state + replan")
    for name in ("hopper", "mini_cheetah"):
        model, _, cfg = pc.case(name)
        prob, sp = pc.problem(name, N=N)
        act = np.flatnonzero(np.asarray(model.actuated))
        nq, nv = model.nq, model.nv
        Kp, Kd = np.zeros((len(act), nq)), np.zeros((len(act), nv))
        for r, j in enumerate(act):
            Kp[r, j + nq - nv], Kd[r, j] = 50.0, 2.0
        q_plan = np.array([synthetic_trajectory(cfg, model, N, seed=b, lower=0.02) for b in range(B)])
        v_plan, tau_plan = np.zeros((B, N + 1, nv)), np.zeros((B, N, nv))
        x0 = np.concatenate([q_plan[:, 0], v_plan[:, 0]], axis=1)
        loop = (1, 2, True, False, np.full(B, sp.Delta0), sp.Delta_max)
        devs = {}
        for leg in "tuh":
            d = hip.HipPath(model, [prob] * B, sp)
            d.mpc_batch_begin(np.zeros(nq, dtype=np.int32), act)
            devs[leg] = d
        samples = {leg: [] for leg in "tuh"}

        def reset(d):
            d.mpc_batch_store(q_plan, v_plan, tau_plan, np.zeros(B))
            d.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=Kp, Kd=Kd)
            d.plant_set_state(0.0, x0)

        for run in range(REPEATS + 1):   # (run 0: the warm-up)
            for leg in "tuh":
                d = devs[leg]
                reset(d)
                t = time.perf_counter()
                for k in range(TICKS):
                    if leg == "t":
                        d.mpc_batch_tick_plants(S, *loop)
                    elif leg == "u":
                        d.mpc_batch_replan(np.full(B, k * S * H), x0, *loop)
                    else:
                        d.plant_step(S, None, status=False)
                        times, x = d.plant_get_state()
                        d.mpc_batch_replan(times, x, *loop)
                if run:
                    samples[leg].append((time.perf_counter() - t) * 1e3 / TICKS)
        for d in devs.values():
            d.close()
        out.append(f"  {name:14s} " + " | ".join(f"({leg}) {np.median(samples[leg]):.3f} ({(max(samples[leg]) - min(samples[leg])) / 2:.3f})" for leg in "tuh"))


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "plant.txt")
    lines = ["plants on the device (csrc/plant.h, csrc/plant_step.h) - tools/plant_bench.py", ""]
    residuals(lines)
    lines.append("")
    timings(lines)
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
