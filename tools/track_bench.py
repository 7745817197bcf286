#!/usr/bin/env python3
"""Writes profiles/track.txt: what rollouts of the plants under the time-varying LQR law cost on the device, beside the
composition of existing pieces that they replace, and how well the law tracks.  Recorded, not gated.

  (d) HipPath.plant_track: R rollouts of N control steps, every launch enqueued at once and waited for once; x, u, dx come back.
  (h) the composition: per control step the host's tvlqr_control for every rollout (tests/cpp/lin_host.cc `control`, a process
      per call, as tests/lin_cases.py drives it), then ONE HipPath.plant_step in hold mode on a batch context of R plants with
      the recorded state and the status back, i.e. a wait - N times.

hopper at N = 50 and mini_cheetah at N = 40, substeps = time_step / sim_time_step of the example YAMLs (50), R = 1 and R = 64.
The nominal is an optimizer solution (a few iterations from the example's guess), the gains are HipPath.plant_tvlqr's about it
with Q = blkdiag(10 I, I), R = 0.1 I, Qf = blkdiag(100 I, 10 I); the rollouts start from the solution's first state offset
by uniform deviations within 1e-2 in tangent coordinates.  WALL time of the calls, the two legs in turn, median of REPEATS samples
with (max - min) / 2 as the spread; a sample of (d) is the mean over a window of at least WINDOW seconds of calls, a sample of (h)
is one composition.  Beside the times: the tracking error |dx_N| (the median and the largest over the R = 64 rollouts, against
|dx_0|) with the gains and with K = 0, over the rollouts that end with status 0 - a rollout that leaves the region where the
local model holds can end with a failed pivot or a non-finite state, which is counted, not hidden.
A run without a GPU measures nothing and says so.

usage: track_bench.py [--out profiles/track.txt]
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
from idto_amd.problem import load_config, make_problem  # noqa: E402

REPEATS, WINDOW = 5, 0.25


def case(name, N, out):
    import lin_cases as lc
    import track_cases as tc
    from idto_amd import hip, optimizer
    cfg, model = load_config(name), load_model(name)
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.max_iterations, sp.verbose = 5, False
    h = float(cfg["sim_time_step"])
    m = int(round(float(cfg["time_step"]) / h))
    nv = model.nv
    opt = optimizer.TrajectoryOptimizer(model, prob, sp)
    sol, stats = optimizer.TrajectoryOptimizerSolution(), optimizer.TrajectoryOptimizerStats()
    opt.Solve(q_guess, sol, stats)
    act = opt.actuated_dofs()
    opt.close()
    x_nom, tau_nom = np.hstack([sol.q, sol.v]), np.array(sol.tau)
    Q, Rw, Qf = np.diag([10.0] * nv + [1.0] * nv), 0.1 * np.eye(len(act)), np.diag([100.0] * nv + [10.0] * nv)
    dev = hip.HipPath(model, prob, sp)
    gains = dev.plant_tvlqr(x_nom[:N], tau_nom, h, m, act, Q, Rw, Qf)
    assert gains.status.tolist() == [0] and not gains.lin_status.any(), (gains.status, gains.lin_status)
    K = gains.K
    rng = np.random.default_rng(2)
    x0_all = np.array([tc.tangent_add(model, x_nom[0], rng.uniform(-1e-2, 1e-2, 2 * nv)) for _ in range(64)])
    exe = lc.built()
    out.append(f"  {name}: N = {N}, nv = {nv}, nu = {len(act)}, {m} substeps of {h} s a step")
    for R in (1, 64):
        x0 = x0_all[:R]
        plants = hip.HipPath(model, [prob] * R if R > 1 else prob, sp)
        plants.plant_begin(h)

        def leg_d():
            return dev.plant_track(x_nom, tau_nom, K, x0, h, m, act)

        def leg_h():
            x, ended = x0.copy(), np.zeros(R, dtype=bool)
            plants.plant_set_state(0.0, x)
            for t in range(N):
                tau = np.tile(tau_nom[t], (R, 1))
                for r in range(R):
                    tau[r, act] = lc.control(exe, model, K[t], x_nom[t], tau_nom[t][act], x[r])
                rec, status = plants.plant_step(m, tau, record_every=m)
                ended |= status[:, 0] != 0   # (a plant that failed keeps its state; its later steps are timed, its numbers not used)
                x = np.where(ended[:, None], x, rec[:, 0])
            return x, ended

        leg_d()   # (the warm-up, which also sizes the window of (d))
        t = time.perf_counter()
        leg_d()
        calls = int(min(500, max(3, np.ceil(WINDOW / (time.perf_counter() - t)))))
        samples = {"d": [], "h": []}
        for _ in range(REPEATS):
            t = time.perf_counter()
            for _ in range(calls):
                r = leg_d()
            samples["d"].append((time.perf_counter() - t) / calls * 1e3)
            t = time.perf_counter()
            xh, ended = leg_h()
            samples["h"].append((time.perf_counter() - t) * 1e3)
        ok = r.status[:, 0] == 0
        same = bool(np.array_equal(ok, ~ended) and np.all(r.x[ok, -1] == xh[ok]))
        plants.close()
        fmt = lambda s: f"{np.median(s):10.3f} ({(max(s) - min(s)) / 2:.3f})"
        out.append(f"    R = {R:2d}: (d) {fmt(samples['d'])} ms, {calls} calls a sample   (h) {fmt(samples['h'])} ms, one composition a sample"
                   f"   {int(ok.sum())} of {R} rollouts end with status 0 (substeps completed: median {int(np.median(r.status[:, 1]))} of {N * m}), "
                   f"in both legs the same ones with == final states: {same}")
    # the same launches with K = 0: the cost of (d) does not depend on the gains' values, only on how far the rollouts get
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        for _ in range(3):
            free = dev.plant_track(x_nom, tau_nom, np.zeros_like(K), x0_all, h, m, act)
        times.append((time.perf_counter() - t) / 3 * 1e3)
    dev.close()
    out.append(f"    R = 64, K = 0: (d) {np.median(times):10.3f} ({(max(times) - min(times)) / 2:.3f}) ms, 3 calls a sample   "
               f"(substeps completed: median {int(np.median(free.status[:, 1]))} of {N * m})")
    for what, res in (("the gains", r), ("K = 0", free)):
        ok = res.status[:, 0] == 0
        if not ok.any():
            out.append(f"    |dx_N| with {what:9s}: none of the 64 rollouts ended with status 0 (codes {sorted(set(res.status[:, 0].tolist()))})")
            continue
        e0, eN = np.linalg.norm(res.dx[ok, 0], axis=1), np.linalg.norm(res.dx[ok, N], axis=1)
        out.append(f"    |dx_N| with {what:9s}: median {np.median(eN):.3e}, largest {eN.max():.3e}   (|dx_0|: median {np.median(e0):.3e}; "
                   f"{int(ok.sum())} of 64 rollouts ended with status 0)")


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "track.txt")
    lines = ["rollouts of the plants under the time-varying LQR law (csrc/plant.h track_kernel) - tools/track_bench.py", "",
             f"ms per call (wall), median of {REPEATS} samples after a warm-up, the legs in turn (spread = (max - min) / 2):",
             "(d) HipPath.plant_track, one wait | (h) per step: lin_host control per rollout + plant_step on R plants + a wait"]
    import torch
    if not torch.cuda.is_available():
        lines.append("no GPU: not measured in this run")
    else:
        for name, N in (("hopper", 50), ("mini_cheetah", 40)):
            case(name, N, lines)
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
