#!/usr/bin/env python3
"""dual_jaco's finite-difference launch with and without its shared pairs (N = 20, forward differences), for
rocprofv3 --kernel-trace --stats: `--drop-shared` removes the nine pairs between the arms, and the model then runs the
generic fd_kernel<8, 0> instead of fd_kernel<8, SHAPE_XCH>.  Also prints the median time of one trust-region
iteration of the example's own solve (its YAML, 50 iterations).

usage: cross_pairs_prof.py [--drop-shared] [--reps 200]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from idto_amd import hip  # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from idto_amd.problem import make_problem  # noqa: E402
from test_model_cross_pairs import drop_pairs, dual_jaco, shared_pairs, touching_trajectory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--drop-shared", action="store_true")
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

model, cfg = dual_jaco()
if args.drop_shared:
    model = drop_pairs(model, shared_pairs(model))
N = 20
prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
q = touching_trajectory(dual_jaco()[0], cfg, N, 0)
dev = hip.HipPath(model, prob, sp)
dev.set_q(q)
for _ in range(args.reps):
    dev.eval_partials()
dev.get("tau")
dev.close()

opt = TrajectoryOptimizer(model, prob, sp)
sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
flag = opt.Solve(q_guess, sol, st)
opt.close()
print(f"dual_jaco{' without shared pairs' if args.drop_shared else ''}: {args.reps} x eval_partials; solve {flag}, "
      f"{len(st.iteration_costs)} iterations, median {np.median(st.iteration_times) * 1e3:.3f} ms per iteration, "
      f"cost {st.iteration_costs[0]:.6g} -> {st.iteration_costs[-1]:.6g}")
