#!/usr/bin/env python3
"""fd_kernel on a capsule model against its sphere counterpart, for rocprofv3 --kernel-trace --stats: 200 x eval_partials
(forward differences) on one model, at a trajectory where its pairs act.

usage: capsule_prof.py spinner|spinner_capsule|dual_jaco|dual_jaco_capsule_hand [--reps 200]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from idto_amd import hip  # noqa: E402
from idto_amd.model import load_model  # noqa: E402
from idto_amd.problem import load_config, make_problem, synthetic_trajectory  # noqa: E402
from test_gpu_capsule import all_gravity, dual_jaco_capsule_hand, example  # noqa: E402
from test_model_cross_pairs import dual_jaco, touching_trajectory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("model", choices=["spinner", "spinner_capsule", "dual_jaco", "dual_jaco_capsule_hand"])
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

if args.model.startswith("spinner"):
    model, cfg = (load_model("spinner"), load_config("spinner")) if args.model == "spinner" else example("spinner_capsule")
    N = int(cfg["num_steps"])
    q = synthetic_trajectory(cfg, model, N, seed=0)
    q[:, 1] = np.linspace(1.5, 1.25, N + 1)
else:
    model, cfg = dual_jaco()
    model = all_gravity(model) if args.model == "dual_jaco" else dual_jaco_capsule_hand()
    N = 20
    q = touching_trajectory(all_gravity(dual_jaco()[0]), cfg, N, 0)
prob, sp, _ = make_problem(cfg, model, num_steps=N)
sp.gradients_method = "forward_differences"
dev = hip.HipPath(model, prob, sp)
dev.set_q(q)
for _ in range(args.reps):
    dev.eval_partials()
dev.get("tau")
print(f"{args.model}: N = {N}, fast_shape {dev.get_option('fast_shape')}, {args.reps} x eval_partials")
dev.close()
