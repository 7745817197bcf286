#!/usr/bin/env python3
"""What a cylinder costs per Gauss-Newton step: a model with cylinders against its counterpart without, at one horizon, on
trajectories where the pairs act.  Run plain, it prints the step's time (a host clock around `reps` x gn_step that ends in a
fetch, after a warm-up); run under rocprofv3 --kernel-trace --stats, the trace gives fd_kernel's time per step
(profiles/cylinder.txt).

usage: cylinder_prof.py mini_cheetah|mini_cheetah_hills|hopper|hopper_on_cylinder [--num-steps 40] [--reps 200] [--warmup 20]
                        [--fd-fast 0]   (0: a model with a tree shape on the generic kernel, the one a cylinder model takes)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import cylinder_cases as cc  # noqa: E402
from idto_amd import hip  # noqa: E402
from idto_amd.model import load_model  # noqa: E402
from idto_amd.problem import load_config, make_problem, synthetic_trajectory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("model", choices=["mini_cheetah", "mini_cheetah_hills", "hopper", "hopper_on_cylinder"])
ap.add_argument("--num-steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--fd-fast", type=int, default=1)
args = ap.parse_args()
N = args.num_steps

if args.model == "mini_cheetah":      # the trajectory of mini_cheetah_hills, on flat ground
    model, cfg = load_model("mini_cheetah"), load_config("mini_cheetah")
    q = cc.trajectory("mini_cheetah_hills", N)[2]
elif args.model == "hopper":          # the trajectory of hopper_on_cylinder without its descent, on flat ground
    model, cfg = load_model("hopper"), load_config("hopper")
    q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
    q[:, 1] = np.linspace(0.0, -0.35, N + 1)
else:
    model, cfg, q = cc.trajectory(args.model, N)
prob, sp, _ = make_problem(cfg, model, num_steps=N)
sp.gradients_method = "forward_differences"
dev = hip.HipPath(model, prob, sp)
dev.set_option("fd_fast", args.fd_fast)
dev.set_q(q)
for _ in range(args.warmup):
    dev.gn_step()
dev.get("step")
t0 = time.perf_counter()
for _ in range(args.reps):
    dev.gn_step()
dev.get("step")
dt = time.perf_counter() - t0
print(f"{args.model}: N = {N}, fast_shape {dev.get_option('fast_shape')}, fd_fast {args.fd_fast}, {args.reps} x gn_step after {args.warmup}: "
      f"{dt / args.reps * 1e6:.2f} us per step")
dev.close()
