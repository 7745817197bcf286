#!/usr/bin/env python3
"""punyo's finite-difference launch (N = 40, forward differences) with its stem and with the stem cut away, for
rocprofv3 --kernel-trace --stats.  `--cut-stem`: the torso re-parented to the world at its pose under q_init, the three
bodies below it and the ball-waist pair dropped - a common body on the world, which fd_kernel<8, SHAPE_XCH> evaluates;
the full model keeps its stem at q_init, so both models see the same contacts and the difference is what the stem costs.
Also prints the median time of one trust-region iteration of the example's own solve (full model only).

usage: punyo_prof.py [--cut-stem] [--reps 200]
       punyo_prof.py --summarize <kernel_trace.csv>     (the four kernels with the most time: block size, calls, median and mean of end - start)"""
import argparse
import copy
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cut-stem", action="store_true")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--summarize")
args = ap.parse_args()

if args.summarize:
    rows, block = {}, {}
    for r in csv.DictReader(open(args.summarize)):
        name = r["Kernel_Name"].split("(")[0]
        rows.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        block.setdefault(name, set()).add(r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")))
    for name, d in sorted(rows.items(), key=lambda kv: -sum(kv[1]))[:4]:   # (the four kernels with the most time)
        print(f"  {name[:52]:<52} block {'/'.join(sorted(block[name])):>7}  calls {len(d):5d}  median {np.median(d):9.2f} us  "
              f"mean {np.mean(d):9.2f} us")
    sys.exit(0)

from idto_amd import hip  # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from idto_amd.problem import make_problem, synthetic_trajectory  # noqa: E402
from test_golden import _neutral_fk  # noqa: E402
from test_model_stem import punyo  # noqa: E402

STEM = 3   # bodies (one DoF each) below the torso


def cut_stem(model, cfg):
    """punyo without waist and glue links: body i - 3 is body i, the torso's joint frame where q_init puts it (every stem
    DoF is 0 there: the neutral pose)"""
    assert not np.any(np.asarray(cfg["q_init"])[:STEM + 1])
    X = _neutral_fk(model)[STEM]
    m = copy.deepcopy(model)
    for f in ("jtype", "X_PF", "axis", "mass", "com", "inertia", "gravity_enabled"):
        setattr(m, f, np.array(getattr(model, f))[STEM:])
    m.parent = np.maximum(np.array(model.parent)[STEM:] - STEM, -1)
    m.X_PF[0] = np.concatenate([X[:3, :3].ravel(), X[:3, 3]])
    m.body_names = model.body_names[STEM:]
    m.body_path = np.array(model.body_path)[STEM:]
    m.common_body = model.common_body - STEM
    m.damping, m.actuated = np.array(model.damping)[STEM:], np.array(model.actuated)[STEM:]
    keep_g = [g for g in range(model.ngeoms) if not 0 <= int(model.geom_body[g]) < STEM]
    new_g = {g: i for i, g in enumerate(keep_g)}
    m.geom_body = np.array([b - STEM if b >= 0 else -1 for b in np.array(model.geom_body)[keep_g]])
    m.geom_type, m.geom_size, m.geom_X = (np.array(getattr(model, f))[keep_g] for f in ("geom_type", "geom_size", "geom_X"))
    keep_p = [k for k in range(model.npairs) if int(model.pair_a[k]) in new_g and int(model.pair_b[k]) in new_g]
    m.pair_a = np.array([new_g[int(model.pair_a[k])] for k in keep_p])
    m.pair_b = np.array([new_g[int(model.pair_b[k])] for k in keep_p])
    m.pair_path = np.array(model.pair_path)[keep_p]
    c = {k: (v[STEM:] if isinstance(v, list) and len(v) in (model.nq, model.nv) else v) for k, v in cfg.items()}
    return m.normalize(), c


model, cfg = punyo()
N = 40
q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
q[:, :STEM] = 0.0                                 # the stem where the cut model has it
q[:, 19] = np.linspace(0.30, 0.27, N + 1)        # the ball against waist, torso and arms
if args.cut_stem:
    model, cfg = cut_stem(model, cfg)
    q = q[:, STEM:]
prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
sp.gradients_method = "forward_differences"
dev = hip.HipPath(model, prob, sp)
dev.set_q(q)
for _ in range(args.reps):
    dev.eval_partials()
dev.get("tau")
dev.gn_step()   # (one step: which assembly ran - 1: the products folded into fd_kernel, 2: assemble_diag_kernel forms them)
what = "punyo, stem cut away" if args.cut_stem else "punyo"
print(f"{what}: nq = {model.nq}, pairs {model.npairs}, stem {len(model.stem)}, N = {N}, fast_shape "
      f"{dev.get_option('fast_shape')}, assembly {dev.get_option('last_assembly')}, {args.reps} x eval_partials")
dev.close()
if not args.cut_stem:
    sp.verbose = False
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    print(f"punyo solve: {flag}, {len(st.iteration_costs)} iterations, median {np.median(st.iteration_times) * 1e3:.3f} ms per "
          f"iteration, cost {st.iteration_costs[0]:.6g} -> {st.iteration_costs[-1]:.6g}")
