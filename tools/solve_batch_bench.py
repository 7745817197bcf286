#!/usr/bin/env python3
"""What a batch at the public interface costs: `TrajectoryOptimizer.solve_batch` against B sequential `Solve` calls and
against the route a caller had before it (idto_hip_tr_solve_batch(_constrained) + idto_hip_get_batch of q, v, tau per
problem), for hopper N = 50 and mini_cheetah N = 40 at B = 1, 8, 64, each model's YAML settings with `--iterations`
iterations.  Every figure is the median of `--runs` runs with the legs taken in turn inside a run, and the spread
(max - min) / median next to it.  Also: the waits for the device inside one idto_hip_tr_solve_batch_fetch (the library's own
trace marks), and whether `only_best` is cheaper.  Writes profiles/solve_batch.txt (or --out).

    python tools/solve_batch_bench.py [--runs 5] [--iterations 10] [--out profiles/solve_batch.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from idto_amd import hip  # noqa: E402
from idto_amd.model import load_model  # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from idto_amd.problem import SCALING, load_config, make_problem, synthetic_trajectory  # noqa: E402


def problems(name, N, B, iterations):
    cfg, model = load_config(name), load_model(name)
    probs, qs, sp = [], [], None
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.001 * b
        prob.Qq = prob.Qq * (1.0 + 0.01 * b)
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, N, seed=b, lower=0.01))
    sp.verbose = False
    sp.max_iterations = iterations
    return model, probs, sp, np.array(qs)


def waits_inside_fetch(opt, qs, probs):
    """trace marks of one solve_batch: the waits the batch loop's call makes"""
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    L.idto_hip_trace_mark.argtypes = [C.c_char_p]
    L.idto_hip_trace_enable(1)
    opt.solve_batch(qs, probs)
    buf = C.create_string_buffer(1 << 20)
    L.idto_hip_trace_dump(buf, len(buf))
    L.idto_hip_trace_enable(0)
    lines = buf.value.decode().splitlines()
    begin = max(i for i, l in enumerate(lines) if "tr_solve begins" in l)
    return sum("waited for the device" in l for l in lines[begin:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_batch.txt"))
    ap.add_argument("--batches", default="1,8,64")
    a = ap.parse_args()
    assert a.runs >= 5, "the record is a median of at least 5 runs"
    out = ["solve_batch_bench: %d iterations a solve, median of %d runs (legs in turn), ms per call [spread]" % (a.iterations, a.runs)]
    for name, N in (("hopper", 50), ("mini_cheetah", 40)):
        for B in [int(x) for x in a.batches.split(",")]:
            model, probs, sp, qs = problems(name, N, B, a.iterations)
            constrained = sp.equality_constraints and len(model.unactuated_dofs) > 0
            dofs = list(model.unactuated_dofs) if constrained else []
            sm = SCALING[sp.scaling_method] if sp.scaling else -1
            opt = TrajectoryOptimizer(model, probs[0], sp)
            singles = [TrajectoryOptimizer(model, probs[b], sp) for b in range(B)]
            raw = hip.HipPath(model, probs, sp)
            raw.set_unactuated_dofs(list(model.unactuated_dofs))

            def leg_batch(only_best=False):
                return opt.solve_batch(qs, probs, only_best=only_best)

            def leg_sequential():
                for b in range(B):
                    singles[b].Solve(qs[b], TrajectoryOptimizerSolution(), TrajectoryOptimizerStats(a.iterations))

            def leg_parent():
                for b in range(B):
                    raw.set_problem_batch(b, probs[b])
                raw.set_q_batch(qs)
                raw.eval_tau()
                if B > 1 and dofs:
                    raw.tr_solve_batch_constrained(a.iterations, sm, sp.scaling, sp.normalize_quaternions, sp.Delta0, sp.Delta_max, dofs)
                elif B > 1:
                    raw.tr_solve_batch(a.iterations, sm, sp.scaling, sp.normalize_quaternions, sp.Delta0, sp.Delta_max)
                else:
                    raw.tr_solve(a.iterations, sm, sp.scaling, sp.normalize_quaternions, sp.Delta0, sp.Delta_max, constrained_dofs=dofs)
                for b in range(B):
                    for k in ("q", "v", "tau"):
                        raw.get(k, problem=b)

            legs = [("solve_batch", leg_batch), ("sequential Solve", leg_sequential), ("tr_solve_batch + get_batch", leg_parent),
                    ("solve_batch only_best", lambda: leg_batch(True))]
            route = leg_batch().batch_route
            for _, f in legs:   # warm-up: contexts, staging, the first launches
                f()
            t = {k: [] for k, _ in legs}
            for _ in range(a.runs):
                for k, f in legs:
                    t0 = time.perf_counter()
                    f()
                    t[k].append(1e3 * (time.perf_counter() - t0))
            waits = waits_inside_fetch(opt, qs, probs) if route else None
            line = "%s N=%d B=%d (%s): " % (name, N, B, "batch loop" if route else "entry by entry")
            line += ", ".join("%s %.3f [%.0f %%]" % (k, statistics.median(v), 100 * (max(v) - min(v)) / statistics.median(v)) for k, v in t.items())
            if waits is not None:
                line += ", waits inside idto_hip_tr_solve_batch_fetch: %d" % waits
            print(line, flush=True)
            out.append(line)
            raw.close()
            opt.close()
            for s in singles:
                s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
