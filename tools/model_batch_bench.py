#!/usr/bin/env python3
"""What per-entry models cost a batch: `TrajectoryOptimizer.solve_batch(models=..., contacts=...)` - every problem its own
model doubles, gravity and contact parameters, read from a parameter record per problem - against
(b) `solve_batch` of the same entries with the one shared model, the code path a batch had before, and (c) B `Solve` calls on
B optimizers each built with its variant, the only route a caller with B models had.  hopper N = 50 and mini_cheetah N = 40
at B = 8, 64, each model's YAML settings with `--iterations` iterations.  Every figure is the median of `--runs` runs with
the legs taken in turn inside a run, and the spread (max - min) next to it.  The bar is (a) against
(b): the difference of the medians within three times the larger spread.  Writes profiles/model_batch.txt (or --out).

    python tools/model_batch_bench.py [--runs 5] [--iterations 10] [--out profiles/model_batch.txt]
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from solve_batch_bench import problems  # noqa: E402


def variant(model, sp, seed):
    """every free table, gravity and the five contact parameters a few percent off (a world-fixed geometry keeps its
    rotation, a floating joint its identity frame: the model's own checks ask for them)"""
    rng = np.random.default_rng(seed)
    m, p = copy.deepcopy(model), copy.deepcopy(sp)

    def off(a):
        a = np.asarray(a, float)
        return a * (1.0 + 0.06 * (rng.random(a.shape) - 0.5))
    for f in ("X_PF", "axis", "mass", "com", "inertia", "damping", "geom_X", "geom_size"):
        new = off(getattr(m, f))
        if f == "geom_X" and m.ngeoms:
            fixed = np.asarray(m.geom_body) < 0
            new[fixed, :9] = np.asarray(m.geom_X, float)[fixed, :9]
        if f == "X_PF":
            floating = np.asarray(m.jtype) == 3
            new[floating] = np.asarray(m.X_PF, float)[floating]
        setattr(m, f, new)
    m.gravity = off(m.gravity) + np.array([0.2, -0.1, 0.0])
    for k in ("contact_stiffness", "dissipation_velocity", "stiction_velocity", "friction_coefficient", "smoothing_factor"):
        setattr(p, k, float(off(getattr(p, k))))
    return m.normalize(), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_batch.txt"))
    ap.add_argument("--batches", default="8,64")
    a = ap.parse_args()
    assert a.runs >= 5, "the record is a median of at least 5 runs"
    out = ["model_batch_bench: %d iterations a solve, median of %d runs (legs in turn), ms per call [max - min]" % (a.iterations, a.runs),
           "(a) solve_batch with a model and contact parameters per entry, (b) solve_batch of the same entries with the shared "
           "model, (c) B Solve calls on B optimizers built with the variants; bar: |a - b| <= 3 x the larger spread"]
    for name, N in (("hopper", 50), ("mini_cheetah", 40)):
        for B in [int(x) for x in a.batches.split(",")]:
            model, probs, sp, qs = problems(name, N, B, a.iterations)
            variants = [variant(model, sp, 7000 + b) for b in range(B)]
            models, sps = [m for m, _ in variants], [p for _, p in variants]
            with_models = TrajectoryOptimizer(model, probs[0], sp)
            shared = TrajectoryOptimizer(model, probs[0], sp)
            singles = [TrajectoryOptimizer(models[b], probs[b], sps[b]) for b in range(B)]

            def leg_a():
                return with_models.solve_batch(qs, probs, models=models, contacts=sps)

            def leg_b():
                return shared.solve_batch(qs, probs)

            def leg_c():
                for b in range(B):
                    singles[b].Solve(qs[b], TrajectoryOptimizerSolution(), TrajectoryOptimizerStats(a.iterations))

            legs = [("(a) per-entry models", leg_a), ("(b) shared model", leg_b), ("(c) B optimizers", leg_c)]
            assert leg_a().batch_route and leg_b().batch_route
            for _, f in legs:   # warm-up: contexts, staging, the first launches
                f()
            t = {k: [] for k, _ in legs}
            for _ in range(a.runs):
                for k, f in legs:
                    t0 = time.perf_counter()
                    f()
                    t[k].append(1e3 * (time.perf_counter() - t0))
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = {k: max(v) - min(v) for k, v in t.items()}
            ka, kb = legs[0][0], legs[1][0]
            diff, bar = med[ka] - med[kb], 3.0 * max(spread[ka], spread[kb])
            line = "%s N=%d B=%d: " % (name, N, B)
            line += ", ".join("%s %.3f [%.3f]" % (k, med[k], spread[k]) for k, _ in legs)
            line += "; a - b = %+.3f ms, bar %.3f ms: %s" % (diff, bar, "within" if abs(diff) <= bar else "EXCEEDED")
            print(line, flush=True)
            out.append(line)
            for o in [with_models, shared] + singles:
                o.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
