#!/usr/bin/env python3
"""What an iteration of the linesearch method costs: `TrajectoryOptimizer.Solve` with method = kLinesearch through the
device-resident loop (idto_hip_ls_solve_fetch: step lengths in waves, one wait) against the host loop (SolveWithLinesearch:
a round trip per step length), which IDTO_OPT_HOST_LOOP=1 selects on the same tree in the same process.  hopper N = 50 and
mini_cheetah N = 40 from their YAML guesses, scaling and constraints off, both linesearch methods, `--iterations` iterations
a solve.  Every figure is ms per iteration as the median of `--runs` runs with the two legs taken in turn inside a run, the
spread (max - min) / median next to it, and the mean linesearch_iterations of the solve.  The feature pays where the device
loop's median is below the host loop's by more than three times the larger spread (in ms).  Writes profiles/linesearch.txt
(or --out).

    python tools/linesearch_bench.py [--runs 5] [--iterations 10] [--out profiles/linesearch.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from idto_amd.model import load_model  # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from idto_amd.problem import load_config, make_problem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linesearch.txt"))
    a = ap.parse_args()
    assert a.runs >= 5, "the record is a median of at least 5 runs"
    assert "IDTO_OPT_HOST_LOOP" not in os.environ
    out = ["linesearch_bench: Solve with method = kLinesearch, %d iterations a solve, scaling and constraints off, YAML guess; "
           "ms per iteration, median of %d runs (legs in turn) [spread]" % (a.iterations, a.runs)]
    for name, N in (("hopper", 50), ("mini_cheetah", 40)):
        for ls in ("armijo", "backtracking"):
            cfg, model = load_config(name), load_model(name)
            prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
            sp.max_iterations, sp.verbose = a.iterations, False
            sp.method, sp.linesearch_method = "linesearch", ls
            sp.scaling, sp.equality_constraints = False, False
            opt = TrajectoryOptimizer(model, prob, sp)

            def leg(host):
                if host:
                    os.environ["IDTO_OPT_HOST_LOOP"] = "1"
                else:
                    os.environ.pop("IDTO_OPT_HOST_LOOP", None)
                st = TrajectoryOptimizerStats()
                t0 = time.perf_counter()
                flag = opt.Solve(q_guess, TrajectoryOptimizerSolution(), st)
                dt = 1e3 * (time.perf_counter() - t0)
                os.environ.pop("IDTO_OPT_HOST_LOOP", None)
                return dt / max(1, len(st.iteration_costs)), st, flag

            for host in (False, True):   # warm-up: allocations, staging, the first launches
                leg(host)
            t = {False: [], True: []}
            stats = {}
            for _ in range(a.runs):
                for host in (False, True):
                    ms, st, flag = leg(host)
                    t[host].append(ms)
                    stats[host] = (st, flag)
            med = {h: statistics.median(v) for h, v in t.items()}
            spread = {h: max(v) - min(v) for h, v in t.items()}
            same = (np.array_equal(stats[False][0].linesearch_iterations, stats[True][0].linesearch_iterations)
                    and np.array_equal(stats[False][0].iteration_costs, stats[True][0].iteration_costs))
            bar = 3 * max(spread.values())
            verdict = "pays" if med[True] - med[False] > bar else ("slower" if med[False] - med[True] > bar else "within the bar")
            line = ("%s N=%d %s: device loop %.3f [%.0f %%], host loop %.3f [%.0f %%], mean linesearch_iterations %.1f, %d iterations ran, "
                    "same iterates: %s, %s (bar %.3f ms)" %
                    (name, N, ls, med[False], 100 * spread[False] / med[False], med[True], 100 * spread[True] / med[True],
                     float(np.mean(stats[False][0].linesearch_iterations)), len(stats[False][0].iteration_costs), same, verdict, bar))
            print(line, flush=True)
            out.append(line)
            opt.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
