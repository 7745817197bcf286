#!/usr/bin/env python3
"""What the batch linesearch loop buys at the public interface: ms per `TrajectoryOptimizer.solve_batch` call with method =
linesearch on this tree against the same call on another build of the project - the parent commit, built beside this tree -
whose solve_batch runs the linesearch method entry by entry (B uploads, B device loops, B waits).

Configurations: hopper N = 50 and mini_cheetah N = 40, B = 8 and 64, Armijo and backtracking, `--iterations` iterations,
scaling and the enforced constraints off (what the device's linesearch loop serves); the problems differ per entry (shifted
q_nom, perturbed v_init, scaled Qq, synthetic guesses).  Every figure is the median of `--runs` runs with the two legs taken
in turn inside a run, and the spread (max - min) / median next to it.  The bar is profiles/fd_tail_bench.txt's: below the
parent by more than three times the larger spread, in every row.  Also written: the mean linesearch_iterations of the
entries, their flags, and the bytes of the candidates' arenas.  Writes profiles/ls_batch.txt (or --out).

The two builds cannot share a process (two libraries of one name): each leg is a worker process of this script that imports
idto_amd from its own root, builds the configuration once, and times one call per request.

    python tools/ls_batch_bench.py --parent DIR [--runs 5] [--iterations 10] [--out profiles/ls_batch.txt]
"""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(name, N, B, ls) for name, N in (("hopper", 50), ("mini_cheetah", 40)) for B in (8, 64)
           for ls in ("armijo", "backtracking")]


def worker(root):
    sys.path.insert(0, root)
    import numpy as np
    from idto_amd.model import load_model
    from idto_amd.optimizer import TrajectoryOptimizer
    from idto_amd.problem import load_config, make_problem, synthetic_trajectory
    opt = None
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "config":
            name, N, B, ls, iterations = cmd[1], int(cmd[2]), int(cmd[3]), cmd[4], int(cmd[5])
            if opt is not None:
                opt.close()
            cfg, model = load_config(name), load_model(name)
            probs, qs, sp = [], [], None
            for b in range(B):
                prob, sp, _ = make_problem(cfg, model, num_steps=N)
                rng = np.random.default_rng(100 + b)
                prob.q_nom = prob.q_nom + 0.01 * b
                prob.v_init = prob.v_init + 0.05 * rng.normal(size=model.nv)
                prob.Qq = prob.Qq * (1.0 + 0.1 * b)
                probs.append(prob)
                qs.append(synthetic_trajectory(cfg, model, N, seed=b, lower=0.01))
            qs = np.array(qs)
            sp.verbose, sp.max_iterations = False, iterations
            sp.method, sp.linesearch_method = "linesearch", ls
            sp.scaling, sp.equality_constraints = False, False
            opt = TrajectoryOptimizer(model, probs[0], sp)
            for _ in range(2):   # warm-up: contexts, staging, the first launches
                res = opt.solve_batch(qs, probs)
            its = [float(np.mean(st.linesearch_iterations)) for st in res.stats if len(st.linesearch_iterations)]
            flags = {}
            for f, e in zip(res.flags, res.errors):
                key = f if not e else "error"
                flags[key] = flags.get(key, 0) + 1
            stride = ((N + 1) * (model.nq + model.nv + model.nv * model.nq) + 2 * N * model.nv + 3 * model.nv * model.nq + 1 + 7) & ~7
            print("ready %d %.3f %d %s" % (int(res.batch_route), float(np.mean(its)) if its else float("nan"), 8 * stride * 64 * B,
                                           ",".join("%s:%d" % kv for kv in sorted(flags.items()))), flush=True)
        elif cmd[0] == "run":
            gc.collect()   # (the interpreter's collector outside the timed call: a full collection is tens of ms at B = 64)
            gc.disable()
            t0 = time.perf_counter()
            opt.solve_batch(qs, probs)
            ms = 1e3 * (time.perf_counter() - t0)
            gc.enable()
            print("%.6f" % ms, flush=True)
    if opt is not None:
        opt.close()


class Leg:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)

    def ask(self, text):
        self.p.stdin.write(text + "\n")
        self.p.stdin.flush()
        reply = self.p.stdout.readline()
        if not reply:
            raise SystemExit("ls_batch_bench: a worker ended (exit %s)" % self.p.wait())
        return reply.split()

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--parent", default=None, help="root of a build of the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ls_batch.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    assert a.parent and a.runs >= 5, "--parent DIR, and the record is a median of at least 5 runs"
    out = ["# ls_batch_bench: TrajectoryOptimizer.solve_batch, method = linesearch, %d iterations, scaling and constraints off" % a.iterations,
           "# ms per call: median of %d runs, the two legs in turn inside a run [spread (max - min) / median]" % a.runs,
           "# tree = this tree (the batch linesearch loop: one device loop, one wait), parent = the commit before it (entry by entry)",
           "# bar: the tree below the parent by more than three times the larger spread"]
    legs = {"tree": Leg(ROOT), "parent": Leg(os.path.abspath(a.parent))}
    every = True
    for name, N, B, ls in CONFIGS:
        info = {k: leg.ask("config %s %d %d %s %d" % (name, N, B, ls, a.iterations)) for k, leg in legs.items()}
        t = {k: [] for k in legs}
        for _ in range(a.runs):
            for k, leg in legs.items():
                t[k].append(float(leg.ask("run")[0]))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        gain = 1.0 - med["tree"] / med["parent"]
        bar = 3.0 * max(spread.values())
        met = gain > bar
        every = every and met
        line = ("%s N=%d B=%d %s: tree %.3f ms [%.1f %%] (%s), parent %.3f ms [%.1f %%] (%s), tree / parent %.3f (%.1f %% below; bar %.1f %%: %s), "
                "mean linesearch_iterations %s (parent %s), flags %s (parent %s), arenas %d bytes" %
                (name, N, B, ls, med["tree"], 100 * spread["tree"], "batch loop" if info["tree"][1] == "1" else "entry by entry",
                 med["parent"], 100 * spread["parent"], "batch loop" if info["parent"][1] == "1" else "entry by entry",
                 med["tree"] / med["parent"], 100 * gain, 100 * bar, "met" if met else "NOT met", info["tree"][2], info["parent"][2],
                 info["tree"][4] if len(info["tree"]) > 4 else "-", info["parent"][4] if len(info["parent"]) > 4 else "-",
                 int(info["tree"][3])))
        line += "; runs: tree " + " ".join("%.2f" % x for x in t["tree"]) + ", parent " + " ".join("%.2f" % x for x in t["parent"])
        print(line, flush=True)
        out.append(line)
    out.append("# the bar is %s in every row" % ("met" if every else "NOT met"))
    for leg in legs.values():
        leg.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
