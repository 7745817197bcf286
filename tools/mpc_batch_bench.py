"""What a tick of B model-predictive controllers costs, three ways (profiles/mpc_batch.txt):

  (a) BatchDeviceModelPredictiveController.update: the whole tick enqueued at once, one wait
      (idto_hip_mpc_batch_replan: mpc_shift_kernel, the batch loop, mpc_store_kernel);
  (b) B DeviceModelPredictiveControllers one after another, each on an optimizer of its own;
  (c) the tick of (a) with the shift and the store on the HOST, built from public calls: the guesses and the shifted
      nominal trajectories by csrc/mpc_spline.h on the host, idto_hip_set_problem_batch x B, idto_hip_set_q_batch,
      idto_hip_eval_tau, idto_hip_tr_solve_batch_fetch, B x 3 host fits.  Its q, v, tau, radii and plans must == (a)'s.

hopper and mini_cheetah, N = 20, the examples' mpc_iters; B = 1 (leg b only), 8, 64.  ms per tick: the median of RUNS runs
of TICKS ticks, the legs taken in turn within a run, and the spread (max - min) of the runs.

    python tools/mpc_batch_bench.py [--out profiles/mpc_batch.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from idto_amd import hip, mpc as M                                   # noqa: E402
from idto_amd.model import load_model                                # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats   # noqa: E402
from idto_amd.problem import SCALING, SolverParameters, load_config, make_problem   # noqa: E402

N, RUNS, TICKS = 20, 5, 8


class HostShell:
    """leg (c): the controllers' state on the host, the batch loop on a hip.HipPath"""

    def __init__(self, model, probs, sp, warm, sel, act):
        self.model, self.probs, self.sp, self.sel, self.act = model, [p for p in probs], sp, sel, act
        self.B, self.nq, self.nv = len(probs), model.nq, model.nv
        self.dt = probs[0].time_step
        self.breaks = np.arange(N + 1) * self.dt
        self.ctx = hip.HipPath(model, probs, sp)
        self.ctx.set_unactuated_dofs(model.unactuated_dofs)
        self.delta = np.full(self.B, sp.Delta0)
        self.q_nom = [np.array(p.q_nom, float) for p in probs]
        self.plans = [self.fit(np.asarray(w.q)[:N + 1], np.asarray(w.v)[:N + 1], np.asarray(w.tau)[:N], 0.0) for w in warm]
        con = bool(sp.equality_constraints) and len(model.unactuated_dofs) > 0
        self.dofs = model.unactuated_dofs if con else ()
        self.scal = SCALING[sp.scaling_method] if sp.scaling else -1

    def fit(self, q, v, tau, start):
        u = np.vstack([tau, tau[-1:]])[:, self.act]
        return dict(start=start, q=q.copy(), mq=M.spline_fit(self.breaks, q), v=v.copy(), mv=M.spline_fit(self.breaks, v),
                    u=u, mu=M.spline_fit(self.breaks, u))

    def update(self, times, x0):
        B, nq = self.B, self.nq
        guess = np.zeros((B, N + 1, nq))
        for b in range(B):
            P = self.plans[b]
            guess[b], self.q_nom[b] = M.shift_reference(self.breaks, P["q"], P["mq"], P["start"], times[b], self.dt, x0[b, :nq],
                                                        self.sel, self.q_nom[b])
            p = self.probs[b]
            p.q_init, p.v_init, p.q_nom = x0[b, :nq].copy(), x0[b, nq:].copy(), self.q_nom[b]
            self.ctx.set_problem_batch(b, p)
        self.ctx.set_q_batch(guess)
        self.ctx.eval_tau()
        out = self.ctx.tr_solve_batch_fetch(self.sp.max_iterations, self.scal, bool(self.sp.scaling), bool(self.sp.normalize_quaternions),
                                            self.delta, self.sp.Delta_max, constrained_dofs=self.dofs, check=False)
        for b in range(B):
            if out["status"][b] & (1 | 2 | 4 | 8 | 32):
                continue
            self.delta[b] = out["delta"][b]
            self.plans[b] = self.fit(out["q"][b], out["v"][b], out["tau"][b], times[b])
        return out


def setup(name, B):
    cfg, model = load_config(name), load_model(name)
    probs, sp = [], None
    for b in range(B):
        prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.001 * b
        probs.append(prob)
    sp.verbose = False
    sp0 = SolverParameters(**{**sp.__dict__, "max_iterations": 10})
    opt = TrajectoryOptimizer(model, probs[0], sp0)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    opt.Solve(q_guess, sol, st)
    opt.close()
    sp1 = SolverParameters(**{**sp.__dict__, "max_iterations": int(cfg.get("mpc_iters", 1))})
    sel = np.asarray(cfg.get("q_nom_relative_to_q_init", [False] * model.nq), dtype=np.int32)
    period = 1.0 / float(cfg.get("controller_frequency", 200.0))
    return model, probs, sp1, [sol] * B, sel, period


def bench(name, B, log):
    model, probs, sp, warm, sel, period = setup(name, B)
    nq = model.nq
    act = np.flatnonzero(np.asarray(model.actuated))
    act = act if act.size else np.arange(model.nv)
    opts = [TrajectoryOptimizer(model, probs[b], sp) for b in range(B)]
    singles = [M.DeviceModelPredictiveController(opts[b], warm[b], actuated=model.actuated, q_nom_relative_to_q_init=sel, strict=False)
               for b in range(B)]
    legs = {"b": []}
    batch = host = opt_b = None
    if B >= 2:
        opt_b = TrajectoryOptimizer(model, probs[0], sp)
        batch = M.BatchDeviceModelPredictiveController(opt_b, warm, actuated=model.actuated, q_nom_relative_to_q_init=sel, problems=probs)
        host = HostShell(model, probs, sp, warm, sel, act)
        legs.update(a=[], c=[])
    rng = np.random.default_rng(1)
    k, equal = 0, True
    for run in range(RUNS + 1):                  # (run 0 warms up: allocations, first launches)
        t = dict.fromkeys(legs, 0.0)
        for _ in range(TICKS):
            k += 1
            times = k * period * (1.0 + 0.01 * np.arange(B))
            x0 = np.array([singles[b].state(times[b]) + 1e-3 * rng.normal(size=nq + model.nv) for b in range(B)])
            t0 = time.perf_counter()
            for b in range(B):
                singles[b].update(times[b], x0[b, :nq], x0[b, nq:], copy=False)
            t["b"] += time.perf_counter() - t0
            if batch is None:
                continue
            t0 = time.perf_counter()
            g, q, v, tau = batch.update(times, x0, copy=False, strict=False)
            t["a"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            out = host.update(times, x0)
            t["c"] += time.perf_counter() - t0
            equal = equal and np.array_equal(out["q"], q) and np.array_equal(out["v"], v) and np.array_equal(out["tau"], tau) \
                and np.array_equal(host.delta, batch.last_radii)
            for b in (0, B - 1):
                tq = times[b] + 0.37 * period
                P = host.plans[b]
                xh = np.concatenate([M.spline_eval(host.breaks, P["q"], [tq - P["start"]])[0], M.spline_eval(host.breaks, P["v"], [tq - P["start"]])[0]])
                equal = equal and np.array_equal(xh, batch.state(b, tq))
        if run:
            for leg in legs:
                legs[leg].append(1e3 * t[leg] / TICKS)
    row = f"{name:13s} N={N} mpc_iters={sp.max_iterations} B={B:3d}"
    for leg in sorted(legs):
        x = np.array(legs[leg])
        row += f" | ({leg}) {np.median(x):8.3f} ms  spread {x.max() - x.min():6.3f}"
    if batch is not None:
        row += f" | (c) == (a): {equal}"
    log(row)
    if batch is not None:
        batch.close(); opt_b.close(); host.ctx.close()
    for s, o in zip(singles, opts):
        s.close(); o.close()
    return {leg: (float(np.median(x)), float(np.max(x) - np.min(x))) for leg, x in legs.items()}, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,8,64")
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f"# tools/mpc_batch_bench.py: ms per tick, median of {RUNS} runs of {TICKS} ticks (legs in turn), spread = max - min of the runs")
    log("# (a) BatchDeviceModelPredictiveController.update  (b) B single controllers in turn  (c) (a)'s tick with the shift and the store on the host")
    ok = True
    for name in ("hopper", "mini_cheetah"):
        for B in [int(x) for x in args.batches.split(",")]:
            res, equal = bench(name, B, log)
            ok = ok and equal
            if "a" in res:
                for other in ("b", "c"):
                    bar = 3 * max(res["a"][1], res[other][1])
                    log(f"#   (a) below ({other}) by {res[other][0] - res['a'][0]:.3f} ms; three times the larger spread: {bar:.3f} ms -> "
                        f"{'holds' if res[other][0] - res['a'][0] > bar else 'NOT measurable'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
