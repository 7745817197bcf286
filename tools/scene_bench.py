#!/usr/bin/env python3
"""Writes profiles/scene_report.txt: the WALL time of one scene report (HipPath.scene_report: the binding, the states' upload,
the launch of csrc/scene_report.h's kernel, the copy back, one wait - every output but the per-pair rows), median of 5 after a
warm-up call, the legs in turn, (max - min) / 2 as the spread:
  mini_cheetah, 41 states (N = 40), batch 1 and 64;  hopper, 51 states (N = 50), batch 1.
For scale, on the same context: idto_hip_eval_tau plus fetching tau (`eval_tau` + `get("tau")`).  The report is not on the
optimizer's path: the figures are recorded, not gated.

usage: scene_bench.py [--out profiles/scene_report.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REPEATS = 5
LEGS = [("mini_cheetah", 40, 1), ("mini_cheetah", 40, 64), ("hopper", 50, 1)]


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "scene_report.txt")
    import torch
    out = ["one scene report (bodies, pairs, tau_contact) | idto_hip_eval_tau + fetching tau: wall microseconds, median of "
           f"{REPEATS} (spread = (max - min) / 2), the legs in turn"]
    if not torch.cuda.is_available():
        out.append("no GPU: the timings were not measured in this run")
    else:
        from idto_amd import hip
        from idto_amd.model import load_model
        from idto_amd.problem import load_config, make_problem, synthetic_trajectory
        legs = []
        for name, N, B in LEGS:
            cfg, model = load_config(name), load_model(name)
            prob, sp, _ = make_problem(cfg, model, num_steps=N)
            q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
            dev = hip.HipPath(model, [prob] * B if B > 1 else prob, sp)
            (dev.set_q_batch(np.tile(q, (B, 1, 1))) if B > 1 else dev.set_q(q))
            dev.eval_tau()
            v = np.asarray(dev.get("v", 0) if B > 1 else dev.get("v")).reshape(N + 1, model.nv)
            x = np.tile(np.hstack([q, v]), (B, 1, 1))
            dev.scene_report(x)
            (dev.set_q_batch(np.tile(q, (B, 1, 1))) if B > 1 else dev.set_q(q))   # (the warm-up of the second leg: a re-evaluation)
            dev.eval_tau()
            legs.append((name, N, B, dev, q, x, [], []))
        for _ in range(REPEATS):
            for name, N, B, dev, q, x, t_scene, t_tau in legs:
                t0 = time.perf_counter()
                dev.scene_report(x)
                t_scene.append(1e6 * (time.perf_counter() - t0))
                (dev.set_q_batch(np.tile(q, (B, 1, 1))) if B > 1 else dev.set_q(q))   # (a new iterate: eval_tau runs again)
                t0 = time.perf_counter()
                dev.eval_tau()
                _ = [dev.get("tau", b) for b in range(B)] if B > 1 else dev.get("tau")
                t_tau.append(1e6 * (time.perf_counter() - t0))
        for name, N, B, dev, q, x, t_scene, t_tau in legs:
            f = lambda t: f"{np.median(t):9.1f} +- {(max(t) - min(t)) / 2:6.1f}"
            out.append(f"  {name:13s} {N + 1} states, batch {B:2d}: {f(t_scene)} | {f(t_tau)}")
            dev.close()
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
