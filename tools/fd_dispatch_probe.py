#!/usr/bin/env python3
"""Every kind of finite-difference launch the library makes, once, on small horizons - to compare two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/fd_dispatch_probe.py run <outputs.npz>
    python tools/fd_dispatch_probe.py compare <trace A.csv> <outputs A.npz> <trace B.csv> <outputs B.npz>

run: contexts at N = 4 for acrobot, hopper, mini_cheetah, allegro_hand and the dual_jaco and punyo fixtures; for each
gradients_method with diagonal weights and with one dense weight, eval_partials and gn_step; forward differences with fd_dedup
0; a batch of 2, without and with per-problem model records; costs_along with 3 candidates (one problem, the batch, the batch
with records).  tau, the slab and asm_terms of every case go into the .npz.  (IDTO_HIP_LIB selects the build.)
compare: the fd_* and gn_fused_kernel rows of the two kernel traces, in order - kernel name, grid, workgroup, LDS size - and
the outputs with ==.  Exit status 1 if anything differs.
"""
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
N = 4
METHODS = ["forward_differences", "central_differences", "central_differences4"]


def load(name):
    from idto_amd.model import load_model
    from idto_amd.problem import load_config
    if os.path.exists(os.path.join(EXAMPLES, name + ".model")):
        return load_model(os.path.join(EXAMPLES, name + ".model")), load_config(os.path.join(EXAMPLES, name + ".yaml"))
    return load_model(name), load_config(name)


def run(out_path):
    import copy
    from idto_amd import hip
    from idto_amd.problem import make_problem, synthetic_trajectory
    out = {}

    def keep(tag, dev, problems=(None,)):
        for b in problems:
            for arr in ("tau", "slab", "asm_terms"):
                out["%s/%s/%s" % (tag, arr, b)] = np.array(dev.get(arr, problem=b))

    for name in ("acrobot", "hopper", "mini_cheetah", "allegro_hand", "dual_jaco", "punyo"):
        model, cfg = load(name)
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
        q2 = np.stack([q, synthetic_trajectory(cfg, model, N, seed=1, lower=0.02)])
        for method in METHODS:
            for dense in (0, 1):
                prob, sp, _ = make_problem(cfg, model, num_steps=N)
                sp.scaling = sp.equality_constraints = False
                sp.gradients_method = method
                if dense:
                    R = np.array(prob.R, dtype=float)
                    R[0, 1] = R[1, 0] = 0.125 * min(R[0, 0], R[1, 1])
                    prob.R = R
                dev = hip.HipPath(model, prob, sp)
                dev.set_q(q)
                dev.eval_partials()
                keep("%s/%s/dense%d/partials" % (name, method, dense), dev)
                dev.gn_step()
                keep("%s/%s/dense%d/step" % (name, method, dense), dev)
                if method == METHODS[0] and not dense:
                    out["%s/costs_along" % name] = dev.costs_along([1.0, 0.5, 0.25])
                    dev.set_option("fd_dedup", 0)
                    dev.set_q(q)
                    dev.gn_step()
                    keep("%s/fd_dedup0/step" % name, dev)
                dev.close()
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.scaling = sp.equality_constraints = False
        for records in (0, 1):
            dev = hip.HipPath(model, [prob, copy.deepcopy(prob)], sp)
            if records:
                sp1 = copy.deepcopy(sp)
                sp1.contact_stiffness = 0.5 * sp.contact_stiffness
                dev.set_model_batch(1, None, sp1)
            dev.set_q_batch(q2)
            dev.gn_step()
            keep("%s/batch2/records%d/step" % (name, records), dev, (0, 1))
            out["%s/batch2/records%d/costs_along" % (name, records)] = dev.costs_along_batch([1.0, 0.5, 0.25])
            dev.close()
        print("probe:", name, "done", flush=True)
    np.savez(out_path, **out)
    print("probe: %d arrays -> %s" % (len(out), out_path))


def fd_rows(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            k = r["Kernel_Name"]
            if "fd_" in k.split("(")[0] or "gn_fused_kernel" in k:
                rows.append((k, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
                             r["Workgroup_Size_Z"], r["LDS_Block_Size"]))
    return rows


def compare(trace_a, npz_a, trace_b, npz_b):
    bad = 0
    a, b = fd_rows(trace_a), fd_rows(trace_b)
    print("dispatches: %d and %d rows of fd_* / gn_fused_kernel; %d distinct kernels" % (len(a), len(b), len(set(r[0] for r in a))))
    if len(a) != len(b):
        bad += 1
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            bad += 1
            print("dispatch %d differs:\n  %s\n  %s" % (i, x, y))
    for r in sorted(set(a)):
        print("  %5d x %s" % (a.count(r), " ".join(r[1:]) + "  " + r[0].split("(")[0]))
    A, B = np.load(npz_a), np.load(npz_b)
    if sorted(A.files) != sorted(B.files):
        bad += 1
        print("the outputs' names differ")
    n = 0
    for k in A.files:
        if k in B.files:
            n += 1
            if not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k], equal_nan=True)):
                bad += 1
                print("output %s differs" % k)
    print("outputs: %d arrays compared with ==" % n)
    print("EQUAL" if not bad else "DIFFERENT: %d findings" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
