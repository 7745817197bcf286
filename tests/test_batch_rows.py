"""host/batch_rows.cc - one problem's statistics rows of the device loop turned into TrajectoryOptimizerStats, the
convergence reason, the radius to keep and a SolverFlag - on the CPU.

tests/cpp/batch_rows_check.cc is a stand-alone program: compiled here together with the unit by g++ with the address and
undefined-behaviour sanitizers, then run on hand-written rows (all accepted, a rejected last row, a converged row followed
by idle rows, each flag, zero iterations; what the single problem's driver reads besides: whether a reason was reported, the
cost of the iterate behind the last row) and holds the stepwise loop's scalars of the same unit - the dogleg step against a
restatement on vectors in each of its three branches, the trust ratio with its eps rule and the descent test's boundary - to
hand-computed values.  The same file checks that the batch entry points exist at every layer:
idto_hip_tr_solve_batch_fetch, idto_opt_solve_batch, TrajectoryOptimizer.solve_batch.
"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_rows_become_stats_flag_and_radius(tmp_path):
    exe = str(tmp_path / "batch_rows_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "batch_rows_check.cc"), os.path.join(CSRC, "host", "batch_rows.cc"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]


def test_the_unit_is_host_only():
    for f in ("batch_rows.h", "batch_rows.cc"):
        text = open(os.path.join(CSRC, "host", f)).read()
        assert not re.search(r"#include\s*[<\"](hip/|idto_hip\.h)", text), f


def test_the_batch_entry_points_are_declared_and_exported():
    from idto_amd import hip, optimizer
    for header, libpath, names, listed in (
            ("idto_hip.h", hip.LIB_PATH, ("idto_hip_tr_solve_batch_fetch", "idto_hip_create_batch_like"), hip.EXPORTED_SYMBOLS),
            ("idto_opt.h", optimizer.LIB_PATH, ("idto_opt_solve_batch", "idto_opt_batch_error"), optimizer.EXPORTED_SYMBOLS)):
        text = open(os.path.join(ROOT, "include", header)).read()
        L = C.CDLL(libpath) if header == "idto_hip.h" else optimizer.lib()
        for name in names:
            assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/{header}"
            assert hasattr(L, name), f"{name} is not exported"
            assert name in listed
    assert callable(getattr(optimizer.TrajectoryOptimizer, "solve_batch", None))
    assert callable(getattr(hip.HipPath, "tr_solve_batch_fetch", None))
