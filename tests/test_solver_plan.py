"""host/solver_plan.cc - which solver kernel serves a system, with which block size, split, grid and LDS - on the CPU.

tests/cpp/solver_plan_check.cc is a stand-alone program: compiled here together with the planner by g++ with the address
and undefined-behaviour sanitizers, then run.  It sweeps block sizes 1 .. 32, horizons 1 .. 140, the batch sizes on either
side of every batch threshold, every solver option and every kind of request, and
  - reproduces tests/golden/solver_plan.txt, recorded from the planning code as it stood inside idto_hip.hip before the
    planner became a unit of its own (a SHA-256 per block size over every row of the sweep; the examples' rows, the
    buffer counts and both contexts' carve offsets in clear text),
  - holds every plan to what the kernels assume of it (LDS within 160 KiB, an instantiated block size, chains that
    partition the rows, row tables and carve-ups that cover the longest chain),
  - checks that the solver's buffers cover the highest index the layouts address.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_solver_plans_match_the_recorded_ones_and_fit_the_kernels(tmp_path):
    exe = str(tmp_path / "solver_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "solver_plan_check.cc"),
                    os.path.join(CSRC, "host", "solver_plan.cc"), os.path.join(CSRC, "host", "context_layout.cc"), "-o", exe],
                   check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "solver_plan.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
