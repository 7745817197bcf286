"""csrc/ls_decide.h - the linesearches' step lengths, early-outs and decisions as pure functions - on the CPU.

tests/cpp/ls_decide_check.cc is a stand-alone program: compiled here by g++ with the address and undefined-behaviour
sanitizers, then run.  It holds both step-length chains to literal doubles, the scans to a plain restatement of the two host
loops (host/trajectory_optimizer.cc ArmijoLinesearch, BacktrackingLinesearch) over seeded cost sequences fed one, three,
seven candidates at a time and all at once, and walks the edge cases: a NaN cost, equal costs, L' = 0, L' > 0, the
early-outs, Armijo exhausted at the limit, backtracking running past the limit and undecided within 64 candidates.  The
same program holds host/ls_rows.cc (the device loop's statistics rows into stats, flag and errors) to hand-made rows, and
host/solver_plan.cc PlanLsWaves to its properties over a sweep - every candidate index exactly once, in order, no wave
wider than the cap - and to the schedules recorded in tests/golden/ls_waves.txt.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_linesearch_decisions_match_the_host_loops(tmp_path):
    exe = str(tmp_path / "ls_decide_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "ls_decide_check.cc"), os.path.join(CSRC, "host", "ls_rows.cc"),
                    os.path.join(CSRC, "host", "solver_plan.cc"), "-o", exe], check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ls_waves.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
