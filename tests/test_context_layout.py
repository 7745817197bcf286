"""host/context_layout.cc - where every per-problem device array of a context lies in its arena - on the CPU.

tests/cpp/context_layout_check.cc is a stand-alone program: compiled here together with the layout unit and the solver
planner by g++ with the address and undefined-behaviour sanitizers, then run.  It
  - reproduces tests/golden/context_layout.txt, recorded from the carve sequences as they stood inside
    idto_hip_create_batch and the KKT context's constructor before the arena became a table (every offset of the examples'
    sizes in clear text, a SHA-256 per nq over a sweep nq = nv = 1 .. 32 x N in {1, 2, 10, 40, 140}, both kinds of context),
  - holds every plan of the sweep to what the kernels assume: 64-byte aligned entries that do not overlap and end within
    an arena stride that is a multiple of 256 bytes, a second set of finite-difference outputs at one constant distance
    from the first, three bands (N + 6) nq^2 doubles apart inside one entry, the solver's arrays at SolverBufferCounts'
    counts, every IDTO_ARR_* id inside its entry,
  - checks the launch sizes against the formulas the kernels carve their LDS by.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_arena_layouts_match_the_recorded_ones_and_hold_what_the_kernels_assume(tmp_path):
    exe = str(tmp_path / "context_layout_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "context_layout_check.cc"),
                    os.path.join(CSRC, "host", "context_layout.cc"), os.path.join(CSRC, "host", "solver_plan.cc"), "-o", exe],
                   check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "context_layout.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
