"""csrc/ls_fetch.h - where the parts of the linesearch loop's staging buffer lie (idto_hip_ls_solve_batch_fetch) - on the CPU.

tests/cpp/ls_fetch_check.cc is a stand-alone program: compiled here by g++ with the address and undefined-behaviour
sanitizers, then run over batches of 1, 2, 3, 37 and 64 problems, 1 and 7 iterations, four model sizes, the batch and the
single form: the parts tile the buffer, the totals are the closed formulas, a problem's block reads rows, q, v, tau, and
with one problem the order is the single fetch's.  g++ compiling the header is what shows that it needs nothing of HIP.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_the_parts_tile_the_staging_buffer(tmp_path):
    exe = str(tmp_path / "ls_fetch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "ls_fetch_check.cc"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
