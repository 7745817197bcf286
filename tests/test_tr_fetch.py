"""csrc/tr_fetch.h - where the parts of the trust-region fetches' staging buffer lie - on the CPU.

tests/cpp/tr_fetch_check.cc is a stand-alone program: compiled here by g++ with the address and undefined-behaviour
sanitizers, then run over batches of 1 (the single-problem form), 2, 3 and 37 problems, 1 and 7 iterations, with and without
only_best and the MPC hook's parts, three model sizes: the parts tile the buffer, the totals are the closed formulas, a
trajectory block reads q, v, tau, dq, w.  g++ compiling the header is what shows that it needs nothing of HIP.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_the_parts_tile_the_staging_buffer(tmp_path):
    exe = str(tmp_path / "tr_fetch_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "tr_fetch_check.cc"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]

