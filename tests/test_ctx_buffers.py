"""host/ctx_buffers.h - the owners of a context's staging and grown buffers (Pinned, Grown, and the device buffer with its
pinned mirror) - on the CPU.

tests/cpp/ctx_buffers_check.cc is a stand-alone program: compiled here by g++ with the address and undefined-behaviour
sanitizers, then run.  It instantiates the owners over a counting fake of the four memory calls (malloc and free underneath,
every call recorded, the n-th allocation made to fail on request) and checks
  - grow, the same size, a smaller size, a larger size: an allocation only on a real growth, the superseded block freed
    exactly once and in front of the new allocation - behind it in the allocate-first mode of the trust-region rows and
    the solve staging,
  - a minimum capacity,
  - the zero fill of the whole of a device buffer,
  - a failed allocation at every position: pointer null, capacity 0, nothing kept, and a later Ensure succeeds,
  - at a scope's end every allocation freed once (no live block, no double free, the sanitizers silent),
  - a moved-from object frees nothing,
  - the pair: a device side that grew while its pinned side failed reports the failure, and the next call makes what is missing.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_ctx_buffers_own_grow_and_free(tmp_path):
    exe = str(tmp_path / "ctx_buffers_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "ctx_buffers_check.cc"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]


def test_ctx_buffers_header_is_host_only():
    text = open(os.path.join(CSRC, "host", "ctx_buffers.h")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
