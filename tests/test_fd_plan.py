"""host/fd_plan.cc - every finite-difference launch's block, evaluations per pass, fold, LDS bytes, grid, shape and kernel -
on the CPU.

tests/cpp/fd_plan_check.cc is a stand-alone program: compiled here together with the unit and host/model_tables.cc by g++
with the address and undefined-behaviour sanitizers, then run on the nine model files of the package and the six example
fixtures.  It
  - reproduces tests/golden/fd_plans.txt line by line: the plans of every model at mode 0 .. 3 with diagonal and dense weights,
    with asm_fold, fd_fast and fd_dedup switched off (mini_cheetah, punyo, dual_jaco, hopper), over batch 1 / 3, per-problem
    model records, resident and 5 candidate points and a shard [1, 3) of N = 4, the fused launch's embedded evaluation and
    create's geometry - recorded from the sizing functions, LaunchFd, LaunchFused, create and fd_launch.hip's go<> as they
    stood before the decision became a unit (ten of those lines are restated in the program),
  - checks the rules' properties for those plans and for a synthetic sweep (nq 1 .. 40, nv = nq or nq - 1, 1 / 2 / 4 paths,
    both parities of the blob, shared-pair bodies, stems, a shape with the lane map): accepted within the 160 KiB or refused
    with the exact message, the block, the chunk, the fold, the lane map's conditions, the kernel family, the grid,
  - holds the closed LDS formula to the kernel's carve-up (fd_sizes.h fd_carve) for every accepted plan, and prints the slack.
"""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")
MODELS = sorted(glob.glob(os.path.join(ROOT, "idto_amd", "models", "*.model"))) + \
    sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "examples", "*.model")))


def test_fd_plans_properties_and_carve_up(tmp_path):
    assert len(MODELS) == 15
    exe = str(tmp_path / "fd_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "fd_plan_check.cc"), os.path.join(CSRC, "host", "fd_plan.cc"),
                    os.path.join(CSRC, "host", "model_tables.cc"), "-o", exe], check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "fd_plans.txt")] + MODELS, capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
