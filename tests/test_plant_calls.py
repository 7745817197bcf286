"""host/plant_calls.cc - what the plant family's entries refuse, the block and LDS of their launches and where a call's arrays
lie in the feature's device buffer and its pinned mirror - on the CPU.

tests/cpp/plant_calls_check.cc is a stand-alone program: compiled here together with the unit by g++ with the address and
undefined-behaviour sanitizers, then run.  It
  - reproduces tests/golden/plant_call_layouts.txt line by line: every offset, count, end of the inputs, start of the outputs,
    total and pinned size of the plants' storage, the scene report, the linearisation and the tracked rollouts, recorded from
    the carve sequences as they stood inside PlantAllocate, idto_hip_scene_report, LinRun and TrackLayout before the layouts
    became tables ((nq, nv) = (2, 2) and (7, 6), batch 1 and 3, 1 and 3 states, 1 and 2 rollouts, nu = 1 and nv, gains of the
    call's own or not, the Riccati recursion or not, each of the report's 15 sets of outputs, PD+ or not, record_capacity 0 and 5),
  - holds the one block and LDS rule to the two pairs of functions it replaced, restated, and to its overflow guard,
  - checks every refusal of every entry by its exact message, the order of the checks by calls with several faults, and one
    accepted call per entry; an entry without a case fails the program.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_plant_calls_layouts_sizes_and_refusals(tmp_path):
    exe = str(tmp_path / "plant_calls_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "plant_calls_check.cc"), os.path.join(CSRC, "host", "plant_calls.cc"), "-o", exe],
                   check=True)
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "plant_call_layouts.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok:"), run.stdout[-4000:] + run.stderr[-4000:]
