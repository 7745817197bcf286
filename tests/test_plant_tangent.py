"""csrc/plant_tangent.h - the tangent coordinates of a plant's state (tangent_add, tangent_sub) and the columns of a
linearisation (lin_perturb_body, lin_difference_body), the text that the host and the device's lin_perturb_kernel and
lin_difference_kernel both compile - on the CPU.

tests/cpp/plant_tangent_check.cc, a stand-alone program compiled here by g++ with the address and undefined-behaviour
sanitizers, holds the header to its defining properties (its head has the list and the bounds): sub(add(q, d), q) = d - exactly
for every joint but a floating one, within 1e-11 at |d| = 1e-6 for that -, add(q, 0) = q bit for bit, the d.w < 0 branch, and
the layout of the columns.  Nothing is loaded into Python.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


def test_header_has_its_defining_properties(tmp_path):
    exe = str(tmp_path / "plant_tangent_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "plant_tangent_check.cc"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0 and "\nok:" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
