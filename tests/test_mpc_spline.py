"""csrc/mpc_spline.h - the MPC shell's arithmetic (the not-a-knot fit, its evaluation, the guess time, the nominal shift,
the control rows) as pure functions that the host classes and the device's batch kernels both compile - on the CPU.

tests/golden/mpc_spline.json (the index of the cases) + mpc_spline.f64 (the numbers, float64) record what
idto_mpc_spline_eval returned for seeded inputs on the commit before the header existed: n = 2, 3, 4, 5, 21, 41 knots x
dim 1, 3, 19 x breaks i * 0.05, i * 0.01 and non-uniform; times below and above the range, on every knot and inside
every interval.  tests/cpp/mpc_spline_check.cc, a stand-alone program compiled here by g++ with the address and
undefined-behaviour sanitizers, holds the header to them with ==, and to the spline's defining properties (its head has
the list and the tolerances); the library, whose PiecewiseCubic now calls the header, is held to them as well.
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")


GOLDEN = os.path.join(ROOT, "tests", "golden", "mpc_spline")


def _cases():
    with open(GOLDEN + ".json") as f:
        cases = json.load(f)["cases"]          # [n, dim, kind of breaks, nt, offset]
    assert len(cases) == 54
    return cases


def test_header_matches_the_recorded_values_and_its_properties(tmp_path):
    exe = str(tmp_path / "mpc_spline_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "mpc_spline_check.cc"), "-o", exe], check=True)
    index = [str(x) for n, dim, _, nt, off in _cases() for x in (n, dim, nt, off)]
    run = subprocess.run([exe, GOLDEN + ".f64"] + index, capture_output=True, text=True)
    assert run.returncode == 0 and "\nok:" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]


def test_library_still_returns_the_recorded_values():
    import numpy as np
    from idto_amd.mpc import spline_eval
    data = np.fromfile(GOLDEN + ".f64", dtype="<f8")
    for n, dim, kind, nt, o in _cases():
        breaks, knots = data[o:o + n], data[o + n:o + n + n * dim].reshape(n, dim)
        o += n + n * dim
        got = spline_eval(breaks, knots, data[o:o + nt])
        assert np.array_equal(got.ravel(), data[o + nt:o + nt + nt * dim]), (n, dim, kind)
