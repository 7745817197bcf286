#!/usr/bin/env python3
"""Second step after tools/make_golden_traj.py <dual_jaco | spinner_capsule | punyo>: measures, on the CPU, how far the
long-double golden of tests/golden/examples/traj_<name>.json and the oracle's frozen-sphere forward differences
(tests/capsule_ref.py frozen_expectation, rows composed from g and g = 0) disagree, per array, relative to the array's
largest entry, and stores

  observed_derivatives    the measured disagreement of the three dtau/dq blocks, the gradient and the H bands;
  tolerance_derivatives   5 x the largest of them, rounded up to one significant digit, never below the 5e-6 of the
                          BASELINE fixtures.

The disagreement is the truncation error of a forward difference with step ~1.5e-8 on a stiff contact law; it scales
with the state, and the device's central-difference run has to fit under the same number, hence the factor.  A model that
would need more than 1e-4 is refused: choose a shallower trajectory.  The GPU tests use the stored numbers only.

This is not a generator: it imports the tests' oracle wrapper.  Run from the repo root:
    python tools/measure_golden_examples.py [name ...]
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_golden_examples as tge  # noqa: E402


def main():
    for name in sys.argv[1:] or tge.TRAJ:
        path = os.path.join(tge.EXAMPLES, f"traj_{name}.json")
        observed = tge.observed_differences(name)
        assert observed["tau"] <= 1e-11, ("tau", observed["tau"])
        fix = json.load(open(path))
        fix["observed_tau"] = observed.pop("tau")
        fix["observed_derivatives"] = observed
        fix["tolerance_derivatives"] = tge.tolerance_rule(observed)
        print(name, "observed", fix["observed_tau"], observed, "-> tolerance_derivatives", fix["tolerance_derivatives"])
        if fix["tolerance_derivatives"] > 1e-4:
            raise SystemExit(name + ": needs more than 1e-4: choose a shallower trajectory")
        with open(path, "w") as f:
            json.dump(fix, f)


if __name__ == "__main__":
    main()
