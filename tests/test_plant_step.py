"""csrc/plant_step.h - the arithmetic of a plant's substep (the un-pivoted LDL^T solve of M a = tau - c, the PD+ law, qdot =
N(q) v, the semi-implicit Euler step) as functions that the host and the device's plant_kernel both compile - on the CPU.

tests/cpp/plant_step_check.cc, a stand-alone program compiled here by g++ with the address and undefined-behaviour
sanitizers, holds the header to its defining properties (its head has the list and the bounds).  The other tests hold it
to the oracle's physics: forward dynamics' residual, and a body in free fall.
"""
import os
import subprocess

import numpy as np
import pytest

import plant_cases as pc
from idto_amd.model import load_model
from idto_amd.problem import ProblemDefinition, SolverParameters
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")
EPS = np.finfo(float).eps


def test_header_has_its_defining_properties(tmp_path):
    exe = str(tmp_path / "plant_step_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "plant_step_check.cc"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "\nok:" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]


@pytest.mark.parametrize("name", pc.MODELS)
def test_forward_dynamics_residual_against_the_oracle(name, record_property):
    """a = M^-1 (tau - c) from the oracle's columns and bias by idto_plant_solve_host, put back into the oracle's inverse
    dynamics: |ID(q, v, a) - tau|_inf <= 8 max(the same residual of numpy.linalg.solve's solution on the same M and c,
    eps (|M|_2 |a|_2 + |c|_inf + |tau|_inf)) - the margin because un-pivoted LDL^T's backward bound carries a larger
    constant than pivoted LU's."""
    orc, model = pc.oracle(name), pc.case(name)[1]
    for k, (q, v, tau) in enumerate(pc.states(name)):
        if k == 0 and model.npairs:
            assert orc.signed_distances(q)[0].min() < 0.0, "state 0 has no active contact"
        a, M, c = pc.host_fd(orc, q, v, tau)
        a_np = np.linalg.solve(M, tau - c)
        r = np.abs(orc.inverse_dynamics(q, v, a) - tau).max()
        r_np = np.abs(orc.inverse_dynamics(q, v, a_np) - tau).max()
        floor = EPS * (np.linalg.norm(M, 2) * np.linalg.norm(a) + np.abs(c).max() + np.abs(tau).max())
        print(f"{name} state {k}: residual {r:.3e}, numpy's {r_np:.3e}, floor {floor:.3e}")
        record_property(f"{name}_{k}", f"{r:.3e} {r_np:.3e}")
        assert r <= 8 * max(r_np, floor), (name, k, r, r_np, floor)


@pytest.mark.parametrize("S", [1, 17, 200])
def test_free_fall(S):
    """free_body under gravity, zero torque, no rotation: after S substeps the linear velocity and the height are v0 - g S h
    and z0 + S h v0z - g h^2 S (S + 1) / 2 (semi-implicit Euler: the position moves with the NEW velocity), within 4 S eps of
    their scale; the horizontal velocity and the quaternion do not move at all."""
    model = load_model("free_body")
    nq, nv, N, h = model.nq, model.nv, 2, 1e-3
    q0 = np.array([1.0, 0, 0, 0, 0.1, 0.2, 0.8])
    v0 = np.array([0, 0, 0, 0.3, -0.2, 1.5])
    prob = ProblemDefinition(num_steps=N, q_init=q0, v_init=np.zeros(nv), Qq=np.eye(nq), Qv=np.eye(nv), Qf_q=np.eye(nq),
                             Qf_v=np.eye(nv), R=np.eye(nv), q_nom=np.tile(q0, (N + 1, 1)), v_nom=np.zeros((N + 1, nv)), time_step=0.05)
    orc = Oracle(model, prob, SolverParameters(verbose=False, scaling=False, equality_constraints=False))
    x = pc.host_rollout(orc, model, h, q0, v0, np.zeros(nv), S)[-1]
    q, v = x[:nq], x[nq:]
    g = -float(model.gravity[2])
    vz, z = v0[5] - g * S * h, q0[6] + S * h * v0[5] - g * h * h * S * (S + 1) / 2
    v_scale = abs(v0[5]) + g * S * h
    z_scale = abs(q0[6]) + S * h * abs(v0[5]) + g * h * h * S * (S + 1) / 2
    assert abs(v[5] - vz) <= 4 * S * EPS * v_scale, (v[5], vz)
    assert abs(q[6] - z) <= 4 * S * EPS * z_scale, (q[6], z)
    assert np.array_equal(v[:5], v0[:5]) and np.array_equal(q[:4], q0[:4])
    for i in (0, 1):   # the horizontal position moves with the constant horizontal velocity
        assert abs(q[4 + i] - (q0[4 + i] + S * h * v0[3 + i])) <= 4 * S * EPS * (abs(q0[4 + i]) + S * h * abs(v0[3 + i]))
