"""A C++ program that asks for the time-varying LQR gains through include/idto/optimizer/tvlqr.h with no Python in its process
(tests/cpp/tvlqr_acrobot.cc, built by build.sh as build/tvlqr_acrobot, in the manner of tests/test_gpu_cpp_consumer.py): the
acrobot at N = 5, a few iterations of Solve, TrajectoryOptimizer::Tvlqr about the solution in substeps of time_step / 4.  It
prints the solution and what the call returned with 17 significant digits, which read back to the same doubles: the Python
route (HipPath.plant_tvlqr) on the printed states, torques and weights must give the printed A, B, K and P bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import ProblemDefinition, SolverParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "tvlqr_acrobot")
SRC = os.path.join(ROOT, "tests", "cpp", "tvlqr_acrobot.cc")
LIBS = [os.path.join(ROOT, "idto_amd", n) for n in ("libidto_hip.so", "libidto_opt.so")]


def _exe():
    deps = [SRC] + LIBS
    if not os.path.exists(EXE) or any(os.path.getmtime(EXE) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
                        "-L" + os.path.join(ROOT, "idto_amd"), "-lidto_opt", "-lidto_hip", "-Wl,-rpath,$ORIGIN/../idto_amd"], check=True)
    return EXE


def _rows(out, name, count):
    rows = {int(t): [float(x) for x in rest.split()] for t, rest in re.findall(rf"^{name} (\d+) (.*)$", out, re.M)}
    assert sorted(rows) == list(range(count)), (name, sorted(rows))
    return np.array([rows[t] for t in range(count)])


@pytest.mark.gpu
def test_cpp_consumer_gets_the_gains_of_the_python_route():
    N, dt = 5, 0.05
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    p = subprocess.run([_exe(), os.path.join(ROOT, "idto_amd", "models", "acrobot.model")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout
    assert re.search(r"^actuated 1$", out, re.M) and re.search(r"^lqr_status 0 lin_ok 1$", out, re.M), out[:400]
    assert re.search(r"^linearize_plant_same 1$", out, re.M)
    assert re.search(r"^refused 1 Tvlqr: time_step / h = .* is not a whole number of substeps$", out, re.M), out[-400:]
    q, v, tau = _rows(out, "q", N + 1), _rows(out, "v", N + 1), _rows(out, "tau", N)
    model = load_model("acrobot")
    nq, nv, n = model.nq, model.nv, 2 * model.nv
    col = lambda M, r, c: M.reshape(-1, c, r).swapaxes(1, 2)   # (printed column-major -> [row, col])
    A, B = col(_rows(out, "A", N), n, n), col(_rows(out, "B", N), n, nv)
    K, P, xn = col(_rows(out, "K", N), 1, n), col(_rows(out, "P", N + 1), n, n), _rows(out, "x_next", N)
    prob = ProblemDefinition(num_steps=N, q_init=q[0], v_init=v[0], Qq=np.eye(nq), Qv=np.eye(nv), Qf_q=np.eye(nq), Qf_v=np.eye(nv),
                             R=np.eye(nv), q_nom=np.tile(q[0], (N + 1, 1)), v_nom=np.zeros((N + 1, nv)), time_step=dt)
    dev = hip.HipPath(model, prob, SolverParameters(verbose=False, scaling=False, equality_constraints=False))
    r = dev.plant_tvlqr(np.hstack([q[:N], v[:N]]), tau, dt / 4, 4, [1], np.diag([10.0, 10, 1, 1]), np.diag([0.1]), np.diag([100.0, 100, 10, 10]))
    dev.close()
    same = lambda a, b: a.shape == b.shape and bool(np.all(a == b))
    assert r.status.tolist() == [0]
    assert same(r.A, A) and same(r.B, B) and same(r.x_next, xn)
    assert same(r.K, K) and same(r.P[0], P)
