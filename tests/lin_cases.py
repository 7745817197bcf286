"""Shared by tests/test_tvlqr_step.py and tests/test_gpu_plant_linearize.py, tests/test_gpu_tvlqr.py: csrc/plant_tangent.h and
csrc/tvlqr_step.h compiled for the host as the stand-alone program tests/cpp/lin_host.cc, driven through files, and the host
composition of a linearisation - the header's perturbed columns, tests/plant_cases.py's host rollouts, the header's central
difference.  Nothing here is loaded into the Python process."""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "cpp", "lin_host.cc")
BUILT = os.path.join(ROOT, "build", "lin_host")   # build.sh's: see built()
EPS_DEFAULT = 6.0554544523933395e-06              # cbrt(2^-52), include/idto_hip.h IDTO_LIN_EPS_DEFAULT
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def compile_host(exe, sanitize):
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if sanitize else []) +
                   ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), SOURCE, "-o", exe], check=True)
    return exe


def built():
    """build/lin_host, the program without sanitizers that build.sh makes (the GPU tests' reference); compiled here if it is
    missing or older than its sources"""
    deps = [SOURCE] + [os.path.join(CSRC, h) for h in ("plant_step.h", "plant_tangent.h", "tvlqr_step.h")]
    if not os.path.exists(BUILT) or any(os.path.getmtime(BUILT) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(BUILT), exist_ok=True)
        compile_host(BUILT, False)
    return BUILT


@functools.lru_cache(maxsize=None)
def sanitized():
    """lin_host compiled with the address and undefined-behaviour sanitizers, once per process (the CPU tests' program)"""
    d = tempfile.mkdtemp(prefix="lin_host_")
    return compile_host(os.path.join(d, "lin_host_san"), True)


def run(exe, mode, *arrays):
    """the arrays, flattened in order, are IN; -> OUT as a flat array"""
    with tempfile.TemporaryDirectory(prefix="lin_io_") as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(fin)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return np.fromfile(fout, dtype=np.float64)


def _tables(model):
    return [model.nbodies, model.nq, model.nv], [np.asarray(model.jtype), np.asarray(model.qstart), np.asarray(model.vstart)]


def columns(nv):
    return 1 + 6 * nv


def perturb(exe, model, x, tau, eps=EPS_DEFAULT):
    """-> (x columns [P, nq + nv], tau columns [P, nv])"""
    dims, tables = _tables(model)
    w = model.nq + model.nv
    out = run(exe, "perturb", dims, [eps], *tables, x, tau).reshape(columns(model.nv), w + model.nv)
    return out[:, :w].copy(), out[:, w:].copy()


def difference(exe, model, finals, eps=EPS_DEFAULT):
    """finals [P, nq + nv] -> (A [n, n], B [n, nv]) as [row, col]"""
    dims, tables = _tables(model)
    nv, n = model.nv, 2 * model.nv
    out = run(exe, "difference", dims, [eps], *tables, finals)
    return out[:n * n].reshape(n, n).T.copy(), out[n * n:].reshape(nv, n).T.copy()


def tvlqr(exe, A, B, actuated, Q, R, Qf):
    """A [S, n, n], B [S, n, nv], Q, Qf [n, n], R [nu, nu], all [row, col] -> (status, K [S, nu, n], P [S + 1, n, n])"""
    A, B = np.asarray(A, dtype=float), np.asarray(B, dtype=float)
    S, n, nv, nu = A.shape[0], A.shape[1], B.shape[2], len(actuated)
    cm = lambda M: np.asarray(M, dtype=float).swapaxes(-1, -2)   # column-major
    out = run(exe, "tvlqr", [S, nv, nu], actuated, cm(A), cm(B), cm(Q), cm(R), cm(Qf))
    K = out[1:1 + S * nu * n].reshape(S, n, nu).swapaxes(1, 2).copy()
    P = out[1 + S * nu * n:].reshape(S + 1, n, n).swapaxes(1, 2).copy()
    return int(out[0]), K, P


def control(exe, model, K, x_nom, u_nom, x):
    dims, tables = _tables(model)
    nu = len(u_nom)
    return run(exe, "control", dims, [nu], *tables, np.asarray(K, dtype=float).T, x_nom, u_nom, x)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (the device's model, the oracle's model, a problem of N = 3, the solver parameters, the oracle, three states (q, v, tau)).
    The models with an example configuration are tests/plant_cases.py's, states(name) included; pendulum and free_body have none:
    unit weights, and states from a fixed seed (positions within 1 of zero - free_body: a random unit quaternion, 0.5 to 1.5 m
    above the ground -, velocities within 0.5, torques within 2, as plant_cases draws them)."""
    import plant_cases as pc
    from idto_amd.model import load_model
    from idto_amd.problem import ProblemDefinition, SolverParameters
    from oracle_lib import Oracle
    if name not in ("pendulum", "free_body"):
        prob, sp = pc.problem(name)
        return pc.case(name)[0], pc.case(name)[1], prob, sp, pc.oracle(name), pc.states(name)
    model = load_model(name)
    nq, nv, N = model.nq, model.nv, 3
    rng = np.random.default_rng(77 + len(name))
    states = []
    for _ in range(3):
        q = rng.uniform(-1.0, 1.0, nq)
        if name == "free_body":
            q[:4] /= np.linalg.norm(q[:4])
            q[6] = 1.0 + 0.5 * q[6]
        states.append((q, rng.uniform(-0.5, 0.5, nv), rng.uniform(-2.0, 2.0, nv)))
    q0 = states[0][0]
    prob = ProblemDefinition(num_steps=N, q_init=q0, v_init=np.zeros(nv), Qq=np.eye(nq), Qv=np.eye(nv), Qf_q=np.eye(nq),
                             Qf_v=np.eye(nv), R=np.eye(nv), q_nom=np.tile(q0, (N + 1, 1)), v_nom=np.zeros((N + 1, nv)), time_step=0.05)
    sp = SolverParameters(verbose=False, scaling=False, equality_constraints=False)
    return model, model, prob, sp, Oracle(model, prob, sp), states


def inputs(name, S):
    """-> (x [S, nq + nv], tau [S, nv]) of the case's first S states"""
    st = case(name)[5][:S]
    return np.array([np.concatenate([q, v]) for q, v, _ in st]), np.array([t for _, _, t in st])


@functools.lru_cache(maxsize=None)
def host_reference(name, S, h, substeps):
    """The host composition about the case's first S states with the default eps, computed once and never changed
    -> (x_next [S, nq + nv], A [S, n, n], B [S, n, nv])"""
    model, orc = case(name)[1], case(name)[4]
    x, tau = inputs(name, S)
    out = [host_linearize(built(), orc, model, x[s], tau[s], h, substeps) for s in range(S)]
    res = tuple(np.array([o[k] for o in out]) for k in range(3))
    for a in res:
        a.setflags(write=False)
    return res


def host_linearize(exe, orc, model, x, tau, h, substeps, eps=EPS_DEFAULT):
    """The host composition about one state -> (x_next, A, B, the columns' final states [P, nq + nv]).  Every column's host
    rollout must end with status 0 - no failed pivot (plant_cases.host_fd asserts it in every substep), every state of every
    substep finite: what plant_kernel reports as PLANT_OK - or the state is no case for the tests; asserted, by column."""
    import plant_cases as pc
    xc, tc = perturb(exe, model, x, tau, eps)
    nq = model.nq
    rollouts = [pc.host_rollout(orc, model, h, xc[c, :nq], xc[c, nq:], tc[c], substeps) for c in range(xc.shape[0])]
    for c, r in enumerate(rollouts):
        assert r.shape == (substeps, nq + model.nv) and np.isfinite(r).all(), f"column {c}: the host rollout did not end with status 0"
    finals = np.array([r[-1] for r in rollouts])
    A, B = difference(exe, model, finals, eps)
    return finals[0].copy(), A, B, finals
