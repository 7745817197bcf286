"""ctypes wrapper over oracle/liboracle.so — the CPU oracle (test infrastructure).

Imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
only; product code (idto_amd/) never imports this.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from idto_amd.model import CContactParams, CModel, CProblem, CSolverParams, CStats, Model, dptr, iptr
from idto_amd.problem import ProblemDefinition, SolverParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def _load(name):
    path = os.path.join(ORACLE_DIR, name)
    if not os.path.exists(path):
        build_oracle()
    lib = C.CDLL(path)
    lib.orc_create.restype = C.c_void_p
    lib.orc_create.argtypes = [C.POINTER(CModel), C.POINTER(CProblem), C.POINTER(CContactParams),
                               C.POINTER(CSolverParams)]
    lib.orc_ws_create.restype = C.c_void_p
    lib.orc_last_error.restype = C.c_char_p
    lib.orc_contact_threshold.restype = C.c_double
    lib.orc_time_gn_steps.restype = C.c_double
    return lib


_libs = {}


def lib(libm=False):
    key = "liboracle_libm.so" if libm else "liboracle.so"
    if key not in _libs:
        _libs[key] = _load(key)
    return _libs[key]


def _d(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class Stats:
    FIELDS = ["iteration_times", "iteration_costs", "linesearch_iterations", "linesearch_alphas",
              "trust_region_radii", "q_norms", "dq_norms", "dqH_norms", "trust_ratios", "gradient_norms", "dL_dqs",
              "h_norms", "merits"]

    def __init__(self, capacity):
        self.c = CStats()
        self.c.capacity = capacity
        self._arr = {}
        for f in self.FIELDS:
            if f == "linesearch_iterations":
                a = np.zeros(capacity, dtype=np.int32)
                setattr(self.c, f, iptr(a))
            else:
                a = np.zeros(capacity)
                setattr(self.c, f, dptr(a))
            self._arr[f] = a

    def __getattr__(self, k):
        if k in Stats.FIELDS:
            return self._arr[k][: self.c.count]
        raise AttributeError(k)

    @property
    def solve_time(self):
        return self.c.solve_time


class Oracle:
    """One TrajectoryOptimizer instance of the CPU oracle."""

    def __init__(self, model: Model, prob: ProblemDefinition, params: SolverParameters, libm=False):
        self.lib = lib(libm)
        self.model, self.prob, self.params = model, prob, params
        self.nq, self.nv, self.N = model.nq, model.nv, prob.num_steps
        cm, self._k1 = model.to_c()
        cp, self._k2 = prob.to_c()
        cc = params.contact_to_c()
        cs = params.to_c()
        self.h = C.c_void_p(self.lib.orc_create(C.byref(cm), C.byref(cp), C.byref(cc), C.byref(cs)))
        if not self.h:
            raise RuntimeError(self.lib.orc_last_error().decode())

    def __del__(self):
        try:
            if self.h:
                self.lib.orc_destroy(self.h)
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.orc_last_error().decode())

    @property
    def num_vars(self):
        return (self.N + 1) * self.nq

    @property
    def num_eq(self):
        return self.lib.orc_num_equality_constraints(self.h)

    @property
    def contact_threshold(self):
        return self.lib.orc_contact_threshold(self.h)

    # ---- physics at one configuration
    def inverse_dynamics(self, q, v, a, full=True):
        tau = np.zeros(self.nv)
        self._chk(self.lib.orc_inverse_dynamics(self.h, dptr(_d(q)), dptr(_d(v)), dptr(_d(a)), int(full), dptr(tau)))
        return tau

    def mass_matrix(self, q):
        M = np.zeros((self.nv, self.nv))
        self._chk(self.lib.orc_mass_matrix(self.h, dptr(_d(q)), dptr(M)))
        return M.T.copy()  # column-major -> [row, col]

    def nplus(self, q):
        N = np.zeros((self.nq, self.nv))
        self._chk(self.lib.orc_nplus(self.h, dptr(_d(q)), dptr(N)))
        return N.T.copy()  # (nv, nq)

    def body_poses(self, q):
        X = np.zeros((self.model.nbodies, 12))
        self._chk(self.lib.orc_body_poses(self.h, dptr(_d(q)), dptr(X)))
        return X

    def signed_distances(self, q):
        n = self.model.npairs
        phi, nr, ca, cb = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        self._chk(self.lib.orc_signed_distances(self.h, dptr(_d(q)), dptr(phi), dptr(nr), dptr(ca), dptr(cb)))
        return phi, nr, ca, cb

    # ---- trajectory-level (q: (N+1, nq))
    def eval_traj(self, q):
        v, a, tau = np.zeros((self.N + 1, self.nv)), np.zeros((self.N, self.nv)), np.zeros((self.N, self.nv))
        cost = C.c_double()
        self._chk(self.lib.orc_eval_traj(self.h, dptr(_d(q)), dptr(v), dptr(a), dptr(tau), C.byref(cost)))
        return v, a, tau, cost.value

    def calc_cost(self, q, v, tau):
        cost = C.c_double()
        self._chk(self.lib.orc_calc_cost(self.h, dptr(_d(q)), dptr(_d(v)), dptr(_d(tau)), C.byref(cost)))
        return cost.value

    def eval_partials(self, q):
        """Returns dict of arrays [t, col(nq), row(nv)] (column-major blocks) ->
        transposed to [t, row(nv), col(nq)]."""
        N, nv, nq = self.N, self.nv, self.nq
        out = {k: np.zeros((n, nq, nv)) for k, n in (("dtau_dqm", N), ("dtau_dqt", N), ("dtau_dqp", N),
                                                      ("dvt_dqt", N + 1), ("dvt_dqm", N + 1))}
        self._chk(self.lib.orc_eval_partials(self.h, dptr(_d(q)), dptr(out["dtau_dqm"]), dptr(out["dtau_dqt"]),
                                             dptr(out["dtau_dqp"]), dptr(out["dvt_dqt"]), dptr(out["dvt_dqm"])))
        return {k: np.ascontiguousarray(v.transpose(0, 2, 1)) for k, v in out.items()}

    def grad_hess(self, q):
        n, nq = self.N + 1, self.nq
        g = np.zeros(n * nq)
        bands = [np.zeros((n, nq, nq)) for _ in range(5)]
        self._chk(self.lib.orc_grad_hess(self.h, dptr(_d(q)), dptr(g), *[dptr(b) for b in bands]))
        return g, [np.ascontiguousarray(b.transpose(0, 2, 1)) for b in bands]  # [blk, row, col]

    def gn_step(self, q):
        g, p = np.zeros(self.num_vars), np.zeros(self.num_vars)
        self._chk(self.lib.orc_gn_step(self.h, dptr(_d(q)), dptr(g), dptr(p)))
        return g, p

    def eval_all(self, q):
        nvars, neq, n, nq = self.num_vars, self.num_eq, self.N + 1, self.nq
        D, gs, h = np.zeros(nvars), np.zeros(nvars), np.zeros(max(neq, 1))
        J = np.zeros((nvars, max(neq, 1)))
        lam, mg = np.zeros(max(neq, 1)), np.zeros(nvars)
        merit = C.c_double()
        bands = [np.zeros((n, nq, nq)) for _ in range(3)]
        eq = self.params.equality_constraints and neq > 0
        null = C.POINTER(C.c_double)()
        self._chk(self.lib.orc_eval_all(self.h, dptr(_d(q)), dptr(D), dptr(gs), dptr(h) if neq else null,
                                        dptr(J) if neq else null, dptr(lam) if eq else null, C.byref(merit),
                                        dptr(mg), *[dptr(b) for b in bands]))
        return dict(D=D, g_scaled=gs, h=h[:neq], J=J.T[:neq].copy(), lam=lam[:neq], merit=merit.value,
                    merit_grad=mg, Hs=[np.ascontiguousarray(b.transpose(0, 2, 1)) for b in bands])

    def dogleg(self, q, Delta):
        dq, dqH = np.zeros(self.num_vars), np.zeros(self.num_vars)
        act = C.c_int()
        self._chk(self.lib.orc_dogleg(self.h, dptr(_d(q)), C.c_double(Delta), dptr(dq), dptr(dqH), C.byref(act)))
        return dq, dqH, bool(act.value)

    def trust_ratio(self, q, dq):
        rho = C.c_double()
        self._chk(self.lib.orc_trust_ratio(self.h, dptr(_d(q)), dptr(_d(dq)), C.byref(rho)))
        return rho.value

    def solve(self, q_guess, capacity=None):
        cap = capacity or max(self.params.max_iterations, 1)
        q, v, tau = np.zeros((self.N + 1, self.nq)), np.zeros((self.N + 1, self.nv)), np.zeros((self.N, self.nv))
        st = Stats(cap)
        flag, reason = C.c_int(), C.c_int()
        self._chk(self.lib.orc_solve(self.h, dptr(_d(q_guess)), dptr(q), dptr(v), dptr(tau), C.byref(st.c),
                                     C.byref(flag), C.byref(reason)))
        return dict(q=q, v=v, tau=tau, stats=st, flag=flag.value, reason=reason.value)

    # warm start
    def create_warm_start(self, q_guess):
        return C.c_void_p(self.lib.orc_ws_create(self.h, dptr(_d(q_guess))))

    def solve_from_warm_start(self, ws, capacity=None):
        cap = capacity or max(self.params.max_iterations, 1)
        q, v, tau = np.zeros((self.N + 1, self.nq)), np.zeros((self.N + 1, self.nv)), np.zeros((self.N, self.nv))
        st = Stats(cap)
        flag, reason = C.c_int(), C.c_int()
        self._chk(self.lib.orc_ws_solve(self.h, ws, dptr(q), dptr(v), dptr(tau), C.byref(st.c), C.byref(flag),
                                        C.byref(reason)))
        return dict(q=q, v=v, tau=tau, stats=st, flag=flag.value, reason=reason.value)

    def ws_get(self, ws):
        q = np.zeros((self.N + 1, self.nq))
        Delta = C.c_double()
        self.lib.orc_ws_get(self.h, ws, dptr(q), C.byref(Delta))
        return q, Delta.value

    def ws_set_q(self, ws, q):
        self.lib.orc_ws_set_q(self.h, ws, dptr(_d(q)))

    def reset_initial_conditions(self, q_init, v_init):
        self.lib.orc_reset_initial_conditions(self.h, dptr(_d(q_init)), dptr(_d(v_init)))

    def update_nominal_trajectory(self, q_nom, v_nom):
        self.lib.orc_update_nominal_trajectory(self.h, dptr(_d(q_nom)), dptr(_d(v_nom)))

    def time_gn_steps(self, q, iters):
        return self.lib.orc_time_gn_steps(self.h, dptr(_d(q)), int(iters))

    def time_gn_parts(self, q, iters):
        """seconds per Gauss-Newton step in [tau, derivatives, assembly, factor + solve]"""
        parts = np.zeros(4)
        self._chk(self.lib.orc_time_gn_parts(self.h, dptr(_d(q)), int(iters), dptr(parts)))
        return dict(zip(("tau", "derivatives", "assembly", "solve"), parts.tolist()))


# ---- block penta-diagonal helpers; blocks given as [blk, row, col] ---------------
def _cm(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.float64).transpose(0, 2, 1))


def penta_make_symmetric(A, B, C_):
    n, bs = A.shape[0], A.shape[1]
    Cc, D, E = _cm(C_), np.zeros((n, bs, bs)), np.zeros((n, bs, bs))
    lib().orc_penta_make_symmetric(n, bs, dptr(_cm(A)), dptr(_cm(B)), dptr(Cc), dptr(D), dptr(E))
    return Cc.transpose(0, 2, 1).copy(), D.transpose(0, 2, 1).copy(), E.transpose(0, 2, 1).copy()


def penta_solve(A, B, C_, D, E, rhs):
    n, bs = A.shape[0], A.shape[1]
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(rhs, dtype=np.float64)).copy())  # [nrhs, n*bs]
    rc = lib().orc_penta_solve(n, bs, dptr(_cm(A)), dptr(_cm(B)), dptr(_cm(C_)), dptr(_cm(D)), dptr(_cm(E)), dptr(x),
                               x.shape[0])
    assert rc == 0
    return x if np.ndim(rhs) == 2 else x[0]


def penta_multiply(A, B, C_, D, E, v):
    n, bs = A.shape[0], A.shape[1]
    out = np.zeros(n * bs)
    lib().orc_penta_multiply(n, bs, dptr(_cm(A)), dptr(_cm(B)), dptr(_cm(C_)), dptr(_cm(D)), dptr(_cm(E)),
                             dptr(_d(v)), dptr(out))
    return out


def penta_make_dense(A, B, C_, D, E):
    n, bs = A.shape[0], A.shape[1]
    M = np.zeros((n * bs, n * bs))
    lib().orc_penta_make_dense(n, bs, dptr(_cm(A)), dptr(_cm(B)), dptr(_cm(C_)), dptr(_cm(D)), dptr(_cm(E)), dptr(M))
    return M.T.copy()


def refined_solution(Hd, rhs, steps=6, half_bandwidth=None):
    """Extended-precision reference solution of H x = rhs (H dense, symmetric positive definite): iterative
    refinement with the residual and the accumulated solution in 80-bit long double (numpy.longdouble;
    x86 extended precision, eps = 1.1e-19), run twice with two different working factorisations
    (LAPACK Cholesky and pivoted LU).  Returns (x, uncertainty): x as float64 and the relative max-norm
    distance between the two runs - the accuracy to which x itself is known (~cond * 1e-19).
    This is the yardstick the solver parity tests measure BOTH device solvers against: the
    reference's algorithm (pivoted-LU block Thomas) and the production block LDL^T.
    half_bandwidth w: H[i, j] = 0 for |i - j| > w (checked) - the same two runs with LAPACK's band Cholesky and band
    pivoted LU as the working factorisations and the long-double residual formed from the 2 w + 1 diagonals: what the
    systems of a few thousand unknowns cost is then the band's share of the dense work."""
    import scipy.linalg as sl
    assert np.finfo(np.longdouble).eps < 1e-18, "long double is not extended precision on this platform"
    Hd = np.asarray(Hd, dtype=np.float64)
    if half_bandwidth is not None:
        return _refined_solution_banded(Hd, np.asarray(rhs, dtype=np.float64).ravel(), steps, int(half_bandwidth))
    Hl, bl = Hd.astype(np.longdouble), np.asarray(rhs, dtype=np.float64).ravel().astype(np.longdouble)
    outs = []
    for kind in ("cho", "lu"):
        fac = sl.cho_factor(Hd) if kind == "cho" else sl.lu_factor(Hd)
        solve = (lambda r: sl.cho_solve(fac, r)) if kind == "cho" else (lambda r: sl.lu_solve(fac, r))
        x = solve(np.asarray(rhs, dtype=np.float64).ravel()).astype(np.longdouble)
        for _ in range(steps):
            r = bl - Hl @ x
            x = x + solve(r.astype(np.float64)).astype(np.longdouble)
        outs.append(x)
    nrm = float(np.abs(outs[0]).max()) + 1e-300
    return outs[0].astype(np.float64), float(np.abs(outs[0] - outs[1]).max()) / nrm


def _refined_solution_banded(Hd, b, steps, w):
    import scipy.linalg as sl
    size = Hd.shape[0]
    assert not np.triu(Hd, w + 1).any() and not np.tril(Hd, -w - 1).any(), "entries outside the band"
    ab = np.zeros((2 * w + 1, size))          # LAPACK band storage: ab[w + i - j, j] = H[i, j]
    for d in range(-w, w + 1):                # d = j - i
        if d >= 0:
            ab[w - d, d:] = np.diagonal(Hd, d)
        else:
            ab[w - d, :size + d] = np.diagonal(Hd, d)
    abl, bl = ab.astype(np.longdouble), b.astype(np.longdouble)

    def residual(x):
        r = bl.copy()
        for d in range(-w, w + 1):
            if d >= 0:
                r[:size - d] -= abl[w - d, d:] * x[d:]
            else:
                r[-d:] -= abl[w - d, :size + d] * x[:size + d]
        return r
    cb = sl.cholesky_banded(ab[w:], lower=True)
    outs = []
    for solve in (lambda r: sl.cho_solve_banded((cb, True), r), lambda r: sl.solve_banded((w, w), ab, r)):
        x = solve(b).astype(np.longdouble)
        for _ in range(steps):
            x = x + solve(residual(x).astype(np.float64)).astype(np.longdouble)
        outs.append(x)
    nrm = float(np.abs(outs[0]).max()) + 1e-300
    return outs[0].astype(np.float64), float(np.abs(outs[0] - outs[1]).max()) / nrm


def penta_scale_by_diagonal(A, B, C_, D, E, s):
    n, bs = A.shape[0], A.shape[1]
    bands = [_cm(x).copy() for x in (A, B, C_, D, E)]
    lib().orc_penta_scale_by_diagonal(n, bs, *[dptr(b) for b in bands], dptr(_d(s)))
    return [b.transpose(0, 2, 1).copy() for b in bands]


def det_sincos(x):
    x = _d(x)
    s, c = np.zeros_like(x), np.zeros_like(x)
    lib().orc_det_sincos(dptr(x), dptr(s), dptr(c), x.size)
    return s, c


def det_exp(x):
    x = _d(x)
    y = np.zeros_like(x)
    lib().orc_det_exp(dptr(x), dptr(y), x.size)
    return y


def det_log(x):
    x = _d(x)
    y = np.zeros_like(x)
    lib().orc_det_log(dptr(x), dptr(y), x.size)
    return y
