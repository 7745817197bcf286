"""`TrajectoryOptimizer` — Python face of the host-side optimizer (libidto_opt.so,
include/idto_opt.h), the counterpart of the reference's pybind11 class
(reference python_bindings/trajectory_optimizer_py.cc:34-59): same method names
(`time_step`, `num_steps`, `Solve`, `CreateWarmStart`, `SolveFromWarmStart`,
`ResetInitialConditions`, `UpdateNominalTrajectory`, `params`, `prob`), with the Drake
plant replaced by a `Model`.  The hot path runs on the MI355X (libidto_hip.so); there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import hip
from .model import CContactParams, CModel, CProblem, CSolverParams, CStats, Model, dptr, iptr
from .problem import ProblemDefinition, SolverParameters

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libidto_opt.so")
_lib = None

SOLVER_FLAGS = ("kSuccess", "kLinesearchMaxIters", "kFactorizationFailed", "kMaxIterationsReached")


def lib():
    global _lib
    if _lib is None:
        hip.lib()  # loads torch's HIP runtime first, then libidto_hip.so (see idto_amd/hip.py)
        if not os.path.exists(LIB_PATH):
            raise hip.HipLibraryMissing(f"{LIB_PATH} not found: run ./build.sh")
        L = C.CDLL(LIB_PATH)
        L.idto_opt_last_error.restype = C.c_char_p
        L.idto_opt_dense_ldlt_solve.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
        L.idto_opt_create.argtypes = [C.POINTER(CModel), C.POINTER(CProblem), C.POINTER(CContactParams),
                                      C.POINTER(CSolverParams), C.c_int, C.POINTER(C.c_void_p)]
        L.idto_opt_create_multi.argtypes = [C.POINTER(CModel), C.POINTER(CProblem), C.POINTER(CContactParams),
                                            C.POINTER(CSolverParams), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        L.idto_opt_destroy.argtypes = [C.c_void_p]
        L.idto_opt_num_steps.argtypes = [C.c_void_p]
        L.idto_opt_time_step.argtypes = [C.c_void_p]
        L.idto_opt_time_step.restype = C.c_double
        L.idto_opt_num_equality_constraints.argtypes = [C.c_void_p]
        P = C.POINTER(C.c_double)
        L.idto_opt_solve.argtypes = [C.c_void_p, P, P, P, P, C.POINTER(CStats), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.idto_opt_solve_batch_models.argtypes = [C.c_void_p, C.c_int, C.POINTER(CProblem), C.POINTER(C.POINTER(CModel)),
                                                  C.POINTER(C.POINTER(CContactParams)), P, C.c_int, P, P, P, C.POINTER(CStats),
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int), P, C.POINTER(C.c_int)]
        L.idto_opt_solve_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(CProblem), P, C.c_int, P, P, P, C.POINTER(CStats),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), P, C.POINTER(C.c_int)]
        L.idto_opt_scene_sizes.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        L.idto_opt_scene_report.argtypes = [C.c_void_p, C.c_int, P, P, P, P, P, P]
        L.idto_opt_actuated_dofs.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.idto_opt_plant_linearize.argtypes = [C.c_void_p, C.c_int, P, P, P, C.c_double, C.c_int, P, P, P, C.POINTER(C.c_int)]
        L.idto_opt_tvlqr.argtypes = [C.c_void_p, P, P, P, C.c_double, P, P, P, P, P, P, P, P, C.POINTER(C.c_int), P, P, C.POINTER(C.c_int)]
        L.idto_opt_track.argtypes = [C.c_void_p, P, P, P, C.c_double, P, P, P, P, P, C.c_int, P, C.c_int, P, P, P, C.POINTER(C.c_int), P, P,
                                     C.POINTER(C.c_int), P, P, P, C.POINTER(C.c_int)]
        L.idto_opt_batch_error.argtypes = [C.c_void_p, C.c_int]
        L.idto_opt_batch_error.restype = C.c_char_p
        L.idto_opt_last_batch_route.argtypes = [C.c_void_p]
        L.idto_opt_ws_create.argtypes = [C.c_void_p, P, C.POINTER(C.c_void_p)]
        L.idto_opt_ws_destroy.argtypes = [C.c_void_p]
        L.idto_opt_ws_set_q.argtypes = [C.c_void_p, C.c_void_p, P]
        L.idto_opt_ws_get.argtypes = [C.c_void_p, C.c_void_p, P, P]
        L.idto_opt_ws_solve.argtypes = [C.c_void_p, C.c_void_p, P, P, P, C.POINTER(CStats), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
        L.idto_opt_reset_initial_conditions.argtypes = [C.c_void_p, P, P]
        L.idto_opt_update_nominal_trajectory.argtypes = [C.c_void_p, P, P]
        L.idto_opt_eval.argtypes = [C.c_void_p, P, P, P, P, P, P, P, P]
        L.idto_opt_dogleg.argtypes = [C.c_void_p, P, C.c_double, P, P, C.POINTER(C.c_int)]
        L.idto_opt_trust_ratio.argtypes = [C.c_void_p, P, P, P]
        I = C.POINTER(C.c_int)
        L.idto_mpc_create.argtypes = [C.c_void_p, P, P, P, I, I, C.c_double, C.POINTER(C.c_void_p)]
        L.idto_mpc_destroy.argtypes = [C.c_void_p]
        L.idto_mpc_num_actuators.argtypes = [C.c_void_p]
        L.idto_mpc_update.argtypes = [C.c_void_p, C.c_double, P, P, P, P, P, P, I]
        L.idto_mpc_state.argtypes = [C.c_void_p, C.c_double, P]
        L.idto_mpc_control.argtypes = [C.c_void_p, C.c_double, P]
        L.idto_mpc_start_time.argtypes = [C.c_void_p]
        L.idto_mpc_start_time.restype = C.c_double
        L.idto_mpc_spline_eval.argtypes = [P, P, C.c_int, C.c_int, P, C.c_int, P]
        L.idto_mpc_stats.argtypes = [C.c_void_p, C.POINTER(CStats), P]
        L.idto_mpc_batch_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(CProblem), P, P, P, I, I, C.POINTER(C.c_void_p)]
        L.idto_mpc_batch_destroy.argtypes = [C.c_void_p]
        L.idto_mpc_batch_num_actuators.argtypes = [C.c_void_p]
        L.idto_mpc_batch_update.argtypes = [C.c_void_p, P, P, P, P, P, P, C.POINTER(CStats), I, P, I]
        L.idto_mpc_batch_state.argtypes = [C.c_void_p, C.c_int, C.c_double, P]
        L.idto_mpc_batch_control.argtypes = [C.c_void_p, C.c_int, C.c_double, P]
        L.idto_mpc_batch_start_time.argtypes = [C.c_void_p, C.c_int]
        L.idto_mpc_batch_start_time.restype = C.c_double
        L.idto_mpc_batch_flag.argtypes = [C.c_void_p, C.c_int]
        L.idto_mpc_batch_error.argtypes = [C.c_void_p, C.c_int]
        L.idto_mpc_batch_error.restype = C.c_char_p
        L.idto_mpc_spline_fit.argtypes = [P, P, C.c_int, C.c_int, P]
        L.idto_mpc_shift_reference.argtypes = [P, P, P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, P, I, P, P]
        L.idto_mpc_batch_plants_begin.argtypes = [C.c_void_p, C.c_double, P, C.c_int, P, C.c_int, C.c_int, C.c_int]
        L.idto_mpc_batch_plants_set_model.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.idto_mpc_batch_plants_set_states.argtypes = [C.c_void_p, P, P]
        L.idto_mpc_batch_plants_step.argtypes = [C.c_void_p, C.c_int]
        L.idto_mpc_batch_plants_state.argtypes = [C.c_void_p, C.c_int, P, P, I]
        L.idto_mpc_batch_plants_tick.argtypes = [C.c_void_p, C.c_int, P, P, P, P, C.POINTER(CStats), I, P, I]
        L.idto_plant_forward_dynamics.argtypes = [C.c_void_p, P, P, P, P, P]
        L.idto_plant_begin.argtypes = [C.c_void_p, C.c_double, C.c_int]
        L.idto_plant_set_state.argtypes = [C.c_void_p, C.c_double, P]
        L.idto_plant_get_state.argtypes = [C.c_void_p, P, P]
        L.idto_plant_step.argtypes = [C.c_void_p, C.c_int, P, C.c_int, P, I]
        L.idto_plant_solve_host.argtypes = [P, P, P, C.c_int, P]
        L.idto_plant_pd_plus_host.argtypes = [P, P, C.c_int, C.c_int, C.c_int, I, P, P, P, P, C.c_int, P, P]
        L.idto_plant_pd_plus_host.restype = None
        L.idto_plant_advance_host.argtypes = [C.c_int, I, I, I, C.c_int, C.c_double, P, P, P]
        L.idto_plant_advance_host.restype = None
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "idto_opt_last_error", "idto_opt_dense_ldlt_solve", "idto_opt_create", "idto_opt_create_multi", "idto_opt_destroy", "idto_opt_num_steps", "idto_opt_time_step",
    "idto_opt_num_equality_constraints", "idto_opt_solve", "idto_opt_ws_create", "idto_opt_ws_destroy",
    "idto_opt_ws_set_q", "idto_opt_ws_get", "idto_opt_ws_solve", "idto_opt_reset_initial_conditions",
    "idto_opt_update_nominal_trajectory", "idto_opt_eval", "idto_opt_dogleg", "idto_opt_trust_ratio",
    "idto_opt_solve_batch", "idto_opt_solve_batch_models", "idto_opt_batch_error", "idto_opt_last_batch_route",
    "idto_opt_scene_sizes", "idto_opt_scene_report",
    "idto_opt_actuated_dofs", "idto_opt_plant_linearize", "idto_opt_tvlqr", "idto_opt_track",
]
MPC_SYMBOLS = ["idto_mpc_create", "idto_mpc_destroy", "idto_mpc_num_actuators", "idto_mpc_update", "idto_mpc_state",
               "idto_mpc_control", "idto_mpc_start_time", "idto_mpc_spline_eval", "idto_mpc_stats",
               "idto_mpc_batch_create", "idto_mpc_batch_destroy", "idto_mpc_batch_num_actuators", "idto_mpc_batch_update",
               "idto_mpc_batch_state", "idto_mpc_batch_control", "idto_mpc_batch_start_time", "idto_mpc_batch_flag",
               "idto_mpc_batch_error", "idto_mpc_spline_fit", "idto_mpc_shift_reference",
               "idto_mpc_batch_plants_begin", "idto_mpc_batch_plants_set_model", "idto_mpc_batch_plants_set_states",
               "idto_mpc_batch_plants_step", "idto_mpc_batch_plants_state", "idto_mpc_batch_plants_tick"]


def _d(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class TrajectoryOptimizerStats:
    """reference optimizer/trajectory_optimizer_solution.h:58-185"""
    FIELDS = ["iteration_times", "iteration_costs", "linesearch_iterations", "linesearch_alphas",
              "trust_region_radii", "q_norms", "dq_norms", "dqH_norms", "trust_ratios", "gradient_norms", "dL_dqs",
              "h_norms", "merits"]

    def __init__(self, capacity=1000):
        self.c = CStats()
        self._arr = {}
        self._reserve(capacity)

    def _reserve(self, capacity):
        """room for `capacity` iterations (Solve sizes it from SolverParameters::max_iterations)"""
        assert self.c.count == 0
        self.c.capacity = capacity
        for f in self.FIELDS:
            a = np.zeros(capacity, dtype=np.int32 if f == "linesearch_iterations" else np.float64)
            setattr(self.c, f, iptr(a) if f == "linesearch_iterations" else dptr(a))
            self._arr[f] = a

    @property
    def truncated(self):
        """True if the solver ran more iterations than the arrays could hold"""
        return self.c.total > self.c.count

    def __getattr__(self, k):
        if k in TrajectoryOptimizerStats.FIELDS:
            return self._arr[k][: self.c.count]
        raise AttributeError(k)

    @property
    def solve_time(self):
        return self.c.solve_time

    def is_empty(self):
        return self.c.count == 0


class TrajectoryOptimizerSolution:
    """reference optimizer/trajectory_optimizer_solution.h:43-52"""

    def __init__(self):
        self.q = self.v = self.tau = None


class BatchSolveResult:
    """what `TrajectoryOptimizer.solve_batch` returns (TrajectoryOptimizer::BatchSolveResult of the C++ API): per entry a
    solution (None where the entry has none: it failed, or only_best was asked and it is not the best), the statistics,
    the SolverFlag name, the error text ("" for an entry with a solution), the convergence reason and the final cost;
    `best`: the entry of the lowest final cost among the usable ones (-1: none); `batch_route`: True when the device's
    batch loop ran the entries, False when they ran one after another."""

    def __init__(self, solutions, stats, flags, errors, reasons, final_costs, best, batch_route):
        self.solutions, self.stats, self.flags, self.errors = solutions, stats, flags, errors
        self.convergence_reasons, self.final_costs, self.best, self.batch_route = reasons, final_costs, best, batch_route


class WarmStart:
    def __init__(self, opt, handle):
        self._opt, self._h = opt, handle

    def set_q(self, q):
        opt = self._opt
        opt._chk(lib().idto_opt_ws_set_q(opt._h, self._h, dptr(_d(q))))

    def get_q(self):
        opt = self._opt
        q = np.zeros((opt.N + 1, opt.nq))
        opt._chk(lib().idto_opt_ws_get(opt._h, self._h, dptr(q), None))
        return q

    @property
    def Delta(self):
        d = C.c_double()
        self._opt._chk(lib().idto_opt_ws_get(self._opt._h, self._h, None, C.byref(d)))
        return d.value

    def __del__(self):
        try:
            lib().idto_opt_ws_destroy(self._h)
        except Exception:
            pass


class TrajectoryOptimizer:
    def __init__(self, model: Model, prob: ProblemDefinition, params: SolverParameters | None = None, device: int = 0,
                 devices=None):
        """`devices`: list of HIP devices of this node to shard the finite-difference grid over
        (devices[0] hosts the optimizer; one RCCL all-gather per evaluation of the partials)"""
        L = lib()
        params = params or SolverParameters()
        self.model, self._prob, self._params = model, prob, params
        self.nq, self.nv, self.N = model.nq, model.nv, prob.num_steps
        cm, self._k1 = model.to_c()
        cp, self._k2 = prob.to_c()
        cc, cs = params.contact_to_c(), params.to_c()
        h = C.c_void_p()
        if devices is None:
            rc = L.idto_opt_create(C.byref(cm), C.byref(cp), C.byref(cc), C.byref(cs), int(device), C.byref(h))
        else:  # sharded over several devices of the node (RCCL all-gather of the partials)
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = L.idto_opt_create_multi(C.byref(cm), C.byref(cp), C.byref(cc), C.byref(cs), arr, len(devices), C.byref(h))
        if rc != 0:
            raise RuntimeError(L.idto_opt_last_error().decode())
        self._h = h

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError(lib().idto_opt_last_error().decode())

    def close(self):
        """release the device context now (otherwise when the object is collected)"""
        if getattr(self, "_h", None):
            lib().idto_opt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API
    def time_step(self):
        return lib().idto_opt_time_step(self._h)

    def num_steps(self):
        return lib().idto_opt_num_steps(self._h)

    def num_equality_constraints(self):
        return lib().idto_opt_num_equality_constraints(self._h)

    def params(self):
        return self._params

    def prob(self):
        return self._prob

    def _outputs(self):
        return np.zeros((self.N + 1, self.nq)), np.zeros((self.N + 1, self.nv)), np.zeros((self.N, self.nv))

    def Solve(self, q_guess, solution: TrajectoryOptimizerSolution, stats: TrajectoryOptimizerStats):
        """returns the SolverFlag name; fills `solution` and `stats` (must be empty)"""
        if not stats.is_empty():
            raise RuntimeError("stats must be empty")
        if stats.c.capacity < self._params.max_iterations:
            stats._reserve(self._params.max_iterations)
        q, v, tau = self._outputs()
        flag, reason = C.c_int(), C.c_int()
        self._chk(lib().idto_opt_solve(self._h, dptr(_d(q_guess)), dptr(q), dptr(v), dptr(tau), C.byref(stats.c),
                                       C.byref(flag), C.byref(reason)))
        solution.q, solution.v, solution.tau = q, v, tau
        self.last_convergence_reason = reason.value
        return SOLVER_FLAGS[flag.value]

    def scene_report(self, solution_or_q, v=None, pair_rows: bool = False):
        """TrajectoryOptimizer::EvalScene, what replaces the reference's EvalPlantContext: body poses and spatial velocities,
        per-pair signed distances, witness points and contact forces and the generalised force of contact at the states of a
        solution - `scene_report(solution)` - or at `scene_report(q, v)` with q [S, nq], v [S, nv].  -> hip.SceneReport; one
        launch of the device, one wait.  The contact inside solution.tau[t] is -tau_contact[t + 1]."""
        from .hip import SceneReport
        q = solution_or_q.q if v is None else solution_or_q
        v = solution_or_q.v if v is None else v
        q, v = np.ascontiguousarray(_d(q)).reshape(-1, self.nq), np.ascontiguousarray(_d(v)).reshape(-1, self.nv)
        if len(q) != len(v):
            raise RuntimeError("scene_report: as many velocities as positions")
        S = len(q)
        sizes = [C.c_int() for _ in range(4)]
        self._chk(lib().idto_opt_scene_sizes(self._h, *[C.byref(s) for s in sizes]))
        nb, npairs, bd, pdn = (s.value for s in sizes)
        bodies, pairs, tau = np.zeros((S, nb, bd)), np.zeros((S, npairs, pdn)), np.zeros((S, self.nv))
        rows = np.zeros((S, npairs, self.nv)) if pair_rows else None
        self._chk(lib().idto_opt_scene_report(self._h, S, dptr(q), dptr(v), dptr(bodies), dptr(pairs), dptr(tau),
                                              dptr(rows) if rows is not None else None))
        return SceneReport(bodies, pairs, tau, rows)

    def actuated_dofs(self):
        """the velocity indices of the controls (every dof of a model without an actuator)"""
        out = np.zeros(self.nv, dtype=np.int32)
        nu = lib().idto_opt_actuated_dofs(self._h, out.ctypes.data_as(C.POINTER(C.c_int)))
        return out[:nu].copy()

    def linearize_plant(self, q, v, tau, h: float, substeps: int):
        """TrajectoryOptimizer::LinearizePlant: q [S, nq], v [S, nv], tau [S, nv] (the held torques) -> (x_next [S, nq + nv],
        A [S, n, n], B [S, n, nv], status [S, 2]) about the map of `substeps` substeps of h, in tangent coordinates (n = 2 nv)"""
        q, v, tau = (np.ascontiguousarray(_d(a)).reshape(-1, w) for a, w in ((q, self.nq), (v, self.nv), (tau, self.nv)))
        if not len(q) == len(v) == len(tau):
            raise RuntimeError("linearize_plant: as many velocities and torques as positions")
        S, nv, n = len(q), self.nv, 2 * self.nv
        xn, A, B, st = np.zeros((S, self.nq + nv)), np.zeros((S, n, n)), np.zeros((S, nv, n)), np.zeros((S, 2), dtype=np.int32)
        self._chk(lib().idto_opt_plant_linearize(self._h, S, dptr(q), dptr(v), dptr(tau), float(h), int(substeps), dptr(xn), dptr(A),
                                                 dptr(B), st.ctypes.data_as(C.POINTER(C.c_int))))
        return xn, np.ascontiguousarray(A.swapaxes(1, 2)), np.ascontiguousarray(B.swapaxes(1, 2)), st

    def tvlqr(self, solution, h: float, Qtheta, Qv, R, Qf_theta, Qf_v):
        """TrajectoryOptimizer::Tvlqr: the time-varying LQR gains about `solution` - its states (q_t, v_t), t = 0 ... N - 1, the held
        torque solution.tau[t], the map of one time step in substeps of h (time_step / h a whole number) - with the weights
        Q = blkdiag(Qtheta, Qv), R [nu, nu], Qf = blkdiag(Qf_theta, Qf_v) in tangent coordinates; the controls are actuated_dofs().
        -> hip.Tvlqr with the leading axis [N] (P: [N + 1]); u = solution.tau[t][actuated] - K[t] @ [q (-) q_t; v - v_t]"""
        from .hip import Tvlqr
        N, nv, n = self.N, self.nv, 2 * self.nv
        nu = len(self.actuated_dofs())
        q, v, tau = (np.ascontiguousarray(_d(a)) for a in (solution.q, solution.v, solution.tau))
        if q.size != (N + 1) * self.nq or v.size != (N + 1) * nv or tau.size != N * nv:
            raise RuntimeError("tvlqr: a solution of this optimizer's horizon is required")
        blocks = [np.ascontiguousarray(_d(M).reshape(nv, nv).T) for M in (Qtheta, Qv, Qf_theta, Qf_v)]
        Rm = np.ascontiguousarray(_d(R).reshape(nu, nu).T)
        xn, A, B, st = np.zeros((N, self.nq + nv)), np.zeros((N, n, n)), np.zeros((N, nv, n)), np.zeros((N, 2), dtype=np.int32)
        K, P, lst = np.zeros((N, n, nu)), np.zeros((N + 1, n, n)), C.c_int()
        self._chk(lib().idto_opt_tvlqr(self._h, dptr(q), dptr(v), dptr(tau), float(h), dptr(blocks[0]), dptr(blocks[1]), dptr(Rm),
                                       dptr(blocks[2]), dptr(blocks[3]), dptr(xn), dptr(A), dptr(B),
                                       st.ctypes.data_as(C.POINTER(C.c_int)), dptr(K), dptr(P), C.byref(lst)))
        A, B, K, P = (np.ascontiguousarray(M.swapaxes(1, 2)) for M in (A, B, K, P))
        return Tvlqr(xn, A, B, st, K, P, np.array([lst.value], dtype=np.int32))

    def track(self, solution, h: float, Qtheta, Qv, R, Qf_theta, Qf_v, x0s, zero_unactuated: bool = False):
        """TrajectoryOptimizer::Track: tvlqr's gains about `solution`, and behind them on the device one rollout per row of x0s
        [R, nq + nv] under u_t = solution.tau[t][actuated] - K[t] @ [q (-) q_t; v - v_t], held over a time step (zero_unactuated:
        solution.tau is zeroed on the unactuated dofs first) - one pass of the device, one wait.
        -> hip.Track with the leading axis [R]: x [R, N, nq + nv], u [R, N, nu], dx [R, N + 1, n], status [R, 2], .tvlqr as tvlqr returns"""
        from .hip import Track, Tvlqr
        N, nv, n = self.N, self.nv, 2 * self.nv
        nu = len(self.actuated_dofs())
        q, v, tau = (np.ascontiguousarray(_d(a)) for a in (solution.q, solution.v, solution.tau))
        if q.size != (N + 1) * self.nq or v.size != (N + 1) * nv or tau.size != N * nv:
            raise RuntimeError("track: a solution of this optimizer's horizon is required")
        x0 = np.ascontiguousarray(_d(x0s)).reshape(-1, self.nq + nv)
        nr = len(x0)
        blocks = [np.ascontiguousarray(_d(M).reshape(nv, nv).T) for M in (Qtheta, Qv, Qf_theta, Qf_v)]
        Rm = np.ascontiguousarray(_d(R).reshape(nu, nu).T)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        xn, A, B, st = np.zeros((N, self.nq + nv)), np.zeros((N, n, n)), np.zeros((N, nv, n)), np.zeros((N, 2), dtype=np.int32)
        K, P, lst = np.zeros((N, n, nu)), np.zeros((N + 1, n, n)), C.c_int()
        x, u, dx, tst = np.zeros((nr, N, self.nq + nv)), np.zeros((nr, N, nu)), np.zeros((nr, N + 1, n)), np.zeros((nr, 2), dtype=np.int32)
        self._chk(lib().idto_opt_track(self._h, dptr(q), dptr(v), dptr(tau), float(h), dptr(blocks[0]), dptr(blocks[1]), dptr(Rm),
                                       dptr(blocks[2]), dptr(blocks[3]), nr, dptr(x0), int(bool(zero_unactuated)), dptr(xn), dptr(A), dptr(B),
                                       ip(st), dptr(K), dptr(P), C.byref(lst), dptr(x), dptr(u), dptr(dx), ip(tst)))
        A, B, K, P = (np.ascontiguousarray(M.swapaxes(1, 2)) for M in (A, B, K, P))
        return Track(x, u, dx, tst, Tvlqr(xn, A, B, st, K, P, np.array([lst.value], dtype=np.int32)))

    def solve_batch(self, q_guesses, problems=None, only_best: bool = False, models=None, contacts=None) -> BatchSolveResult:
        """TrajectoryOptimizer::SolveBatch: entry b is `Solve(q_guesses[b])` on an optimizer made with `problems[b]` (None:
        this optimizer's own problem for every entry), all entries through ONE loop on the device - the trust-region batch
        loop or, with method = linesearch, the batch linesearch loop - where the configuration allows it (DESIGN.md section
        12.1), one after another otherwise.
        models / contacts: per entry a Model of the optimizer's topology / SolverParameters whose contact parameters the
        entry takes (None, or an entry None: the optimizer's own).  Such a batch runs the batch loops only (DESIGN.md section
        12.2): what they do not serve, B < 2 and a model that differs in a shared table raise before any device work."""
        q = _d(q_guesses)
        if q.ndim != 3 or q.shape[1:] != (self.N + 1, self.nq):
            raise RuntimeError(f"solve_batch: q_guesses must be [B, {self.N + 1}, {self.nq}]")
        B = q.shape[0]
        carr, keep = None, []
        if problems is not None:
            if len(problems) != B:
                raise RuntimeError(f"solve_batch: q_guesses and problems disagree in length ({B} and {len(problems)})")
            carr = (CProblem * B)()
            for b, pr in enumerate(problems):
                if pr.num_steps != self.N or np.shape(pr.q_nom) != (self.N + 1, self.nq) or np.shape(pr.v_nom) != (self.N + 1, self.nv) \
                        or np.size(pr.q_init) != self.nq or np.size(pr.v_init) != self.nv:
                    raise RuntimeError(f"solve_batch: problem {b} has another num_steps or other sizes than the optimizer's")
                carr[b], k = pr.to_c()
                keep.append(k)
        sq, sv, st = np.zeros((B, self.N + 1, self.nq)), np.zeros((B, self.N + 1, self.nv)), np.zeros((B, self.N, self.nv))
        stats = [TrajectoryOptimizerStats(max(self._params.max_iterations, 1)) for _ in range(B)]
        cst = (CStats * B)()
        for b in range(B):
            cst[b] = stats[b].c
        flags, reasons, best = (C.c_int * B)(), (C.c_int * B)(), C.c_int(-1)
        costs = np.zeros(B)
        marr = carr_c = None
        if models is not None or contacts is not None:
            for what, seq in (("models", models), ("contacts", contacts)):
                if seq is not None and len(seq) != B:
                    raise RuntimeError(f"solve_batch: q_guesses and {what} disagree in length ({B} and {len(seq)})")
            if models is not None:
                marr = (C.POINTER(CModel) * B)()
                for b, m in enumerate(models):
                    if m is not None:
                        cm, k = m.to_c()
                        keep.append((cm, k))
                        marr[b] = C.pointer(cm)
            if contacts is not None:
                carr_c = (C.POINTER(CContactParams) * B)()
                for b, sp in enumerate(contacts):
                    if sp is not None:
                        cc = sp.contact_to_c()
                        keep.append(cc)
                        carr_c[b] = C.pointer(cc)
        self._chk(lib().idto_opt_solve_batch_models(self._h, B, carr, marr, carr_c, dptr(q), int(only_best), dptr(sq), dptr(sv),
                                                    dptr(st), cst, flags, reasons, dptr(costs), C.byref(best)))
        errors = [lib().idto_opt_batch_error(self._h, b).decode() for b in range(B)]
        sols = []
        for b in range(B):
            stats[b].c = cst[b]   # (count, total and solve_time were written into the array's copy; the series are shared)
            has = not errors[b] and SOLVER_FLAGS[flags[b]] in ("kSuccess", "kMaxIterationsReached") and (not only_best or b == best.value)
            if has:
                sol = TrajectoryOptimizerSolution()
                sol.q, sol.v, sol.tau = sq[b], sv[b], st[b]
                sols.append(sol)
            else:
                sols.append(None)
        return BatchSolveResult(sols, stats, [SOLVER_FLAGS[f] for f in flags], errors, list(reasons), costs, best.value,
                                bool(lib().idto_opt_last_batch_route(self._h) == 1))

    def CreateWarmStart(self, q_guess):
        h = C.c_void_p()
        self._chk(lib().idto_opt_ws_create(self._h, dptr(_d(q_guess)), C.byref(h)))
        return WarmStart(self, h)

    def SolveFromWarmStart(self, warm_start: WarmStart, solution: TrajectoryOptimizerSolution,
                           stats: TrajectoryOptimizerStats):
        if stats.is_empty() and stats.c.capacity < self._params.max_iterations:
            stats._reserve(self._params.max_iterations)
        q, v, tau = self._outputs()
        flag, reason = C.c_int(), C.c_int()
        self._chk(lib().idto_opt_ws_solve(self._h, warm_start._h, dptr(q), dptr(v), dptr(tau), C.byref(stats.c),
                                          C.byref(flag), C.byref(reason)))
        solution.q, solution.v, solution.tau = q, v, tau
        self.last_convergence_reason = reason.value
        return SOLVER_FLAGS[flag.value]

    def ResetInitialConditions(self, q_init, v_init):
        self._chk(lib().idto_opt_reset_initial_conditions(self._h, dptr(_d(q_init)), dptr(_d(v_init))))
        self._prob.q_init, self._prob.v_init = np.array(q_init, float), np.array(v_init, float)

    def UpdateNominalTrajectory(self, q_nom, v_nom):
        self._chk(lib().idto_opt_update_nominal_trajectory(self._h, dptr(_d(q_nom)), dptr(_d(v_nom))))
        self._prob.q_nom, self._prob.v_nom = np.array(q_nom, float), np.array(v_nom, float)

    # ---- what the reference's C++ tests reach through TrajectoryOptimizerTester
    def eval(self, q):
        nvars, neq = (self.N + 1) * self.nq, self.num_equality_constraints()
        cost, merit = C.c_double(), C.c_double()
        out = dict(gradient=np.zeros(nvars), scaled_gradient=np.zeros(nvars), scale_factors=np.zeros(nvars),
                   merit_gradient=np.zeros(nvars))
        lam = np.zeros(max(neq, 1))
        use_eq = bool(self._params.equality_constraints) and neq > 0
        self._chk(lib().idto_opt_eval(self._h, dptr(_d(q)), C.byref(cost), dptr(out["gradient"]),
                                      dptr(out["scaled_gradient"]), dptr(out["scale_factors"]),
                                      dptr(lam) if use_eq else None, C.byref(merit), dptr(out["merit_gradient"])))
        out.update(cost=cost.value, merit=merit.value, lagrange_multipliers=lam[:neq] if use_eq else np.zeros(0))
        return out

    def dogleg(self, q, Delta):
        nvars = (self.N + 1) * self.nq
        dq, dqH, act = np.zeros(nvars), np.zeros(nvars), C.c_int()
        self._chk(lib().idto_opt_dogleg(self._h, dptr(_d(q)), float(Delta), dptr(dq), dptr(dqH), C.byref(act)))
        return dq, dqH, bool(act.value)

    def trust_ratio(self, q, dq):
        rho = C.c_double()
        self._chk(lib().idto_opt_trust_ratio(self._h, dptr(_d(q)), dptr(_d(dq)), C.byref(rho)))
        return rho.value
