"""ctypes binding of libidto_hip.so (include/idto_hip.h): the MI355X implementation
of IDTO's per-iteration gradient/Hessian path.

There is no CPU fallback: loading fails loudly if the library has not been built
(`./build.sh` or `__graft_entry__.build()`), and creating a context fails if no
HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .model import CContactParams, CModel, CProblem, Model, dptr
from .problem import ProblemDefinition, SolverParameters

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IDTO_HIP_LIB") or os.path.join(_HERE, "libidto_hip.so")   # (IDTO_HIP_LIB: a variant build, tools/fd_variants.sh)

ARR = dict(q=0, v=1, a=2, tau=3, nplus=4, dtau_dqm=5, dtau_dqt=6, dtau_dqp=7, gradient=8, H_A=9, H_B=10, H_C=11,
           step=12, cost=13, slab=14, debug=15, hbands=16, tr_dq=17, tr_w=18, tr_scale=19, asm_terms=20, con_S=21, con_lambda=22)

_lib = None

PLANT_HOLD, PLANT_PD_PLUS = 0, 1
PLANT_MAX_SUBSTEPS = 4096


SCENE_MODELS_PROBLEMS, SCENE_MODELS_PLANTS = 0, 1
SCENE_BODY_DOUBLES, SCENE_PAIR_DOUBLES = 18, 20


class SceneReport:
    """What idto_hip_scene_report returns, as named views of its arrays (include/idto_hip.h IDTO_SCENE_PAIR_*).  Leading axes:
    [batch, nstates] (a single problem: [nstates]), then the body or the pair.
      bodies [..., nbodies, 18]: X_WB [..., 12] = R_WB row-major, p;  V_WB [..., 6] = w, v of the body origin
      pairs [..., npairs, 20]: active (bool), phi, normal (A towards B), Ca, Cb, vn, vt, fn, force (on body B at (Ca + Cb) / 2)
      tau_contact [..., nv]: the generalised force that contact applies;  tau_pairs [..., npairs, nv] or None: its rows"""

    def __init__(self, bodies, pairs, tau_contact, tau_pairs):
        self.bodies, self.pairs, self.tau_contact, self.tau_pairs = bodies, pairs, tau_contact, tau_pairs
        self.X_WB, self.V_WB = bodies[..., 0:12], bodies[..., 12:18]
        self.active = pairs[..., 0] != 0.0
        self.phi = pairs[..., 1]
        self.normal, self.Ca, self.Cb = pairs[..., 2:5], pairs[..., 5:8], pairs[..., 8:11]
        self.vn, self.vt = pairs[..., 11], pairs[..., 12:15]
        self.fn, self.force = pairs[..., 15], pairs[..., 16:19]


LIN_EPS_DEFAULT = 6.0554544523933395e-06   # cbrt(2^-52), IDTO_LIN_EPS_DEFAULT


class Tvlqr:
    """What idto_hip_plant_tvlqr returns (include/idto_hip.h).  Leading axes [batch, nstates] (a single problem given without the
    batch axis: [nstates]); matrices as [row, col], deviations in tangent coordinates [dtheta (nv); dv (nv)], n = 2 nv.
      x_next [..., nq + nv], A [..., n, n], B [..., n, nv], lin_status [..., 2]: the linearisation (HipPath.plant_linearize)
      K [..., nu, n]: u = u_nom - K_t dx;  P [batch, nstates + 1, n, n]: the cost-to-go, P[..., -1] = Qf
      status [batch]: 0, or 1 + t for the first step t whose R + Bu^T P Bu has a bad pivot (K, P NaN from t downward)"""

    def __init__(self, x_next, A, B, lin_status, K, P, status):
        self.x_next, self.A, self.B, self.lin_status, self.K, self.P, self.status = x_next, A, B, lin_status, K, P, status


class Track:
    """What idto_hip_plant_track / idto_hip_plant_tvlqr_track return (include/idto_hip.h).  Leading axes [batch, nrollouts] (a
    single problem given without the batch axis: [nrollouts]); S control steps, n = 2 nv.
      x [..., S, nq + nv]: the state behind every step;  u [..., S, nu], dx [..., S + 1, n]: the law's control and deviation
      in front of step t, dx[..., S, :] the final state's;  status [..., 2]: {code, substeps completed} - the rows of a rollout
      behind its last completed step are NaN
      tvlqr: the Tvlqr of idto_hip_plant_tvlqr_track, else None"""

    def __init__(self, x, u, dx, status, tvlqr=None):
        self.x, self.u, self.dx, self.status, self.tvlqr = x, u, dx, status, tvlqr


class CPlantParams(C.Structure):
    """idto_plant_params_t (include/idto_hip.h)"""
    _fields_ = [("h", C.c_double), ("mode", C.c_int), ("Kp", C.POINTER(C.c_double)), ("kp_size", C.c_int),
                ("Kd", C.POINTER(C.c_double)), ("kd_size", C.c_int), ("feed_forward", C.c_int),
                ("record_capacity", C.c_int), ("block_threads", C.c_int)]


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build the HIP extension first (./build.sh). "
                "idto_amd has no CPU fallback for the hot path.")
        # torch ships its own ROCm runtime; load it FIRST so that this library binds to the
        # same libamdhip64 (two HIP runtimes in one process lose the device for one of them).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.idto_hip_last_error.restype = C.c_char_p
        L.idto_hip_create.argtypes = [C.POINTER(CModel), C.POINTER(CProblem), C.POINTER(CContactParams), C.c_int,
                                      C.POINTER(C.c_void_p)]
        L.idto_hip_create_batch.argtypes = [C.POINTER(CModel), C.POINTER(CProblem), C.POINTER(CContactParams), C.c_int,
                                            C.c_int, C.POINTER(C.c_void_p)]
        L.idto_hip_batch_size.argtypes = [C.c_void_p]
        L.idto_hip_set_problem_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(CProblem)]
        L.idto_hip_set_model_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(CModel), C.POINTER(CContactParams)]
        L.idto_hip_check_model_batch.argtypes = L.idto_hip_set_model_batch.argtypes
        L.idto_hip_set_q_batch.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.idto_hip_gn_step_batch.argtypes = [C.c_void_p]
        L.idto_hip_get_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_solver_status_batch.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.idto_hip_comm_unique_id.argtypes = [C.c_char_p, C.c_int]
        L.idto_hip_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.idto_hip_comm_init_all.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.idto_hip_gn_step_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        for f in ("comm_destroy", "allgather_slab", "gn_step_sharded"):
            getattr(L, "idto_hip_" + f).argtypes = [C.c_void_p]
        L.idto_hip_tr_prepare.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_tr_trial.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_double)]
        L.idto_hip_tr_accept.argtypes = [C.c_void_p]
        L.idto_hip_tr_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                        C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.idto_hip_tr_solve_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double,
                                              C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.idto_hip_tr_solve_batch_constrained.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                                          C.c_double, C.c_double, C.POINTER(C.c_int), C.c_int,
                                                          C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.idto_hip_tr_solve_fetch.argtypes = L.idto_hip_tr_solve.argtypes + [C.POINTER(C.c_double)] * 5
        L.idto_hip_tr_solve_batch_fetch.argtypes = (
            [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double,
             C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
            + [C.POINTER(C.c_double)] * 5 + [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)])
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.idto_hip_mpc_batch_begin.argtypes = [C.c_void_p, pi, pi, C.c_int]
        L.idto_hip_mpc_batch_store.argtypes = [C.c_void_p, pd, pd, pd, pd, pd]
        L.idto_hip_mpc_batch_shift.argtypes = [C.c_void_p, pd, pd, pd, pd]
        L.idto_hip_mpc_batch_replan.argtypes = ([C.c_void_p, pd, pd, C.c_int, C.c_int, C.c_int, C.c_int, pd, C.c_double, C.c_double,
                                                 pi, C.c_int, pd, pd, pd, pd, pd, pd, pi, pi, pd, pd])
        L.idto_hip_forward_dynamics.argtypes = [C.c_void_p, pd, pd, pd, pd, pd]
        L.idto_hip_plant_begin.argtypes = [C.c_void_p, C.POINTER(CPlantParams)]
        L.idto_hip_plant_set_model.argtypes = [C.c_void_p, C.c_int, C.POINTER(CModel), C.POINTER(CContactParams)]
        L.idto_hip_plant_set_state.argtypes = [C.c_void_p, pd, pd]
        L.idto_hip_plant_get_state.argtypes = [C.c_void_p, pd, pd]
        L.idto_hip_plant_step.argtypes = [C.c_void_p, C.c_int, pd, C.c_int, pd, pi]
        L.idto_hip_mpc_batch_tick_plants.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, pd, C.c_double, C.c_double,
                                                      pi, C.c_int, pd, pd, pd, pd, pd, pd, pi, pi, pd, pd, pd, pi])
        L.idto_hip_scene_sizes.argtypes = [C.c_void_p, pi, pi, pi, pi]
        L.idto_hip_scene_report.argtypes = [C.c_void_p, C.c_int, pd, C.c_int, pd, pd, pd, pd]
        pl = C.POINTER(C.c_long)
        L.idto_hip_lin_sizes.argtypes = [C.c_void_p, C.c_int, C.c_int, pi, pi, pl, pl, pl, pl, pl]
        L.idto_hip_plant_linearize.argtypes = [C.c_void_p, C.c_int, pd, pd, C.c_double, C.c_int, C.c_double, C.c_int, pd, pd, pd, pi]
        L.idto_hip_plant_tvlqr.argtypes = ([C.c_void_p, C.c_int, pd, pd, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, pi, pd, pd, pd,
                                            pd, pd, pd, pi, pd, pd, pi])
        L.idto_hip_plant_track.argtypes = ([C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, pi, pd, pd, pd, C.c_int, pd, C.c_int,
                                            pd, pd, pd, pi])
        L.idto_hip_plant_tvlqr_track.argtypes = ([C.c_void_p, C.c_int, pd, pd, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, pi, pd, pd,
                                                  pd, C.c_int, pd, C.c_int, pd, pd, pd, pi, pd, pd, pi, pd, pd, pd, pi])
        L.idto_hip_tr_reject.argtypes = [C.c_void_p]
        L.idto_hip_tr_set_scale_memory.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.idto_hip_tr_set_convergence.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.idto_hip_set_unactuated_dofs.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.idto_hip_destroy.argtypes = [C.c_void_p]
        L.idto_hip_set_problem.argtypes = [C.c_void_p, C.POINTER(CProblem)]
        L.idto_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.idto_hip_get_stream.argtypes = [C.c_void_p]
        L.idto_hip_get_stream.restype = C.c_void_p
        L.idto_hip_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.idto_hip_set_q.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.idto_hip_set_q_device.argtypes = [C.c_void_p, C.c_void_p]
        L.idto_hip_trial_cost.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]
        L.idto_hip_costs_along.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_ls_alphas.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_ls_solve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_ls_solve_fetch.argtypes = L.idto_hip_ls_solve.argtypes + [C.POINTER(C.c_double)] * 3
        L.idto_hip_costs_along_batch.argtypes = L.idto_hip_costs_along.argtypes
        L.idto_hip_ls_solve_batch_fetch.argtypes = L.idto_hip_ls_solve.argtypes + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_int)]
        for f in ("eval_tau", "eval_partials", "grad_hess", "gn_step", "sync", "timing_reset"):
            getattr(L, "idto_hip_" + f).argtypes = [C.c_void_p]
        L.idto_hip_factor_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.idto_hip_solve_host.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_solve_dense_ldlt.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.idto_hip_constraint_schur.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double),
                                                C.POINTER(C.c_double)]
        L.idto_hip_constraint_schur_begin.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.idto_hip_prefetch.argtypes = [C.c_void_p, C.c_int]
        L.idto_hip_constraint_solve.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 4
        L.idto_hip_constraint_step.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double)]
        L.idto_hip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.idto_hip_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
        L.idto_hip_timing_enable.argtypes = [C.c_void_p, C.c_int]
        L.idto_hip_timing_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.idto_hip_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.idto_hip_device_ptr.argtypes = [C.c_void_p, C.c_int]
        L.idto_hip_device_ptr.restype = C.c_void_p
        L.idto_hip_array_size.argtypes = [C.c_void_p, C.c_int]
        L.idto_hip_array_size.restype = C.c_long
        L.idto_hip_slab_stride.argtypes = [C.c_void_p]
        L.idto_hip_solver_status.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.idto_hip_math_probe.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int] + [C.POINTER(C.c_double)] * 6
        _lib = L
    return _lib


EXPORTED_SYMBOLS = [
    "idto_hip_last_error", "idto_hip_create", "idto_hip_destroy", "idto_hip_set_problem", "idto_hip_set_stream",
    "idto_hip_get_stream", "idto_hip_set_shard", "idto_hip_set_q", "idto_hip_set_q_device", "idto_hip_eval_tau", "idto_hip_eval_tau_partials", "idto_hip_trial_cost", "idto_hip_costs_along", "idto_hip_ls_alphas", "idto_hip_ls_solve", "idto_hip_ls_solve_fetch", "idto_hip_costs_along_batch", "idto_hip_ls_solve_batch_fetch", "idto_hip_constraint_schur",
    "idto_hip_constraint_schur_begin", "idto_hip_constraint_solve", "idto_hip_constraint_step", "idto_hip_prefetch",
    "idto_hip_eval_partials", "idto_hip_grad_hess", "idto_hip_factor_solve", "idto_hip_gn_step", "idto_hip_solve_host",
    "idto_hip_solve_dense_ldlt", "idto_hip_dense_solve_count",
    "idto_hip_set_option", "idto_hip_get_option",
    "idto_hip_timing_enable", "idto_hip_timing_reset", "idto_hip_timing_get", "idto_hip_sync", "idto_hip_get",
    "idto_hip_device_ptr", "idto_hip_array_size", "idto_hip_slab_stride", "idto_hip_math_probe",
    "idto_hip_solver_status", "idto_hip_create_batch", "idto_hip_create_batch_like", "idto_hip_batch_size", "idto_hip_set_problem_batch", "idto_hip_set_model_batch", "idto_hip_check_model_batch",
    "idto_hip_set_q_batch", "idto_hip_gn_step_batch", "idto_hip_get_batch", "idto_hip_get_many", "idto_hip_solver_status_batch",
    "idto_hip_tr_prepare", "idto_hip_tr_trial", "idto_hip_tr_accept", "idto_hip_tr_reject", "idto_hip_tr_set_scale_memory", "idto_hip_tr_set_convergence", "idto_hip_tr_solve", "idto_hip_tr_solve_fetch", "idto_hip_tr_solve_batch", "idto_hip_tr_solve_batch_constrained", "idto_hip_tr_solve_batch_fetch", "idto_hip_set_unactuated_dofs",
    "idto_hip_mpc_batch_begin", "idto_hip_mpc_batch_store", "idto_hip_mpc_batch_shift", "idto_hip_mpc_batch_replan",
    "idto_hip_forward_dynamics", "idto_hip_plant_begin", "idto_hip_plant_set_model", "idto_hip_plant_set_state",
    "idto_hip_plant_get_state", "idto_hip_plant_step", "idto_hip_mpc_batch_tick_plants",
    "idto_hip_scene_sizes", "idto_hip_scene_report",
    "idto_hip_lin_sizes", "idto_hip_plant_linearize", "idto_hip_plant_tvlqr",
    "idto_hip_plant_track", "idto_hip_plant_tvlqr_track",
    "idto_hip_rccl_info", "idto_hip_comm_unique_id", "idto_hip_comm_init", "idto_hip_comm_init_all", "idto_hip_comm_destroy",
    "idto_hip_allgather_slab", "idto_hip_gn_step_sharded", "idto_hip_gn_step_multi", "idto_hip_eval_partials_multi",
    "idto_hip_trace_enable", "idto_hip_trace_mark", "idto_hip_trace_dump",
]


LS_MAX_CANDIDATES = 64
LS_ROW = 12


def ls_alphas(linesearch_method: int, m: int):
    """the step lengths the linesearch tries, as the host loop forms them (0 kArmijo, 1 kBacktracking; idto_hip_ls_alphas)"""
    out = np.empty(int(m))
    _chk(lib().idto_hip_ls_alphas(int(linesearch_method), int(m), dptr(out)))
    return out


class HipError(RuntimeError):
    pass


class FactorizationFailed(HipError):
    """IDTO_HIP_FACTORIZATION_FAILED: H is not numerically positive definite (the reference's
    PentaDiagonalFactorizationStatus::kFailure, optimizer/penta_diagonal_solver.h:181-185)"""


class SolverTimeout(HipError):
    """IDTO_HIP_SOLVER_TIMEOUT: a multi-workgroup solver launch did not find its partner workgroups resident; the
    context has stepped down to a variant with fewer co-resident workgroups - repeat the call"""


FACTORIZATION_FAILED = 2
SOLVER_TIMEOUT = 3


def _chk(rc):
    if rc == FACTORIZATION_FAILED:
        raise FactorizationFailed(lib().idto_hip_last_error().decode())
    if rc == SOLVER_TIMEOUT:
        raise SolverTimeout(lib().idto_hip_last_error().decode())
    if rc != 0:
        raise HipError(f"idto_hip error {rc}: {lib().idto_hip_last_error().decode()}")


class HipPath:
    """One problem resident on one MI355X: the device side of TrajectoryOptimizer."""

    def __init__(self, model: Model, prob, params: SolverParameters, device: int = 0):
        """`prob`: one ProblemDefinition, or a list of them = a batch of problems of the same model and
        horizon advanced together (idto_hip_create_batch); see HipBatch"""
        L = lib()
        probs = list(prob) if isinstance(prob, (list, tuple)) else [prob]
        self.batch = len(probs)
        self.model, self.prob, self.params = model, probs[0], params
        self.nq, self.nv, self.N = model.nq, model.nv, probs[0].num_steps
        cm, self._k1 = model.to_c()
        carr = (CProblem * self.batch)()
        self._k2 = []
        for b, pr in enumerate(probs):
            cp, keep = pr.to_c()
            carr[b] = cp
            self._k2.append(keep)
        cc = params.contact_to_c()
        h = C.c_void_p()
        _chk(L.idto_hip_create_batch(C.byref(cm), carr, C.byref(cc), int(device), self.batch, C.byref(h)))
        self.h = h
        self.device = device
        from .problem import GRADIENTS
        gm = GRADIENTS[params.gradients_method]
        if gm:  # 1 central, 2 central4 (SolverParameters::gradients_method); others are refused by the library
            _chk(L.idto_hip_set_option(self.h, b"gradients_method", gm))

    def close(self):
        if getattr(self, "h", None):
            lib().idto_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs
    def set_q(self, q):
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
        assert q.size == (self.N + 1) * self.nq
        _chk(lib().idto_hip_set_q(self.h, dptr(q)))

    def set_q_batch(self, q):
        """q: [batch, N+1, nq]"""
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
        assert q.size == self.batch * (self.N + 1) * self.nq
        _chk(lib().idto_hip_set_q_batch(self.h, dptr(q)))

    def set_problem_batch(self, b: int, prob: ProblemDefinition):
        cp, keep = prob.to_c()
        _chk(lib().idto_hip_set_problem_batch(self.h, int(b), C.byref(cp)))

    def set_model_batch(self, b: int, model: Model = None, params: SolverParameters = None):
        """idto_hip_set_model_batch: problem b of the batch gets `model` (same topology; None: the batch's) and the contact
        parameters of `params` (None: the batch's)"""
        cm, keep = model.to_c() if model is not None else (None, None)
        cc = params.contact_to_c() if params is not None else None
        _chk(lib().idto_hip_set_model_batch(self.h, int(b), C.byref(cm) if cm is not None else None,
                                            C.byref(cc) if cc is not None else None))

    # ---- plants on the device (include/idto_hip.h idto_hip_forward_dynamics, idto_hip_plant_*)
    def forward_dynamics(self, x, tau_applied):
        """x: [batch, nq + nv], tau_applied: [batch, nv] -> (a [batch, nv], M [batch, nv, nv], bias [batch, nv])"""
        B, nq, nv = self.batch, self.nq, self.nv
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(B, nq + nv))
        tau = np.ascontiguousarray(np.asarray(tau_applied, dtype=np.float64).reshape(B, nv))
        a, M, bias = np.zeros((B, nv)), np.zeros((B, nv, nv)), np.zeros((B, nv))
        _chk(lib().idto_hip_forward_dynamics(self.h, dptr(x), dptr(tau), dptr(a), dptr(M), dptr(bias)))
        return a, np.ascontiguousarray(M.transpose(0, 2, 1)), bias   # (column-major blocks -> [row, col])

    def plant_begin(self, h: float, mode: int = PLANT_HOLD, Kp=None, Kd=None, feed_forward: bool = False,
                    record_capacity: int = 0, block_threads: int = 0):
        """idto_hip_plant_begin: B plants stepped with the substep h; PD+: Kp [nu, nq], Kd [nu, nv] on the stored plans"""
        prm = CPlantParams()
        prm.h, prm.mode, prm.feed_forward = float(h), int(mode), int(bool(feed_forward))
        prm.record_capacity, prm.block_threads = int(record_capacity), int(block_threads)
        keep = []
        for name, K in (("Kp", Kp), ("Kd", Kd)):
            if K is not None:
                K = np.ascontiguousarray(np.asarray(K, dtype=np.float64))
                keep.append(K)
                setattr(prm, name, dptr(K))
                setattr(prm, name.lower() + "_size", int(K.size))
        _chk(lib().idto_hip_plant_begin(self.h, C.byref(prm)))

    def plant_set_model(self, b: int, model: Model = None, params: SolverParameters = None):
        """plant b gets `model` (the context's topology; None: the context's) and the contact parameters of `params`"""
        cm, keep = model.to_c() if model is not None else (None, None)
        cc = params.contact_to_c() if params is not None else None
        _chk(lib().idto_hip_plant_set_model(self.h, int(b), C.byref(cm) if cm is not None else None,
                                            C.byref(cc) if cc is not None else None))

    def plant_set_state(self, times, x):
        times = np.ascontiguousarray(np.broadcast_to(np.asarray(times, dtype=np.float64), (self.batch,)))
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.batch, self.nq + self.nv))
        _chk(lib().idto_hip_plant_set_state(self.h, dptr(times), dptr(x)))

    def plant_get_state(self):
        """-> (times [batch], x [batch, nq + nv])"""
        times, x = np.zeros(self.batch), np.zeros((self.batch, self.nq + self.nv))
        _chk(lib().idto_hip_plant_get_state(self.h, dptr(times), dptr(x)))
        return times, x

    def plant_step(self, substeps: int, tau_hold=None, record_every: int = 0, status: bool = True):
        """idto_hip_plant_step: `substeps` substeps of every plant in one launch.  -> (recorded states [batch,
        substeps // record_every, nq + nv] or None, status [batch, 2] = (code, substeps completed) or None); with
        record_every = 0 and status = False the launch is enqueued only, nothing is waited for"""
        B = self.batch
        tau = None if tau_hold is None else np.ascontiguousarray(np.asarray(tau_hold, dtype=np.float64).reshape(B, self.nv))
        rec = np.zeros((B, int(substeps) // int(record_every), self.nq + self.nv)) if record_every else None
        st = np.zeros((B, 2), dtype=np.int32) if status else None
        _chk(lib().idto_hip_plant_step(self.h, int(substeps), dptr(tau) if tau is not None else None, int(record_every),
                                       dptr(rec) if rec is not None else None,
                                       st.ctypes.data_as(C.POINTER(C.c_int)) if st is not None else None))
        return rec, st

    # ---- the scene report (include/idto_hip.h idto_hip_scene_report)
    def scene_sizes(self):
        """-> (nbodies, npairs, doubles per body, doubles per pair)"""
        out = [C.c_int() for _ in range(4)]
        _chk(lib().idto_hip_scene_sizes(self.h, *[C.byref(o) for o in out]))
        return tuple(o.value for o in out)

    def scene_report(self, x, models: int = SCENE_MODELS_PROBLEMS, pair_rows: bool = False) -> SceneReport:
        """x: [batch, nstates, nq + nv] (a single problem: [nstates, nq + nv]) = [q; v] per state -> SceneReport.  models:
        SCENE_MODELS_PROBLEMS (problem b's physics) or SCENE_MODELS_PLANTS (plant b's); pair_rows: tau_pairs as well"""
        B, w = self.batch, self.nq + self.nv
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        squeeze = B == 1 and x.ndim == 2
        x = x.reshape(B, -1, w)
        S = x.shape[1]
        nb, npairs, bd, pdn = self.scene_sizes()
        bodies, pairs = np.zeros((B, S, nb, bd)), np.zeros((B, S, npairs, pdn))
        tau, rows = np.zeros((B, S, self.nv)), (np.zeros((B, S, npairs, self.nv)) if pair_rows else None)
        _chk(lib().idto_hip_scene_report(self.h, int(S), dptr(x), int(models), dptr(bodies), dptr(pairs), dptr(tau),
                                         dptr(rows) if rows is not None else None))
        if squeeze:   # (a single problem given as [nstates, nq + nv])
            bodies, pairs, tau, rows = bodies[0], pairs[0], tau[0], (rows[0] if rows is not None else None)
        return SceneReport(bodies, pairs, tau, rows)

    # ---- the plants' linearisation and the LQR gains about it (include/idto_hip.h idto_hip_plant_linearize, idto_hip_plant_tvlqr)
    def _lin_inputs(self, x, tau):
        B, w = self.batch, self.nq + self.nv
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        squeeze = B == 1 and x.ndim == 2
        x = x.reshape(B, -1, w)
        S = x.shape[1]
        tau = np.ascontiguousarray(np.asarray(tau, dtype=np.float64).reshape(B, S, self.nv))
        return x, tau, S, squeeze

    def lin_sizes(self, nstates: int, nu: int = 0):
        """idto_hip_lin_sizes -> (n = 2 nv, columns per state, the doubles of x_next, A, B, K, P for nstates states and nu controls)"""
        n, cols = C.c_int(), C.c_int()
        counts = [C.c_long() for _ in range(5)]
        _chk(lib().idto_hip_lin_sizes(self.h, int(nstates), int(nu), C.byref(n), C.byref(cols), *[C.byref(c) for c in counts]))
        return (n.value, cols.value) + tuple(c.value for c in counts)

    def plant_linearize(self, x, tau, h: float, substeps: int, eps: float = LIN_EPS_DEFAULT, models: int = SCENE_MODELS_PROBLEMS):
        """x: [batch, nstates, nq + nv] (a single problem: [nstates, nq + nv]), tau: [batch, nstates, nv] the held torques ->
        (x_next [batch, nstates, nq + nv], A [batch, nstates, n, n], B [batch, nstates, n, nv], status [batch, nstates, 2]) about
        the map of `substeps` substeps of h, in tangent coordinates, as [row, col]"""
        x, tau, S, squeeze = self._lin_inputs(x, tau)
        B, nv, n = self.batch, self.nv, 2 * self.nv
        xn, A, Bm = np.zeros((B, S, self.nq + nv)), np.zeros((B, S, n, n)), np.zeros((B, S, nv, n))
        st = np.zeros((B, S, 2), dtype=np.int32)
        _chk(lib().idto_hip_plant_linearize(self.h, int(S), dptr(x), dptr(tau), float(h), int(substeps), float(eps), int(models),
                                            dptr(xn), dptr(A), dptr(Bm), st.ctypes.data_as(C.POINTER(C.c_int))))
        A, Bm = np.ascontiguousarray(A.swapaxes(-1, -2)), np.ascontiguousarray(Bm.swapaxes(-1, -2))   # (column-major -> [row, col])
        return (xn[0], A[0], Bm[0], st[0]) if squeeze else (xn, A, Bm, st)

    def plant_tvlqr(self, x, tau, h: float, substeps: int, actuated, Q, R, Qf, eps: float = LIN_EPS_DEFAULT,
                    models: int = SCENE_MODELS_PROBLEMS) -> Tvlqr:
        """plant_linearize's inputs, the actuated velocity indices [nu] and the weights Q, Qf [n, n], R [nu, nu] in tangent
        coordinates -> Tvlqr"""
        x, tau, S, squeeze = self._lin_inputs(x, tau)
        B, nv, n = self.batch, self.nv, 2 * self.nv
        act = np.ascontiguousarray(np.asarray(actuated, dtype=np.int32).ravel())
        nu = act.size
        Q, Qf = (np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(n, n).T) for M in (Q, Qf))
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(nu, nu).T)
        xn, A, Bm = np.zeros((B, S, self.nq + nv)), np.zeros((B, S, n, n)), np.zeros((B, S, nv, n))
        st, lst = np.zeros((B, S, 2), dtype=np.int32), np.zeros(B, dtype=np.int32)
        K, P = np.zeros((B, S, n, nu)), np.zeros((B, S + 1, n, n))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _chk(lib().idto_hip_plant_tvlqr(self.h, int(S), dptr(x), dptr(tau), float(h), int(substeps), float(eps), int(models), int(nu),
                                        ip(act), dptr(Q), dptr(R), dptr(Qf), dptr(xn), dptr(A), dptr(Bm), ip(st), dptr(K), dptr(P), ip(lst)))
        A, Bm, K, P = (np.ascontiguousarray(M.swapaxes(-1, -2)) for M in (A, Bm, K, P))
        if squeeze:
            xn, A, Bm, st, K = xn[0], A[0], Bm[0], st[0], K[0]
        return Tvlqr(xn, A, Bm, st, K, P, lst)

    # ---- the plants under the time-varying LQR law (include/idto_hip.h idto_hip_plant_track, idto_hip_plant_tvlqr_track)
    def _track_inputs(self, x_nom, tau_nom, x0):
        B, w = self.batch, self.nq + self.nv
        x_nom = np.ascontiguousarray(np.asarray(x_nom, dtype=np.float64))
        squeeze = B == 1 and x_nom.ndim == 2
        x_nom = x_nom.reshape(B, -1, w)
        S = x_nom.shape[1] - 1
        tau_nom = np.ascontiguousarray(np.asarray(tau_nom, dtype=np.float64).reshape(B, S, self.nv))
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(B, -1, w))
        return x_nom, tau_nom, x0, S, x0.shape[1], squeeze

    def _track_outputs(self, S, R, nu):
        B, n = self.batch, 2 * self.nv
        return np.zeros((B, R, S, self.nq + self.nv)), np.zeros((B, R, S, nu)), np.zeros((B, R, S + 1, n)), np.zeros((B, R, 2), dtype=np.int32)

    def plant_track(self, x_nom, tau_nom, K, x0, h: float, substeps: int, actuated, models: int = SCENE_MODELS_PROBLEMS,
                    max_launch_substeps: int = 0) -> Track:
        """x_nom: [batch, S + 1, nq + nv] (a single problem: [S + 1, nq + nv]), tau_nom: [batch, S, nv], K: [batch, S, nu, n] as
        [row, col], x0: [batch, nrollouts, nq + nv] -> Track: the rollouts of S steps of `substeps` substeps of h under
        u_t = tau_nom_t[actuated] - K_t [q (-) q*_t; v - v*_t], held over a step"""
        x_nom, tau_nom, x0, S, R, squeeze = self._track_inputs(x_nom, tau_nom, x0)
        B, n = self.batch, 2 * self.nv
        act = np.ascontiguousarray(np.asarray(actuated, dtype=np.int32).ravel())
        nu = act.size
        K = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(B, S, nu, n).swapaxes(-1, -2))   # ([row, col] -> column-major)
        x, u, dx, st = self._track_outputs(S, R, nu)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _chk(lib().idto_hip_plant_track(self.h, int(S), int(substeps), float(h), int(models), int(nu), ip(act), dptr(x_nom), dptr(tau_nom),
                                        dptr(K), int(R), dptr(x0), int(max_launch_substeps), dptr(x), dptr(u), dptr(dx), ip(st)))
        return Track(x[0], u[0], dx[0], st[0]) if squeeze else Track(x, u, dx, st)

    def plant_tvlqr_track(self, x, tau, x0, h: float, substeps: int, actuated, Q, R, Qf, eps: float = LIN_EPS_DEFAULT,
                          models: int = SCENE_MODELS_PROBLEMS, max_launch_substeps: int = 0) -> Track:
        """plant_tvlqr about the first S of x's S + 1 states, and behind it on the device plant_track about x and tau with the
        gains where the recursion left them: one wait -> Track with .tvlqr"""
        x, tau, x0, S, nroll, squeeze = self._track_inputs(x, tau, x0)
        B, nv, n = self.batch, self.nv, 2 * self.nv
        act = np.ascontiguousarray(np.asarray(actuated, dtype=np.int32).ravel())
        nu = act.size
        Q, Qf = (np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(n, n).T) for M in (Q, Qf))
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(nu, nu).T)
        xn, A, Bm = np.zeros((B, S, self.nq + nv)), np.zeros((B, S, n, n)), np.zeros((B, S, nv, n))
        st, lst = np.zeros((B, S, 2), dtype=np.int32), np.zeros(B, dtype=np.int32)
        K, P = np.zeros((B, S, n, nu)), np.zeros((B, S + 1, n, n))
        xo, u, dx, tst = self._track_outputs(S, nroll, nu)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _chk(lib().idto_hip_plant_tvlqr_track(self.h, int(S), dptr(x), dptr(tau), float(h), int(substeps), float(eps), int(models), int(nu),
                                              ip(act), dptr(Q), dptr(R), dptr(Qf), int(nroll), dptr(x0), int(max_launch_substeps), dptr(xn),
                                              dptr(A), dptr(Bm), ip(st), dptr(K), dptr(P), ip(lst), dptr(xo), dptr(u), dptr(dx), ip(tst)))
        A, Bm, K, P = (np.ascontiguousarray(M.swapaxes(-1, -2)) for M in (A, Bm, K, P))
        if squeeze:
            xn, A, Bm, st, K = xn[0], A[0], Bm[0], st[0], K[0]
            xo, u, dx, tst = xo[0], u[0], dx[0], tst[0]
        return Track(xo, u, dx, tst, Tvlqr(xn, A, Bm, st, K, P, lst))

    def solver_status_batch(self):
        out = (C.c_int * self.batch)()
        _chk(lib().idto_hip_solver_status_batch(self.h, out))
        return [bool(x) for x in out]

    def set_q_device(self, ptr: int):
        _chk(lib().idto_hip_set_q_device(self.h, C.c_void_p(ptr)))

    def set_problem(self, prob: ProblemDefinition):
        cp, self._k2 = prob.to_c()
        self.prob = prob
        _chk(lib().idto_hip_set_problem(self.h, C.byref(cp)))

    def set_stream(self, stream_ptr: int):
        _chk(lib().idto_hip_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- multi-GPU: RCCL communicator inside the library (include/idto_hip.h)
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """collective over the `world` ranks (ncclCommInitRank); sets this context's k-range shard"""
        _chk(lib().idto_hip_comm_init(self.h, unique_id, int(rank), int(world)))

    def comm_destroy(self):
        _chk(lib().idto_hip_comm_destroy(self.h))

    def allgather_slab(self):
        _chk(lib().idto_hip_allgather_slab(self.h))

    def gn_step_sharded(self):
        _chk(lib().idto_hip_gn_step_sharded(self.h))

    # ---- trust-region bookkeeping on the device (include/idto_hip.h idto_hip_tr_*)
    def tr_prepare(self, scaling_method: int = -1, with_lambda: bool = False):
        out = np.zeros(9)
        _chk(lib().idto_hip_tr_prepare(self.h, int(scaling_method), int(with_lambda), dptr(out)))
        return out

    def tr_trial(self, a: float, b: float, scaling: bool, normalize_quaternions: bool = False, with_lambda: bool = False,
                 speculate_scaling_method: int = -2):
        out = np.zeros(4)
        _chk(lib().idto_hip_tr_trial(self.h, float(a), float(b), int(scaling), int(normalize_quaternions),
                                     int(with_lambda), int(speculate_scaling_method), dptr(out)))
        return out

    def tr_reject(self):
        _chk(lib().idto_hip_tr_reject(self.h))

    def tr_set_scale_memory(self, D_prev=None):
        """the adaptive scalings' previous D (None: ones, a fresh state)"""
        if D_prev is None:
            _chk(lib().idto_hip_tr_set_scale_memory(self.h, None))
        else:
            _chk(lib().idto_hip_tr_set_scale_memory(self.h, dptr(np.ascontiguousarray(D_prev, dtype=np.float64))))

    def tr_solve(self, iterations: int, scaling_method: int, scaling: bool, normalize_quaternions: bool, Delta0: float,
                 Delta_max: float, eta: float = 0.0, constrained_dofs=()):
        """the whole trust-region loop on the device (idto_hip_tr_solve): (rows [iterations, 17], final Delta)"""
        rows = np.zeros((int(iterations), 17))
        delta = C.c_double(0.0)
        dofs = np.ascontiguousarray(np.asarray(constrained_dofs, dtype=np.int32))
        self.last_tr_rows = rows   # (filled even when the call reports a failed factorisation)
        _chk(lib().idto_hip_tr_solve(self.h, int(iterations), int(scaling_method), int(scaling), int(normalize_quaternions),
                                     float(Delta0), float(Delta_max), float(eta),
                                     dofs.ctypes.data_as(C.POINTER(C.c_int)) if dofs.size else None, int(dofs.size),
                                     dptr(rows), C.byref(delta)))
        return rows, delta.value

    def tr_solve_batch(self, iterations: int, scaling_method: int, scaling: bool, normalize_quaternions: bool, Delta0,
                       Delta_max: float, eta: float = 0.0):
        """idto_hip_tr_solve_batch: (rows [batch, iterations, 17], final Delta [batch])"""
        B = self.batch
        rows = np.zeros((B, int(iterations), 17))
        d0 = np.ascontiguousarray(np.broadcast_to(np.asarray(Delta0, dtype=np.float64), (B,)))
        delta = np.zeros(B)
        self.last_tr_rows = rows
        _chk(lib().idto_hip_tr_solve_batch(self.h, int(iterations), int(scaling_method), int(scaling), int(normalize_quaternions),
                                           dptr(d0), float(Delta_max), float(eta), dptr(rows), dptr(delta)))
        return rows, delta

    def tr_solve_batch_constrained(self, iterations: int, scaling_method: int, scaling: bool, normalize_quaternions: bool, Delta0,
                                   Delta_max: float, constrained_dofs, eta: float = 0.0):
        """idto_hip_tr_solve_batch_constrained: the batch's loop with the equality constraints enforced on `constrained_dofs`"""
        B = self.batch
        rows = np.zeros((B, int(iterations), 17))
        d0 = np.ascontiguousarray(np.broadcast_to(np.asarray(Delta0, dtype=np.float64), (B,)))
        delta = np.zeros(B)
        dofs = np.ascontiguousarray(np.asarray(constrained_dofs, dtype=np.int32))
        self.last_tr_rows = rows
        _chk(lib().idto_hip_tr_solve_batch_constrained(self.h, int(iterations), int(scaling_method), int(scaling),
                                                       int(normalize_quaternions), dptr(d0), float(Delta_max), float(eta),
                                                       dofs.ctypes.data_as(C.POINTER(C.c_int)), len(dofs), dptr(rows), dptr(delta)))
        return rows, delta

    def _traj_buffers(self, T: int):
        N, nq, nv = self.N, self.nq, self.nv
        return dict(q=np.zeros((T, N + 1, nq)), v=np.zeros((T, N + 1, nv)), tau=np.zeros((T, N, nv)),
                    dq=np.zeros((T, N + 1, nq)), w=np.zeros((T, N + 1, nq)))

    def tr_solve_fetch(self, iterations: int, scaling_method: int, scaling: bool, normalize_quaternions: bool, Delta0: float,
                       Delta_max: float, eta: float = 0.0, constrained_dofs=()):
        """idto_hip_tr_solve_fetch: (rows [iterations, 17], final Delta, dict of q, v, tau, dq, w)"""
        rows = np.zeros((int(iterations), 17))
        delta = C.c_double(0.0)
        dofs = np.ascontiguousarray(np.asarray(constrained_dofs, dtype=np.int32))
        out = {k: a[0] for k, a in self._traj_buffers(1).items()}
        self.last_tr_rows = rows
        _chk(lib().idto_hip_tr_solve_fetch(self.h, int(iterations), int(scaling_method), int(scaling), int(normalize_quaternions),
                                           float(Delta0), float(Delta_max), float(eta),
                                           dofs.ctypes.data_as(C.POINTER(C.c_int)) if dofs.size else None, int(dofs.size),
                                           dptr(rows), C.byref(delta), *[dptr(out[k]) for k in ("q", "v", "tau", "dq", "w")]))
        return rows, delta.value, out

    def tr_solve_batch_fetch(self, iterations: int, scaling_method: int, scaling: bool, normalize_quaternions: bool, Delta0,
                             Delta_max: float, eta: float = 0.0, constrained_dofs=(), only_best: bool = False,
                             check: bool = True):
        """idto_hip_tr_solve_batch_fetch: the batch's loop, every problem's rows, radius, cost, status and trajectories
        (only_best: the best problem's trajectories alone, leading dimension 1) and the index of the best problem, under
        ONE wait.  Returns a dict: rows [B, iterations, 17], delta [B], q, v, tau, dq, w, final_cost [B], status [B], best,
        rc (the call's return code; check=False hands IDTO_HIP_FACTORIZATION_FAILED back there instead of raising)."""
        B = self.batch
        rows = np.zeros((B, int(iterations), 17))
        d0 = np.ascontiguousarray(np.broadcast_to(np.asarray(Delta0, dtype=np.float64), (B,)))
        delta = np.zeros(B)
        dofs = np.ascontiguousarray(np.asarray(constrained_dofs, dtype=np.int32))
        out = self._traj_buffers(1 if only_best else B)
        final_cost = np.zeros(B)
        status = np.zeros(B, dtype=np.int32)
        best = C.c_int(-2)
        self.last_tr_rows = rows
        rc = lib().idto_hip_tr_solve_batch_fetch(
            self.h, int(iterations), int(scaling_method), int(scaling), int(normalize_quaternions), dptr(d0), float(Delta_max),
            float(eta), dofs.ctypes.data_as(C.POINTER(C.c_int)) if dofs.size else None, int(dofs.size), dptr(rows), dptr(delta),
            int(only_best), *[dptr(out[k]) for k in ("q", "v", "tau", "dq", "w")], dptr(final_cost),
            status.ctypes.data_as(C.POINTER(C.c_int)), C.byref(best))
        if check or rc not in (0, FACTORIZATION_FAILED):
            _chk(rc)
        out.update(rows=rows, delta=delta, final_cost=final_cost, status=status, best=best.value, rc=rc)
        return out

    # ---- B model-predictive controllers on a batch context (include/idto_hip.h idto_hip_mpc_batch_*)
    def mpc_plan_len(self):
        return 1 + 2 * (self.N + 1) * (self.nq + self.nv + self._mpc_nu)

    def mpc_split_plan(self, plan):
        """one problem's plan [IDTO_MPC_PLAN_LEN] as a dict: start_time, and y / m [N + 1, dim] of the q, v, u splines"""
        n, out, o = self.N + 1, dict(start_time=float(plan[0])), 1
        for name, dim in (("q", self.nq), ("v", self.nv), ("u", self._mpc_nu)):
            out["y_" + name] = plan[o:o + n * dim].reshape(n, dim)
            out["m_" + name] = plan[o + n * dim:o + 2 * n * dim].reshape(n, dim)
            o += 2 * n * dim
        return out

    def mpc_batch_begin(self, selector, actuated_dofs):
        sel = np.ascontiguousarray(np.asarray(selector, dtype=np.int32))
        act = np.ascontiguousarray(np.asarray(actuated_dofs, dtype=np.int32))
        assert sel.size == self.nq
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _chk(lib().idto_hip_mpc_batch_begin(self.h, ip(sel), ip(act), int(act.size)))
        self._mpc_nu = int(act.size)

    def mpc_batch_store(self, q, v, tau, start_times):
        """the plans of B solutions from the host ([B, N+1, nq], [B, N+1, nv], [B, N, nv], [B]): plans [B, plan_len]"""
        B, N = self.batch, self.N
        q, v, tau, t0 = (np.ascontiguousarray(np.asarray(x, dtype=np.float64)) for x in (q, v, tau, start_times))
        assert q.size == B * (N + 1) * self.nq and v.size == B * (N + 1) * self.nv and tau.size == B * N * self.nv and t0.size == B
        plans = np.zeros((B, self.mpc_plan_len()))
        _chk(lib().idto_hip_mpc_batch_store(self.h, dptr(q), dptr(v), dptr(tau), dptr(t0), dptr(plans)))
        return plans

    def mpc_batch_shift(self, times, x0):
        """the front half of a tick: (guess [B, N+1, nq], q_nom [B, N+1, nq]) as the device left them"""
        B = self.batch
        times, x0 = (np.ascontiguousarray(np.asarray(x, dtype=np.float64)) for x in (times, x0))
        assert times.size == B and x0.size == B * (self.nq + self.nv)
        guess, q_nom = np.zeros((B, self.N + 1, self.nq)), np.zeros((B, self.N + 1, self.nq))
        _chk(lib().idto_hip_mpc_batch_shift(self.h, dptr(times), dptr(x0), dptr(guess), dptr(q_nom)))
        return guess, q_nom

    def _mpc_tick(self, substeps, times, x0, iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta,
                  constrained_dofs):
        B, N, nq, nv = self.batch, self.N, self.nq, self.nv
        out = dict(rows=np.zeros((B, int(iterations), 17)), Delta=np.zeros(B), q=np.zeros((B, N + 1, nq)), v=np.zeros((B, N + 1, nv)),
                   tau=np.zeros((B, N, nv)), final_cost=np.zeros(B), status=np.zeros(B, dtype=np.int32), guess=np.zeros((B, N + 1, nq)),
                   plans=np.zeros((B, self.mpc_plan_len())))
        d0 = np.ascontiguousarray(np.broadcast_to(np.asarray(Delta0, dtype=np.float64), (B,)))
        dofs = np.ascontiguousarray(np.asarray(constrained_dofs, dtype=np.int32))
        best = C.c_int(-1)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        tail = [int(iterations), int(scaling_method), int(scaling), int(normalize_quaternions), dptr(d0), float(Delta_max), float(eta),
                ip(dofs) if dofs.size else None, int(dofs.size), dptr(out["rows"]), dptr(out["Delta"]), dptr(out["q"]), dptr(out["v"]),
                dptr(out["tau"]), dptr(out["final_cost"]), ip(out["status"]), C.byref(best), dptr(out["guess"]), dptr(out["plans"])]
        if substeps is None:
            times, x0 = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (times, x0))
            assert times.size == B and x0.size == B * (nq + nv)
            rc = lib().idto_hip_mpc_batch_replan(self.h, dptr(times), dptr(x0), *tail)
        else:
            out["x_after"], out["plant_status"] = np.zeros((B, nq + nv)), np.zeros((B, 2), dtype=np.int32)
            rc = lib().idto_hip_mpc_batch_tick_plants(self.h, int(substeps), *tail, dptr(out["x_after"]), ip(out["plant_status"]))
        if rc != FACTORIZATION_FAILED:   # (a controller whose factorisation failed keeps its plan: its status says so)
            _chk(rc)
        out["best"] = best.value
        return out

    def mpc_batch_replan(self, times, x0, iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta=0.0,
                         constrained_dofs=()):
        """idto_hip_mpc_batch_replan: one tick of the B controllers from times [B] and x0 [B, nq + nv]; a dict of its outputs"""
        return self._mpc_tick(None, times, x0, iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta,
                              constrained_dofs)

    def mpc_batch_tick_plants(self, substeps, iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta=0.0,
                              constrained_dofs=()):
        """idto_hip_mpc_batch_tick_plants: `substeps` PD+ substeps of the plants, then the re-plan from their states, under one
        wait; the re-plan's outputs and x_after [B, nq + nv]"""
        return self._mpc_tick(int(substeps), None, None, iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max,
                              eta, constrained_dofs)

    def tr_set_convergence(self, tolerances=None):
        """[rel_cost, abs_cost, rel_gradient_along_dq, abs_gradient_along_dq, rel_state, abs_state] or None (no checks)"""
        if tolerances is None:
            _chk(lib().idto_hip_tr_set_convergence(self.h, None))
        else:
            t = np.ascontiguousarray(np.asarray(tolerances, dtype=np.float64))
            assert t.size == 6
            _chk(lib().idto_hip_tr_set_convergence(self.h, dptr(t)))

    def set_unactuated_dofs(self, dofs):
        dofs = np.ascontiguousarray(np.asarray(dofs, dtype=np.int32))
        _chk(lib().idto_hip_set_unactuated_dofs(self.h, dofs.ctypes.data_as(C.POINTER(C.c_int)), int(dofs.size)))

    def tr_accept(self):
        _chk(lib().idto_hip_tr_accept(self.h))

    def set_shard(self, k_begin: int, k_end: int):
        _chk(lib().idto_hip_set_shard(self.h, int(k_begin), int(k_end)))

    # ---- path pieces (asynchronous on the context's stream)
    def eval_tau(self):
        _chk(lib().idto_hip_eval_tau(self.h))

    def eval_tau_partials(self):
        """eval_tau for a q whose partials come next: one finite-difference launch for both (the next eval_partials is done)"""
        _chk(lib().idto_hip_eval_tau_partials(self.h))

    def constraint_schur(self, dofs):
        """S = J H^-1 J^T (n_eq x n_eq) and J H^-1 g for the constraint tau_t[dofs] = 0 (after grad_hess)"""
        dofs = np.ascontiguousarray(np.asarray(dofs, dtype=np.int32))
        neq = dofs.size * self.N
        S, Jy = np.empty((neq, neq), order="F"), np.empty(neq)
        _chk(lib().idto_hip_constraint_schur(self.h, dofs.ctypes.data_as(C.POINTER(C.c_int)), int(dofs.size),
                                             S.ctypes.data_as(C.POINTER(C.c_double)), dptr(Jy)))
        return S, Jy

    def constraint_solve(self, dofs, h):
        """multipliers entirely on the device: returns (ok, lambda, H^-1 (g + J^T lambda), J^T lambda);
        ok False: S numerically singular, use constraint_schur + a pivoted host solve"""
        dofs = np.ascontiguousarray(np.asarray(dofs, dtype=np.int32))
        h = np.ascontiguousarray(np.asarray(h, dtype=np.float64))
        n = (self.N + 1) * self.nq
        _chk(lib().idto_hip_constraint_schur_begin(self.h, dofs.ctypes.data_as(C.POINTER(C.c_int)), int(dofs.size)))
        lam, step, jtl = np.empty(h.size), np.empty(n), np.empty(n)
        rc = lib().idto_hip_constraint_solve(self.h, dptr(h), dptr(lam), dptr(step), dptr(jtl))
        if rc not in (0, 1):
            _chk(rc)
        return rc == 0, lam, step, jtl

    def constraint_step(self, lam):
        """H^-1 (g + J^T lambda) and J^T lambda, from the factors kept by constraint_schur"""
        lam = np.ascontiguousarray(np.asarray(lam, dtype=np.float64))
        n = (self.N + 1) * self.nq
        step, jtl = np.empty(n), np.empty(n)
        _chk(lib().idto_hip_constraint_step(self.h, dptr(lam), dptr(step), dptr(jtl)))
        return step, jtl

    def trial_cost(self, q):
        """upload q, evaluate tau and the cost, return (tau (N, nv), cost) with one synchronisation"""
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
        assert q.size == (self.N + 1) * self.nq
        tau = np.empty((self.N, self.nv))
        cost = C.c_double()
        _chk(lib().idto_hip_trial_cost(self.h, dptr(q), dptr(tau), C.byref(cost)))
        return tau, cost.value

    def costs_along(self, alphas, normalize_quaternions: bool = False):
        """L(q + alpha dq) for up to LS_MAX_CANDIDATES step lengths along the last solve's step dq, one launch set and one
        wait (idto_hip_costs_along); the resident iterate is not disturbed"""
        alphas = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).ravel())
        costs = np.empty(alphas.size)
        _chk(lib().idto_hip_costs_along(self.h, dptr(alphas), int(alphas.size), int(bool(normalize_quaternions)), dptr(costs)))
        return costs

    def ls_solve(self, iterations, linesearch_method=0, max_linesearch_iterations=50, normalize_quaternions=False,
                 fetch=True):
        """the linesearch method's loop on the device, one wait (idto_hip_ls_solve_fetch): returns a dict with rows
        [iterations, LS_ROW] and - fetch - the final iterate's q, v, tau"""
        rows = np.zeros((int(iterations), LS_ROW))
        args = (self.h, int(iterations), int(linesearch_method), int(max_linesearch_iterations), int(bool(normalize_quaternions)),
                dptr(rows))
        if not fetch:
            _chk(lib().idto_hip_ls_solve(*args))
            return dict(rows=rows)
        out = dict(rows=rows, q=np.zeros((self.N + 1, self.nq)), v=np.zeros((self.N + 1, self.nv)), tau=np.zeros((self.N, self.nv)))
        _chk(lib().idto_hip_ls_solve_fetch(*args, dptr(out["q"]), dptr(out["v"]), dptr(out["tau"])))
        return out

    def costs_along_batch(self, alphas, normalize_quaternions: bool = False):
        """(a batch context) L_b(q_b + alpha dq_b) for every problem b at the same step lengths, one launch set and one wait
        (idto_hip_costs_along_batch): costs [B, m]; nothing resident of any problem is disturbed"""
        alphas = np.ascontiguousarray(np.asarray(alphas, dtype=np.float64).ravel())
        costs = np.empty((self.batch, alphas.size))
        _chk(lib().idto_hip_costs_along_batch(self.h, dptr(alphas), int(alphas.size), int(bool(normalize_quaternions)), dptr(costs)))
        return costs

    def ls_solve_batch(self, iterations, linesearch_method=0, max_linesearch_iterations=50, normalize_quaternions=False,
                       check: bool = True):
        """(a batch context) the linesearch method's loop of every problem side by side, one wait
        (idto_hip_ls_solve_batch_fetch).  Returns a dict: rows [B, iterations, LS_ROW], q, v, tau [B, ...], final_cost [B],
        status [B] (the OR of each problem's row flags), rc (check=False hands IDTO_HIP_FACTORIZATION_FAILED back there
        instead of raising)."""
        B, N = self.batch, self.N
        out = dict(rows=np.zeros((B, int(iterations), LS_ROW)), q=np.zeros((B, N + 1, self.nq)), v=np.zeros((B, N + 1, self.nv)),
                   tau=np.zeros((B, N, self.nv)), final_cost=np.zeros(B), status=np.zeros(B, dtype=np.int32))
        rc = lib().idto_hip_ls_solve_batch_fetch(
            self.h, int(iterations), int(linesearch_method), int(max_linesearch_iterations), int(bool(normalize_quaternions)),
            dptr(out["rows"]), dptr(out["q"]), dptr(out["v"]), dptr(out["tau"]), dptr(out["final_cost"]),
            out["status"].ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc not in (0, FACTORIZATION_FAILED):
            _chk(rc)
        out["rc"] = rc
        return out

    def eval_partials(self):
        _chk(lib().idto_hip_eval_partials(self.h))

    def grad_hess(self):
        _chk(lib().idto_hip_grad_hess(self.h))

    def factor_solve(self, rhs_ptr: int | None = None, nrhs: int = 1, x_ptr: int | None = None):
        _chk(lib().idto_hip_factor_solve(self.h, C.c_void_p(rhs_ptr) if rhs_ptr else None, int(nrhs),
                                         C.c_void_p(x_ptr) if x_ptr else None))

    def solve_host(self, rhs):
        """H X = rhs for host right-hand sides [nrhs, (N+1)*nq]"""
        rhs = np.ascontiguousarray(np.atleast_2d(np.asarray(rhs, dtype=np.float64)))
        x = np.zeros_like(rhs)
        _chk(lib().idto_hip_solve_host(self.h, dptr(rhs), rhs.shape[0], dptr(x)))
        return x

    def solve_dense_ldlt(self, rhs):
        """H x = rhs by a dense LDL^T of MakeDense() (SolverParameters::linear_solver = kDenseLdlt, TO.cc:2088-2093)"""
        rhs = np.ascontiguousarray(np.asarray(rhs, dtype=np.float64).ravel())
        x = np.zeros_like(rhs)
        _chk(lib().idto_hip_solve_dense_ldlt(self.h, dptr(rhs), dptr(x)))
        return x

    def set_option(self, name: str, value: int):
        _chk(lib().idto_hip_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        _chk(lib().idto_hip_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def gn_step(self):
        _chk(lib().idto_hip_gn_step(self.h))

    def sync(self):
        _chk(lib().idto_hip_sync(self.h))

    def solver_status(self):
        """(failed, failed_rows_total) of the most recent factorisation; synchronises"""
        f, n = C.c_int(), C.c_int()
        _chk(lib().idto_hip_solver_status(self.h, C.byref(f), C.byref(n)))
        return bool(f.value), n.value

    # ---- timing (HIP events on the context's stream)
    def timing_enable(self, on=True):
        """True / 1: time every launch; s > 1: every s-th launch; False / 0: off"""
        _chk(lib().idto_hip_timing_enable(self.h, int(on)))

    def timing_reset(self):
        _chk(lib().idto_hip_timing_reset(self.h))

    def timing_get(self, which: int):
        ms, n = C.c_double(), C.c_int()
        _chk(lib().idto_hip_timing_get(self.h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- outputs
    def array_size(self, name):
        return lib().idto_hip_array_size(self.h, ARR[name])

    def device_ptr(self, name):
        return lib().idto_hip_device_ptr(self.h, ARR[name])

    @property
    def slab_stride(self):
        return lib().idto_hip_slab_stride(self.h)

    def prefetch(self, name):
        """enqueue the copy of a contiguous array now; the next get(name) waits only for it"""
        _chk(lib().idto_hip_prefetch(self.h, ARR[name]))

    def get(self, name, problem=None):
        """array `name` of problem 0 (through the prefetch staging if one is pending), or of problem
        `problem` of a batch"""
        out = np.zeros(self.array_size(name))
        if problem is None:
            _chk(lib().idto_hip_get(self.h, ARR[name], dptr(out)))
        else:
            _chk(lib().idto_hip_get_batch(self.h, ARR[name], int(problem), dptr(out)))
        N, nq, nv = self.N, self.nq, self.nv
        if name == "q":
            return out.reshape(N + 1, nq)
        if name == "v":
            return out.reshape(N + 1, nv)
        if name in ("a", "tau"):
            return out.reshape(N, nv)
        if name == "nplus":
            return out.reshape(N + 1, nq, nv).transpose(0, 2, 1).copy()
        if name.startswith("dtau"):
            return out.reshape(N, nq, nv).transpose(0, 2, 1).copy()  # [t, row(nv), col(nq)]
        if name.startswith("H_"):
            return out.reshape(N + 1, nq, nq).transpose(0, 2, 1).copy()  # [blk, row, col]
        if name == "cost":
            return float(out[0])
        return out


def rccl_info():
    """(path of the librccl this process resolved, its version code)"""
    buf, ver = C.create_string_buffer(1024), C.c_int(0)
    lib().idto_hip_rccl_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    _chk(lib().idto_hip_rccl_info(buf, 1024, C.byref(ver)))
    return buf.value.decode(), int(ver.value)


def comm_unique_id() -> bytes:
    """rank 0: the 128-byte id every rank passes to HipPath.comm_init"""
    buf = C.create_string_buffer(128)
    _chk(lib().idto_hip_comm_unique_id(buf, 128))
    return buf.raw


def comm_init_all(paths):
    """one process, one HipPath per device: ncclCommInitAll"""
    arr = (C.c_void_p * len(paths))(*[p.h for p in paths])
    _chk(lib().idto_hip_comm_init_all(arr, len(paths)))


def gn_step_multi(paths):
    arr = (C.c_void_p * len(paths))(*[p.h for p in paths])
    _chk(lib().idto_hip_gn_step_multi(arr, len(paths)))


def math_probe(x, device=0):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    outs = [np.zeros_like(x) for _ in range(6)]
    _chk(lib().idto_hip_math_probe(device, dptr(x), x.size, *[dptr(o) for o in outs]))
    return dict(zip(("sqrt", "recip", "sin", "cos", "exp", "log"), outs))
