"""Model-predictive-control shell around the optimizer: the caller of the hot path in the
reference's closed-loop examples (reference examples/mpc_controller.{h,cc}): at every replan
the last solution, stored as cubic splines, is time-shifted into the initial guess, the nominal
trajectory is shifted for the DoFs marked `q_nom_relative_to_q_init`, the initial condition is
reset and `SolveFromWarmStart` runs `mpc_iters` iterations from the previous trust-region
radius.  Drake's LeafSystem plumbing (ports, abstract state) is replaced by plain method calls.

`BatchDeviceModelPredictiveController` is B such controllers of one model whose tick is ONE device pass, waited for once
(idto::examples::mpc::BatchModelPredictiveController; idto_mpc_batch_* of include/idto_opt.h).

Two implementations of the same shell:
  * `DeviceModelPredictiveController` - the product: the C++ class of include/idto/examples/mpc_controller.h inside
    libidto_opt.so through the C-ABI (idto_mpc_* of include/idto_opt.h);
  * `ModelPredictiveController` / `Interpolator` - the same logic in numpy / scipy over the Python optimizer binding; the
    tests hold the C++ shell against it (scipy's not-a-knot CubicSpline is the independent spline).
Both clamp the query time to the stored trajectory's time range, as Drake's PiecewisePolynomial::value does.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.interpolate import CubicSpline


@dataclass
class StoredTrajectory:
    """reference examples/mpc_controller.h:43-55"""
    start_time: float = -1.0
    q: CubicSpline = None   # generalized positions
    v: CubicSpline = None   # generalized velocities
    u: CubicSpline = None   # control torques (actuated DoFs)


class ModelPredictiveController:
    """reference examples/mpc_controller.cc:13-138.  `optimizer` is an
    idto_amd.optimizer.TrajectoryOptimizer (or anything with the same methods)."""

    def __init__(self, optimizer, warm_start_solution, actuated=None):
        self.opt = optimizer
        self.time_step = optimizer.time_step()
        self.num_steps = optimizer.num_steps() + 1          # knots, as in the reference (:16)
        prob = optimizer.prob()
        self.nq, self.nv = len(prob.q_init), len(prob.v_init)
        act = np.ones(self.nv, bool) if actuated is None else np.asarray(actuated, bool)
        self.actuated = act if act.any() else np.ones(self.nv, bool)   # B = I without actuators
        self.warm_start = optimizer.CreateWarmStart(np.asarray(warm_start_solution.q))
        self.stored = StoredTrajectory()
        self.store_optimizer_solution(warm_start_solution, 0.0, self.stored)
        self.last_stats = None

    # ModelPredictiveController::UpdateAbstractState (:43-85)
    def update(self, t: float, q0, v0) -> StoredTrajectory:
        from .optimizer import TrajectoryOptimizerSolution, TrajectoryOptimizerStats
        q0, v0 = np.asarray(q0, float), np.asarray(v0, float)
        params, prob = self.opt.params(), self.opt.prob()
        sel = np.asarray(params.q_nom_relative_to_q_init, float)
        if sel.size != self.nq:
            raise ValueError("q_nom_relative_to_q_init must have one entry per position (mpc_controller.cc:45)")
        q_guess = self.update_initial_guess(self.stored, t)
        q_guess[0] = q0                      # the guess must be consistent with the initial condition
        self._last_guess = np.array(q_guess)
        self.warm_start.set_q(q_guess)
        q_nom = np.asarray(prob.q_nom, float)
        q_nom_new = q_nom + sel * (q0 - q_nom[0])           # (:62-69)
        self.opt.UpdateNominalTrajectory(q_nom_new, np.asarray(prob.v_nom, float))
        self.opt.ResetInitialConditions(q0, v0)
        sol, stats = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
        self.opt.SolveFromWarmStart(self.warm_start, sol, stats)
        self.last_stats = stats
        self.store_optimizer_solution(sol, t, self.stored)
        return self.stored

    # UpdateInitialGuess (:87-97)
    def update_initial_guess(self, stored: StoredTrajectory, current_time: float):
        start = current_time - stored.start_time
        ts = start + self.time_step * np.arange(self.num_steps)
        return np.asarray(stored.q(_clamp(stored.q, ts)), float)

    # StoreOptimizerSolution (:99-138): cubic splines with continuous second derivatives
    # (Drake's default end condition is not-a-knot, scipy's default too)
    def store_optimizer_solution(self, solution, start_time: float, stored: StoredTrajectory):
        q, v, tau = (np.asarray(x, float) for x in (solution.q, solution.v, solution.tau))
        n = self.num_steps
        ts = self.time_step * np.arange(n)
        u = np.vstack([tau, tau[-1:]])[:, self.actuated]    # undefined at the last step: repeat (:122-126)
        stored.start_time = float(start_time)
        bc = "not-a-knot" if n >= 4 else "natural"
        stored.q = CubicSpline(ts, q[:n], bc_type=bc)
        stored.v = CubicSpline(ts, v[:n], bc_type=bc)
        stored.u = CubicSpline(ts, u[:n], bc_type=bc)


def _clamp(spline, t):
    """PiecewisePolynomial::value evaluates at the closest point of the trajectory's time range"""
    return np.clip(t, spline.x[0], spline.x[-1])


class Interpolator:
    """reference examples/mpc_controller.cc:140-178: x(t) and u(t) of a stored trajectory"""

    @staticmethod
    def state(traj: StoredTrajectory, t: float):
        s = t - traj.start_time
        return np.concatenate([traj.q(_clamp(traj.q, s)), traj.v(_clamp(traj.v, s))])

    @staticmethod
    def control(traj: StoredTrajectory, t: float):
        return np.asarray(traj.u(_clamp(traj.u, t - traj.start_time)), float)


class DeviceModelPredictiveController:
    """idto::examples::mpc::ModelPredictiveController + Interpolator of libidto_opt.so (include/idto_opt.h idto_mpc_*).
    `optimizer`: an idto_amd.optimizer.TrajectoryOptimizer whose max_iterations is the example's mpc_iters."""

    def __init__(self, optimizer, warm_start_solution, actuated=None, q_nom_relative_to_q_init=None, replan_period=0.0,
                 strict=True):
        """strict: update() raises when a re-plan's factorisation fails (the C++ controller keeps the previous plan and
        reports SolverFlag::kFactorizationFailed through last_flag(); a caller that ignores the flag would otherwise
        run on the old plan with no signal).  strict=False: return the previous plan, `last_flag == 2`."""
        import ctypes as C
        self.strict = bool(strict)
        from . import optimizer as O
        self._O, self._C = O, C
        self.opt = optimizer
        prob = optimizer.prob()
        self.N, self.nq, self.nv = optimizer.num_steps(), len(prob.q_init), len(prob.v_init)
        q, v, tau = (O._d(x) for x in (warm_start_solution.q, warm_start_solution.v, warm_start_solution.tau))
        act = None if actuated is None else np.ascontiguousarray(np.asarray(actuated, dtype=np.int32))
        sel = q_nom_relative_to_q_init
        if sel is None:
            sel = optimizer.params().q_nom_relative_to_q_init
        sel = None if sel is None or len(sel) == 0 else np.ascontiguousarray(np.asarray(sel, dtype=np.int32))
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        h = C.c_void_p()
        self._chk(O.lib().idto_mpc_create(optimizer._h, O.dptr(q), O.dptr(v), O.dptr(tau), ip(act), ip(sel),
                                          float(replan_period), C.byref(h)))
        self._h = h
        self.nu = O.lib().idto_mpc_num_actuators(self._h)
        self.last_cost = None

    def _chk(self, rc):
        if rc:
            raise RuntimeError(self._O.lib().idto_opt_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._O.lib().idto_mpc_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _buffers(self):
        """the re-plan's input / output buffers and their ctypes pointers, made once: a re-plan is ~0.2 ms, five fresh
        arrays, five pointer casts and two byref objects per call were 15 - 20 us of it on the Python side"""
        O, C = self._O, self._C
        b = getattr(self, "_buf", None)
        if b is None:
            x0 = np.zeros(self.nq + self.nv)
            g, q = np.zeros((self.N + 1, self.nq)), np.zeros((self.N + 1, self.nq))
            v, tau = np.zeros((self.N + 1, self.nv)), np.zeros((self.N, self.nv))
            cost, flag = C.c_double(), C.c_int()
            ptrs = tuple(O.dptr(a) for a in (x0, g, q, v, tau)) + (C.byref(cost), C.byref(flag))
            b = self._buf = (x0, g, q, v, tau, cost, flag, ptrs, O.lib().idto_mpc_update)
        return b

    def update(self, t, q0, v0, copy=True):
        """UpdateAbstractState: returns (q_guess, q, v, tau) of this replan.  copy=False: the controller's own output
        buffers, overwritten by the next update (what a C++ caller of idto_mpc_update holds)"""
        x0, g, q, v, tau, cost, flag, ptrs, fn = self._buffers()
        x0[:self.nq] = q0
        x0[self.nq:] = v0
        if fn(self._h, t, *ptrs):
            raise RuntimeError(self._O.lib().idto_opt_last_error().decode())
        self.last_cost = cost.value
        self.last_flag = flag.value
        if flag.value == 2 and self.strict:   # SolverFlag::kFactorizationFailed: (q, v, tau) are the PREVIOUS plan's
            raise RuntimeError("MPC re-plan at t = %g: the factorisation failed; the previous plan stays in force "
                               "(strict=False returns it, last_flag == 2 says so)" % t)
        return (g.copy(), q.copy(), v.copy(), tau.copy()) if copy else (g, q, v, tau)

    @property
    def start_time(self):
        return self._O.lib().idto_mpc_start_time(self._h)

    def state(self, t):
        x = np.zeros(self.nq + self.nv)
        self._chk(self._O.lib().idto_mpc_state(self._h, float(t), self._O.dptr(x)))
        return x

    def control(self, t):
        u = np.zeros(self.nu)
        self._chk(self._O.lib().idto_mpc_control(self._h, float(t), self._O.dptr(u)))
        return u


    def last_stats(self):
        """(TrajectoryOptimizerStats of the last update's solve, the trust-region radius the next update starts from)"""
        O, C = self._O, self._C
        st = O.TrajectoryOptimizerStats(max(self.opt.params().max_iterations, 1))
        r = C.c_double()
        self._chk(O.lib().idto_mpc_stats(self._h, C.byref(st.c), C.byref(r)))
        return st, r.value


class BatchDeviceModelPredictiveController:
    """idto::examples::mpc::BatchModelPredictiveController of libidto_opt.so (include/idto_opt.h idto_mpc_batch_*): B
    controllers of `optimizer`'s model, horizon and parameters - controller b equals a DeviceModelPredictiveController on
    an optimizer of its own made with problems[b] - whose tick is enqueued on the device at once and waited for once.
    Every controller re-plans in every tick.  Configurations the device's batch loop does not serve (linesearch, adaptive
    scalings, dense weights, several devices, verbose, the debug switches, the dense linear solver, the child-context
    constraint route, B < 2) raise RuntimeError with the configuration's name: use B single controllers."""

    def __init__(self, optimizer, warm_start_solutions, actuated=None, q_nom_relative_to_q_init=None, problems=None,
                 strict=True):
        """strict: update() raises when a controller's re-plan failed or the tick did not count, as
        DeviceModelPredictiveController's does; update(strict=...) overrides it for one tick."""
        import ctypes as C
        from . import optimizer as O
        from .model import CProblem
        self.strict = bool(strict)
        self._O, self._C = O, C
        self.opt = optimizer
        prob = optimizer.prob()
        self.N, self.nq, self.nv = optimizer.num_steps(), len(prob.q_init), len(prob.v_init)
        self.B = B = len(warm_start_solutions)
        q = O._d(np.array([np.asarray(w.q, float)[:self.N + 1] for w in warm_start_solutions]).reshape(B, self.N + 1, self.nq))
        v = O._d(np.array([np.asarray(w.v, float)[:self.N + 1] for w in warm_start_solutions]).reshape(B, self.N + 1, self.nv))
        tau = O._d(np.array([np.asarray(w.tau, float)[:self.N] for w in warm_start_solutions]).reshape(B, self.N, self.nv))
        act = None if actuated is None else np.ascontiguousarray(np.asarray(actuated, dtype=np.int32))
        sel = q_nom_relative_to_q_init
        if sel is None:
            sel = optimizer.params().q_nom_relative_to_q_init
        sel = None if sel is None or len(sel) == 0 else np.ascontiguousarray(np.asarray(sel, dtype=np.int32))
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        carr, keep = None, []
        if problems is not None:
            if len(problems) != B:
                raise RuntimeError(f"one problem per controller ({B} warm starts, {len(problems)} problems)")
            carr = (CProblem * B)()
            for b, pr in enumerate(problems):
                carr[b], k = pr.to_c()
                keep.append(k)
        h = C.c_void_p()
        self._chk(O.lib().idto_mpc_batch_create(optimizer._h, B, carr, O.dptr(q), O.dptr(v), O.dptr(tau), ip(act), ip(sel), C.byref(h)))
        self._h = h
        self.nu = O.lib().idto_mpc_batch_num_actuators(self._h)
        self.last_flags = [0] * B
        self.last_radii = np.full(B, float(optimizer.params().Delta0))
        self.last_stats = None

    def _chk(self, rc):
        if rc:
            raise RuntimeError(self._O.lib().idto_opt_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._O.lib().idto_mpc_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _buffers(self):
        """the tick's input / output buffers and their ctypes pointers, made once (as DeviceModelPredictiveController's)"""
        O, C = self._O, self._C
        b = getattr(self, "_buf", None)
        if b is None:
            B, N, nq, nv = self.B, self.N, self.nq, self.nv
            times, x0 = np.zeros(B), np.zeros((B, nq + nv))
            g, q = np.zeros((B, N + 1, nq)), np.zeros((B, N + 1, nq))
            v, tau = np.zeros((B, N + 1, nv)), np.zeros((B, N, nv))
            stats = [O.TrajectoryOptimizerStats(max(self.opt.params().max_iterations, 1)) for _ in range(B)]
            cst = (O.CStats * B)()
            for i in range(B):
                cst[i] = stats[i].c
            flags, radii, ok = (C.c_int * B)(), np.zeros(B), C.c_int()
            ptrs = tuple(O.dptr(a) for a in (times, x0, g, q, v, tau)) + (cst, flags, O.dptr(radii), C.byref(ok))
            b = self._buf = (times, x0, g, q, v, tau, stats, cst, flags, radii, ok, ptrs, O.lib().idto_mpc_batch_update)
        return b

    # ---- B plants beside the controllers (BeginPlants ... TickWithPlants; include/idto_opt.h idto_mpc_batch_plants_*)
    def begin_plants(self, sim_time_step, Kp, Kd, feed_forward=False, record_capacity=0):
        """plant b: simulated on the device at sim_time_step under PD+ on controller b's stored plan; Kp [nu, nq], Kd [nu, nv]
        (idto_amd.problem.mpc_parameters reads them from an example's configuration)"""
        O = self._O
        Kp, Kd = O._d(Kp), O._d(Kd)
        self._chk(O.lib().idto_mpc_batch_plants_begin(self._h, float(sim_time_step), O.dptr(Kp), int(Kp.size), O.dptr(Kd), int(Kd.size),
                                                      int(bool(feed_forward)), int(record_capacity)))

    def set_plant_model(self, b, model=None, params=None):
        """plant b gets `model` (the controllers' topology) and the contact parameters of `params`; None: the controllers'"""
        C = self._C
        cm, keep = model.to_c() if model is not None else (None, None)
        cc = params.contact_to_c() if params is not None else None
        self._chk(self._O.lib().idto_mpc_batch_plants_set_model(self._h, int(b), C.byref(cm) if cm is not None else None,
                                                                C.byref(cc) if cc is not None else None))

    def set_plant_states(self, times, x):
        O = self._O
        times = O._d(np.broadcast_to(np.asarray(times, float), (self.B,)))
        x = O._d(np.asarray(x, float).reshape(self.B, self.nq + self.nv))
        self._chk(O.lib().idto_mpc_batch_plants_set_states(self._h, O.dptr(times), O.dptr(x)))

    def step_plants(self, substeps):
        """`substeps` substeps of every plant in one launch"""
        self._chk(self._O.lib().idto_mpc_batch_plants_step(self._h, int(substeps)))

    def plant_state(self, b):
        """(time, [q; v], status of the last step) of plant b"""
        C, O = self._C, self._O
        t, x, st = np.zeros(1), np.zeros(self.nq + self.nv), C.c_int()
        self._chk(O.lib().idto_mpc_batch_plants_state(self._h, int(b), O.dptr(t), O.dptr(x), C.byref(st)))
        return float(t[0]), x, st.value

    def tick_with_plants(self, substeps, copy=True, strict=None):
        """step_plants(substeps), then update(the plants' times, the plants' states), as ONE device pass waited for once: what
        update returns"""
        return self._tick(self._O.lib().idto_mpc_batch_plants_tick, (int(substeps),), copy, strict)

    def update(self, times, x0s, copy=True, strict=None):
        """UpdateAll: controller b re-plans at times[b] from x0s[b] = [q0; v0].  Returns (q_guess, q, v, tau), each
        [B, ...]; a controller whose re-plan failed keeps its previous plan and solution.  strict: raise when any
        controller's re-plan failed or the tick did not count (strict=False: `last_flags[b] == 2` / `last_tick_ok`
        say so, `error(b)` why).  copy=False: the controllers' own output buffers, overwritten by the next update."""
        times_b, x0_b = self._buffers()[:2]
        times_b[:] = times
        x0_b[:] = np.asarray(x0s, float).reshape(self.B, self.nq + self.nv)
        return self._tick(self._buffers()[-1], self._buffers()[-2][:2], copy, strict)

    def _tick(self, fn, head, copy, strict):
        """one tick through `fn(handle, *head, the output pointers)` and the bookkeeping behind it"""
        strict = self.strict if strict is None else bool(strict)
        times_b, x0_b, g, q, v, tau, stats, cst, flags, radii, ok, ptrs, _ = self._buffers()
        if fn(self._h, *head, *ptrs[2:]):
            raise RuntimeError(self._O.lib().idto_opt_last_error().decode())
        for b in range(self.B):
            stats[b].c = cst[b]
        self.last_stats = stats
        self.last_flags = list(flags)
        self.last_radii = radii.copy()
        self.last_tick_ok = bool(ok.value)
        if strict and not self.last_tick_ok:
            raise RuntimeError("MPC tick: " + self.error(-1) + "; every controller keeps its plan")
        if strict and any(f == 2 for f in self.last_flags):
            bad = [b for b, f in enumerate(self.last_flags) if f == 2]
            raise RuntimeError("MPC tick: the re-plan of controller(s) %s failed (%s); their previous plans stay in force "
                               "(strict=False returns them, last_flags[b] == 2 says so)" % (bad, self.error(bad[0])))
        return (g.copy(), q.copy(), v.copy(), tau.copy()) if copy else (g, q, v, tau)

    def error(self, b):
        return self._O.lib().idto_mpc_batch_error(self._h, int(b)).decode()

    def start_time(self, b):
        return self._O.lib().idto_mpc_batch_start_time(self._h, int(b))

    def flag(self, b):
        return self._O.lib().idto_mpc_batch_flag(self._h, int(b))

    def state(self, b, t):
        x = np.zeros(self.nq + self.nv)
        self._chk(self._O.lib().idto_mpc_batch_state(self._h, int(b), float(t), self._O.dptr(x)))
        return x

    def control(self, b, t):
        u = np.zeros(self.nu)
        self._chk(self._O.lib().idto_mpc_batch_control(self._h, int(b), float(t), self._O.dptr(u)))
        return u


def spline_fit(breaks, knots):
    """csrc/mpc_spline.h on the host: the knot derivatives [n, dim] of the not-a-knot cubic through `knots` [n, dim]"""
    from . import optimizer as O
    breaks, knots = O._d(breaks), O._d(knots)
    n, dim = knots.shape
    m = np.zeros((n, dim))
    if O.lib().idto_mpc_spline_fit(O.dptr(breaks), O.dptr(knots), n, dim, O.dptr(m)):
        raise RuntimeError(O.lib().idto_opt_last_error().decode())
    return m


def shift_reference(breaks, y_q, m_q, start_time, time, time_step, q0, selector, q_nom):
    """csrc/mpc_spline.h on the host: (guess [n, nq], shifted q_nom [n, nq]) of one controller's tick"""
    import ctypes as C
    from . import optimizer as O
    breaks, y_q, m_q, q0 = O._d(breaks), O._d(y_q), O._d(m_q), O._d(q0)
    n, nq = y_q.shape
    q_nom = np.array(q_nom, dtype=np.float64).reshape(n, nq).copy()
    sel = np.ascontiguousarray(np.asarray(selector, dtype=np.int32))
    guess = np.zeros((n, nq))
    if O.lib().idto_mpc_shift_reference(O.dptr(breaks), O.dptr(y_q), O.dptr(m_q), n, nq, float(start_time), float(time),
                                        float(time_step), O.dptr(q0), sel.ctypes.data_as(C.POINTER(C.c_int)), O.dptr(q_nom),
                                        O.dptr(guess)):
        raise RuntimeError(O.lib().idto_opt_last_error().decode())
    return guess, q_nom


def spline_eval(breaks, knots, times):
    """PiecewiseCubic of include/idto/examples/mpc_controller.h (C++, host only): values at `times`"""
    from . import optimizer as O
    breaks, knots, times = O._d(breaks), O._d(knots), O._d(np.atleast_1d(times))
    n, dim = knots.shape
    out = np.zeros((len(times), dim))
    if O.lib().idto_mpc_spline_eval(O.dptr(breaks), O.dptr(knots), n, dim, O.dptr(times), len(times), O.dptr(out)):
        raise RuntimeError(O.lib().idto_opt_last_error().decode())
    return out
