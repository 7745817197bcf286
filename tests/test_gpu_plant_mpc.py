"""Plants under the PD+ law on the controllers' stored plans (include/idto_hip.h idto_hip_plant_begin with
IDTO_PLANT_PD_PLUS; csrc/plant.h, csrc/plant_step.h, csrc/mpc_spline.h).

hopper and mini_cheetah, N = 8, B = 3, the gains of the example configurations (Kp 100 / Kd 5 on hopper's two actuated
joints without the nominal control; 50 / 2 on mini_cheetah's twelve with it) plus a small dense part, so that a row's sum
has more than one term.  After S substeps the states == the host restatement: the nominal [q, v, u] at t0 + s h from the
stored plan's splines (idto_mpc_spline_eval: the host's PiecewiseCubic, clamped to the plan's range), the torque from
idto_plant_pd_plus_host, the physics from the oracle, the step from idto_plant_advance_host.  The plants start in the
plan's second half and run past its end, so that the clamp is taken.

The tick (idto_hip_mpc_batch_tick_plants): everything it returns == the composition a caller would write without it - the
same plant_step on a twin context, the plants' states fetched to the host, then idto_hip_mpc_batch_replan(times, x0) - over
three ticks of two iterations, so that from the second tick on the plants track plans that the controllers produced; and the
host trace shows exactly one "waited for the device" per tick.

The same two properties one layer up, on BatchDeviceModelPredictiveController (BatchModelPredictiveController through
idto_mpc_batch_plants_*) with the gains, sim_time_step and feed_forward of the example configurations
(idto_amd.problem.mpc_parameters): step_plants against the host restatement whose nominal values are batch.state(b, t) and
batch.control(b, t); tick_with_plants(S) against step_plants(S) on a twin, plant_state fetched to the host, then
update(times, x0) - guesses, q, v, tau, every statistics series but the times, flags, radii and the stored plans.
"""
import ctypes as C

import numpy as np
import pytest

import plant_cases as pc
from idto_amd import hip, optimizer
from idto_amd import mpc as M
from idto_amd.model import dptr, iptr
from idto_amd.problem import synthetic_trajectory

pytestmark = pytest.mark.gpu

B, N, H = 3, 8, 1e-3


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def _gains(name, model, act):
    nq, nv, nu = model.nq, model.nv, len(act)
    kp, kd, ff = (100.0, 5.0, False) if name == "hopper" else (50.0, 2.0, True)
    rng = np.random.default_rng(7)
    Kp, Kd = 0.01 * rng.uniform(-1, 1, (nu, nq)), 0.01 * rng.uniform(-1, 1, (nu, nv))
    for r, j in enumerate(act):
        Kp[r, j + (nq - nv)] += kp     # (the position of velocity j: behind the floating base's extra quaternion entry)
        Kd[r, j] += kd
    return Kp, Kd, ff


def _pd_plus_host(Kp, Kd, act, q, v, qn, vn, ff, un):
    nu, nq = Kp.shape
    tau = np.zeros(Kd.shape[1])
    a = np.ascontiguousarray(act, dtype=np.int32)
    optimizer.lib().idto_plant_pd_plus_host(dptr(np.ascontiguousarray(Kp)), dptr(np.ascontiguousarray(Kd)), nu, nq, Kd.shape[1], iptr(a),
                                            dptr(np.ascontiguousarray(q)), dptr(np.ascontiguousarray(v)), dptr(np.ascontiguousarray(qn)),
                                            dptr(np.ascontiguousarray(vn)), int(ff), dptr(np.ascontiguousarray(un)), dptr(tau))
    return tau


@pytest.mark.parametrize("name,S", [("hopper", 4), ("mini_cheetah", 3)])
def test_pd_plus_steps_equal_the_host_restatement(name, S):
    model, _, cfg = pc.case(name)
    orc = pc.oracle(name)
    nq, nv = model.nq, model.nv
    act = np.flatnonzero(np.asarray(model.actuated))
    prob, sp = pc.problem(name, N=N)
    dt = prob.time_step
    rng = np.random.default_rng(3)
    q_plan = np.array([synthetic_trajectory(cfg, model, N, seed=b, lower=0.02) for b in range(B)])
    v_plan, tau_plan = rng.uniform(-0.3, 0.3, (B, N + 1, nv)), rng.uniform(-2, 2, (B, N, nv))
    start = np.array([0.0, 0.1, -0.05])
    Kp, Kd, ff = _gains(name, model, act)
    dev = hip.HipPath(model, [prob] * B, sp)
    dev.mpc_batch_begin(np.zeros(nq, dtype=np.int32), act)
    dev.mpc_batch_store(q_plan, v_plan, tau_plan, start)
    dev.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=Kp, Kd=Kd, feed_forward=ff)
    # plant b starts two substeps before the end of its plan: the last substeps are evaluated at the clamped time
    t0 = start + N * dt - 2 * H
    x0 = np.array([np.concatenate([q_plan[b, N - 1], v_plan[b, N - 1]]) for b in range(B)])
    dev.plant_set_state(t0, x0)
    with pytest.raises(hip.HipError, match="PD\\+ forms the torque itself"):
        dev.plant_step(S, np.zeros((B, nv)))
    rec, status = dev.plant_step(S, None, record_every=1)
    times, x_end = dev.plant_get_state()
    dev.close()
    assert status.tolist() == [[0, S]] * B
    breaks = np.arange(N + 1) * dt
    for b in range(B):
        u_knots = np.vstack([tau_plan[b][:, act], tau_plan[b][-1:, act]])   # (the last knot repeats the row before it)
        q, v = x0[b, :nq].copy(), x0[b, nq:].copy()
        for s in range(S):
            t = (t0[b] + s * H) - start[b]
            qn, vn, un = (M.spline_eval(breaks, k, [t])[0] for k in (q_plan[b], v_plan[b], u_knots))
            tau = _pd_plus_host(Kp, Kd, act, q, v, qn, vn, ff, un)
            a = pc.host_fd(orc, q, v, tau)[0]
            q, v = pc.advance_host(model, H, q, v, a)
            assert _same(rec[b, s], np.concatenate([q, v])), (name, b, s, np.abs(rec[b, s] - np.concatenate([q, v])).max())
        assert _same(x_end[b], rec[b, -1]) and times[b] == t0[b] + S * H


def _trace(fn):
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    L.idto_hip_trace_enable(1)
    try:
        out = fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        L.idto_hip_trace_dump(buf, len(buf))
        L.idto_hip_trace_enable(0)
    return out, buf.value.decode()


NOT_THE_CLOCK = [c for c in range(17) if c != 10]   # (the statistics rows without TRR_CLOCK)


@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_tick_with_plants_equals_the_composition_under_one_wait(name):
    S, iters, loop = 17, 2, (2, True, False)   # double_sqrt scaling, no quaternion normalisation
    model, _, cfg = pc.case(name)
    nq, nv = model.nq, model.nv
    act = np.flatnonzero(np.asarray(model.actuated))
    prob, sp = pc.problem(name, N=N)
    dt = prob.time_step
    rng = np.random.default_rng(5)
    q_plan = np.array([synthetic_trajectory(cfg, model, N, seed=b, lower=0.02) for b in range(B)])
    v_plan, tau_plan = rng.uniform(-0.1, 0.1, (B, N + 1, nv)), rng.uniform(-1, 1, (B, N, nv))
    Kp, Kd, ff = _gains(name, model, act)
    x0 = np.array([np.concatenate([q_plan[b, 0], v_plan[b, 0]]) for b in range(B)])
    sel = np.zeros(nq, dtype=np.int32)
    sel[::2] = 1
    ctxs = []
    for _ in range(2):
        dev = hip.HipPath(model, [prob] * B, sp)
        dev.mpc_batch_begin(sel, act)
        dev.mpc_batch_store(q_plan, v_plan, tau_plan, np.zeros(B))
        dev.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=Kp, Kd=Kd, feed_forward=ff)
        dev.plant_set_state(np.array([0.0, 0.01, 0.02]), x0)
        ctxs.append(dev)
    tick, twin = ctxs
    radii_a = radii_b = np.full(B, sp.Delta0)
    for k in range(3):
        a, marks = _trace(lambda: tick.mpc_batch_tick_plants(S, iters, *loop, radii_a, sp.Delta_max))
        assert marks.count("waited for the device") == 1, marks
        twin.plant_step(S, None, status=False)
        times, x = twin.plant_get_state()
        b_ = twin.mpc_batch_replan(times, x, iters, *loop, radii_b, sp.Delta_max)
        assert _same(a["x_after"], x), (name, k)
        for key in ("guess", "q", "v", "tau", "status", "Delta", "final_cost", "plans"):
            assert _same(a[key], b_[key]), (name, k, key)
        assert _same(a["rows"][:, :, NOT_THE_CLOCK], b_["rows"][:, :, NOT_THE_CLOCK]), (name, k)
        assert a["best"] == b_["best"]
        ta, xa = tick.plant_get_state()
        assert _same(ta, times) and _same(xa, x)
        radii_a, radii_b = a["Delta"], b_["Delta"]
    with pytest.raises(hip.HipError, match="mpc_batch_tick_plants: substeps must be in"):
        tick.mpc_batch_tick_plants(0, iters, *loop, radii_a, sp.Delta_max)
    # a second idto_hip_mpc_batch_begin: the plants' LDS was sized for the first one's plans
    tick.mpc_batch_begin(sel, act)
    with pytest.raises(hip.HipError, match="idto_hip_mpc_batch_begin was called again after idto_hip_plant_begin"):
        tick.plant_step(1, None)
    tick.close()
    twin.close()
    hold = hip.HipPath(model, [prob] * B, sp)
    hold.mpc_batch_begin(sel, act)
    hold.plant_begin(H)
    with pytest.raises(hip.HipError, match="the plants track the stored plans: idto_hip_plant_begin with IDTO_PLANT_PD_PLUS"):
        hold.mpc_batch_tick_plants(S, iters, *loop, np.full(B, sp.Delta0), sp.Delta_max)
    hold.close()


# ---- the controllers' layer
from idto_amd.model import load_model                                                                    # noqa: E402
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats  # noqa: E402
from idto_amd.problem import SolverParameters, load_config, make_problem, mpc_parameters                  # noqa: E402

STATS = [f for f in TrajectoryOptimizerStats.FIELDS if f != "iteration_times"]


def _same_series(a, b):
    """== entry by entry; a series the trust-region method does not fill (the linesearch's) is NaN on both sides"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _batch_controllers(name, count):
    """`count` identical batch controllers of B problems of the example (own nominal trajectories and weights), N = 8,
    max_iterations 2, their plants begun with the example's closed-loop parameters and put on the plans' start"""
    cfg, model = load_config(name), load_model(name)
    probs, warm, sp = [], [], None
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.01 * b
        probs.append(prob)
    sp.verbose = False
    sp0 = SolverParameters(**{**sp.__dict__, "max_iterations": 6})
    for b in range(B):
        opt = TrajectoryOptimizer(model, probs[b], sp0)
        sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
        opt.Solve(synthetic_trajectory(cfg, model, N, seed=b, lower=0.01), sol, st)
        opt.close()
        warm.append(sol)
    sp1 = SolverParameters(**{**sp.__dict__, "max_iterations": 2})
    sel = np.zeros(model.nq, dtype=np.int32)
    sel[::2] = 1
    par = mpc_parameters(cfg, model)
    out = []
    for _ in range(count):
        opt = TrajectoryOptimizer(model, probs[0], sp1)
        batch = M.BatchDeviceModelPredictiveController(opt, warm, actuated=model.actuated, q_nom_relative_to_q_init=sel, problems=probs,
                                                       strict=False)
        batch.begin_plants(par["sim_time_step"], par["Kp"], par["Kd"], par["feed_forward"])
        batch.set_plant_states(np.zeros(B), np.array([batch.state(b, 0.0) for b in range(B)]) + 0.01)
        out.append((batch, opt))
    return model, par, out


def test_yaml_front_end_reads_the_closed_loop_keys():
    for name, substeps, kp, kd, ff in (("hopper", 10, 100.0, 5.0, False), ("mini_cheetah", 17, 50.0, 2.0, True)):
        model = load_model(name)
        par = mpc_parameters(load_config(name), model)
        act = np.flatnonzero(np.asarray(model.actuated))
        assert (par["sim_time_step"], par["substeps_per_tick"], par["feed_forward"]) == (1e-3, substeps, ff)
        assert par["Kp"].shape == (len(act), model.nq) and par["Kd"].shape == (len(act), model.nv)
        for r, j in enumerate(act):
            assert par["Kp"][r, j + model.nq - model.nv] == kp and par["Kd"][r, j] == kd
        assert np.count_nonzero(par["Kp"]) == len(act) and np.count_nonzero(par["Kd"]) == len(act)


@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_step_plants_equals_the_restatement_on_the_controllers_plans(name):
    S = 4
    model, par, ((batch, opt),) = _batch_controllers(name, 1)
    orc = pc.oracle(name)
    nq = model.nq
    act = np.flatnonzero(np.asarray(model.actuated))
    h = par["sim_time_step"]
    start = [batch.plant_state(b) for b in range(B)]
    batch.step_plants(S)
    for b in range(B):
        t0, x, status = start[b]
        q, v = x[:nq].copy(), x[nq:].copy()
        for s in range(S):
            t = t0 + s * h
            xn, un = batch.state(b, t), batch.control(b, t)
            tau = _pd_plus_host(par["Kp"], par["Kd"], act, q, v, xn[:nq], xn[nq:], par["feed_forward"], un)
            q, v = pc.advance_host(model, h, q, v, pc.host_fd(orc, q, v, tau)[0])
        t1, x1, status = batch.plant_state(b)
        assert _same(x1, np.concatenate([q, v])), (name, b, np.abs(x1 - np.concatenate([q, v])).max())
        assert t1 == t0 + S * h and status == 0
    batch.close(); opt.close()


@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_tick_with_plants_equals_step_plants_then_update(name):
    model, par, ((tick, opt_a), (twin, opt_b)) = _batch_controllers(name, 2)
    S = par["substeps_per_tick"]
    for k in range(3):
        (g, q, v, tau), marks = _trace(lambda: tick.tick_with_plants(S))
        assert marks.count("waited for the device") == 1, marks
        twin.step_plants(S)
        states = [twin.plant_state(b) for b in range(B)]
        times, x0 = np.array([s[0] for s in states]), np.array([s[1] for s in states])
        rg, rq, rv, rtau = twin.update(times, x0)
        what = (name, "tick", k)
        assert _same(g, rg) and _same(q, rq) and _same(v, rv) and _same(tau, rtau), what
        assert tick.last_flags == twin.last_flags and _same(tick.last_radii, twin.last_radii) and tick.last_tick_ok and twin.last_tick_ok, what
        for b in range(B):
            for f in STATS:
                assert _same_series(getattr(tick.last_stats[b], f), getattr(twin.last_stats[b], f)), what + (b, f)
            ta, xa, sa = tick.plant_state(b)
            assert ta == times[b] and _same(xa, x0[b]) and sa == 0, what + (b,)
            assert tick.start_time(b) == twin.start_time(b) == times[b]
            for tq in (times[b], times[b] + 0.004, times[b] + 0.3, times[b] - 1.0):
                assert _same(tick.state(b, tq), twin.state(b, tq)) and _same(tick.control(b, tq), twin.control(b, tq)), what + (b, tq)
    with pytest.raises(RuntimeError, match="substeps must be in"):
        tick.tick_with_plants(0)
    for c, o in ((tick, opt_a), (twin, opt_b)):
        c.close(); o.close()
