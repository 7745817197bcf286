"""B model-predictive controllers in one device pass per tick (include/idto_hip.h idto_hip_mpc_batch_*, csrc/mpc_batch.h;
idto::examples::mpc::BatchModelPredictiveController through idto_mpc_batch_* and BatchDeviceModelPredictiveController).

The bar is == throughout: the two kernels compile csrc/mpc_spline.h, the text the host classes run; neither side contracts
a * b + c, and the device's division is IEEE (tests/test_gpu_kats.py::test_device_arithmetic_is_ieee holds that).  The
yardstick of a tick is B single controllers (DeviceModelPredictiveController), each on an optimizer of its own - on the
models whose batch entries equal their single Solve bit for bit (hopper, mini_cheetah; small models in a batch of more
than two differ from it by the solver's round-off, tests/test_gpu_solve_batch.py).  Times are left out.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from idto_amd import hip
from idto_amd import mpc as M
from idto_amd.model import load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import SolverParameters, load_config, make_problem, synthetic_trajectory

pytestmark = pytest.mark.gpu

B = 3
STATS = [f for f in TrajectoryOptimizerStats.FIELDS if f != "iteration_times"]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _trace(fn):
    """fn(), and the host trace's marks while it ran"""
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


def _actuated_dofs(model):
    act = np.flatnonzero(np.asarray(model.actuated))
    return act if act.size else np.arange(model.nv)


def _mixed_selector(nq):
    sel = np.zeros(nq, dtype=np.int32)
    sel[::2] = 1          # both values, for every model (nq >= 2)
    return sel


# ---- the two kernels alone
@pytest.mark.parametrize("N", [1, 2, 3, 6])   # the line, the parabola, the first general system, one with interior rows
@pytest.mark.parametrize("name", ["acrobot", "hopper"])
def test_store_and_shift_equal_the_header_on_the_host(name, N):
    cfg, model = load_config(name), load_model(name)
    nq, nv = model.nq, model.nv
    probs, sp = [], None
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.01 * b + 0.003 * np.arange(N + 1)[:, None]
        probs.append(prob)
    dt = probs[0].time_step
    ctx = hip.HipPath(model, probs, sp)
    sel, act = _mixed_selector(nq), _actuated_dofs(model)
    ctx.mpc_batch_begin(sel, act)
    rng = np.random.default_rng(7 + N)
    q, v, tau = rng.normal(size=(B, N + 1, nq)), rng.normal(size=(B, N + 1, nv)), 30 * rng.normal(size=(B, N, nv))
    start = np.array([0.0, 0.3, -0.125])
    plans = ctx.mpc_batch_store(q, v, tau, start)
    breaks = np.arange(N + 1) * dt                      # i * time_step, as StoreOptimizerSolution forms them
    P = [ctx.mpc_split_plan(plans[b]) for b in range(B)]
    for b in range(B):
        u = np.vstack([tau[b], tau[b][-1:]])[:, act]    # u[i] = tau[min(i, N - 1)][actuated]
        assert P[b]["start_time"] == start[b]
        for k, y in (("q", q[b]), ("v", v[b]), ("u", u)):
            assert np.array_equal(P[b]["y_" + k], y), (b, k)
            assert np.array_equal(P[b]["m_" + k], M.spline_fit(breaks, y)), (b, k)
    # every problem at another time: time - start an exact multiple of dt (upper_bound's boundary), strictly inside an
    # interval, beyond the horizon (every row clamped)
    times = np.array([start[0] + 1 * dt, start[1] + 0.37 * dt, start[2] + (N + 2.5) * dt])
    assert times[0] - start[0] == dt
    q_nom = [np.array(p.q_nom, float) for p in probs]
    for tick in range(2):                               # (twice: q_nom is shifted in place, cumulatively)
        x0 = rng.normal(size=(B, nq + nv))
        guess, q_nom_dev = ctx.mpc_batch_shift(times, x0)
        ctx.eval_tau()
        for b in range(B):
            g_ref, q_nom[b] = M.shift_reference(breaks, P[b]["y_q"], P[b]["m_q"], start[b], times[b], dt, x0[b, :nq], sel, q_nom[b])
            assert np.array_equal(guess[b], g_ref), (tick, b)
            assert np.array_equal(q_nom_dev[b], q_nom[b]), (tick, b)
            assert np.array_equal(guess[b][0], x0[b, :nq])
            # PiecewiseCubic on the host, fitted from the knots: the same values at the guess's times
            probe = (times[b] - start[b]) + np.arange(1, N + 1) * dt
            assert np.array_equal(guess[b][1:], M.spline_eval(breaks, q[b], probe)), (tick, b)
            assert np.array_equal(ctx.get("q", b).reshape(N + 1, nq), guess[b])                 # the resident q is the guess
            assert np.array_equal(ctx.get("v", b).reshape(N + 1, nv)[0], x0[b, nq:])            # v_init = v0
            for i in np.flatnonzero(sel == 0):                                                  # not selected: bit for bit
                assert np.array_equal(q_nom_dev[b][:, i], np.asarray(probs[b].q_nom)[:, i])
        assert np.array_equal(guess[2][1:], np.tile(M.spline_eval(breaks, q[2], [breaks[-1]]), (N, 1)))   # clamped
        times = times + np.array([dt, 0.11 * dt, 0.5 * dt])
    ctx.close()


# ---- a tick equals B single controllers
def _controllers(name, N=20, max_iterations=2, bad=None, Delta0=None):
    """B problems of the example (own nominal trajectories and weights), their warm starts, B single controllers each on
    an optimizer of its own, and the batch controller"""
    cfg, model = load_config(name), load_model(name)
    probs, warm, sp = [], [], None
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.01 * b
        prob.Qq = prob.Qq * (1.0 + 0.1 * b)
        probs.append(prob)
    sp.verbose = False
    if bad is not None:
        sp.equality_constraints = False
    sp0 = SolverParameters(**{**sp.__dict__, "max_iterations": 6})
    for b in range(B):
        opt = TrajectoryOptimizer(model, probs[b], sp0)
        sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
        opt.Solve(synthetic_trajectory(cfg, model, N, seed=b, lower=0.01), sol, st)
        opt.close()
        warm.append(sol)
    if bad is not None:   # tests/test_gpu_solve_batch.py::test_one_failing_entry_is_its_own: exactly zero rows in this problem's Hessian
        p = copy.deepcopy(probs[bad])
        for W in (p.Qq, p.Qv, p.Qf_q, p.Qf_v):
            W[0, :] = 0.0
            W[:, 0] = 0.0
        p.R[:] = 0.0
        probs[bad] = p
    sp1 = SolverParameters(**{**sp.__dict__, "max_iterations": max_iterations})
    if Delta0 is not None:
        sp1.Delta0 = Delta0
    sel = _mixed_selector(model.nq)
    opts = [TrajectoryOptimizer(model, probs[b], sp1) for b in range(B)]
    singles = [M.DeviceModelPredictiveController(opts[b], warm[b], actuated=model.actuated, q_nom_relative_to_q_init=sel, strict=False)
               for b in range(B)]
    opt_b = TrajectoryOptimizer(model, probs[0], sp1)
    batch = M.BatchDeviceModelPredictiveController(opt_b, warm, actuated=model.actuated, q_nom_relative_to_q_init=sel, problems=probs)
    return model, sp1, singles, opts, batch, opt_b


PERIODS = np.array([0.0100, 0.0137, 0.0213])   # non-commensurate tick times, one clock per controller
# per controller: the size of the state estimate's disturbance.  With the examples' own Delta0 (hopper 1e-3, mini_cheetah
# 1e-1) the radius clips every step of four ticks of two iterations and none is rejected, whatever the disturbance (tried
# up to 10.0 on the third controller); the controllers below therefore start from DELTA0 = 100: the single controllers then
# reject steps in most ticks (trust ratios down to -30) and end their first tick on radii of 25 ... 200, which differ
# between the controllers - the test asserts both of the yardstick's own run.
DELTA0 = 100.0
X0_SCALE = np.array([0.002, 0.05, 0.3])


def _close(singles, opts, batch, opt_b):
    batch.close(); opt_b.close()
    for s, o in zip(singles, opts):
        s.close(); o.close()


@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_tick_equals_single_controllers(name):
    model, sp, singles, opts, batch, opt_b = _controllers(name, Delta0=DELTA0)
    nq = model.nq
    rng = np.random.default_rng(5)
    radii_after_first, rejected, waits = None, False, []
    for k in range(1, 5):
        times = k * PERIODS
        # the state estimates: every controller's own plan at its own time, disturbed
        x0 = np.array([singles[b].state(times[b]) + X0_SCALE[b] * rng.normal(size=nq + model.nv) for b in range(B)])
        ref = []
        for b in range(B):
            assert np.array_equal(batch.state(b, times[b]), singles[b].state(times[b]))
            g, q, v, tau = singles[b].update(times[b], x0[b, :nq], x0[b, nq:])
            st, radius = singles[b].last_stats()
            ref.append((g, q, v, tau, st, radius, singles[b].last_flag))
            assert singles[b].last_flag in (0, 3)
            rejected = rejected or bool(np.any(st.trust_ratios <= 0.0))   # (eta = 0: a step is accepted when rho > 0)
        if k == 1:
            radii_after_first = [r[5] for r in ref]
        (g, q, v, tau), marks = _trace(lambda: batch.update(times, x0))
        waits.append(marks.count("waited for the device"))
        for b in range(B):
            rg, rq, rv, rtau, st, radius, flag = ref[b]
            what = (name, "tick", k, "controller", b)
            assert _same(g[b], rg) and _same(q[b], rq) and _same(v[b], rv) and _same(tau[b], rtau), what
            for f in STATS:
                assert _same(getattr(batch.last_stats[b], f), getattr(st, f)), what + (f,)
            assert batch.last_flags[b] == flag and batch.flag(b) == flag, what
            assert batch.last_radii[b] == radius, what
            assert batch.start_time(b) == singles[b].start_time == times[b]
            for tq in (times[b], times[b] + 0.4 * PERIODS[b], times[b] + 3.3 * PERIODS[b], times[b] + 100.0, times[b] - 1.0):
                assert np.array_equal(batch.state(b, tq), singles[b].state(tq)), what
                assert np.array_equal(batch.control(b, tq), singles[b].control(tq)), what
    _close(singles, opts, batch, opt_b)
    # what makes the comparison above mean something: a radius that moved (a lost radius would otherwise pass) and a rejected step
    assert any(r != sp.Delta0 for r in radii_after_first) and len(set(radii_after_first)) > 1, radii_after_first
    assert rejected
    assert waits == [1, 1, 1, 1], waits


def test_one_controller_fails_and_keeps_its_plan():
    bad = 1
    model, sp, singles, opts, batch, opt_b = _controllers("hopper", max_iterations=4, bad=bad)
    nq = model.nq
    rng = np.random.default_rng(6)
    for k in range(1, 3):
        times = k * PERIODS
        x0 = np.array([singles[b].state(times[b]) + 0.002 * rng.normal(size=nq + model.nv) for b in range(B)])
        probes = [times[bad], times[bad] + 0.013, times[bad] + 0.4, times[bad] + 50.0]
        before = [(batch.state(bad, t), batch.control(bad, t), batch.start_time(bad)) for t in probes]
        radius_before = batch.last_radii[bad]
        with pytest.raises(RuntimeError, match="controller"):
            batch.update(times, x0)                       # strict, as the single controller's update
        # (the strict call has run the tick: the plans below are this tick's; the next tick goes on from them)
        assert batch.last_tick_ok and batch.last_flags[bad] == 2 and batch.flag(bad) == 2 and batch.error(bad) != ""
        assert batch.last_radii[bad] == radius_before
        for t, (x, u, t0) in zip(probes, before):
            assert np.array_equal(batch.state(bad, t), x) and np.array_equal(batch.control(bad, t), u) and batch.start_time(bad) == t0
        for b in range(B):
            if b == bad:
                singles[b].update(times[b], x0[b, :nq], x0[b, nq:])
                assert singles[b].last_flag == 2          # the yardstick's own controller fails the same way
                continue
            g, q, v, tau = singles[b].update(times[b], x0[b, :nq], x0[b, nq:])
            assert singles[b].last_flag in (0, 3) and batch.last_flags[b] == singles[b].last_flag
            for tq in (times[b], times[b] + 0.0041, times[b] + 100.0):
                assert np.array_equal(batch.state(b, tq), singles[b].state(tq)), (k, b)
                assert np.array_equal(batch.control(b, tq), singles[b].control(tq)), (k, b)
            assert batch.last_radii[b] == singles[b].last_stats()[1]
    _close(singles, opts, batch, opt_b)


# ---- what the batch loop does not serve is refused by name, before any device work
# name -> (solver parameters to set, the optimizer's constructor arguments, controllers)
REFUSALS = {
    "linesearch": (dict(method="linesearch"), {}, B),
    "adaptive": (dict(scaling=True, scaling_method="adaptive_sqrt"), {}, B),
    "dense weights": ({}, {}, B),
    "several devices": ({}, dict(devices=[0]), B),   # (the sharded constructor; tests/test_gpu_multi.py uses it on one device too)
    "verbose": (dict(verbose=True), {}, B),
    "debug": (dict(print_debug_data=True), {}, B),
    "kDenseLdlt": (dict(linear_solver="dense_ldlt"), {}, B),
    "child-context": (dict(equality_constraints=True), {}, B),
    "B < 2": ({}, {}, 1),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_unserved_configurations_are_refused_by_name(case, monkeypatch):
    params, kw, nb = REFUSALS[case]
    cfg, model = load_config("hopper"), load_model("hopper")
    prob, sp, _ = make_problem(cfg, model, num_steps=6)
    sp.verbose, sp.max_iterations = False, 2
    for k, x in params.items():
        setattr(sp, k, x)
    if case == "dense weights":
        prob.Qq = prob.Qq.copy()
        prob.Qq[0, 1] = prob.Qq[1, 0] = 1e-3
    if case == "child-context":
        monkeypatch.setenv("IDTO_CON_KKT", "0")
    opt = TrajectoryOptimizer(model, prob, sp, **kw)
    warm = TrajectoryOptimizerSolution()
    warm.q, warm.v, warm.tau = np.zeros((7, model.nq)), np.zeros((7, model.nv)), np.zeros((6, model.nv))
    err = {}

    def create():
        try:
            M.BatchDeviceModelPredictiveController(opt, [warm] * nb, actuated=model.actuated,
                                                   q_nom_relative_to_q_init=_mixed_selector(model.nq))
        except RuntimeError as e:
            err["text"] = str(e)
    _, marks = _trace(create)
    opt.close()
    assert case.lower() in err.get("text", "").lower(), err
    assert "ModelPredictiveControllers, each on an optimizer of its own" in err["text"]
    assert marks == "", marks                  # no device work: not one mark of an upload or a launch
