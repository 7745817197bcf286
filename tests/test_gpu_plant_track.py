"""Plants under the time-varying LQR law on the device (include/idto_hip.h idto_hip_plant_track, idto_hip_plant_tvlqr_track;
csrc/plant.h plant_body with LAW, track_kernel) and the optimizer's route to them (TrajectoryOptimizer.track).

The bar is == : the law is csrc/tvlqr_step.h's tvlqr_control, the text that tests/cpp/lin_host.cc compiles for the host - a row of
u one lane's left-to-right sum -, and a step's substeps are plant_kernel's, so a tracked rollout equals the composition of the
existing pieces that it replaces (tests/track_cases.py composition): per step the host's control, then plant_step in hold mode on
a twin context.  That the numbers are right and not merely the same on both sides is the upright pendulum's test.  S <= 3 steps
of m <= 4 substeps, R <= 3 rollouts, except there (24 steps of 50) and on the optimizer's route (5 steps of 50: the example's own
simulation step).
No test provokes a device fault: a NaN gain, an overflowing velocity and a failed pivot end a rollout with a status word.
"""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import lin_cases as lc
import track_cases as tc
from idto_amd import hip, optimizer
from idto_amd.model import load_model
from idto_amd.problem import ProblemDefinition, SolverParameters, load_config, make_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, M = 1e-3, 2


def _same(a, b):
    """== entry by entry, NaN in the same places counting as equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _same_track(a, b):
    return _same(a.x, b.x) and _same(a.u, b.u) and _same(a.dx, b.dx) and a.status.tolist() == b.status.tolist()


def _context(name, B=1, model=None, sp=None):
    dev_model, _, prob, sp0, _, _ = lc.case(name)
    return hip.HipPath(model if model is not None else dev_model, [prob] * B if B > 1 else prob, sp if sp is not None else sp0)


def _track(name, x_nom, tau_nom, K, x0, act, m=M, model=None, sp=None, **kw):
    dev = _context(name, model=model, sp=sp)
    r = dev.plant_track(x_nom, tau_nom, K, x0, H, m, act, **kw)
    dev.close()
    return r


def _report(what, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    print(f"{what}: {int((got != ref).sum())} of {got.size} entries differ, the largest by {np.abs(got - ref).max():.3e}")


# every instantiation of track_kernel: <2> pendulum, acrobot; <3> hopper, mini_cheetah; <4> allegro_hand; <8> jaco_ball; the
# exchange form dual_jaco; the stem punyo
@pytest.mark.parametrize("name,S", [("pendulum", 3), ("acrobot", 3), ("hopper", 3), ("allegro_hand", 2), ("jaco_ball", 2), ("dual_jaco", 2),
                                    ("punyo", 2), ("mini_cheetah", 2)])
def test_rollouts_equal_the_composition_of_the_existing_pieces(name, S):
    R = 2
    x_nom, tau_nom, K, x0, act = tc.inputs(name, S, R)
    dev = _context(name)
    one = dev.plant_track(x_nom, tau_nom, K, x0, H, M, act, max_launch_substeps=M)   # every step a launch of its own
    all_ = dev.plant_track(x_nom, tau_nom, K, x0, H, M, act)
    dev.close()
    assert one.status.tolist() == [[0, S * M]] * R and _same_track(one, all_)
    n = 2 * lc.case(name)[0].nv
    assert one.x.shape == (R, S, x_nom.shape[1]) and one.u.shape == (R, S, len(act)) and one.dx.shape == (R, S + 1, n)
    twin = _context(name)
    twin.plant_begin(H)
    for r in range(R):
        x, u, dx = tc.composition(twin, name, x_nom, tau_nom, K, x0[r], act, M)
        for what, got, ref in (("x", all_.x[r], x), ("u", all_.u[r], u), ("dx", all_.dx[r], dx)):
            _report(f"{name} rollout {r} {what}", got, ref)
        assert _same(all_.x[r], x) and _same(all_.u[r], u) and _same(all_.dx[r], dx), r
    twin.close()
    assert np.abs(all_.dx[:, 0]).max() > 1e-3   # (the offsets are there)


def test_zero_deviation():
    """from x*_0 itself: dx row 0 is exactly 0, u row 0 the nominal torque's actuated entries, and the state behind step 0 what
    plant_linearize's nominal column ends at"""
    name, S = "hopper", 2
    x_nom, tau_nom, K, _, act = tc.inputs(name, S, 1)
    dev = _context(name)
    r = dev.plant_track(x_nom, tau_nom, K, x_nom[:1], H, 4, act)
    xn = dev.plant_linearize(x_nom[:1], tau_nom[:1], H, 4)[0]
    dev.close()
    assert r.status.tolist() == [[0, S * 4]]
    assert np.all(r.dx[0, 0] == 0.0) and _same(r.u[0, 0], tau_nom[0][act]) and _same(r.x[0, 0], xn[0])


def test_quaternion_sign():
    """free_body: x0 with the quaternion negated is the same rotation - d.w < 0 in tangent_sub, the short way round: row 0 of u
    and dx are the un-negated rollout's"""
    name, S = "free_body", 2
    x_nom, tau_nom, K, x0, act = tc.inputs(name, S, 1)
    assert len(act) == 6
    neg = x0.copy()
    neg[:, :4] = -neg[:, :4]
    r = _track(name, x_nom, tau_nom, K, np.vstack([x0, neg]), act)
    assert r.status.tolist() == [[0, S * M]] * 2
    assert np.abs(r.dx[0, 0, :3]).max() > 1e-4
    assert _same(r.u[0, 0], r.u[1, 0]) and _same(r.dx[0, 0], r.dx[1, 0])


def _hopper_variant(scale):
    base, sp = load_model("hopper"), lc.case("hopper")[3]
    m, p = copy.deepcopy(base), copy.deepcopy(sp)
    m.mass = np.asarray(m.mass) * scale
    m.inertia = np.asarray(m.inertia) * scale
    p.contact_stiffness *= 0.5
    p.friction_coefficient = 0.2
    return m.normalize(), p


def test_a_batch_the_models_and_the_rollouts_of_a_problem():
    """two hoppers with inputs of their own, problem 1 heavier on a softer, more slippery ground - through set_model_batch and,
    with SCENE_MODELS_PLANTS, through plant_set_model: problem b == a context built with model b; R = 3 rollouts of one problem
    == three calls with R = 1"""
    name, S, R = "hopper", 2, 3
    ins = [tc.inputs(name, S, R, seed=s) for s in (1, 2)]
    act = ins[0][4]
    stack = lambda k: np.array([i[k] for i in ins])
    base, sp = lc.case(name)[0], lc.case(name)[3]
    heavy, sp_h = _hopper_variant(1.3)
    solo = [_track(name, *ins[b][:4], act, model=mdl, sp=p) for b, (mdl, p) in enumerate([(base, sp), (heavy, sp_h)])]
    on_base = _track(name, *ins[1][:4], act)
    assert not _same(solo[1].x, on_base.x)
    dev = _context(name, B=2)
    dev.set_model_batch(1, heavy, sp_h)
    r = dev.plant_track(stack(0), stack(1), stack(2), stack(3), H, M, act)
    dev.close()
    assert r.x.shape == (2, R, S, base.nq + base.nv) and r.status.tolist() == [[[0, S * M]] * R] * 2
    for b in range(2):
        assert _same(r.x[b], solo[b].x) and _same(r.u[b], solo[b].u) and _same(r.dx[b], solo[b].dx), b
    dev = _context(name, B=2)
    with pytest.raises(hip.HipError, match="plant_track: the plants' models were asked for: call idto_hip_plant_begin"):
        dev.plant_track(stack(0), stack(1), stack(2), stack(3), H, M, act, models=hip.SCENE_MODELS_PLANTS)
    dev.plant_begin(H)
    dev.plant_set_model(1, heavy, sp_h)
    dev.plant_set_state(0.5, stack(0)[:, 0])
    plants = dev.plant_track(stack(0), stack(1), stack(2), stack(3), H, M, act, models=hip.SCENE_MODELS_PLANTS)
    problems = dev.plant_track(stack(0), stack(1), stack(2), stack(3), H, M, act)
    times, x_now = dev.plant_get_state()
    dev.close()
    assert _same(times, [0.5, 0.5]) and _same(x_now, stack(0)[:, 0])   # (the plants' states are untouched)
    assert _same(plants.x[0], solo[0].x) and _same(plants.x[1], solo[1].x) and _same(plants.u[1], solo[1].u)
    assert _same(problems.x[0], solo[0].x) and _same(problems.x[1], on_base.x)
    dev = _context(name)
    for k in range(R):
        one = dev.plant_track(*ins[0][:3], ins[0][3][k:k + 1], H, M, act)
        assert _same(one.x[0], solo[0].x[k]) and _same(one.u[0], solo[0].u[k]) and _same(one.dx[0], solo[0].dx[k]), k
    dev.close()


def test_status_words():
    """a NaN in K_1 of problem 1 ends its rollouts with {2, m}: u and x NaN from row 1 on, dx from row 2 on (row 1 is finite: the
    state is) - problem 0 is what it is alone; a velocity of 1e200 in one rollout's x0 ends that rollout with code 2, the other
    is what it is alone; a pendulum without mass or inertia ends with code 1 (the pivot) at substep 0"""
    name, S, R = "acrobot", 3, 2
    x_nom, tau_nom, K, x0, act = tc.inputs(name, S, R)
    bad_K = K.copy()
    bad_K[1, 0, 2] = np.nan
    alone = _track(name, x_nom, tau_nom, K, x0, act)
    dev = _context(name, B=2)
    r = dev.plant_track([x_nom] * 2, [tau_nom] * 2, [K, bad_K], [x0] * 2, H, M, act)
    dev.close()
    assert r.status[0].tolist() == [[0, S * M]] * R and r.status[1].tolist() == [[2, M]] * R
    assert _same(r.x[0], alone.x) and _same(r.u[0], alone.u) and _same(r.dx[0], alone.dx)
    assert _same(r.x[1, :, 0], alone.x[:, 0]) and _same(r.u[1, :, 0], alone.u[:, 0]) and _same(r.dx[1, :, :2], alone.dx[:, :2])
    assert np.isnan(r.x[1, :, 1:]).all() and np.isnan(r.u[1, :, 1:]).all() and np.isnan(r.dx[1, :, 2:]).all()
    assert np.isfinite(r.dx[1, :, 1]).all()
    fast = x0.copy()
    fast[1, -1] = 1e200
    r = _track(name, x_nom, tau_nom, K, fast, act)
    assert r.status[0].tolist() == [0, S * M] and r.status[1, 0] == 2 and r.status[1, 1] < M
    assert _same(r.x[0], alone.x[0]) and _same(r.dx[0], alone.dx[0]) and np.isnan(r.x[1]).all()
    pend = copy.deepcopy(load_model("pendulum"))
    pend.mass = np.zeros_like(np.asarray(pend.mass, dtype=float))
    pend.inertia = np.zeros_like(np.asarray(pend.inertia, dtype=float))
    x_nom, tau_nom, K, x0, act = tc.inputs("pendulum", S, 1)
    r = _track("pendulum", x_nom, tau_nom, K, x0, act, model=pend.normalize())
    assert r.status.tolist() == [[1, 0]]
    assert np.isnan(r.x).all() and np.isnan(r.u).all() and np.isfinite(r.dx[0, 0]).all() and np.isnan(r.dx[0, 1:]).all()


def test_gains_and_rollouts_in_one_pass():
    """plant_tvlqr_track == plant_tvlqr about the first S states, then plant_track with the K it returned"""
    name, S, R = "hopper", 3, 2
    x_nom, tau_nom, _, x0, act = tc.inputs(name, S, R)
    Q, Rw, Qf = tc.weights(lc.case(name)[0].nv, len(act), 5)
    dev = _context(name)
    both = dev.plant_tvlqr_track(x_nom, tau_nom, x0, H, 4, act, Q, Rw, Qf)
    gains = dev.plant_tvlqr(x_nom[:S], tau_nom, H, 4, act, Q, Rw, Qf)
    then = dev.plant_track(x_nom, tau_nom, gains.K, x0, H, 4, act)
    dev.close()
    assert gains.status.tolist() == [0] and both.tvlqr.status.tolist() == [0] and both.status.tolist() == [[0, S * 4]] * R
    for k in ("x_next", "A", "B", "K", "P"):
        assert _same(getattr(both.tvlqr, k), getattr(gains, k)), k
    assert _same_track(both, then)
    assert np.abs(then.u - tau_nom[None][:, :, act]).max() > 0.0   # (the law acts)


def _consumer():
    exe, src = os.path.join(ROOT, "build", "track_pendulum"), os.path.join(ROOT, "tests", "cpp", "track_pendulum.cc")
    deps = [src] + [os.path.join(ROOT, "idto_amd", n) for n in ("libidto_hip.so", "libidto_opt.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L" + os.path.join(ROOT, "idto_amd"), "-lidto_opt", "-lidto_hip", "-Wl,-rpath,$ORIGIN/../idto_amd"], check=True)
    return exe


def _rows(out, name, count):
    rows = {int(t): [float(x) for x in rest.split()] for t, rest in re.findall(rf"^{name} (\d+) (.*)$", out, re.M)}
    assert sorted(rows) == list(range(count)), (name, sorted(rows))
    return np.array([rows[t] for t in range(count)])


def test_the_optimizer_route_equals_the_device_call_on_the_solutions_states():
    """TrajectoryOptimizer.track(solution, ...) for the hopper at N = 5 == HipPath.plant_tvlqr_track on (q_t, v_t), t <= N, and
    tau_t with substeps = time_step / h, the block-diagonal weights and the model's actuated dofs; zero_unactuated zeroes the
    nominal torque off them.  h is the example's sim_time_step, 50 substeps a step: the step at which its stiff ground is
    simulated (at time_step / 4 the rollouts of this solution, in contact, end with a failed pivot after four steps)"""
    name, N, SUB = "hopper", 5, 50
    cfg, model = load_config(name), load_model(name)
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.max_iterations, sp.verbose = 3, False
    opt = optimizer.TrajectoryOptimizer(model, prob, sp)
    sol, stats = optimizer.TrajectoryOptimizerSolution(), optimizer.TrajectoryOptimizerStats()
    opt.Solve(q_guess, sol, stats)
    nv, act = model.nv, opt.actuated_dofs()
    Q, Rw, Qf = tc.weights(nv, len(act), 8)
    Qf[:nv, nv:] = Qf[nv:, :nv] = 0.0
    h = prob.time_step / SUB
    assert h == float(cfg["sim_time_step"])
    x = np.hstack([sol.q, sol.v])
    rng = np.random.default_rng(3)
    x0 = np.array([tc.tangent_add(model, x[0], rng.uniform(-1e-3, 1e-3, 2 * nv)) for _ in range(2)])
    blocks = (Q[:nv, :nv], Q[nv:, nv:], Rw, Qf[:nv, :nv], Qf[nv:, nv:])
    r = opt.track(sol, h, *blocks, x0)
    rz = opt.track(sol, h, *blocks, x0, zero_unactuated=True)
    with pytest.raises(RuntimeError, match="is not a whole number of substeps"):
        opt.track(sol, prob.time_step / 4.5, *blocks, x0)
    opt.close()
    dev = hip.HipPath(model, prob, sp)
    d = dev.plant_tvlqr_track(x, sol.tau, x0, h, SUB, act, Q, Rw, Qf)
    tau_z = np.array(sol.tau)
    tau_z[:, [j for j in range(nv) if j not in act.tolist()]] = 0.0
    dz = dev.plant_tvlqr_track(x, tau_z, x0, h, SUB, act, Q, Rw, Qf)
    dev.close()
    print("status of the rollouts:", d.status.tolist(), "with zero_unactuated:", dz.status.tolist())
    assert d.status.tolist() == [[0, N * SUB]] * 2 and d.tvlqr.status.tolist() == [0]
    assert _same_track(r, d) and _same(r.tvlqr.K, d.tvlqr.K) and _same(r.tvlqr.P, d.tvlqr.P[0]) and _same(r.tvlqr.A, d.tvlqr.A)
    assert _same_track(rz, dz) and _same(rz.tvlqr.K, dz.tvlqr.K) and not _same(rz.x, r.x)


def test_cpp_consumer_gets_the_rollouts_of_the_python_route():
    """tests/cpp/track_pendulum.cc, no Python in its process: what it prints with 17 significant digits is what
    HipPath.plant_tvlqr_track gives on the printed states, torques, weights and initial states"""
    N, dt, R = 5, 0.05, 2
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    p = subprocess.run([_consumer(), os.path.join(ROOT, "idto_amd", "models", "pendulum.model")], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout
    assert re.search(r"^actuated 0$", out, re.M) and re.search(r"^lqr_status 0 lin_ok 1 track_ok 1$", out, re.M), out[:400]
    assert re.search(r"^tvlqr_same 1$", out, re.M)
    assert re.search(r"^refused 1 Tvlqr: time_step / h = .* is not a whole number of substeps$", out, re.M), out[-400:]
    assert re.findall(r"^status (\d+) (\d+) (\d+)$", out, re.M) == [("0", "0", "20"), ("1", "0", "20")]
    q, v, tau, x0 = _rows(out, "q", N + 1), _rows(out, "v", N + 1), _rows(out, "tau", N), _rows(out, "x0", R)
    model = load_model("pendulum")
    prob = ProblemDefinition(num_steps=N, q_init=q[0], v_init=v[0], Qq=np.eye(1), Qv=np.eye(1), Qf_q=np.eye(1), Qf_v=np.eye(1),
                             R=np.eye(1), q_nom=np.tile(q[0], (N + 1, 1)), v_nom=np.zeros((N + 1, 1)), time_step=dt)
    dev = hip.HipPath(model, prob, SolverParameters(verbose=False, scaling=False, equality_constraints=False))
    r = dev.plant_tvlqr_track(np.hstack([q, v]), tau, x0, dt / 4, 4, [0], np.diag([10.0, 1]), np.diag([0.1]), np.diag([100.0, 10]))
    dev.close()
    assert r.status.tolist() == [[0, 20]] * R
    assert _same(r.tvlqr.K.reshape(N, 2), _rows(out, "K", N))
    assert _same(r.x.reshape(R * N, 2), _rows(out, "x", R * N)) and _same(r.u.reshape(R * N, 1), _rows(out, "u", R * N))
    assert _same(r.dx.reshape(R * (N + 1), 2), _rows(out, "dx", R * (N + 1)))


def test_refusals_by_name_leave_the_context_usable():
    name, S, R = "acrobot", 3, 2
    x_nom, tau_nom, K, x0, act = tc.inputs(name, S, R)
    dev = _context(name)
    good = dev.plant_track(x_nom, tau_nom, K, x0, H, M, act)
    w, nv = dev.nq + dev.nv, dev.nv
    call = lambda **kw: dev.plant_track(kw.pop("x_nom", x_nom), kw.pop("tau_nom", tau_nom), kw.pop("K", K), kw.pop("x0", x0), kw.pop("h", H),
                                        kw.pop("m", M), kw.pop("act", act), **kw)
    nan_x, inf_tau, nan_x0 = x_nom.copy(), tau_nom.copy(), x0.copy()
    nan_x[S, 1], inf_tau[1, 0], nan_x0[1, 2] = np.nan, np.inf, np.nan
    many = 65537
    refused = [
        ("x_nom is not finite at index %d" % (S * w + 1), lambda: call(x_nom=nan_x)),
        ("tau_nom is not finite at index %d" % nv, lambda: call(tau_nom=inf_tau)),
        ("x0 is not finite at index %d" % (w + 2), lambda: call(x0=nan_x0)),
        ("nsteps must be >= 1", lambda: call(x_nom=x_nom[:1], tau_nom=np.zeros((0, nv)), K=np.zeros((0, len(act), 2 * nv)))),
        ("nrollouts must be >= 1", lambda: call(x0=np.zeros((0, w)))),
        ("rollouts, more than 65536 in one call", lambda: call(x0=np.tile(x0[:1], (many, 1)))),
        (r"substeps must be in \[1, 4096\]", lambda: call(m=0)),
        (r"substeps must be in \[1, 4096\]", lambda: call(m=4097)),
        (r"max_launch_substeps is 0 or in \[substeps, 4096\]", lambda: call(max_launch_substeps=M - 1)),
        (r"max_launch_substeps is 0 or in \[substeps, 4096\]", lambda: call(max_launch_substeps=4097)),
        ("the substep h must be > 0 and finite", lambda: call(h=0.0)),
        ("the substep h must be > 0 and finite", lambda: call(h=np.inf)),
        (r"nu must be in \[1, nv\]", lambda: call(act=[0, 1, 1], K=np.zeros((S, 3, 2 * nv)))),
        (r"actuated\[0\] is not a velocity index", lambda: call(act=[2])),
        ("models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS", lambda: call(models=7)),
        ("the plants' models were asked for", lambda: call(models=hip.SCENE_MODELS_PLANTS)),
    ]
    for text, refusal in refused:
        with pytest.raises(hip.HipError, match="plant_track: .*" + text):
            refusal()
        assert _same_track(dev.plant_track(x_nom, tau_nom, K, x0, H, M, act), good), text
    Q, Rw, Qf = tc.weights(nv, len(act), 7)
    for text, kw in (("eps must be > 0 and finite", dict(eps=0.0)), (r"max_launch_substeps is 0 or in \[substeps, 4096\]", dict(max_launch_substeps=1)),
                     ("Q is not finite at index 0", dict(Q=np.full_like(Q, np.nan)))):
        with pytest.raises(hip.HipError, match="plant_tvlqr_track: .*" + text):
            dev.plant_tvlqr_track(x_nom, tau_nom, x0, H, M, act, kw.pop("Q", Q), Rw, Qf, **kw)
        assert _same_track(dev.plant_track(x_nom, tau_nom, K, x0, H, M, act), good), text
    dev.close()


def test_the_gains_hold_the_upright_pendulum_and_nothing_else_does():
    """The numbers are right, not merely equal: the pendulum about its upright equilibrium x* = (pi, 0), tau* = 0, gains from
    plant_tvlqr with Q = I, R = 0.1, Qf = 100 I, x0 offset by 1e-3 in angle, m = 50 substeps of 1 ms a step.  With the gains
    |dx_S| <= 0.5 |dx_0|; with K = 0 the deviation grows, |dx_S| >= 2 |dx_0|.
    The host composition (lin_cases.host_linearize, lin_cases.tvlqr, lin_cases.control, plant_cases.host_rollout), evaluated on the
    CPU before this test was written, gives at S = 10 the ratios 0.367 and 18.7: the first margin is 1.4, under 4, so the horizon
    is S = 24 (1200 substeps, a launch holds 81 steps: one launch), where the host composition gives
        |dx_S| / |dx_0| = 0.1008 with the gains (margin 4.96) and 365.8 with K = 0 (margin 183)."""
    S, m = 24, 50
    xs = np.array([np.pi, 0.0])
    x_nom, tau_nom = np.tile(xs, (S + 1, 1)), np.zeros((S, 1))
    x0 = np.array([[np.pi + 1e-3, 0.0]])
    dev = _context("pendulum")
    held = dev.plant_tvlqr_track(x_nom, tau_nom, x0, H, m, [0], np.eye(2), 0.1 * np.eye(1), 100.0 * np.eye(2))
    free = dev.plant_track(x_nom, tau_nom, np.zeros((S, 1, 2)), x0, H, m, [0])
    dev.close()
    assert held.status.tolist() == [[0, S * m]] and free.status.tolist() == [[0, S * m]] and held.tvlqr.status.tolist() == [0]
    norm = lambda r, t: float(np.linalg.norm(r.dx[0, t]))
    print(f"|dx_S| / |dx_0|: {norm(held, S) / norm(held, 0):.4f} with the gains, {norm(free, S) / norm(free, 0):.2f} with K = 0")
    assert abs(norm(held, 0) - 1e-3) < 1e-15 and np.all(free.u == 0.0)
    assert norm(held, S) <= 0.5 * norm(held, 0)
    assert norm(free, S) >= 2.0 * norm(free, 0)
