"""The time-varying LQR gains on the device (include/idto_hip.h idto_hip_plant_tvlqr; csrc/plant_lin.h tvlqr_kernel,
csrc/tvlqr_step.h) and the optimizer's route to them (TrajectoryOptimizer.tvlqr).

The bar is == : tvlqr_kernel's arithmetic is csrc/tvlqr_step.h, the text that tests/cpp/lin_host.cc compiles for the host, an
entry of a product one lane's left-to-right sum - so K and P equal the host program's on the A and B that the same call
returned, and those equal plant_linearize's.  That the recursion's numbers are right, and not merely the same on both sides,
is tests/test_tvlqr_step.py's (the numpy restatement, the cost-to-go identity).  S = 3 states (mini_cheetah: 2), 4 substeps.
"""
import numpy as np
import pytest

import lin_cases as lc
from idto_amd import hip, optimizer
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem

pytestmark = pytest.mark.gpu

H, SUB = 1e-3, 4


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def _weights(nv, nu, seed):
    """symmetric positive definite Q, Qf [n, n] (Q block diagonal as TrajectoryOptimizer.tvlqr builds it, Qf dense) and R [nu, nu]"""
    rng = np.random.default_rng(seed)

    def spd(m, scale):
        M = rng.uniform(-1, 1, (m, m))
        return scale * (M @ M.T / m + np.eye(m))
    Q = np.zeros((2 * nv, 2 * nv))
    Q[:nv, :nv], Q[nv:, nv:] = spd(nv, 10.0), spd(nv, 1.0)
    return Q, spd(nu, 0.1), spd(2 * nv, 100.0)


def _actuated(name):
    model = lc.case(name)[0]
    act = np.flatnonzero(np.asarray(model.actuated))
    return act if len(act) else np.arange(model.nv)   # (free_body has no actuator: every dof, nu = 6)


@pytest.mark.parametrize("name,S", [("acrobot", 3), ("hopper", 3), ("free_body", 3), ("mini_cheetah", 2)])
def test_gains_equal_the_host_recursion_on_the_calls_own_linearisation(name, S):
    x, tau = lc.inputs(name, S)
    act = _actuated(name)
    nv, nu = lc.case(name)[0].nv, len(act)
    assert (name, nu, nv) in (("acrobot", 1, 2), ("hopper", 2, 5), ("free_body", 6, 6), ("mini_cheetah", 12, 18))
    Q, R, Qf = _weights(nv, nu, 5)
    dev = hip.HipPath(lc.case(name)[0], lc.case(name)[2], lc.case(name)[3])
    r = dev.plant_tvlqr(x, tau, H, SUB, act, Q, R, Qf)
    xn, A, B, status = dev.plant_linearize(x, tau, H, SUB)
    dev.close()
    assert r.status.tolist() == [0] and r.lin_status.tolist() == [[0, 0]] * S and status.tolist() == [[0, 0]] * S
    assert _same(r.A, A) and _same(r.B, B) and _same(r.x_next, xn)
    st, K, P = lc.tvlqr(lc.built(), r.A, r.B, act, Q, R, Qf)
    for what, got, ref in (("K", r.K, K), ("P", r.P[0], P)):
        d = np.abs(got - ref)
        print(f"{name} {what}: {int((got != ref).sum())} of {d.size} entries differ, the largest by {d.max():.3e} (largest entry {np.abs(ref).max():.3e})")
    assert st == 0 and _same(r.K, K) and _same(r.P[0], P)
    assert _same(r.P[0, S], Qf)
    for t in range(S + 1):
        assert _same(r.P[0, t], r.P[0, t].T), t


def test_a_batch_and_a_failed_state():
    """two acrobots; state 1 of problem 1 overflows: its linearisation is NaN and the recursion of problem 1 ends at t = 1 -
    status 1 + 1, K and P NaN from there down, P_2 and K_2 as without it; problem 0 is what it is alone"""
    name, S = "acrobot", 3
    x, tau = lc.inputs(name, S)
    act = _actuated(name)
    Q, R, Qf = _weights(2, 1, 6)
    bad = x.copy()
    bad[1, -1] = 1e200
    model, prob, sp = lc.case(name)[0], lc.case(name)[2], lc.case(name)[3]
    dev = hip.HipPath(model, [prob, prob], sp)
    r = dev.plant_tvlqr(np.array([x, bad]), np.array([tau, tau]), H, SUB, act, Q, R, Qf)
    dev.close()
    solo = hip.HipPath(model, prob, sp)
    r0 = solo.plant_tvlqr(x, tau, H, SUB, act, Q, R, Qf)
    solo.close()
    assert r.status.tolist() == [0, 2] and r.lin_status[1].tolist() == [[0, 0], [2, 0], [0, 0]]
    assert _same(r.K[0], r0.K) and _same(r.P[0], r0.P[0]) and _same(r.A[0], r0.A)
    assert np.isnan(r.K[1, :2]).all() and np.isnan(r.P[1, :2]).all()
    assert _same(r.K[1, 2], r0.K[2]) and _same(r.P[1, 2:], r0.P[0, 2:])


def test_refusals_by_name_leave_the_context_usable():
    name, S = "acrobot", 3
    x, tau = lc.inputs(name, S)
    act = _actuated(name)
    Q, R, Qf = _weights(2, 1, 7)
    dev = hip.HipPath(lc.case(name)[0], lc.case(name)[2], lc.case(name)[3])
    good = dev.plant_tvlqr(x, tau, H, SUB, act, Q, R, Qf)
    nanQ = Q.copy()
    nanQ[0, 0] = np.nan
    refused = [
        ("Q is not finite at index 0", lambda: dev.plant_tvlqr(x, tau, H, SUB, act, nanQ, R, Qf)),
        ("R is not finite", lambda: dev.plant_tvlqr(x, tau, H, SUB, act, Q, np.full((1, 1), np.inf), Qf)),
        (r"actuated\[0\] is not a velocity index", lambda: dev.plant_tvlqr(x, tau, H, SUB, [2], Q, R, Qf)),
        (r"nu must be in \[1, nv\]", lambda: dev.plant_tvlqr(x, tau, H, SUB, [0, 1, 1], Q, np.eye(3), Qf)),
        ("eps must be > 0 and finite", lambda: dev.plant_tvlqr(x, tau, H, SUB, act, Q, R, Qf, eps=-1.0)),
        (r"substeps must be in \[1, 4096\]", lambda: dev.plant_tvlqr(x, tau, H, 0, act, Q, R, Qf)),
    ]
    for text, call in refused:
        with pytest.raises(hip.HipError, match="plant_tvlqr: .*" + text):
            call()
        again = dev.plant_tvlqr(x, tau, H, SUB, act, Q, R, Qf)
        assert _same(again.K, good.K) and _same(again.P, good.P), text
    dev.close()


def test_the_optimizer_route_equals_the_device_call_on_the_solutions_states():
    """TrajectoryOptimizer.tvlqr(solution, ...) for the hopper at N = 5 == HipPath.plant_tvlqr on (q_t, v_t, tau_t), t < N, with
    substeps = time_step / h, Q = blkdiag(Qtheta, Qv), Qf = blkdiag(Qf_theta, Qf_v) and the model's actuated dofs"""
    name, N = "hopper", 5
    cfg, model = load_config(name), load_model(name)
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.max_iterations, sp.verbose = 3, False
    opt = optimizer.TrajectoryOptimizer(model, prob, sp)
    sol, stats = optimizer.TrajectoryOptimizerSolution(), optimizer.TrajectoryOptimizerStats()
    opt.Solve(q_guess, sol, stats)
    nv = model.nv
    act = opt.actuated_dofs()
    assert act.tolist() == np.flatnonzero(np.asarray(model.actuated)).tolist()
    Q, R, Qf = _weights(nv, len(act), 8)
    Qf[:nv, nv:] = Qf[nv:, :nv] = 0.0
    h = prob.time_step / SUB
    r = opt.tvlqr(sol, h, Q[:nv, :nv], Q[nv:, nv:], R, Qf[:nv, :nv], Qf[nv:, nv:])
    with pytest.raises(RuntimeError, match="is not a whole number of substeps"):
        opt.tvlqr(sol, prob.time_step / 4.5, Q[:nv, :nv], Q[nv:, nv:], R, Qf[:nv, :nv], Qf[nv:, nv:])
    xn, A, B, st = opt.linearize_plant(sol.q[:N], sol.v[:N], sol.tau, h, SUB)
    opt.close()
    assert r.status.tolist() == [0] and r.lin_status.tolist() == [[0, 0]] * N
    x = np.hstack([sol.q[:N], sol.v[:N]])
    dev = hip.HipPath(model, prob, sp)
    d = dev.plant_tvlqr(x, sol.tau, h, SUB, act, Q, R, Qf)
    dev.close()
    assert _same(r.A, d.A) and _same(r.B, d.B) and _same(r.x_next, d.x_next)
    assert _same(r.K, d.K) and _same(r.P, d.P[0])
    assert _same(A, d.A) and _same(B, d.B) and _same(xn, d.x_next) and st.tolist() == [[0, 0]] * N
