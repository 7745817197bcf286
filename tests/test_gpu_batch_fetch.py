"""idto_hip_tr_solve_batch_fetch: the batch's trust-region loop that brings every problem's rows, radius, cost, status and
trajectories back under ONE wait and chooses the best problem on the device (trust_region.h tr_gather_batch_kernel).
Everything it returns must == what idto_hip_tr_solve_batch(_constrained) + idto_hip_get_batch return on a second batch
context with the same inputs; column 10 of the rows (the device clock) is left out of every comparison."""
import copy

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.problem import SCALING
from oracle_lib import Oracle
from test_dense_weights import balanced_dense_problem
from test_gpu_batch import _problems, _same

pytestmark = pytest.mark.gpu

COLS = [c for c in range(17) if c != 10]
TRAJ = ("q", "v", "tau", "dq", "w")
N, B = 20, 3
SM = SCALING["double_sqrt"]
# name -> (iterations, constraints enforced)
CASES = {"hopper": (6, True), "mini_cheetah": (4, False)}
ELIGIBLE_MASK = 1 | 2 | 4 | 8 | 32


def _rejecting_radius(model, prob, sp, q, iters, constrained):
    """a radius with which the CPU oracle's solve of this problem ENDS on a rejected step (trust ratio well below the
    threshold 0, so that the device's round-off cannot turn it into an acceptance)"""
    for Delta0 in (10.0, 0.5, 100.0, 30.0, 5.0, 2.0, 1.0, 1e3):
        s = copy.deepcopy(sp)
        s.method, s.scaling, s.scaling_method, s.equality_constraints = "trust_region", True, "double_sqrt", constrained
        s.check_convergence, s.max_iterations, s.Delta0 = False, iters, Delta0
        rho = Oracle(model, prob, s).solve(q)["stats"].trust_ratios
        if len(rho) == iters and rho[-1] < -0.5:
            return Delta0
    return None


def _expected_best(final_cost, status):
    ok = [b for b in range(len(status)) if (status[b] & ELIGIBLE_MASK) == 0 and np.isfinite(final_cost[b])]
    if not ok:
        return -1
    lowest = min(final_cost[b] for b in ok)
    return min(b for b in ok if final_cost[b] == lowest)   # (numpy's argmin with the lowest index among equals)


def _run_parent_route(model, probs, sp, qs, d0, iters, dofs):
    bd = hip.HipPath(model, probs, sp)
    bd.set_q_batch(qs)
    bd.eval_tau()
    if dofs:
        rows, delta = bd.tr_solve_batch_constrained(iters, SM, True, False, d0, 1e5, dofs)
    else:
        rows, delta = bd.tr_solve_batch(iters, SM, True, False, d0, 1e5)
    out = dict(rows=rows, delta=delta)
    for k in ("q", "v", "tau", "tr_dq", "tr_w"):
        out[k.replace("tr_", "")] = np.array([bd.get(k, problem=b) for b in range(B)])
    bd.close()
    return out


def _run_fetch(model, probs, sp, qs, d0, iters, dofs, **kw):
    bd = hip.HipPath(model, probs, sp)
    bd.set_q_batch(qs)
    bd.eval_tau()
    return bd, bd.tr_solve_batch_fetch(iters, SM, True, False, d0, 1e5, constrained_dofs=dofs, **kw)


@pytest.fixture(scope="module")
def cases():
    """per case: the inputs, the parent route's results and the fetch call's (computed once, never modified)"""
    out = {}
    for name, (iters, constrained) in CASES.items():
        model, probs, sp, qs = _problems(name, N, B)
        dofs = list(model.unactuated_dofs) if constrained else []
        assert bool(dofs) == constrained
        d0 = np.array([1e-1 * (1 + 0.5 * b) for b in range(B)])
        if name == "hopper":   # (problem 0 is to end on a rejected step)
            Delta0 = _rejecting_radius(model, probs[0], sp, qs[0], iters, constrained)
            assert Delta0 is not None, "no radius makes the oracle end on a rejected step: the case tests nothing"
            d0[0] = Delta0
        want = _run_parent_route(model, probs, sp, qs, d0, iters, dofs)
        ctx, got = _run_fetch(model, probs, sp, qs, d0, iters, dofs)
        out[name] = dict(model=model, probs=probs, sp=sp, qs=qs, d0=d0, iters=iters, dofs=dofs, want=want, got=got, ctx=ctx)
    yield out
    for c in out.values():
        c["ctx"].close()


def test_the_cases_end_on_an_accepted_and_on_a_rejected_step(cases):
    last = np.concatenate([c["want"]["rows"][:, -1, 9] for c in cases.values()])
    assert (last != 0.0).any() and (last == 0.0).any(), ("the case tests nothing: last steps accepted", last)
    for c in cases.values():
        assert c["want"]["rows"][:, :, 9].sum() > 0


@pytest.mark.parametrize("name", list(CASES))
def test_fetch_equals_solve_batch_and_get_batch(cases, name):
    c = cases[name]
    want, got = c["want"], c["got"]
    assert got["rc"] == 0
    assert np.array_equal(got["rows"][:, :, COLS], want["rows"][:, :, COLS])
    assert np.array_equal(got["delta"], want["delta"])
    for k in TRAJ:
        assert _same(got[k].reshape(B, -1), want[k].reshape(B, -1)), k
    if c["dofs"]:
        assert np.all(np.isfinite(want["rows"][:, :, 8])) and np.all(want["rows"][:, 0, 8] > 0.0)   # |h|: the constraints ran


@pytest.mark.parametrize("name", list(CASES))
def test_costs_statuses_and_the_best_problem(cases, name):
    got = cases[name]["got"]
    rows = got["rows"]
    for b in range(B):
        last = rows[b, -1]
        assert got["final_cost"][b] == (last[13] if last[9] != 0.0 else last[0]), b
        assert got["status"][b] == np.bitwise_or.reduce(rows[b, :, 14].astype(np.int64)), b
    assert got["best"] == _expected_best(got["final_cost"], got["status"])
    assert 0 <= got["best"] < B


@pytest.mark.parametrize("name", list(CASES))
def test_only_best_brings_the_best_problems_block_and_every_row(cases, name):
    c = cases[name]
    full = c["got"]
    ctx, got = _run_fetch(c["model"], c["probs"], c["sp"], c["qs"], c["d0"], c["iters"], c["dofs"], only_best=True)
    ctx.close()
    assert got["best"] == full["best"]
    for k in TRAJ:
        assert got[k].shape[0] == 1 and _same(got[k][0], full[k][full["best"]]), k
    assert np.array_equal(got["rows"][:, :, COLS], full["rows"][:, :, COLS])
    assert np.array_equal(got["delta"], full["delta"])
    assert np.array_equal(got["final_cost"], full["final_cost"]) and np.array_equal(got["status"], full["status"])


@pytest.mark.parametrize("name", list(CASES))
def test_the_context_is_usable_afterwards(cases, name):
    """a Gauss-Newton step of the batch from the final iterates == the single contexts' (as tests/test_gpu_batch.py checks
    for idto_hip_tr_solve_batch)"""
    c = cases[name]
    bd = c["ctx"]
    for b in range(B):   # (the iterates are resident: what the fetch brought back is what idto_hip_get_batch reads)
        for k in ("q", "v", "tau"):
            assert _same(bd.get(k, problem=b), c["got"][k][b]), (b, k)
    bd.gn_step()
    for b in range(B):
        dev = hip.HipPath(c["model"], c["probs"][b], c["sp"])
        dev.set_q(c["got"]["q"][b])
        dev.gn_step()
        assert _same(bd.get("step", problem=b), dev.get("step")), b
        dev.close()


def test_a_failed_factorisation_is_that_problems_own():
    """hopper, unconstrained: problem 1 gets a Hessian with exactly zero rows (zero weight on DoF 0, R = 0: the way
    tests/test_gpu_status.py makes one).  Its status carries bit 32 and it cannot be the best; the others come out as in
    the healthy batch; the call reports IDTO_HIP_FACTORIZATION_FAILED with every output filled."""
    model, probs, sp, qs = _problems("hopper", N, B)
    d0 = np.array([1e-1 * (1 + 0.5 * b) for b in range(B)])
    iters = 4
    ctx, good = _run_fetch(model, probs, sp, qs, d0, iters, [])
    ctx.close()
    assert good["rc"] == 0 and not (good["status"] & 32).any()
    bad = copy.deepcopy(probs[1])
    for W in (bad.Qq, bad.Qv, bad.Qf_q, bad.Qf_v):
        W[0, :] = 0.0
        W[:, 0] = 0.0
    bad.R[:] = 0.0
    ctx, got = _run_fetch(model, [probs[0], bad, probs[2]], sp, qs, d0, iters, [], check=False)
    ctx.close()
    assert got["rc"] == hip.FACTORIZATION_FAILED
    assert [bool(s & 32) for s in got["status"]] == [False, True, False]
    assert got["best"] in (0, 2) and got["best"] == _expected_best(got["final_cost"], got["status"])
    for b in (0, 2):
        assert np.array_equal(got["rows"][b][:, COLS], good["rows"][b][:, COLS]), b
        assert got["delta"][b] == good["delta"][b] and got["final_cost"][b] == good["final_cost"][b]
        for k in TRAJ:
            assert _same(got[k][b], good[k][b]), (b, k)


def test_a_context_of_one_equals_tr_solve_fetch():
    for name, (iters, constrained) in CASES.items():
        model, probs, sp, qs = _problems(name, N, B)
        dofs = list(model.unactuated_dofs) if constrained else []
        res = []
        for batch_form in (False, True):
            dev = hip.HipPath(model, probs[1], sp)
            dev.set_q(qs[1])
            dev.eval_tau()
            if batch_form:
                r = dev.tr_solve_batch_fetch(iters, SM, True, False, [0.15], 1e5, constrained_dofs=dofs)
                assert r["best"] == 0 and r["status"][0] == 0
                last = r["rows"][0, -1]
                assert r["final_cost"][0] == (last[13] if last[9] != 0.0 else last[0])
                res.append((r["rows"][0], r["delta"][0], {k: r[k][0] for k in TRAJ}))
            else:
                res.append(dev.tr_solve_fetch(iters, SM, True, False, 0.15, 1e5, constrained_dofs=dofs))
            dev.close()
        (r0, d0, t0), (r1, d1, t1) = res
        assert np.array_equal(r0[:, COLS], r1[:, COLS]) and d0 == d1
        for k in TRAJ:
            assert _same(t0[k], t1[k]), (name, k)


# name, N, constraints enforced, option con_kkt, dense cost weights
ROUTES = {"small launch": ("acrobot", 3, False, 1, False), "small launch, one constraint": ("acrobot", 3, True, 1, False),
          "kkt": ("hopper", 4, True, 1, False), "schur chain": ("hopper", 4, True, 0, False),
          "dense weights, no lookahead": ("hopper", 4, False, 1, True)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_tr_solve_fetch_equals_tr_solve_and_get_on_every_route(route):
    """the single-problem fetch against idto_hip_tr_solve + idto_hip_get, on the routes through the loop that the batch
    cases above do not take.  3 iterations whose accepted steps are odd in number: the iterate ends in the SECOND output set
    (TRS_CUR != 0), where a gather that reads the wrong set, or a wrong swap behind it, shows in v and tau"""
    name, n, constrained, kkt, dense = ROUTES[route]
    if dense:
        model, prob, sp, q = balanced_dense_problem(name, n)
    else:
        model, probs, sp, qs = _problems(name, n, 2)
        prob, q = probs[1], qs[1]
    dofs = list(model.unactuated_dofs) if constrained else []
    assert bool(dofs) == constrained
    res = []
    for fetch in (False, True):
        dev = hip.HipPath(model, prob, sp)
        dev.set_option("con_kkt", kkt)
        dev.set_q(q)
        dev.eval_tau()
        if fetch:
            res.append(dev.tr_solve_fetch(3, SM, True, False, 0.15, 1e5, constrained_dofs=dofs))
        else:
            rows, delta = dev.tr_solve(3, SM, True, False, 0.15, 1e5, constrained_dofs=dofs)
            res.append((rows, delta, {k.replace("tr_", ""): dev.get(k) for k in ("q", "v", "tau", "tr_dq", "tr_w")}))
        assert dev.solver_status() == (False, 0)
        dev.close()
    (r0, d0, t0), (r1, d1, t1) = res
    assert r0[:, 9].sum() % 2 == 1, ("the case tests nothing: the iterate ends in the first output set", r0[:, 9])
    assert np.array_equal(r0[:, COLS], r1[:, COLS]) and d0 == d1
    # (OPEN DEFECT, older than this test: without the two-set evaluation tr_decide still flips TRS_CUR on an accepted step and the
    # single-problem epilogue of idto_hip_tr_solve follows it, so idto_hip_get reads v and tau from a set that route never writes,
    # while the fetch reads the set that was written.  Until that is fixed the single-set arrays are what can be compared on this
    # route; then `dense` leaves this line and v, tau are compared like everywhere else.)
    for k in (("q", "dq", "w") if dense else TRAJ):
        assert _same(np.reshape(t0[k], t1[k].shape), t1[k]), (route, k)   # (idto_hip_get hands dq and w back flat)


def test_the_child_context_route_is_refused(monkeypatch):
    monkeypatch.setenv("IDTO_CON_KKT", "0")
    model, probs, sp, qs = _problems("hopper", N, B)
    bd = hip.HipPath(model, probs, sp)
    bd.set_q_batch(qs)
    with pytest.raises(hip.HipError, match=r"error -1: .*child-context route"):
        bd.tr_solve_batch_fetch(3, SM, True, False, [0.1] * B, 1e5, constrained_dofs=list(model.unactuated_dofs))
    bd.close()
