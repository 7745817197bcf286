"""TrajectoryOptimizer.solve_batch (TrajectoryOptimizer::SolveBatch through idto_opt_solve_batch): entry b of a batch is
Solve(q_guesses[b]) on an optimizer made with problems[b] - bit for bit where the batch and one problem alone run the same
solver kernels, to the solver's round-off where they do not (small models in a batch of more than two), and entry by entry
where the device's batch loop does not serve the configuration.  Times (iteration_times, solve_time) are left out."""
import copy

import numpy as np
import pytest

from idto_amd.model import load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory

pytestmark = pytest.mark.gpu

N, B = 20, 3
STATS = [f for f in TrajectoryOptimizerStats.FIELDS if f != "iteration_times"]
# tests/test_gpu_batch.py's tolerances of its converging cases: rel_cost_reduction, rel_state_change
CONVERGENCE = dict(rel_cost_reduction=1e-2, abs_cost_reduction=0.0, rel_gradient_along_dq=0.0, abs_gradient_along_dq=0.0,
                   rel_state_change=1e-3, abs_state_change=0.0)
# acrobot, N = 20, 6 iterations: max |q(Solve) - q(Solve under IDTO_SOLVER_BAND=0)| over the three problems below, i.e.
# what the scalar band factorisation and the block kernels differ by on one problem alone (measured on an MI355X with the
# single-problem Solve, which this batch call does not touch); the batch may differ from Solve by 10x that.
ACROBOT_Q_YARDSTICK = 1.007e-07
ACROBOT_Q_MARGIN = 10.0 * ACROBOT_Q_YARDSTICK


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _problems(name, num_steps=N, batch=B, max_iterations=None):
    """`batch` problems of the example with its YAML parameters: different nominal trajectories, initial velocities,
    weights and guesses (as tests/test_gpu_batch.py builds them)"""
    cfg, model = load_config(name), load_model(name)
    probs, qs, sp = [], [], None
    for b in range(batch):
        prob, sp, _ = make_problem(cfg, model, num_steps=num_steps)
        rng = np.random.default_rng(100 + b)
        prob.q_nom = prob.q_nom + 0.01 * b
        prob.v_init = prob.v_init + 0.05 * rng.normal(size=model.nv)
        prob.Qq = prob.Qq * (1.0 + 0.1 * b)
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, num_steps, seed=b, lower=0.01))
    sp.verbose = False
    if max_iterations is not None:
        sp.max_iterations = max_iterations
    return model, probs, sp, np.array(qs)


def _solve_alone(model, prob, sp, q):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q, sol, st)
    reason = opt.last_convergence_reason
    opt.close()
    return flag, sol, st, reason


def _assert_entry_equals(res, b, single, what=""):
    flag, sol, st, reason = single
    assert res.flags[b] == flag, (what, b, res.flags[b], flag, res.errors[b])
    assert res.convergence_reasons[b] == reason, (what, b)
    for f in STATS:
        assert _same(getattr(res.stats[b], f), getattr(st, f)), (what, b, f, getattr(res.stats[b], f), getattr(st, f))
    if flag in ("kSuccess", "kMaxIterationsReached"):
        assert res.errors[b] == "" and res.solutions[b] is not None, (what, b, res.errors[b])
        for k in ("q", "v", "tau"):
            assert _same(getattr(res.solutions[b], k), getattr(sol, k)), (what, b, k)
    else:
        assert res.solutions[b] is None and res.errors[b] != ""


def _expected_best(res):
    ok = [b for b in range(len(res.flags)) if res.flags[b] in ("kSuccess", "kMaxIterationsReached") and not res.errors[b]
          and np.isfinite(res.final_costs[b])]
    if not ok:
        return -1
    lowest = min(res.final_costs[b] for b in ok)
    return min(b for b in ok if res.final_costs[b] == lowest)


@pytest.mark.parametrize("name,iters", [("hopper", 6), ("mini_cheetah", 4)])
def test_every_entry_equals_its_single_solve(name, iters):
    model, probs, sp, qs = _problems(name, max_iterations=iters)
    singles = [_solve_alone(model, probs[b], sp, qs[b]) for b in range(B)]
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs)
    assert res.batch_route, "the device's batch loop did not take this configuration: the case tests nothing"
    for b in range(B):
        _assert_entry_equals(res, b, singles[b], name)
        assert len(res.stats[b].iteration_costs) == iters
    assert res.best == _expected_best(res) and 0 <= res.best < B
    # the final cost is the cost of the entry's solution (entry 0's problem is this optimizer's own)
    assert res.final_costs[0] == opt.eval(res.solutions[0].q)["cost"]
    # only_best: the same call with the best entry's solution alone; a second call at the same B reuses the batch context
    only = opt.solve_batch(qs, probs, only_best=True)
    assert only.best == res.best and only.flags == res.flags and _same(only.final_costs, res.final_costs)
    assert [s is not None for s in only.solutions] == [b == res.best for b in range(B)]
    for k in ("q", "v", "tau"):
        assert _same(getattr(only.solutions[res.best], k), getattr(res.solutions[res.best], k)), k
    for b in range(B):
        for f in STATS:
            assert _same(getattr(only.stats[b], f), getattr(res.stats[b], f)), (b, f)
    # problems = None: the optimizer's own problem for every entry
    own = opt.solve_batch(qs)
    for b in range(B):
        _assert_entry_equals(own, b, _solve_alone(model, probs[0], sp, qs[b]), name + " own problem")
    opt.close()


def test_some_entries_stop_early_on_the_convergence_criteria():
    """hopper with check_convergence and the tolerances of tests/test_gpu_batch.py's converging cases.  With the YAML's
    Delta0 = 1e-3 every problem of this kind meets the state-change criterion in its first iteration (the CPU oracle says
    so for any weights and guesses tried: |dq| <= Delta0 |D| is far below 1e-3 |q|), so that "not all stop early" cannot
    hold; the radius is 1 here, with which no entry meets a criterion in 6 iterations, and entry 0's weights are 1e4 times
    the others', which shortens its steps (D ~ diag(H)^-1/4) below the state-change bound."""
    model, probs, sp, qs = _problems("hopper", max_iterations=6)
    sp.check_convergence = True
    for k, v in CONVERGENCE.items():
        setattr(sp, k, v)
    sp.Delta0 = 1.0
    for W in ("Qq", "Qv", "Qf_q", "Qf_v", "R"):
        setattr(probs[0], W, getattr(probs[0], W) * 1e4)
    singles = [_solve_alone(model, probs[b], sp, qs[b]) for b in range(B)]
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs)
    opt.close()
    assert res.batch_route
    early = [len(res.stats[b].iteration_costs) < sp.max_iterations for b in range(B)]
    assert any(early) and not all(early), ("the case tests nothing: entries that stopped early", early)
    for b in range(B):
        _assert_entry_equals(res, b, singles[b], "convergence")
        assert (res.convergence_reasons[b] != 0) == early[b]
        assert res.flags[b] == ("kSuccess" if early[b] else "kMaxIterationsReached")


def test_small_models_in_a_batch_agree_to_the_solvers_round_off(monkeypatch):
    """acrobot (blocks of 2), B = 3: the batch keeps the block kernels, one problem alone takes the scalar band
    factorisation - the entries agree with Solve within 10x what Solve itself differs by with and without
    IDTO_SOLVER_BAND=0 on one problem alone.  (Equality with Solve under IDTO_SOLVER_BAND=0 does not hold: the variable does
    not put acrobot's single context on the batch's kernels - its dq_norms differ from the batch's in the ninth digit.)"""
    model, probs, sp, qs = _problems("acrobot", max_iterations=6)
    singles = [_solve_alone(model, probs[b], sp, qs[b]) for b in range(B)]
    monkeypatch.setenv("IDTO_SOLVER_BAND", "0")
    singles_block = [_solve_alone(model, probs[b], sp, qs[b]) for b in range(B)]
    monkeypatch.delenv("IDTO_SOLVER_BAND")
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs)
    opt.close()
    assert res.batch_route
    yardstick = max(np.abs(singles[b][1].q - singles_block[b][1].q).max() for b in range(B))
    diff = max(np.abs(res.solutions[b].q - singles[b][1].q).max() for b in range(B))
    print("acrobot: |q(Solve) - q(Solve, IDTO_SOLVER_BAND=0)| = %.3e, |q(solve_batch) - q(Solve)| = %.3e" % (yardstick, diff))
    assert diff <= ACROBOT_Q_MARGIN, (diff, ACROBOT_Q_MARGIN)
    for b in range(B):
        assert res.flags[b] == singles[b][0] and res.errors[b] == ""
        assert len(res.stats[b].iteration_costs) == len(singles[b][2].iteration_costs)


@pytest.mark.parametrize("case", ["linesearch", "dense_weights"])
def test_what_the_batch_loop_does_not_serve_runs_entry_by_entry(case):
    if case == "linesearch":
        model, probs, sp, qs = _problems("acrobot", max_iterations=5)
        sp.method = "linesearch"
    else:
        model, probs, sp, qs = _problems("hopper", num_steps=6, max_iterations=3)
        nq = model.nq
        probs[1].Qq = probs[1].Qq + 0.05 * np.ones((nq, nq))   # (symmetric positive definite, not diagonal)
    singles = [_solve_alone(model, probs[b], sp, qs[b]) for b in range(B)]
    opt = TrajectoryOptimizer(model, probs[0], sp)
    sol0, st0 = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag0 = opt.Solve(qs[0], sol0, st0)
    res = opt.solve_batch(qs, probs)
    assert not res.batch_route
    for b in range(B):
        _assert_entry_equals(res, b, singles[b], case)
    assert res.best == _expected_best(res)
    # the optimizer's own problem is back on its context
    sol1, st1 = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    assert opt.Solve(qs[0], sol1, st1) == flag0
    for k in ("q", "v", "tau"):
        assert _same(getattr(sol1, k), getattr(sol0, k)), k
    for f in STATS:
        assert _same(getattr(st1, f), getattr(st0, f)), f
    opt.close()


def test_refusals():
    model, probs, sp, qs = _problems("hopper", max_iterations=2)
    opt = TrajectoryOptimizer(model, probs[0], sp)
    with pytest.raises(RuntimeError, match="disagree in length"):
        opt.solve_batch(qs, probs[:2])
    _, longer, _, _ = _problems("hopper", num_steps=N + 1, batch=1)
    with pytest.raises(RuntimeError, match="num_steps"):
        opt.solve_batch(qs, [probs[0], longer[0], probs[2]])
    with pytest.raises(RuntimeError, match="q_guesses"):
        opt.solve_batch(qs[:, :-1], probs)
    # ... and the optimizer goes on
    assert opt.solve_batch(qs, probs).batch_route
    opt.close()


def test_one_failing_entry_is_its_own():
    """hopper without enforced constraints; entry 1's Hessian has exactly zero rows (zero weight on DoF 0, R = 0: the way
    tests/test_gpu_status.py makes one)"""
    model, probs, sp, qs = _problems("hopper", max_iterations=4)
    sp.equality_constraints = False
    bad = copy.deepcopy(probs[1])
    for W in (bad.Qq, bad.Qv, bad.Qf_q, bad.Qf_v):
        W[0, :] = 0.0
        W[:, 0] = 0.0
    bad.R[:] = 0.0
    batch = [probs[0], bad, probs[2]]
    assert _solve_alone(model, bad, sp, qs[1])[0] == "kFactorizationFailed"
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, batch)
    opt.close()
    assert res.batch_route
    assert res.flags[1] == "kFactorizationFailed" and res.errors[1] != "" and res.solutions[1] is None
    for b in (0, 2):
        assert res.flags[b] != "kFactorizationFailed"
        _assert_entry_equals(res, b, _solve_alone(model, batch[b], sp, qs[b]), "beside a failing entry")
    assert res.best in (0, 2) and res.best == _expected_best(res)
