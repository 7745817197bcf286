"""The dense cost-weight paths of the library - a non-diagonal Qq, Qv, R, Qf_q or Qf_v is legal input, and from
`weights_diagonal` = 0 on no production configuration's code runs: assemble_kernel with acc_atwb / acc_vec_w_mat
(csrc/kernels.h), the e^T W e branch of cost_body, `last_assembly` 3 (the folded products, the fused launch, gn_small and the
assembly inside the solver's launch each decline), the trust-region loop without the two-set evaluation, the C-ABI's
refusals and the host's choice of loop.

The inputs are tests/test_dense_weights.py's balanced weights, whose every off-diagonal block shows in H, g and the cost far
above round-off (conditions checked there, on the CPU); the expectation is the oracle, bit for bit, and -
so that this file stands without it - the plain block formulas of tests/test_golden_examples.py assemble() on the device's
own v, tau, partials and N+.  The horizons are the smallest that reach every branch of assemble_kernel: N = 1 (i = N only),
2 (i = N - 1 with Qf_v, the first B), 3 (the first A, the first i < N - 1 with the M terms), 6 (interior rows)."""
import copy
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
from idto_amd import hip
from idto_amd.problem import SCALING, load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_dense_weights import (HORIZONS, KEYS, LOWER, PLAIN_RTOL, balanced_dense_problem, diagonal_of,
                                oracle_expectation, plain_differences)
from test_golden_examples import BANDS, PARTIALS
from test_gpu_solver_accuracy import errors

pytestmark = pytest.mark.gpu

NAMES = tuple(LOWER)
FORWARD = "forward_differences"
ASSEMBLED = ("gradient",) + BANDS
DENSE_KERNEL = 3              # `last_assembly`: assemble_kernel
DIAGONAL_FORMS = (1, 2, 4, 5)   # ... assemble_terms_kernel, assemble_diag's rows (the fused launch), inside the solver's launch, gn_small
SERIES = ("iteration_costs", "trust_region_radii", "trust_ratios", "q_norms", "dq_norms", "dqH_norms", "gradient_norms",
          "dL_dqs", "h_norms", "merits")


def other_values(prob):
    """the same problem with other dense weights: the off-diagonals halved, each weight scaled differently (exactly
    symmetric and positive definite like the ones it starts from: 0.5 W + 0.5 diag W)"""
    p = copy.deepcopy(prob)
    for k, c in zip(KEYS, (1.5, 0.75, 1.25, 2.0, 0.5)):
        W = np.asarray(getattr(prob, k))
        setattr(p, k, c * (0.5 * W + 0.5 * diagonal_of(W)))
    return p


def step_arrays(dev, q=None, problem=None):
    """gn_step (at q, if given), then eval_tau: the assembled arrays, the step, tau and the cost"""
    if q is not None:
        dev.set_q(q)
    dev.gn_step()
    out = {k: dev.get(k, problem) for k in ASSEMBLED + ("step",)}
    out["last_assembly"] = dev.get_option("last_assembly")
    dev.eval_tau()
    out["tau"], out["cost"] = dev.get("tau", problem), dev.get("cost", problem)
    return out


def same_arrays(a, b, keys=ASSEMBLED + ("step", "tau", "cost")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. bits
BITS = ([(n, N, KEYS, FORWARD) for n in NAMES for N in HORIZONS] + [(n, 3, (k,), FORWARD) for n in NAMES for k in KEYS]
        + [(n, 3, KEYS, m) for n in NAMES for m in ("central_differences", "central_differences4")])


@pytest.mark.parametrize("name,N,which,method", BITS, ids=lambda x: "+".join(x) if isinstance(x, tuple) else str(x))
def test_dense_assembly_and_cost_match_the_oracle_bit_for_bit(name, N, which, method):
    model, prob, sp, q = balanced_dense_problem(name, N, which=which)
    sp.gradients_method = method
    orc = Oracle(model, prob, sp)
    want = oracle_expectation(name, N, which)
    g, bands = (want["gradient"].ravel(), want["bands"]) if method == FORWARD else orc.grad_hess(q)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("weights_diagonal") == 0
    dev.set_q(q)
    dev.eval_tau()
    cost = dev.get("cost")
    assert cost == want["cost"] and np.array_equal(dev.get("tau"), want["tau"])

    def held():
        assert dev.get_option("last_assembly") == DENSE_KERNEL
        assert np.array_equal(dev.get("gradient"), np.asarray(g).ravel())
        for key, b in zip(BANDS, bands):
            assert np.array_equal(dev.get(key), b), key

    dev.eval_partials()
    dev.grad_hess()
    held()
    dev.gn_step()
    held()
    assert dev.solver_status() == (False, 0)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    held()
    assert np.array_equal(dev.get("step"), orc.gn_step(q)[1])
    # ... and the plain formulas on the device's own v, tau, partials and N+
    A, B, C = (dev.get(k) for k in BANDS)
    seen = plain_differences(prob, q, dev.get("v"), dev.get("tau"), {k: dev.get(k) for k in PARTIALS}, dev.get("nplus"),
                             dev.get("gradient"), (A, B, C), cost)
    print(name, N, which, method, "largest |device - plain formulas| / largest entry:", seen)
    for key, val in seen.items():
        assert val <= PLAIN_RTOL, (key, val)
    assert all(np.array_equal(C[i], C[i].T) for i in range(N + 1)) and np.array_equal(C[0], np.eye(model.nq))
    assert not B[0].any() and not B[1].any() and not A[0].any() and not A[1].any() and (N < 2 or not A[2].any())
    dev.close()


# ---- 2. the production solver on a dense-weight system
@pytest.mark.parametrize("name", NAMES)
def test_production_solver_on_a_dense_weight_system(name):
    """tests/test_gpu_solver_accuracy.py's gate, unchanged, on the default solver's step of the all-dense N = 6 system"""
    N = 6
    model, prob, sp, q = balanced_dense_problem(name, N)
    want = oracle_expectation(name, N)
    g, bands = want["gradient"].ravel(), want["bands5"]
    p_ref, unc = ol.refined_solution(ol.penta_make_dense(*bands), -g)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    fwd_lu, bwd_lu = errors(bands, g, dev.get("step"), p_ref)
    dev.set_option("reference_solver", 0)
    dev.gn_step()
    assert dev.solver_status() == (False, 0) and dev.get_option("last_assembly") == DENSE_KERNEL
    code = dev.get_option("last_solver")
    fwd, bwd = errors(bands, g, dev.get("step"), p_ref)
    print(name, "last_solver", code, "forward", fwd, "LU", fwd_lu, "unc", unc, "backward", bwd, "LU", bwd_lu)
    assert fwd <= 4 * fwd_lu + 16 * unc + 1e-12, ("forward error", fwd, "LU", fwd_lu, "unc", unc)
    # (ROWWISE there: the band factorisation 6, two workgroups 1, the seven-workgroup one 2 without its recursion-form tail)
    rowwise = code in (1, 6) or (code == 2 and dev.get_option("nd_recursion") == 0)
    cap = 1e-12 if rowwise else min(1e-11, max(1e-12, 0.01 * bwd_lu))
    assert bwd <= cap, ("componentwise backward error", bwd, "cap", cap, "LU", bwd_lu)
    dev.close()


# ---- 3. switching on one context
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["hopper", "mini_cheetah", "acrobot"])
def test_switching_between_diagonal_and_dense_weights_on_one_context(name, fused):
    """set_problem diagonal -> dense -> diagonal -> dense with other values: no folded product, fused plan or small-model
    launch of the problem before survives the switch.  At this horizon the diagonal problems of all three take the fused
    launch; with option fused = 0 they take what the longer horizons take - the products folded into fd_kernel and
    combined, or gn_small's one workgroup (acrobot)"""
    N = 6
    model, dense, sp, q = balanced_dense_problem(name, N)
    diagonal = balanced_dense_problem(name, N, which=())[1]
    sequence = [(diagonal, False), (dense, True), (diagonal, False), (other_values(dense), True)]
    dev = hip.HipPath(model, diagonal, sp)
    dev.set_option("fused", fused)
    dev.set_q(q)
    forms = []
    for i, (prob, is_dense) in enumerate(sequence):
        if i:
            dev.set_problem(prob)
        got = step_arrays(dev)
        assert dev.get_option("weights_diagonal") == (0 if is_dense else 1)
        forms.append(got["last_assembly"])
        fresh = hip.HipPath(model, prob, sp)
        fresh.set_option("fused", fused)
        want = step_arrays(fresh, q)
        fresh.close()
        same_arrays(got, want)
        assert got["last_assembly"] == want["last_assembly"], (i, forms)
    print(name, "fused", fused, "last_assembly", forms)
    assert forms[1] == forms[3] == DENSE_KERNEL and forms[0] == forms[2] and forms[0] in DIAGONAL_FORMS
    dev.close()


# ---- 4. batch
@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_dense_batch_equals_single_contexts_and_the_oracle(name):
    """three problems with different weights (the second's are diagonal: the context as a whole is dense) and different
    nominal trajectories and trajectories: assemble_kernel and cost_kernel take their problem's data by blockIdx.y"""
    N = 3
    model, p0, sp, _ = balanced_dense_problem(name, N)
    probs = [p0, balanced_dense_problem(name, N, which=())[1], other_values(p0)]
    cfg = load_config(name)
    for b, p in enumerate(probs):
        p.q_nom = p.q_nom + 0.01 * b
    qs = np.array([synthetic_trajectory(cfg, model, N, seed=1 + b, lower=LOWER[name]) for b in range(3)])
    batch = hip.HipPath(model, probs, sp)
    assert batch.get_option("weights_diagonal") == 0
    batch.set_q_batch(qs)
    batch.eval_tau()
    costs = [batch.get("cost", b) for b in range(3)]
    taus = [batch.get("tau", b) for b in range(3)]
    batch.gn_step()
    assert batch.get_option("last_assembly") == DENSE_KERNEL and batch.solver_status_batch() == [False] * 3
    for b in range(3):
        got = {k: batch.get(k, b) for k in ASSEMBLED + ("step",)}
        got["tau"], got["cost"] = taus[b], costs[b]
        one = hip.HipPath(model, probs[b], sp)
        same_arrays(got, step_arrays(one, qs[b]))
        one.close()
        orc = Oracle(model, probs[b], sp)
        _, _, tau, cost = orc.eval_traj(qs[b])
        g, bands = orc.grad_hess(qs[b])
        assert got["cost"] == cost and np.array_equal(got["tau"], tau) and np.array_equal(got["gradient"], g)
        for key, want in zip(BANDS, bands):
            assert np.array_equal(got[key], want), (b, key)
    batch.close()


# ---- 5. the trust-region loop
# name -> (N, scaling method, iterations, normalize_quaternions)
LOOPS = {"hopper": (12, "sqrt", 8, False), "acrobot": (12, "double_sqrt", 12, False), "mini_cheetah": (8, "double_sqrt", 6, True)}
# the runs held to the oracle: the three above, the adaptive scaling (the stepwise loop of the host) and enforced
# constraints (the host loop)
TRACKED = [(n,) + LOOPS[n] + (False,) for n in LOOPS] + [("acrobot", 12, "adaptive_double_sqrt", 12, False, False),
                                                          ("hopper", 12, "double_sqrt", 8, False, True),
                                                          ("acrobot", 12, "double_sqrt", 12, False, True)]


def loop_problem(name, N, method, iters, quat, constrained):
    """the balanced dense problem with the configuration's guess and radius.  acrobot: with these weights the
    configuration's own guess (all zeros) gives a nearly quadratic problem on which the oracle rejects no step for any
    radius, so its double_sqrt run starts from a rough guess (amplitude 22, seed 8) with Delta0 = 1, where the oracle
    rejects steps 6, 7 and 9 of the twelve and accepts the others - of the rough guesses with a rejection (amplitudes
    12 .. 30, seeds 1 .. 8, Delta0 1 .. 1000) the one whose oracle run moves least under a perturbation of the guess by
    1e-13 .. 1e-12 relative and under another libm: costs 7e-9, q 1e-7, a hundredth of the tolerances it is held to"""
    model, prob, sp, _ = balanced_dense_problem(name, N)
    cfg = load_config(name)
    q_guess = make_problem(cfg, model, num_steps=N)[2]
    if name == "acrobot" and method == "double_sqrt" and not constrained:
        q_guess = synthetic_trajectory(cfg, model, N, seed=8, amplitude=22.0)
        sp.Delta0 = 1.0
    if name == "acrobot" and constrained:
        # (with the configuration's Delta0 = 1000 the constraint violation falls to 1e-8 within the twelve iterations, and
        # below 1e-2 the oracle itself does not reproduce its h_norms to rtol 1e-5: its run from a guess perturbed by
        # 1e-12, or with another libm, differs by 3 .. 12 times that tolerance for every Delta0 from 0.1 to 1000 - what an
        # implementation with another solver shows as well: 2.7e-5 .. 1.2e-2 relative at h <= 4e-3 on the device.  With
        # Delta0 = 0.01 the steps stay radius-limited, h between 0.7 and 80, and the oracle's own differences at a hundredth
        # of every tolerance; the run has one nearly rejected step, after which the radius shrinks)
        sp.Delta0 = 0.01
    sp.scaling, sp.scaling_method, sp.normalize_quaternions = True, method, quat
    sp.equality_constraints = constrained
    sp.max_iterations, sp.verbose = iters, False
    return model, prob, sp, q_guess


def run_solve(case):
    from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
    model, prob, sp, q_guess = loop_problem(*case)
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    return sol, st, flag, opt.num_equality_constraints()


@functools.lru_cache(maxsize=None)
def default_solve(case):
    """Solve as the host chooses its loop (computed once per case, shared by (a) and (b))"""
    assert "IDTO_OPT_STEPWISE" not in os.environ and "IDTO_OPT_HOST_LOOP" not in os.environ
    return run_solve(case)


@pytest.mark.parametrize("name", list(LOOPS))
def test_resident_loop_equals_stepwise_loop_with_dense_weights(name, monkeypatch):
    """idto_hip_tr_solve without the two-set evaluation (idto_hip_gn_step again at the iterate, every iteration) walks
    exactly the iterates of the loop that returns to the host twice per iteration"""
    case = (name,) + LOOPS[name] + (False,)
    iters = case[3]
    monkeypatch.delenv("IDTO_OPT_STEPWISE", raising=False)
    monkeypatch.delenv("IDTO_OPT_HOST_LOOP", raising=False)
    a_sol, a_st, a_flag, _ = default_solve(case)
    monkeypatch.setenv("IDTO_OPT_STEPWISE", "1")
    b_sol, b_st, b_flag, _ = run_solve(case)
    assert a_flag == b_flag
    for series in SERIES:
        x, y = getattr(a_st, series), getattr(b_st, series)
        assert x.size == iters and np.array_equal(x, y), (series, x, y)
    assert np.array_equal(a_sol.q, b_sol.q) and np.array_equal(a_sol.v, b_sol.v) and np.array_equal(a_sol.tau, b_sol.tau)
    print(name, "trust ratios", a_st.trust_ratios)
    if name == "acrobot":   # a rejected step is where this route differs from the production one
        assert (a_st.trust_ratios <= 0).any()


@pytest.mark.parametrize("case", TRACKED, ids=lambda c: "-".join(str(x) for x in c))
def test_solve_with_dense_weights_tracks_the_oracle(case, monkeypatch):
    """the tolerances of tests/test_gpu_optimizer.py test_solve_tracks_the_oracle.  Dense weights with enforced constraints
    are refused by idto_hip_tr_solve: Solve must take the host loop for them, not raise"""
    monkeypatch.delenv("IDTO_OPT_STEPWISE", raising=False)
    monkeypatch.delenv("IDTO_OPT_HOST_LOOP", raising=False)
    name, N, method, iters, quat, constrained = case
    model, prob, sp, q_guess = loop_problem(*case)
    orc = Oracle(model, prob, sp)
    ref = orc.solve(q_guess)
    sol, st, flag, neq = default_solve(case)
    assert neq == orc.num_eq and (neq > 0 or not constrained)
    assert st.iteration_costs.size == iters and flag == "kMaxIterationsReached"
    rc = ref["stats"]
    print(case, "costs", st.iteration_costs, "oracle", rc.iteration_costs, "ratios", st.trust_ratios)
    assert np.allclose(st.iteration_costs, rc.iteration_costs, rtol=1e-6), (st.iteration_costs, rc.iteration_costs)
    assert np.allclose(st.trust_region_radii, rc.trust_region_radii, rtol=1e-12)
    assert np.allclose(st.h_norms, rc.h_norms, rtol=1e-5, atol=1e-9)
    assert np.abs(sol.q - ref["q"]).max() <= 1e-5 * max(1.0, np.abs(ref["q"]).max())


def test_c_abi_refusals_with_dense_weights_leave_the_context_usable():
    """idto_hip_tr_solve's three refusals, each with its message; nothing is left enqueued (the stream drains), and the
    context that refused goes on: the batch with a step equal to single contexts', the single context with a
    non-adaptive unconstrained loop whose rows are a fresh context's"""
    N, iters = 6, 4
    model, prob, sp, q = balanced_dense_problem("hopper", N)
    dofs = list(model.unactuated_dofs)
    assert dofs
    dsq, adaptive = SCALING["double_sqrt"], SCALING["adaptive_double_sqrt"]
    # 1: a batch context
    probs = [prob, other_values(prob)]
    batch = hip.HipPath(model, probs, sp)
    batch.set_q_batch(np.array([q, q]))
    batch.eval_tau()
    with pytest.raises(hip.HipError, match=re.escape("tr_solve on a batch context needs the two-set evaluation (diagonal cost weights)")):
        batch.tr_solve_batch(iters, dsq, True, False, 1e-1, 1e5)
    batch.sync()
    batch.gn_step()
    for b in range(2):
        one = hip.HipPath(model, probs[b], sp)
        one.set_q(q)
        one.gn_step()
        for k in ASSEMBLED + ("step",):
            assert np.array_equal(batch.get(k, b), one.get(k)), (b, k)
        one.close()
    batch.close()
    # 2 and 3 on one context, then the loop it does serve
    dev, fresh = hip.HipPath(model, prob, sp), hip.HipPath(model, prob, sp)
    for d in (dev, fresh):
        d.set_unactuated_dofs(dofs)
        d.set_q(q)
        d.eval_tau()
    with pytest.raises(hip.HipError, match=re.escape("tr_solve: the adaptive scalings need the gated assembly (diagonal cost weights)")):
        dev.tr_solve(iters, adaptive, True, False, 1e-1, 1e5)
    dev.sync()
    with pytest.raises(hip.HipError, match=re.escape("tr_solve: enforced constraints need diagonal cost weights")):
        dev.tr_solve(iters, dsq, True, False, 1e-1, 1e5, constrained_dofs=dofs)
    dev.sync()
    assert np.array_equal(dev.get("q"), q)
    out = []
    for d in (dev, fresh):
        rows, delta = d.tr_solve(iters, dsq, True, False, 1e-1, 1e5)
        out.append((np.delete(rows, 10, axis=1), delta, d.get("q"), d.get("tr_dq")))   # (column 10 is the device clock)
        assert d.solver_status() == (False, 0)
        d.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    # steps were accepted (column 9) and no flag was raised (column 14, the 13th once the clock is taken out)
    assert out[0][0][:, 9].any() and (out[0][0][:, 13] == 0).all()
