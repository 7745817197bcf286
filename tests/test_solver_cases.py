"""The inputs of tests/test_gpu_solver_block_sizes.py, proven usable on the CPU: every matrix of the sweep is exactly
banded and as badly conditioned as asked for, its extended-precision solution is known well enough to measure against, and
the bars the device solvers are held to are reachable - the oracle's pivoted LU (what `reference_solver = 1` restates bit
for bit) and the float64 restatement of the padded un-pivoted block LDL^T (solver_cases.ldlt_padded_numpy) both meet them.
A case that could not would have to change here, not the bar there."""
import time

import numpy as np
import pytest

import oracle_lib as ol
import solver_cases as sc

BWD_BAR = 1e-12   # tests/test_gpu_solver_accuracy.py: the row-by-row substitutions


def forward_bar(fwd_lu, unc):
    return 4 * fwd_lu + 16 * unc + 1e-12


def test_the_block_size_table_is_the_planners():
    """(host/solver_plan.cc SolverBlockSize; tests/golden/solver_plan.txt pins the planner itself)"""
    for K, ks in sc.BLOCK_SIZES.items():
        assert all(sc.solver_block_size(k) == K for k in ks), K
    assert [sc.solver_block_size(k, True) for k in (4, 7, 15, 24, 25, 28, 29, 30)] == [4, 8, 16, 24, 30, 30, 29, 30]
    for k, n in sc.LONG:
        assert n * sc.solver_block_size(k) > 4096 >= (n - 1) * sc.solver_block_size(k)   # the first horizon past the LDS copy


def test_which_solves_fit_the_lds():
    """solver_cases.ldl_fits restates penta_ldl_layout: 32 x 32 blocks leave 1894 doubles for the right-hand side and rt"""
    assert sc.ldl_lds_doubles(41, 32) == 21360 and sc.ldl_lds_doubles(41, 32, 24) == 20238
    assert [n for n in range(1, 200) if not sc.ldl_fits(n, 32, False)] == list(range(28, 129))
    assert [n for n in range(1, 200) if not sc.ldl_fits(n, 32, True)] == list(range(49, 129))
    assert all(sc.ldl_fits(n, K, ts) for K in (8, 16, 19, 23, 24) for n in range(1, 600) for ts in (False, True))


@pytest.mark.parametrize("k", sorted({k for k, _, _ in sc.SWEEP}))
def test_revolute_star_is_a_model_of_that_size(k):
    m = sc.revolute_star(k)
    assert (m.nq, m.nv, m.nbodies, m.npairs, m.ngeoms, m.common_body) == (k, k, k, 0, 0, -1)
    assert m.npaths <= 4 and np.bincount(m.body_path).max() <= 8 and (m.mass > 0).all() and (m.inertia[:, :3] > 0).all()
    assert m.unactuated_dofs == []
    prob, sp, q = sc.star_problem(m, 12)
    assert q.shape == (13, k) and np.array_equal(q[0], prob.q_init)
    # the oracle takes it: a Gauss-Newton Hessian of block size k that is positive definite
    sp.scaling = sp.equality_constraints = False
    g, bands = ol.Oracle(m, prob, sp).grad_hess(q)
    assert np.linalg.eigvalsh(ol.penta_make_dense(*bands)).min() > 0


@pytest.mark.parametrize("k,nu", [(6, 1), (13, 2), (21, 3), (25, 3), (26, 3)])
def test_revolute_star_with_unactuated_joints(k, nu):
    m = sc.revolute_star(k, nu)
    assert m.unactuated_dofs == list(range(nu)) and m.nq == k


@pytest.mark.parametrize("k,n,cond_target", sc.SWEEP)
def test_case_is_usable_and_the_bars_are_reachable(k, n, cond_target):
    t0 = time.perf_counter()
    c = sc.case(k, n, cond_target)
    t_case = time.perf_counter() - t0
    assert np.array_equal(ol.penta_make_dense(*c.bands), c.H)                    # exactly banded, exactly symmetric
    assert 0.01 * cond_target <= c.cond <= 100 * cond_target, c.cond
    assert c.unc <= 1e-15, c.unc
    fwd_lu, bwd_lu = sc.errors(c.H, c.b, ol.penta_solve(*c.bands, c.b), c.x_ref)
    x, x_pad, pivots = sc.ldlt_padded_numpy(c.bands[:3], c.b, c.K)
    fwd, bwd = sc.errors(c.H, c.b, x, c.x_ref)
    print(f"k {k} n {n} K {c.K} cond {c.cond:.2e} unc {c.unc:.1e}  LU fwd {fwd_lu:.2e} bwd {bwd_lu:.2e}  "
          f"LDL^T fwd {fwd:.2e} bwd {bwd:.2e}  case {t_case:.2f} s")
    assert not x_pad.any() and np.array_equal(pivots[:, k:], np.ones((n, c.K - k)))   # the pad is decoupled: x = 0, d = 1
    assert (pivots > 0).all()
    assert fwd_lu <= forward_bar(fwd_lu, c.unc) and bwd_lu <= BWD_BAR, (fwd_lu, bwd_lu)
    assert fwd <= forward_bar(fwd_lu, c.unc) and bwd <= BWD_BAR, (fwd, fwd_lu, bwd)
    if (k, n) in sc.LONG:
        assert t_case <= 3.0, t_case
