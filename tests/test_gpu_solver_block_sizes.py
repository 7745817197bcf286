"""Accuracy gate for every instantiated block size of the un-pivoted block LDL^T solvers (tests/test_gpu_solver_accuracy.py
holds the exact sizes of the example models to it; here: the padded instantiations 8 / 16 / 24 / 32, the path that no
longer keeps the right-hand side in LDS, the substitution kernel behind them, and directed ill-conditioned matrices at
19 and 23).

Contexts come from solver_cases.revolute_star(k) - any nq = k <= 32 - and their Hessian bands are overwritten
(test_gpu_penta.DeviceSolver), so every one of the n block rows is an unknown.  tests/test_solver_cases.py proves on the CPU
that every input is usable and every bar reachable.  The bars are those of tests/test_gpu_solver_accuracy.py, against
oracle_lib.refined_solution (known to `unc`):
  * forward error <= 4 x that of `reference_solver = 1` (the pivoted-LU block Thomas) on the same context + 16 unc + 1e-12,
  * componentwise backward error max |H x - b| / (|H| |x| + |b|) <= 1e-12 for the row-by-row substitutions (every padded
    case: the two-workgroup kernel); the recursion-form tails the planner picks at 19 / 23 keep that file's own cap,
  * solver_status() == (False, 0): the pad pivots are 1 and trip neither pivot test.
`last_solver` says which kernel a case held: 1 two workgroups (or one: two_sided = 0 / n < 10), 4 pipelined chains, 2 seven
workgroups.  Every case's figures go to solver_block_sizes.json in the directory IDTO_RECORD_DIR names (default:
build/records)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import solver_cases as sc
from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import ProblemDefinition, SolverParameters, make_problem, synthetic_trajectory
from test_gpu_penta import DeviceSolver
from test_gpu_solver_accuracy import errors as band_errors

pytestmark = pytest.mark.gpu

BWD_BAR = 1e-12
TWO = dict(solver_band=0, solver_pipe=0, solver_nd=0, debug_pipe_tail=0)   # the two-workgroup kernel whatever the planner prefers
PLANNERS = {19: 4, 23: 2}   # k -> last_solver of the planner's own choice from n = 24 on
ALL_K = [k for ks in sc.BLOCK_SIZES.values() for k in ks]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_DIR = os.environ.get("IDTO_RECORD_DIR") or os.path.join(ROOT, "build", "records")
_RECORDS = []


def _record(**kw):
    _RECORDS.append({k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in kw.items()})
    os.makedirs(RECORD_DIR, exist_ok=True)
    with open(os.path.join(RECORD_DIR, "solver_block_sizes.json"), "w") as f:
        json.dump(_RECORDS, f, indent=1)


def forward_bar(fwd_lu, unc):
    return 4 * fwd_lu + 16 * unc + 1e-12


def variants(k, n, defaults):
    """(label, two_sided, options, last_solver expected, backward cap as a function of the LU's backward error);
    defaults: the solver options of a fresh context, i.e. the planner's own choice"""
    rowwise = lambda bwd_lu: BWD_BAR
    recursion = lambda bwd_lu: min(1e-11, max(1e-12, 0.01 * bwd_lu))   # tests/test_gpu_solver_accuracy.py
    out = []
    if k in PLANNERS and n >= 24:
        out.append(("planner", True, defaults, PLANNERS[k], recursion))
    out.append(("two_sided", True, TWO, 1, rowwise))
    out.append(("one_sided", False, TWO, 1, rowwise))
    return out


def fresh_options(s):
    return {name: s.dev.get_option(name) for name in ("solver_band", "solver_pipe", "solver_nd")}


def refused(s, b, n, K, two_sided, options):
    """32 x 32 blocks leave no room for the right-hand side and rt of more than 27 local rows in LDS (solver_cases.ldl_fits:
    one-sided n = 28 .. 128, of this sweep n = 41): the planner says so instead of launching, and that is what is held"""
    if sc.ldl_fits(n, K, two_sided):
        return False
    with pytest.raises(hip.HipError, match="do not fit the LDS carve-up"):
        s.solve(b, two_sided=two_sided, **options)
    return True


def held_to_the_bars(s, c, tag, defaults):
    """every variant of the context `s` on the case `c`"""
    s.set_bands(*c.bands[:3])
    fwd_lu, bwd_lu = sc.errors(c.H, c.b, s.solve(c.b, reference=True), c.x_ref)
    assert s.last_solver == 3
    for label, two_sided, options, code, cap in variants(c.k, c.n, defaults):
        if refused(s, c.b, c.n, c.K, two_sided, options):
            _record(test=tag, k=c.k, K=c.K, n=c.n, cond=c.cond, variant=label, refused=True)
            continue
        x = s.solve(c.b, two_sided=two_sided, **options)
        fwd, bwd = sc.errors(c.H, c.b, x, c.x_ref)
        _record(test=tag, k=c.k, K=c.K, n=c.n, cond=c.cond, variant=label, last_solver=s.last_solver, fwd=fwd, bwd=bwd,
                fwd_lu=fwd_lu, bwd_lu=bwd_lu, unc=c.unc)
        print(f"k {c.k} K {c.K} n {c.n} cond {c.cond:.1e} {label}: solver {s.last_solver} fwd {fwd:.2e} (LU {fwd_lu:.2e}, unc {c.unc:.1e}) "
              f"bwd {bwd:.2e} (LU {bwd_lu:.2e})")
        assert s.last_solver == code, (label, s.last_solver)
        assert fwd <= forward_bar(fwd_lu, c.unc), (label, "forward error", fwd, "LU", fwd_lu, "unc", c.unc, "cond", c.cond)
        assert bwd <= cap(bwd_lu), (label, "componentwise backward error", bwd, "cap", cap(bwd_lu), "LU", bwd_lu)
        assert s.dev.solver_status() == (False, 0), label


@pytest.mark.parametrize("n", sc.HORIZONS)
@pytest.mark.parametrize("k", ALL_K)
def test_every_block_size_is_as_accurate_as_the_pivoted_lu(k, n):
    """penta_ldl_kernel<8 | 16 | 24 | 32, PADDED> (and <19>, <23>; at 19 / 23 also penta_pipe_kernel<19> and
    penta_nd_kernel<23> with its recursion tail) on directed matrices: cond 1e4 and the largest target the reference
    resolves at the horizon (solver_cases.CONDS), one workgroup (n = 3, 9), the first two-sided splits (10, 11), 24, 41"""
    s = DeviceSolver(k, n)
    assert s.dev.get_option("fast_shape") == 0
    defaults = fresh_options(s)
    for cond_target in sc.CONDS[n]:
        held_to_the_bars(s, sc.case(k, n, cond_target), "sweep", defaults)
    s.close()


@pytest.mark.parametrize("k,n", sc.LONG)
def test_right_hand_side_outside_lds(k, n):
    """n K > 4096: penta_ldl_layout's bl_size == 0 - the right-hand side is read from memory row by row, rt is parked in
    x, and the back substitution is the general (not the push-form) one.  K = 32 at n = 129, 24 at 171, 16 at 257, 8 at 513:
    the first horizon past the LDS copy for each, all of which a context accepts (its LDS bounds reach n K = 4862)."""
    K = sc.solver_block_size(k)
    assert n * K > 4096 >= (n - 1) * K
    s = DeviceSolver(k, n)
    held_to_the_bars(s, sc.case(k, n, sc.LONG_COND), "long", fresh_options(s))
    s.close()


@pytest.mark.parametrize("n", [11, 41])
@pytest.mark.parametrize("k", ALL_K)
def test_many_right_hand_sides_on_every_block_size(k, n):
    """penta_apply_kernel<8 | 16 | 24 | 32> (penta_factor_transpose_kernel in front of the last three) behind the
    factor-only pass of penta_ldl_kernel: 3 columns, and as many as make nrhs n K > 4096.  Columns f b with f = 1, -2, 0.5,
    one independent column r = H u, then f b / f r in turn; each as accurate as the better-known of the single-column solve
    and LAPACK's pivoted LU (the bar of test_many_right_hand_sides_are_as_accurate_as_one)."""
    K = sc.solver_block_size(k)
    many = max(5, 4096 // (n * K) + 1)
    assert many * n * K > 4096
    s = DeviceSolver(k, n)
    for cond_target in sc.CONDS[n]:
        c = sc.case(k, n, cond_target)
        s.set_bands(*c.bands[:3])
        r = c.H @ np.random.default_rng(k * n).uniform(-1, 1, n * k)
        r_ref, r_unc = ol.refined_solution(c.H, r)
        base = [(c.b, c.x_ref, c.unc), (r, r_ref, r_unc)]
        f3 = (1.0, -2.0, 0.5)
        plan = [(0, f) for f in f3] + [(1, 1.0)] + [(j & 1, f3[j % 3]) for j in range(many - 4)]
        for two_sided in (True, False):
            if refused(s, c.b, n, K, two_sided, TWO):
                continue
            one = []   # per base column: max(single-column error, LU error), relative to max |x_ref|
            for rhs, ref, _ in base:
                scale = np.abs(ref).max()
                err_one = np.abs(s.solve(rhs, two_sided=two_sided, **TWO) - ref).max() / scale
                err_lu = np.abs(np.linalg.solve(c.H, rhs) - ref).max() / scale
                one.append(max(err_one, err_lu))
            for cols in (plan[:3], plan):
                X = s.solve(np.stack([f * base[w][0] for w, f in cols]), two_sided=two_sided, **TWO)
                assert s.last_solver == 1 and X.shape == (len(cols), n * k)
                worst = 0.0
                for j, (w, f) in enumerate(cols):
                    _, ref, unc = base[w]
                    err = np.abs(X[j] - f * ref).max() / np.abs(ref).max() / abs(f)
                    worst = max(worst, err)
                    assert err <= 4 * one[w] + 16 * unc + 1e-12, (two_sided, len(cols), j, err, one[w], unc)
                _record(test="many", k=k, K=K, n=n, cond=c.cond, variant="two_sided" if two_sided else "one_sided",
                        last_solver=s.last_solver, columns=len(cols), fwd=worst, fwd_one=max(one), unc=max(c.unc, r_unc))
                assert s.dev.solver_status() == (False, 0)
    s.close()


@pytest.mark.parametrize("k", [7, 21])
def test_identity_bands_return_the_right_hand_side_bit_for_bit(k):
    n = 11
    s = DeviceSolver(k, n)
    Z, I = np.zeros((n, k, k)), np.tile(np.eye(k), (n, 1, 1))
    s.set_bands(Z, Z, I)
    b = np.linspace(-3, 12.4, n * k)
    B = np.stack([b, -2.0 * b, 0.5 * b])
    for two_sided in (True, False):
        assert np.array_equal(s.solve(b, two_sided=two_sided), b) and s.last_solver == 1
        assert np.array_equal(s.solve(B, two_sided=two_sided), B) and s.last_solver == 1
    assert s.dev.solver_status() == (False, 0)
    s.close()


def test_failed_factorisation_is_reported_on_a_padded_size():
    """k = 7 in blocks of 8, n = 12: the C block of an interior row zeroed - the matrix is indefinite, its pivots there are
    not positive.  Reported as tests/test_gpu_status.py has it at exact sizes (status, failed rows, FactorizationFailed for
    host right-hand sides), the pad pivots do not hide it, and the context then solves a definite matrix cleanly."""
    k, n = 7, 12
    H = sc.banded_spd(n, k, 1e4, seed=5)
    A, B, C, D, E = sc.from_lower_dense(H, n, k)
    b = H @ np.linspace(-3, 12.4, n * k)
    bad = C.copy()
    bad[5] = 0.0
    s = DeviceSolver(k, n)
    for two_sided in (True, False):
        s.set_bands(A, B, bad)
        s.solve(b, two_sided=two_sided)
        assert s.last_solver == 1
        failed, rows = s.dev.solver_status()
        assert failed and rows >= 1
        with pytest.raises(hip.FactorizationFailed):
            s.dev.solve_host(b[None, :])
        rows = s.dev.solver_status()[1]
        s.set_bands(A, B, C)
        x = s.solve(b, two_sided=two_sided)
        assert s.dev.solver_status() == (False, rows)   # (the count is the context's total)
        x_ref, unc = ol.refined_solution(H, b)
        fwd, bwd = sc.errors(H, b, x, x_ref)
        assert bwd <= BWD_BAR and fwd <= forward_bar(sc.errors(H, b, s.solve(b, reference=True), x_ref)[0], unc)
    s.close()


# ---- the padded sizes on real systems: Gauss-Newton Hessians of models with nq = 7, 14, 21
def _real_system(name, N):
    if name == "free_body":   # nq = 7: the problem of test_gpu_parity.test_edge_horizons_and_padded_blocks
        model = load_model(name)
        nq, nv = model.nq, model.nv
        q0 = np.array([1.0, 0, 0, 0, 0.1, 0.2, 0.3])
        prob = ProblemDefinition(num_steps=N, q_init=q0, v_init=np.zeros(nv), Qq=np.eye(nq), Qv=0.1 * np.eye(nv),
                                 Qf_q=10 * np.eye(nq), Qf_v=np.eye(nv), R=0.5 * np.eye(nv),
                                 q_nom=np.tile(q0, (N + 1, 1)), v_nom=np.zeros((N + 1, nv)), time_step=0.05)
        sp = SolverParameters(verbose=False)
        q = np.tile(q0, (N + 1, 1)) + 0.05 * np.random.default_rng(N).normal(size=(N + 1, nq))
        q[0] = q0
    elif name == "jaco":      # nq = 14: the arm and its box (tests/test_gpu_gravity_switch.py)
        from test_gpu_gravity_switch import example
        model, cfg = example(name)
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.0)
    else:                     # nq = 21: punyo with its capsules (tests/test_gpu_stem.py)
        from test_model_stem import punyo, punyo_trajectory
        model, cfg = punyo()
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        q = punyo_trajectory(cfg, model, N, 0)
    sp.scaling = sp.equality_constraints = False
    return model, prob, sp, q


@pytest.mark.parametrize("N", [20, 40])
@pytest.mark.parametrize("name,nq", [("free_body", 7), ("jaco", 14), ("punyo", 21)])
def test_padded_blocks_on_real_systems(name, nq, N):
    """g and the bands are read back from the device (the oracle knows no capsules); the step of the two-workgroup kernel,
    two- and one-sided, against the two bars, and three columns through solve_host against the many-column bar"""
    model, prob, sp, q = _real_system(name, N)
    assert model.nq == nq and sc.solver_block_size(nq) > nq
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    g = dev.get("gradient").ravel()
    low = [dev.get(key) for key in ("H_A", "H_B", "H_C")]
    Cs, Dm, Em = ol.penta_make_symmetric(*low)
    bands = (low[0], low[1], Cs, Dm, Em)
    Hd = ol.penta_make_dense(*bands)
    p_ref, unc = ol.refined_solution(Hd, -g)
    fwd_lu, bwd_lu = band_errors(bands, g, dev.get("step"), p_ref)
    err_lapack = np.abs(np.linalg.solve(Hd, -g) - p_ref).max() / np.abs(p_ref).max()
    dev.set_option("reference_solver", 0)
    for two_sided in (1, 0):
        dev.set_option("two_sided", two_sided)
        dev.gn_step()
        assert dev.get_option("last_solver") == 1
        assert np.array_equal(dev.get("gradient").ravel(), g)
        fwd, bwd = band_errors(bands, g, dev.get("step"), p_ref)
        _record(test="real", config=name, k=nq, K=sc.solver_block_size(nq), n=N + 1, cond=np.linalg.cond(Hd),
                variant="two_sided" if two_sided else "one_sided", last_solver=1, fwd=fwd, bwd=bwd, fwd_lu=fwd_lu, bwd_lu=bwd_lu, unc=unc)
        assert fwd <= forward_bar(fwd_lu, unc), (two_sided, "forward error", fwd, "LU", fwd_lu, "unc", unc)
        assert bwd <= BWD_BAR, (two_sided, "componentwise backward error", bwd, "LU", bwd_lu)
        X = dev.solve_host(np.stack([-g, 2.0 * g, -0.5 * g]))
        assert dev.get_option("last_solver") == 1
        for col, f in enumerate((1.0, -2.0, 0.5)):
            err = np.abs(X[col] - f * p_ref).max() / np.abs(p_ref).max() / abs(f)
            assert err <= 4 * max(fwd, err_lapack) + 16 * unc + 1e-12, (two_sided, col, err, fwd, err_lapack, unc)
        assert dev.solver_status() == (False, 0)
    dev.close()
