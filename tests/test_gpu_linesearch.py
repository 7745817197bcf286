"""idto_hip_costs_along: the cost at many step lengths along the Newton step, one launch set and one wait, against
idto_hip_trial_cost at the same trial points one by one.  Bar: BIT-EXACT (==).  The trial points are formed here as the
host's linesearch forms them (host/trajectory_optimizer.cc ArmijoLinesearch): step = fl(alpha dq_i), fl(q_i + step), then
per quaternion n = sqrt(((w w + x x) + y y) + z z) and four divisions - numpy's elementwise double arithmetic, no
contraction - and the candidates' kernels evaluate the same expressions in the same order, so any difference is a bug.

Shapes: horizons 1, 2, 3 (the smallest: the first and last time steps' special cases are the whole trajectory) of a
revolute chain (acrobot), a planar floating base with contact (hopper) and a quaternion floating base (mini_cheetah, with
and without normalisation); 1, 2, 7 and 64 candidates (64 = IDTO_LS_MAX_CANDIDATES, the cap) with the step lengths 1.0,
0.0 and 0.8^17 among them."""
import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 64)


def step_lengths():
    """64 step lengths: the Armijo chain as the host forms it, reordered so that 1.0, 0.0 and 0.8^17 come first"""
    chain = hip.ls_alphas(0, hip.LS_MAX_CANDIDATES)
    x, want = 1.0, []
    for _ in range(hip.LS_MAX_CANDIDATES):
        want.append(x)
        x *= 0.8
    assert chain.tolist() == want and chain[0] == 1.0 and chain[2] == 0.6400000000000001
    back = hip.ls_alphas(1, hip.LS_MAX_CANDIDATES)
    assert back.tolist() == want
    rest = [a for j, a in enumerate(chain) if j not in (0, 17, 63)]
    return np.array([chain[0], 0.0, chain[17]] + rest)


def trial_point(model, q, dq, alpha, normalize):
    step = alpha * dq
    qt = q + step
    if normalize:
        for qs in model.quaternion_starts:
            w = qt[:, qs:qs + 4]
            n = np.sqrt(((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) + w[:, 3] * w[:, 3])
            qt[:, qs:qs + 4] = w / n[:, None]
    return qt


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("name,normalize", [("acrobot", False), ("hopper", False), ("mini_cheetah", False),
                                            ("mini_cheetah", True)])
def test_costs_along_equal_trial_costs(name, normalize, N):
    cfg = load_config(name)
    model = load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = False
    sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=1, lower=0.01)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.eval_tau()
    dev.gn_step()
    dq = dev.get("step").reshape(N + 1, model.nq)
    before = {k: np.array(dev.get(k)) for k in ("cost", "gradient", "step", "tau", "v", "hbands", "dtau_dqt", "q")}
    assert np.all(np.isfinite(dq)) and np.all(dq[0] == 0.0) and np.any(dq != 0.0)
    if model.quaternion_starts:   # (the step takes the quaternions off the unit sphere: normalising changes the trial point)
        assert not np.array_equal(trial_point(model, q, dq, 1.0, True), trial_point(model, q, dq, 1.0, False))

    alphas = step_lengths()
    along = {m: dev.costs_along(alphas[:m], normalize_quaternions=normalize) for m in SIZES}
    # the resident iterate is what it was
    for k, ref in before.items():
        now = np.array(dev.get(k))
        assert now.shape == ref.shape and np.all((now == ref) | (np.isnan(now) & np.isnan(ref))), k
    # ... and evaluating it again gives the same cost (nothing the evaluation reads was touched)
    dev.eval_tau()
    assert np.array(dev.get("cost")).ravel()[0] == before["cost"].ravel()[0]

    # the reference: every trial point on its own, once
    ref = np.array([dev.trial_cost(trial_point(model, q, dq, a, normalize))[1] for a in alphas])
    assert np.all(np.isfinite(ref)) and len(set(ref.tolist())) >= 8
    if not normalize:
        assert ref[1] == before["cost"].ravel()[0]   # alpha = 0.0: the iterate itself
    for m in SIZES:
        print(name, normalize, N, m, "max |diff|", np.abs(along[m] - ref[:m]).max())
        assert along[m].tolist() == ref[:m].tolist(), (name, N, m)


def test_costs_along_refuses_what_it_cannot_serve():
    cfg = load_config("acrobot")
    model = load_model("acrobot")
    prob, sp, _ = make_problem(cfg, model, num_steps=2)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(synthetic_trajectory(cfg, model, 2, seed=1))
    dev.gn_step()
    for bad in (np.zeros(0), np.ones(hip.LS_MAX_CANDIDATES + 1)):
        with pytest.raises(hip.HipError):
            dev.costs_along(bad)
    batch = hip.HipPath(model, [prob, prob], sp)
    with pytest.raises(hip.HipError):
        batch.costs_along([1.0])


# ---------------------------------------------------------------------------------------------------------------------
# The linesearch method's loop on the device (idto_hip_ls_solve, TrajectoryOptimizer::Solve with method = kLinesearch)
# against the host loop (SolveWithLinesearch under IDTO_OPT_HOST_LOOP=1), which this loop replaces where it is eligible and
# which stays untouched.  Bar: == for every compared field.  The device loop runs the host loop's own launches for the
# Newton step, forms every trial point with the host's two roundings, sums L', the norms and the trust ratio's dot
# products in one thread in index order (the host's Dot / Norm) and forms H step in PentaDiagonalMatrix::MultiplyBy's
# order, so there is no reordered sum anywhere and no tolerance to work out.
import ctypes as C
import functools

from idto_amd.optimizer import (SOLVER_FLAGS, TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats)
from oracle_lib import Oracle

# (config, N, linesearch, iterations, max_linesearch_iterations, synthetic guess, the ORACLE's linesearch_iterations, its flag)
LOOP_CASES = {
    "acrobot-backtracking": ("acrobot", 3, "backtracking", 8, 50, False, [3, 2, 1, 1, 2, 0, 0, 0], "kSuccess"),
    "hopper-armijo": ("hopper", 4, "armijo", 8, 50, False, [5, 13, 10, 5, 6, 8, 4, 10], "kSuccess"),
    "hopper-backtracking": ("hopper", 4, "backtracking", 8, 50, False, [7, 3, 10, 8, 7, 18, 10, 10], "kSuccess"),
    "cheetah-armijo": ("mini_cheetah", 6, "armijo", 6, 50, True, [1, 1, 1, 1, 1, 3], "kSuccess"),
    "cheetah-backtracking": ("mini_cheetah", 6, "backtracking", 6, 50, True, [2, 1, 1, 1, 1, 6], "kSuccess"),
    "hopper-armijo-limit8": ("hopper", 4, "armijo", 6, 8, False, [5, 8], "kLinesearchMaxIters"),
    "hopper-backtracking-limit8": ("hopper", 4, "backtracking", 6, 8, False, [7, 3, 10], "kLinesearchMaxIters"),
}
EQUAL_SERIES = ("linesearch_iterations", "linesearch_alphas", "iteration_costs", "dL_dqs", "trust_ratios", "q_norms", "dq_norms",
                "gradient_norms", "h_norms", "dqH_norms", "merits")


def loop_problem(key, **overrides):
    name, N, ls, iters, max_ls, synth, _, _ = LOOP_CASES[key]
    cfg, model = load_config(name), load_model(name)
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.max_iterations, sp.verbose, sp.num_threads = iters, False, 1
    sp.method, sp.linesearch_method, sp.max_linesearch_iterations = "linesearch", ls, max_ls
    sp.scaling, sp.equality_constraints = False, False
    for k, v in overrides.items():
        setattr(sp, k, v)
    if synth:
        q_guess = synthetic_trajectory(cfg, model, N, seed=1, lower=0.01)
    return model, prob, sp, q_guess


def traced_solve(model, prob, sp, q_guess):
    """Solve, and whether it went through idto_hip_ls_solve (a trace mark)"""
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    L.idto_hip_trace_enable(1)
    try:
        flag = opt.Solve(q_guess, sol, st)
    finally:
        buf = C.create_string_buffer(1 << 20)
        L.idto_hip_trace_dump(buf, len(buf))
        L.idto_hip_trace_enable(0)
    lines = buf.value.decode().splitlines()
    return sol, st, flag, sum("hip: ls_solve begins" in l for l in lines)


def assert_same_solve(a, b, what):
    (sa, ta, fa), (sb, tb, fb) = a, b
    assert fa == fb, what
    for series in EQUAL_SERIES:
        x, y = np.asarray(getattr(ta, series), dtype=float), np.asarray(getattr(tb, series), dtype=float)
        print(what, series, "device", x.tolist(), "host", y.tolist())
        assert x.shape == y.shape and np.all((x == y) | (np.isnan(x) & np.isnan(y))), (what, series)
    assert np.all(np.isnan(ta.trust_region_radii))
    for k in ("q", "v", "tau"):
        assert np.array_equal(np.asarray(getattr(sa, k)), np.asarray(getattr(sb, k))), (what, k)


@pytest.mark.parametrize("key", list(LOOP_CASES))
def test_device_loop_equals_host_loop(key, monkeypatch):
    model, prob, sp, q_guess = loop_problem(key)
    want_ls, want_flag = LOOP_CASES[key][6:]
    ref = Oracle(model, prob, sp).solve(q_guess)
    # what the case is there for is a property of the ORACLE's run, not of the code under test
    assert list(ref["stats"].linesearch_iterations) == want_ls and SOLVER_FLAGS[ref["flag"]] == want_flag
    monkeypatch.delenv("IDTO_OPT_HOST_LOOP", raising=False)
    sd, td, fd, calls = traced_solve(model, prob, sp, q_guess)
    assert calls == 1, "Solve did not take the device loop"
    monkeypatch.setenv("IDTO_OPT_HOST_LOOP", "1")
    sh, th, fh, calls = traced_solve(model, prob, sp, q_guess)
    assert calls == 0
    assert_same_solve((sd, td, fd), (sh, th, fh), key)
    assert fd == SOLVER_FLAGS[ref["flag"]]
    assert list(td.linesearch_iterations) == want_ls   # (and the oracle's, which the host loop has tracked all along)


def device_rows(key, waves, fetch=True):
    model, prob, sp, q_guess = loop_problem(key)
    name, N, ls, iters, max_ls = LOOP_CASES[key][:5]
    dev = hip.HipPath(model, prob, sp)
    dev.set_unactuated_dofs(model.unactuated_dofs)
    dev.set_option("ls_waves", waves)
    dev.set_q(q_guess)
    out = dev.ls_solve(iters, 0 if ls == "armijo" else 1, max_ls, sp.normalize_quaternions, fetch=fetch)
    assert dev.get_option("ls_solves") == 1
    out["q_resident"], out["tau_resident"], out["cost_resident"] = dev.get("q"), dev.get("tau"), dev.get("cost")
    dev.close()
    return out


@pytest.mark.parametrize("key", ["hopper-armijo", "hopper-backtracking", "hopper-armijo-limit8", "hopper-backtracking-limit8"])
def test_rows_do_not_depend_on_the_waves(key):
    """One, three, five candidates a wave and the planned schedule: the same rows (but the clock) and the same iterate.
    At N = 4 the planned schedule is ONE wave (tests/golden/ls_waves.txt), so it is the narrow waves that carry a scan
    across launches - Armijo's step length, backtracking's armijo_met, L_old and step length live in device memory between
    ls_scan_kernel launches - and that decide in a late wave, behind which the accepted alpha (backtracking: alpha / rho) is
    evaluated once more.  The test asserts that the deciding candidates do lie beyond the first wave."""
    want_ls = LOOP_CASES[key][6]
    backtracking = LOOP_CASES[key][2] == "backtracking"
    runs = {w: device_rows(key, w) for w in (0, 1, 3, 5)}
    ref = runs[0]
    ran = len(want_ls)
    assert np.all(ref["rows"][:ran, 10] > 0) and np.all(ref["rows"][ran:] == 0)
    assert ref["rows"][:ran, 2].tolist() == want_ls
    assert ref["rows"][:ran, 11].tolist() == [0] * (ran - 1) + [64 if "limit8" in key else 0]
    # the index of the deciding candidate: Armijo's ls_iters-th (index ls_iters - 1), backtracking's index ls_iters
    deciding = [n if backtracking else n - 1 for n in want_ls]
    for w in (1, 3, 5):
        assert any(d >= w for d in deciding), "no iteration decides behind the first wave of %d" % w
    for w in (1, 3):
        assert any(d >= 2 * w for d in deciding), "no iteration decides behind the second wave of %d" % w
    cols = [c for c in range(hip.LS_ROW) if c != 10]
    for w, r in runs.items():
        assert np.array_equal(r["rows"][:, cols], ref["rows"][:, cols]), w
        assert np.array_equal(r["q"], ref["q"]) and np.array_equal(r["tau"], ref["tau"]) and np.array_equal(r["v"], ref["v"]), w
        # what came back under the loop's wait is what is resident
        assert np.array_equal(r["q"], r["q_resident"]) and np.array_equal(r["tau"], r["tau_resident"])
        assert r["cost_resident"] == r["rows"][ran - 1, 9]


def test_one_wait():
    model, prob, sp, q_guess = loop_problem("hopper-armijo")
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q_guess)
    dev.ls_solve(2, 0, 50)   # (allocations, which synchronise, are made on first use)
    dev.set_q(q_guess)
    L.idto_hip_trace_enable(1)
    dev.ls_solve(8, 0, 50)
    buf = C.create_string_buffer(1 << 20)
    L.idto_hip_trace_dump(buf, len(buf))
    L.idto_hip_trace_enable(0)
    lines = buf.value.decode().splitlines()
    begin = max(i for i, l in enumerate(lines) if "ls_solve begins" in l)
    assert sum("waited for the device" in l for l in lines[begin:]) == 1, lines[begin:]
    dev.close()


@pytest.mark.parametrize("change", [dict(scaling=True), dict(equality_constraints=True), dict(max_linesearch_iterations=65)])
def test_what_the_device_loop_does_not_serve_takes_the_host_loop(change, monkeypatch):
    key = "hopper-armijo" if "max_linesearch_iterations" in change else "acrobot-backtracking"
    model, prob, sp, q_guess = loop_problem(key, max_iterations=3, **change)
    if "equality_constraints" in change:
        assert len(model.unactuated_dofs) > 0
    monkeypatch.delenv("IDTO_OPT_HOST_LOOP", raising=False)
    sa, ta, fa, calls = traced_solve(model, prob, sp, q_guess)
    assert calls == 0, "Solve took the device loop"
    monkeypatch.setenv("IDTO_OPT_HOST_LOOP", "1")
    sb, tb, fb, _ = traced_solve(model, prob, sp, q_guess)
    assert_same_solve((sa, ta, fa), (sb, tb, fb), str(change))
