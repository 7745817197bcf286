"""The linesearch method for a batch of problems: idto_hip_costs_along_batch, idto_hip_ls_solve_batch_fetch and
TrajectoryOptimizer.solve_batch with method = linesearch.  Bar: BIT-EXACT (==) everywhere.

No sum is reordered anywhere: the batch launches are the single problem's kernels with the problem in the grid (the
ls_* kernels) or the same fd_body behind another kernel entry (fd_along_batch_kernel), every problem has its own loop state
and its own gate and stop words.  So the candidates' costs equal idto_hip_trial_cost problem by problem whatever solver
produced dq, and the loop equals the single problem's device loop wherever batch and single problem run the same solver
kernel - hopper and mini_cheetah at B = 3 do (tests/test_gpu_solve_batch.py relies on the same); small models in a batch of
more than two take other solver kernels, their step lengths are discrete decisions, and no == loop
test is made for them.

What the loop cases are there for are properties of the ORACLE's runs (asserted first): the entries' linesearch_iterations
differ from each other, so problems decide in different waves of the same iteration, and with the limit of 8 the entries
stop after different numbers of rows, so one problem idles behind its flag while the others iterate."""
import ctypes as C
import functools

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.optimizer import SOLVER_FLAGS, TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 64)
EQUAL_SERIES = ("linesearch_iterations", "linesearch_alphas", "iteration_costs", "dL_dqs", "trust_ratios", "q_norms", "dq_norms",
                "gradient_norms", "h_norms", "dqH_norms", "merits")
RESIDENT = ("q", "v", "tau", "cost", "gradient", "step", "hbands")


def step_lengths():
    """tests/test_gpu_linesearch.py's: the Armijo chain as the host forms it, reordered so that 1.0, 0.0 and 0.8^17 come first"""
    chain = hip.ls_alphas(0, hip.LS_MAX_CANDIDATES)
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


def _same(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def batch_problems(name, num_steps, batch, yaml_guess_first=False):
    """tests/test_gpu_solve_batch.py's recipe: shifted q_nom, perturbed v_init, scaled Qq, synthetic guesses; scaling and the
    enforced constraints off (what the linesearch loop on the device serves)"""
    cfg, model = load_config(name), load_model(name)
    probs, qs, sp = [], [], None
    for b in range(batch):
        prob, sp, q_yaml = make_problem(cfg, model, num_steps=num_steps)
        rng = np.random.default_rng(100 + b)
        prob.q_nom = prob.q_nom + 0.01 * b
        prob.v_init = prob.v_init + 0.05 * rng.normal(size=model.nv)
        prob.Qq = prob.Qq * (1.0 + 0.1 * b)
        probs.append(prob)
        qs.append(q_yaml if (yaml_guess_first and b == 0) else synthetic_trajectory(cfg, model, num_steps, seed=b, lower=0.01))
    sp.verbose, sp.num_threads = False, 1
    sp.scaling, sp.equality_constraints = False, False
    return model, probs, sp, np.array(qs)


# ---------------------------------------------------------------------------------------------------------------------
# 1. costs_along_batch against trial costs, problem by problem
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("name,normalize", [("acrobot", False), ("hopper", False), ("mini_cheetah", False),
                                            ("mini_cheetah", True)])
def test_costs_along_batch_equal_trial_costs(name, normalize, N, B):
    model, probs, sp, qs = batch_problems(name, N, B)
    dev = hip.HipPath(model, probs, sp)
    dev.set_q_batch(qs)
    dev.eval_tau()
    dev.gn_step()
    dqs = [dev.get("step", problem=b).reshape(N + 1, model.nq) for b in range(B)]
    before = [{k: np.array(dev.get(k, problem=b)) for k in RESIDENT} for b in range(B)]
    for b in range(B):
        assert np.all(np.isfinite(dqs[b])) and np.all(dqs[b][0] == 0.0) and np.any(dqs[b] != 0.0)
        assert _same(before[b]["q"], qs[b])
    assert not _same(dqs[0], dqs[1])   # (the problems do differ)

    alphas = step_lengths()
    along = {m: dev.costs_along_batch(alphas[:m], normalize_quaternions=normalize) for m in SIZES}
    # every resident array of every problem is bitwise what it was
    for b in range(B):
        for k, ref in before[b].items():
            assert _same(np.array(dev.get(k, problem=b)), ref), (b, k)
    dev.close()

    # the reference: every trial point of problem b on its own, on a single-problem context made with problem b, once
    for b in range(B):
        single = hip.HipPath(model, probs[b], sp)
        ref = np.array([single.trial_cost(trial_point(model, qs[b], dqs[b], a, normalize))[1] for a in alphas])
        single.close()
        assert np.all(np.isfinite(ref)) and len(set(ref.tolist())) >= 8
        if not normalize:
            assert ref[1] == before[b]["cost"].ravel()[0]   # alpha = 0.0: the iterate itself
        for m in SIZES:
            assert along[m].shape == (B, m)
            print(name, normalize, N, B, b, m, "max |diff|", np.abs(along[m][b] - ref[:m]).max())
            assert along[m][b].tolist() == ref[:m].tolist(), (name, N, B, b, m)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the loop against single solves
B3 = 3
# (config, N, linesearch, iterations, max_linesearch_iterations, entry 0 from the YAML guess,
#  the ORACLE's linesearch_iterations per entry (None: not pinned), its flag per entry)
LOOP_CASES = {
    "hopper-armijo": ("hopper", 4, "armijo", 8, 50, True,
                      [[5, 14, 9, 2, 8, 7, 9, 11], [1, 5, 8, 9, 1, 2, 1, 5], [1, 1, 1, 3, 5, 7, 6, 5]], ["kSuccess"] * 3),
    "hopper-backtracking": ("hopper", 4, "backtracking", 8, 50, True, None, ["kSuccess"] * 3),
    "hopper-armijo-limit8": ("hopper", 4, "armijo", 6, 8, True, None, ["kLinesearchMaxIters", "kLinesearchMaxIters", "kSuccess"]),
    "hopper-backtracking-limit8": ("hopper", 4, "backtracking", 6, 8, True, [[7, 5, 8], [1, 6, 9], [1, 3, 7, 10]],
                                   ["kLinesearchMaxIters"] * 3),
    "cheetah-armijo": ("mini_cheetah", 6, "armijo", 6, 50, False, None, ["kSuccess"] * 3),
    "cheetah-backtracking": ("mini_cheetah", 6, "backtracking", 6, 50, False,
                             [[3, 1, 1, 1, 6, 1], [2, 1, 1, 1, 1, 5], [3, 1, 1, 1, 5, 2]], ["kSuccess"] * 3),
}
# rows the oracle runs with the limit of 8 (hopper, Armijo): entries 0 and 1 stop early, entry 2 runs all 6
LIMIT8_ARMIJO_ROWS = [2, 3, 6]


@functools.lru_cache(maxsize=None)
def loop_case(key):
    name, N, ls, iters, max_ls, yaml_first = LOOP_CASES[key][:6]
    model, probs, sp, qs = batch_problems(name, N, B3, yaml_guess_first=yaml_first)
    sp.max_iterations = iters
    sp.method, sp.linesearch_method, sp.max_linesearch_iterations = "linesearch", ls, max_ls
    return model, probs, sp, qs


@functools.lru_cache(maxsize=None)
def oracle_runs(key):
    model, probs, sp, qs = loop_case(key)
    return [Oracle(model, probs[b], sp).solve(qs[b]) for b in range(B3)]


def assert_oracle_properties(key):
    """what the case is there for, from the oracle's runs - not from the code under test"""
    want_ls, want_flags = LOOP_CASES[key][6:]
    refs = oracle_runs(key)
    got_ls = [list(r["stats"].linesearch_iterations) for r in refs]
    got_flags = [SOLVER_FLAGS[r["flag"]] for r in refs]
    print(key, "oracle linesearch_iterations", got_ls, "flags", got_flags)
    assert got_flags == want_flags, (key, got_flags)
    if want_ls is not None:
        assert got_ls == want_ls, (key, got_ls)
    if key == "hopper-armijo-limit8":
        assert [len(x) for x in got_ls] == LIMIT8_ARMIJO_ROWS
    # the entries' linesearch_iterations differ from each other ...
    assert got_ls[0] != got_ls[1] and got_ls[1] != got_ls[2] and got_ls[0] != got_ls[2]
    # ... within one iteration, so that problems decide at different candidates of the same iteration
    both = min(len(x) for x in got_ls)
    assert any(len({x[k] for x in got_ls}) > 1 for k in range(both))
    return got_ls, got_flags


def solve_alone(model, prob, sp, q):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    try:
        flag = opt.Solve(q, sol, st)
    except RuntimeError as e:   # (where the reference throws: the entry's own error text in a batch)
        flag = "raised: " + str(e)
    opt.close()
    return flag, sol, st


def assert_entry_equals_solve(res, b, single, what):
    flag, sol, st = single
    if flag.startswith("raised: "):
        assert res.errors[b] == flag[len("raised: "):] and res.solutions[b] is None, (what, b, res.errors[b], flag)
        return
    assert res.flags[b] == flag, (what, b, res.flags[b], flag, res.errors[b])
    assert res.errors[b] == "", (what, b, res.errors[b])
    for series in EQUAL_SERIES:
        x, y = np.asarray(getattr(res.stats[b], series), dtype=float), np.asarray(getattr(st, series), dtype=float)
        print(what, b, series, "batch", x.tolist(), "single", y.tolist())
        assert _same(x, y), (what, b, series)
    assert np.all(np.isnan(res.stats[b].trust_region_radii))
    if res.solutions[b] is not None:   # (solve_batch hands a solution back for kSuccess / kMaxIterationsReached)
        for k in ("q", "v", "tau"):
            assert _same(getattr(res.solutions[b], k), getattr(sol, k)), (what, b, k)
    else:
        assert flag not in ("kSuccess", "kMaxIterationsReached")


def device_batch_rows(key, waves):
    model, probs, sp, qs = loop_case(key)
    ls, iters, max_ls = LOOP_CASES[key][2:5]
    dev = hip.HipPath(model, probs, sp)
    dev.set_unactuated_dofs(model.unactuated_dofs)
    dev.set_option("ls_waves", waves)
    dev.set_q_batch(qs)
    out = dev.ls_solve_batch(iters, 0 if ls == "armijo" else 1, max_ls, sp.normalize_quaternions)
    assert dev.get_option("ls_batch_solves") == 1 and dev.get_option("ls_solves") == 0
    out["q_resident"] = np.array([dev.get("q", problem=b) for b in range(B3)])
    out["tau_resident"] = np.array([dev.get("tau", problem=b) for b in range(B3)])
    out["cost_resident"] = np.array([np.ravel(dev.get("cost", problem=b))[0] for b in range(B3)])
    dev.close()
    return out


def device_single_rows(key, b):
    model, probs, sp, qs = loop_case(key)
    ls, iters, max_ls = LOOP_CASES[key][2:5]
    dev = hip.HipPath(model, probs[b], sp)
    dev.set_unactuated_dofs(model.unactuated_dofs)
    dev.set_q(qs[b])
    out = dev.ls_solve(iters, 0 if ls == "armijo" else 1, max_ls, sp.normalize_quaternions)
    dev.close()
    return out


NOT_THE_CLOCK = [c for c in range(hip.LS_ROW) if c != 10]


@pytest.mark.parametrize("key", list(LOOP_CASES))
def test_batch_loop_equals_single_solves(key):
    got_ls, got_flags = assert_oracle_properties(key)
    model, probs, sp, qs = loop_case(key)
    singles = [solve_alone(model, probs[b], sp, qs[b]) for b in range(B3)]
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs)
    assert res.batch_route, "solve_batch did not take the device's batch linesearch loop"
    for b in range(B3):
        assert_entry_equals_solve(res, b, singles[b], key)
        assert res.flags[b] == got_flags[b]
        assert list(res.stats[b].linesearch_iterations) == got_ls[b]   # (and the oracle's, which the single loop tracks)
    ok = [b for b in range(B3) if res.flags[b] in ("kSuccess", "kMaxIterationsReached")]
    want_best = min(ok, key=lambda b: (res.final_costs[b], b)) if ok else -1
    assert res.best == want_best
    for b in ok:
        assert np.isfinite(res.final_costs[b]) and res.final_costs[b] <= res.stats[b].iteration_costs[0]
    if key in ("hopper-armijo", "cheetah-backtracking"):
        # only_best: the same call with the best entry's solution alone; a second call at the same B reuses the batch context
        only = opt.solve_batch(qs, probs, only_best=True)
        assert only.batch_route and only.best == res.best and only.flags == res.flags and _same(only.final_costs, res.final_costs)
        assert [s is not None for s in only.solutions] == [b == res.best for b in range(B3)]
        for k in ("q", "v", "tau"):
            assert _same(getattr(only.solutions[res.best], k), getattr(res.solutions[res.best], k)), k
        # problems = None: the optimizer's own problem for every entry
        own = opt.solve_batch(qs)
        assert own.batch_route
        for b in range(B3):
            assert_entry_equals_solve(own, b, solve_alone(model, probs[0], sp, qs[b]), key + " own problem")
    opt.close()
    # The same at the C-ABI, where the iterate also comes back behind a row with flag 64 (kLinesearchMaxIters): rows (but
    # the clock), q, v, tau, the final cost and the status of every problem against idto_hip_ls_solve_fetch on a
    # single-problem context made with that problem.
    batch = device_batch_rows(key, 0)
    for b in range(B3):
        one = device_single_rows(key, b)
        assert np.array_equal(batch["rows"][b][:, NOT_THE_CLOCK], one["rows"][:, NOT_THE_CLOCK]), (key, b)
        for k in ("q", "v", "tau"):
            assert np.array_equal(batch[k][b], one[k]), (key, b, k)
        ran = len(got_ls[b])
        assert np.all(batch["rows"][b][:ran, 10] > 0) and np.all(batch["rows"][b][ran:] == 0)
        assert batch["rows"][b][:ran, 2].tolist() == got_ls[b]
        assert batch["status"][b] == (64 if got_flags[b] == "kLinesearchMaxIters" else 0)
        assert batch["final_cost"][b] == batch["rows"][b][ran - 1, 9] == batch["cost_resident"][b]
        assert np.array_equal(batch["q"][b], batch["q_resident"][b]) and np.array_equal(batch["tau"][b], batch["tau_resident"][b])
    assert batch["rc"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows do not depend on the waves
@pytest.mark.parametrize("key", ["hopper-armijo", "hopper-backtracking", "hopper-armijo-limit8", "hopper-backtracking-limit8"])
def test_batch_rows_do_not_depend_on_the_waves(key):
    """One, three, five candidates per problem a wave and the planned schedule: the same rows (but the clock) and iterates.
    The scans live in device memory between ls_scan_kernel launches, one per problem; problems that decide behind different
    waves of one iteration idle behind their own gate words for different numbers of waves."""
    backtracking = LOOP_CASES[key][2] == "backtracking"
    runs = {w: device_batch_rows(key, w) for w in (0, 1, 3, 5)}
    ref = runs[0]
    for w, r in runs.items():
        assert np.array_equal(r["rows"][:, :, NOT_THE_CLOCK], ref["rows"][:, :, NOT_THE_CLOCK]), w
        for k in ("q", "v", "tau", "final_cost", "status"):
            assert np.array_equal(r[k], ref[k]), (w, k)
    # from the rows: in some iteration two problems decide behind different waves (the index of the deciding candidate:
    # Armijo's ls_iters-th, index ls_iters - 1; backtracking's index ls_iters)
    ran = [int(np.sum(ref["rows"][b][:, 10] > 0)) for b in range(B3)]
    deciding = [[int(n) if backtracking else int(n) - 1 for n in ref["rows"][b][:ran[b], 2]] for b in range(B3)]
    print(key, "deciding candidates", deciding)
    for w in (1, 3, 5):
        found = any(deciding[a][k] // w != deciding[b][k] // w
                    for a in range(B3) for b in range(a + 1, B3) for k in range(min(ran[a], ran[b])))
        assert found, "no iteration in which two problems decide behind different waves of %d" % w
    if "limit8" in key:
        assert len(set(ran)) > 1, "every problem stopped after the same number of rows"


# ---------------------------------------------------------------------------------------------------------------------
# 4. one wait
def test_one_wait():
    key = "hopper-armijo"
    model, probs, sp, qs = loop_case(key)
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    dev = hip.HipPath(model, probs, sp)
    dev.set_q_batch(qs)
    dev.ls_solve_batch(2, 0, 50)   # (allocations, which synchronise, are made on first use)
    dev.set_q_batch(qs)
    L.idto_hip_trace_enable(1)
    dev.ls_solve_batch(8, 0, 50)
    buf = C.create_string_buffer(1 << 20)
    L.idto_hip_trace_dump(buf, len(buf))
    L.idto_hip_trace_enable(0)
    lines = buf.value.decode().splitlines()
    begin = max(i for i, l in enumerate(lines) if "ls_solve_batch begins" in l)
    assert sum("waited for the device" in l for l in lines[begin:]) == 1, lines[begin:]
    assert dev.get_option("ls_batch_solves") == 2
    dev.close()
    dev = hip.HipPath(model, probs, sp)
    dev.set_q_batch(qs)
    dev.ls_solve_batch(2, 0, 50)
    assert dev.get_option("ls_batch_solves") == 1
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals by name
def test_refusals_by_name():
    model, probs, sp, qs = loop_case("hopper-armijo")
    single = hip.HipPath(model, probs[0], sp)
    single.set_q(qs[0])
    single.gn_step()
    with pytest.raises(hip.HipError, match="batch contexts"):
        single.ls_solve_batch(2, 0, 50)
    with pytest.raises(hip.HipError, match="batch contexts"):
        single.costs_along_batch([1.0])
    single.close()
    dev = hip.HipPath(model, probs, sp)
    dev.set_q_batch(qs)
    with pytest.raises(hip.HipError, match="IDTO_LS_MAX_CANDIDATES"):
        dev.ls_solve_batch(2, 0, hip.LS_MAX_CANDIDATES + 1)
    with pytest.raises(hip.HipError, match="linesearch_method"):
        dev.ls_solve_batch(2, 2, 50)
    dev.gn_step()
    for bad in (np.zeros(0), np.ones(hip.LS_MAX_CANDIDATES + 1)):
        with pytest.raises(hip.HipError, match="step lengths"):
            dev.costs_along_batch(bad)
    assert dev.get_option("ls_batch_solves") == 0
    dev.close()


@pytest.mark.parametrize("case", ["scaling", "dense_weights"])
def test_what_the_batch_linesearch_loop_does_not_serve_runs_entry_by_entry(case):
    # (scaling: tests/test_gpu_linesearch.py's case for it, acrobot with backtracking - both sides run entry by entry here, so
    # the batch's other solver kernels for small models do not come into it)
    model, probs, sp, qs = batch_problems("acrobot" if case == "scaling" else "hopper", 3 if case == "scaling" else 4, B3)
    sp.max_iterations = 3
    sp.method, sp.max_linesearch_iterations = "linesearch", 50
    sp.linesearch_method = "backtracking" if case == "scaling" else "armijo"
    if case == "scaling":
        # (with scaling the reference divides a scaled gradient by an unscaled Hessian and throws "not a descent direction" for
        # most problems; entry 0 is that file's case itself - the YAML problem and guess -, the other entries keep the recipe and
        # their error texts are compared where they throw)
        cfg = load_config("acrobot")
        probs[0], _, q_yaml = make_problem(cfg, model, num_steps=3)
        qs[0] = q_yaml
        sp.scaling = True
    else:
        nq = model.nq
        probs[1].Qq = probs[1].Qq + 0.05 * np.ones((nq, nq))   # (symmetric positive definite, not diagonal)
    singles = [solve_alone(model, probs[b], sp, qs[b]) for b in range(B3)]
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs)
    opt.close()
    assert not res.batch_route
    assert any(not s[0].startswith("raised: ") for s in singles), "every single Solve raised: the case compares no solution"
    for b in range(B3):
        assert_entry_equals_solve(res, b, singles[b], case)
