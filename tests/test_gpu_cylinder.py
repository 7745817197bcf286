"""Cylinders on the device (include/idto_model.h, csrc/id_eval.h cylinder_reduce): the cylinder side of a sphere-cylinder
pair becomes the sphere or the box of the region that the sphere's centre is in, then the existing expressions run.

The oracle knows no cylinders.  Three yardsticks, as for capsules: tests/cylinder_ref.py (the closed form in numpy) for the
geometry, the oracle on cylinder_ref.frozen_model - frozen again at every perturbed configuration - for tau and its
difference quotients, and tests/golden/cylinder/kane_mini_cheetah_hills.json (tests/test_model_cylinder.py) for tau from
a generator that shares no code with either.  Tolerances: GEOMETRY_TOL as measured by tests/test_cylinder_host.py on the
CPU; TAU_REL and BLOCK_REL as derived in tests/test_gpu_capsule.py, whose derivation holds unchanged.

The plants' host restatement of tests/test_gpu_plant.py is the ORACLE's physics plus the exported step functions; the
oracle cannot express a cylinder, so the plant test here holds the bias and every substep to the oracle on frozen_model
within TAU_REL carried through the step, not to ==."""
from fractions import Fraction

import numpy as np
import pytest

import cylinder_cases as cc
import cylinder_ref as cyl
import oracle_lib as ol
import plant_cases as pc
from idto_amd import hip
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import make_problem
from test_cylinder_host import GEOMETRY_TOL, geometry_error, sp_of
from test_gpu_capsule import ARRAYS, BLOCK_REL, PARTIALS, TAU_REL
from test_gpu_fast_shape import same

pytestmark = pytest.mark.gpu


# ---- 1. geometry and force through scene_report
def fma(a, b, c):
    """a b + c rounded once (the device's __builtin_fma), by exact rational arithmetic"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def contact_pair_force(sp, phi, n, vn, vt):
    """csrc/id_eval.h contact_pair's fn and force on B from a row's phi, normal, vn and vt, operation by operation"""
    k, vd, vs, mu, sigma = (sp.contact_stiffness, sp.dissipation_velocity, sp.stiction_velocity, sp.friction_coefficient,
                            sp.smoothing_factor)
    s = vn / vd
    dissipation = (1 - s) if s < 0 else ((s - 2) * (s - 2) / 4 if s < 2 else 0.0)
    exponent = -phi / sigma
    if exponent >= 37:
        compliant = -k * phi
    else:
        compliant = sigma * k * float(ol.det_log(np.array([1 + float(ol.det_exp(np.array([exponent]))[0])]))[0])
    fn = compliant * dissipation
    vt2 = fma(vt[2], vt[2], fma(vt[1], vt[1], vt[0] * vt[0]))
    den = np.sqrt(vs * vs + vt2)
    force = np.array([n[i] * fn + ((-vt[i]) / den * mu) * fn for i in range(3)])
    return fn, force


@pytest.mark.parametrize("role", cc.ROLES)
def test_scene_report_meets_the_rule_at_the_directed_states(role):
    worst, active = 0.0, 0
    for name, state in cc.directed_labels():
        model, q, v, a = cc.directed(name, state, role)
        prob, sp = sp_of(name, model)
        dev = hip.HipPath(model, prob, sp)
        assert dev.get_option("fast_shape") == 0
        rep = dev.scene_report(np.concatenate([q, v])[None, :])
        dev.close()
        want = cc.expected_pairs(model, q, name)
        threshold = cyl.Frozen(model, prob, sp).base.contact_threshold
        for k in range(model.npairs):
            label = (name, state, k, want[k]["region"])
            e = geometry_error(rep.pairs[0, k, 1:11], want[k])
            worst = max(worst, e)
            assert e <= GEOMETRY_TOL, label + (e,)
            if abs(want[k]["phi"] - threshold) > GEOMETRY_TOL:
                assert bool(rep.active[0, k]) == (want[k]["phi"] <= threshold), label
            if rep.active[0, k]:
                active += 1
                fn, force = contact_pair_force(sp, rep.phi[0, k], rep.normal[0, k], rep.vn[0, k], rep.vt[0, k])
                assert rep.fn[0, k] == fn and np.array_equal(rep.force[0, k], force), label
                assert fn > 0
            else:
                assert rep.fn[0, k] == 0 and not np.any(rep.force[0, k]), label
    assert active >= len(cc.directed_labels())
    print("scene_report: largest |difference| from cylinder_ref", worst, "bar", GEOMETRY_TOL)


# ---- 2. tau and its difference quotients against the oracle on frozen models
# (the trajectories make the cylinders act - cylinder_cases.FROZEN, frozen_case; tests/test_model_cylinder.py checks those
# conditions with the frozen oracle alone, in a run without a GPU)
FROZEN = cc.FROZEN


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_cylinders_equal_the_oracle_on_frozen_models(name):
    model, prob, sp, q, N = cc.frozen_case(name)
    v, a, tau, tau_no_cyl, P = cyl.frozen_expectation(model, prob, sp, q)
    n_act = int(np.count_nonzero(np.abs(tau - tau_no_cyl).max(axis=1) > 1e-3))
    assert n_act >= N // 2, n_act
    if name == "mini_cheetah_hills":
        assert cc.hill_and_ground_together(model, prob, sp, q)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("v"), v) and same(dev.get("a"), a)
    got = dev.get("tau")
    scale = np.maximum(np.abs(tau).max(axis=1), 1.0)
    err = np.abs(got - tau).max(axis=1)
    print(name, "largest |tau - frozen oracle| / scale", (err / scale).max())
    assert np.all(err <= TAU_REL * scale), (err / scale).max()
    dev.eval_partials()
    for k in PARTIALS:
        g, w = dev.get(k), P[k]
        nan = np.isnan(w)   # (the oracle's NaN entries: blocks the reference leaves undefined)
        assert np.array_equal(np.isnan(g), nan), k
        bound = BLOCK_REL * max(np.abs(w[~nan]).max(), 1.0)
        print(name, k, "largest difference", np.abs(g - w)[~nan].max(), "bound", bound)
        assert np.abs(g - w)[~nan].max() <= bound, (k, np.abs(g - w)[~nan].max(), bound)
    dev.close()


# ---- 3. a batch == single contexts
def test_batch_equals_single_contexts():
    N, B = 20, 3
    model, cfg, _ = cc.trajectory("hopper_on_cylinder", N)
    sp = make_problem(cfg, model, num_steps=N)[1]
    sp.scaling = sp.equality_constraints = False
    probs, qs = [], []
    for b in range(B):
        prob = make_problem(cfg, model, num_steps=N)[0]
        prob.q_nom = prob.q_nom + 0.01 * b
        probs.append(prob)
        q = cc.trajectory("hopper_on_cylinder", N)[2]
        q[1:, 0] -= 0.004 * b
        qs.append(q)
    batch = hip.HipPath(model, probs, sp)
    assert batch.get_option("fast_shape") == 0
    batch.set_option("reference_solver", 1)
    batch.set_q_batch(np.array(qs))
    batch.gn_step()
    arrays = ARRAYS + ("step",)
    got = {(k, b): batch.get(k, b) for k in arrays for b in range(B)}
    batch.close()
    for b in range(B):
        one = hip.HipPath(model, probs[b], sp)
        one.set_option("reference_solver", 1)
        one.set_q(qs[b])
        one.gn_step()
        for k in arrays:
            assert same(got[(k, b)], one.get(k)), (k, b)
        assert np.abs(one.get("tau")).max() > 0
        one.close()


# ---- 4. terrain per problem
def test_a_batch_of_cheetahs_on_hills_of_their_own():
    N, heights = 8, (0.03, 0.05, 0.08)
    base, cfg, q = cc.trajectory("mini_cheetah_hills", N)
    models = [cc.hills([h, h])[0] for h in heights]
    prob, sp, _ = make_problem(cfg, base, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    batch = hip.HipPath(base, [prob] * len(heights), sp)
    batch.set_option("reference_solver", 1)
    for b, m in enumerate(models):
        batch.set_model_batch(b, m)
    batch.set_q_batch(np.array([q] * len(heights)))
    batch.gn_step()
    arrays = ARRAYS + ("step",)
    got = {(k, b): batch.get(k, b) for k in arrays for b in range(len(heights))}
    batch.close()
    for b, m in enumerate(models):
        one = hip.HipPath(m, prob, sp)
        one.set_option("reference_solver", 1)
        one.set_q(q)
        one.gn_step()
        for k in arrays:
            assert same(got[(k, b)], one.get(k)), (k, b)
        one.close()
    assert not same(got[("tau", 0)], got[("tau", 2)])   # (the heights matter)


# ---- 5. the trust-region loops and the solve on the fixture
def solve(model, prob, sp, q_guess):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    return flag, sol, st


def over_the_hill(cfg):
    """the fixture's problem started in front of the first hill (x = 2): the base at x = 1.55, its front feet on the
    hill's flank; the nominal x is relative to q_init in the YAML, so that the walk of 0.4 m goes up the hill"""
    cfg = dict(cfg)
    for key in ("q_init", "q_guess"):
        cfg[key] = list(cfg[key])
        cfg[key][4] = cfg[key][4] + 1.55
    return cfg


def test_resident_loop_equals_stepwise_loop(monkeypatch):
    model, cfg = cc.hills()
    prob, sp, q_guess = make_problem(over_the_hill(cfg), model, num_steps=10)
    sp.max_iterations, sp.verbose = 6, False
    monkeypatch.delenv("IDTO_OPT_STEPWISE", raising=False)
    a_flag, a_sol, a_st = solve(model, prob, sp, q_guess)
    monkeypatch.setenv("IDTO_OPT_STEPWISE", "1")
    b_flag, b_sol, b_st = solve(model, prob, sp, q_guess)
    assert a_flag == b_flag
    for series in ("iteration_costs", "trust_region_radii", "trust_ratios", "q_norms", "dq_norms", "dqH_norms",
                   "gradient_norms", "dL_dqs", "h_norms", "merits"):
        x, y = getattr(a_st, series), getattr(b_st, series)
        assert x.size == 6 and np.array_equal(x, y), (series, x, y)
    assert np.array_equal(a_sol.q, b_sol.q) and np.array_equal(a_sol.v, b_sol.v) and np.array_equal(a_sol.tau, b_sol.tau)


def test_mini_cheetah_hills_solve_end_to_end(record_property):
    """the fixture with its YAML at N = 20: max_iters iterations, finite statistics, the cost falls"""
    model, cfg = cc.hills()
    prob, sp, q_guess = make_problem(cfg, model, num_steps=20)
    sp.verbose = False
    flag, sol, st = solve(model, prob, sp, q_guess)
    costs = np.array(st.iteration_costs)
    record_property("solve", dict(flag=str(flag), iterations=len(costs), cost_first=float(costs[0]),
                                  cost_last=float(costs[-1]), ms_per_iteration=float(np.median(st.iteration_times) * 1e3)))
    assert flag == "kMaxIterationsReached" and len(costs) == sp.max_iterations
    for k in ("iteration_costs", "trust_region_radii", "q_norms", "dq_norms", "gradient_norms", "dL_dqs", "h_norms",
              "merits", "iteration_times"):
        assert np.all(np.isfinite(np.array(getattr(st, k)))), k
    assert np.all(np.isfinite(sol.q))
    assert costs[-1] < costs[0]


# ---- 6. a plant on a hill
H_PLANT = 1e-3


def resting_state():
    """the hopper standing on the top of the world cylinder of hopper_on_cylinder, its foot 5 mm in"""
    model, cfg, q = cc.trajectory("hopper_on_cylinder", 20)
    return model, cfg, q[1].copy()


def test_forward_dynamics_at_the_directed_states():
    """M == the oracle's columns (no contact in them); the bias within TAU_REL of the oracle on the frozen model; the
    acceleration == the exported solve on the device's own M and bias"""
    worst = 0.0
    for state in cc.STATES:
        model, q, v, _ = cc.directed("hopper", state, "sphere_first")
        prob, sp = sp_of("hopper", model)
        fr = cyl.Frozen(model, prob, sp)
        tau = np.array([0.0, 0.0, 0.0, 0.3, -0.2])
        dev = hip.HipPath(model, prob, sp)
        a, M, bias = dev.forward_dynamics(np.concatenate([q, v])[None, :], tau[None, :])
        dev.close()
        M_ref = pc.host_fd(fr.base, q, v, tau)[1]
        c_ref = fr.tau(q, v, np.zeros(model.nv))
        assert same(M[0], M_ref), state
        err = np.abs(bias[0] - c_ref).max() / max(np.abs(c_ref).max(), 1.0)
        worst = max(worst, err)
        assert err <= TAU_REL, (state, err)
        assert same(a[0], pc.solve_host(M[0], tau, bias[0])[0]), state
    print("forward dynamics: largest |bias - frozen oracle| / scale", worst)


def test_a_hopper_resting_on_the_cylinder_steps_as_the_frozen_oracle():
    """8 substeps in hold mode.  Substep s is compared with one host substep FROM THE DEVICE'S state s - 1: the oracle's M,
    the frozen oracle's bias, the exported solve and advance.  The bias may differ by TAU_REL of its scale, the
    acceleration then by |M^-1| times that, v by h times that and q by h times that again."""
    S = 8
    model, cfg, q0 = resting_state()
    prob, sp = make_problem(cfg, model, num_steps=3)[:2]
    fr = cyl.Frozen(model, prob, sp)
    nq, nv = model.nq, model.nv
    x0 = np.concatenate([q0, np.zeros(nv)])
    tau = np.zeros(nv)
    dev = hip.HipPath(model, prob, sp)
    dev.plant_begin(H_PLANT)
    dev.plant_set_state(0.0, x0[None, :])
    rec, status = dev.plant_step(S, tau[None, :], record_every=1)
    dev.close()
    assert status.tolist() == [[0, S]]
    x, worst = x0, 0.0
    for s in range(S):
        q, v = x[:nq], x[nq:]
        M = pc.host_fd(fr.base, q, v, tau)[1]
        c = fr.tau(q, v, np.zeros(nv))
        assert np.abs(c - fr.base.inverse_dynamics(q, v, np.zeros(nv))).max() > 1e-3   # (the cylinder carries the hopper)
        a_ref, piv = pc.solve_host(M, tau, c)
        assert piv == -1
        q_ref, v_ref = pc.advance_host(model, H_PLANT, q, v, a_ref)
        da = np.abs(np.linalg.inv(M)).sum(axis=1).max() * TAU_REL * max(np.abs(c).max(), 1.0)
        bound = H_PLANT * da + 4 * np.finfo(float).eps * max(np.abs(rec[0, s]).max(), 1.0)
        err = np.abs(rec[0, s] - np.concatenate([q_ref, v_ref])).max()
        worst = max(worst, err / bound)
        assert err <= bound, (s, err, bound)
        x = rec[0, s]
    print("plant: largest difference / bound", worst)
