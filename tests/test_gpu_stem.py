"""A stem of bodies below the common body on the device (include/idto_model.h): fd_kernel<8, SHAPE_STEM> over
id_eval<8, true, true>, chosen for every model whose common body has a parent.

The oracle treats a stem body as an ordinary body (oracle/rigid_body.h), so the bit-exact parity of DESIGN.md §3.2
carries over: punyo with zero-length capsules (its spheres, bit for bit) and every body's weight on equals the oracle; a
chain described as a stem equals the same chain through the kernels that served it before; the fixture as it is
(capsules with length, a weightless humanoid) is held against the oracle on frozen sphere models, composed by rows from
g and g = 0 (the humanoid and the ball meet only in contact, which does not depend on g).  The trajectories make a pair
of every class act (tests/test_model_stem.py checks that with the oracle)."""
import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_gpu_capsule import BLOCK_REL, TAU_REL, TWO_DOF_CFG, example, frozen_expectation
from test_gpu_fast_shape import SHAPES, outputs, same
from test_model_stem import (BAD_STEM, HUMANOID, PARTIALS, all_gravity, as_spheres, bad_stem_model,
                             hopper_on_a_planar_stem, jaco_chain_and_stems, no_gravity, punyo, punyo_trajectory, synthetic_stem_model, zero_length)

pytestmark = pytest.mark.gpu


# ---- 1. bits
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("method", ["forward_differences", "central_differences", "central_differences4"])
def test_punyo_with_zero_length_capsules_equals_the_oracle(seed, method):
    model, cfg = punyo()
    dev_model, orc_model = zero_length(all_gravity(model)), as_spheres(all_gravity(model))
    N = 40
    q = punyo_trajectory(cfg, orc_model, N, seed)
    prob, sp, _ = make_problem(cfg, orc_model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = method
    orc = Oracle(orc_model, prob, sp)
    v, a, tau, cost = orc.eval_traj(q)
    dev = hip.HipPath(dev_model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("v"), v) and same(dev.get("a"), a) and same(dev.get("tau"), tau)
    for t in range(N + 1):
        assert same(dev.get("nplus")[t], orc.nplus(q[t]))
    assert dev.get("cost") == cost
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    P = orc.eval_partials(q)
    for k in PARTIALS:
        assert same(dev.get(k), P[k]), k
    assert same(dev.get("tau"), tau)
    g, bands = orc.grad_hess(q)
    assert same(dev.get("gradient"), g)
    assert same(dev.get("H_A"), bands[0]) and same(dev.get("H_B"), bands[1]) and same(dev.get("H_C"), bands[2])
    dev.close()


# ---- 2. new code against old code
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("method", [0, 1])
def test_a_chain_described_as_a_stem_gives_the_chains_bits(seed, method):
    """the jaco arm with a stem of 2 and of 3 (fd_kernel<8, SHAPE_STEM>) == the arm as one chain off the world
    (fd_kernel<8, 0>): every output of the finite differences, the assembly and the step"""
    cfg, chain, stems = jaco_chain_and_stems()
    N = 10
    q = synthetic_trajectory(cfg, chain, N, seed=seed, lower=0.02)
    prob, sp, _ = make_problem(cfg, chain, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = ["forward_differences", "central_differences"][method]
    shape, want = outputs(chain, prob, sp, q, 1, gradients_method=method)
    assert shape == 0
    if seed == 0:   # (... which are the oracle's)
        orc = Oracle(chain, prob, sp)
        assert same(want["tau"], orc.eval_traj(q)[2])
        P = orc.eval_partials(q)
        for k in PARTIALS:
            assert same(want[k], P[k]), k
    for ns, m in stems.items():
        shape, got = outputs(m, prob, sp, q, 1, gradients_method=method)
        assert shape == 0
        for k in want:
            assert same(got[k], want[k]), (ns, k)


@pytest.mark.parametrize("method", [0, 1])
def test_a_stem_that_starts_with_a_planar_joint_gives_the_chains_bits(method):
    """the hopper with its leg as the common body (the planar torso below it) == the hopper as it is, through its fast
    shape and through the generic fd_kernel<3, 0>, == the oracle"""
    cfg, chain, stem = hopper_on_a_planar_stem()
    N = 20
    q = synthetic_trajectory(cfg, chain, N, seed=0, lower=0.01)
    prob, sp, _ = make_problem(cfg, chain, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = ["forward_differences", "central_differences"][method]
    shape, want = outputs(chain, prob, sp, q, 1, gradients_method=method)
    assert shape == SHAPES["hopper"]
    _, generic = outputs(chain, prob, sp, q, 0, gradients_method=method)
    shape, got = outputs(stem, prob, sp, q, 1, gradients_method=method)
    assert shape == 0
    for k in want:
        assert same(got[k], want[k]) and same(got[k], generic[k]), k
    orc = Oracle(chain, prob, sp)
    assert same(got["tau"], orc.eval_traj(q)[2])
    P = orc.eval_partials(q)
    for k in PARTIALS:
        assert same(got[k], P[k]), k


@pytest.mark.parametrize("method", ["forward_differences", "central_differences"])
def test_synthetic_stem_of_four_equals_the_oracle(method):
    """IDTO_MAX_STEM stem bodies; the third carries four pairs (ground pairs of a body not adjacent to the world, pairs
    with a chain body); the common body is touched from three paths"""
    model, cfg = synthetic_stem_model(), punyo()[1]
    N = 12
    q = punyo_trajectory(cfg, model, N, 1)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = method
    orc = Oracle(model, prob, sp)
    v, a, tau, cost = orc.eval_traj(q)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    assert same(dev.get("v"), v) and same(dev.get("a"), a) and same(dev.get("tau"), tau)
    P = orc.eval_partials(q)
    for k in PARTIALS:
        assert same(dev.get(k), P[k]), k
    g, bands = orc.grad_hess(q)
    assert same(dev.get("gradient"), g)
    assert same(dev.get("H_A"), bands[0]) and same(dev.get("H_B"), bands[1]) and same(dev.get("H_C"), bands[2])
    assert same(dev.get("step"), orc.gn_step(q)[1])
    dev.eval_tau()
    assert dev.get("cost") == cost
    dev.close()


# ---- 3. the fixture as it is
def test_punyo_fixture_equals_the_oracle_on_frozen_sphere_models():
    """Capsules with length, the humanoid weightless.  The oracle has one gravity vector and no capsules: expected are
    the frozen-sphere expectations (test_gpu_capsule.py) with g = 0 on the humanoid's rows and with g on the ball's.
    Every perturbed configuration freezes a model of its own."""
    model, cfg = punyo()
    N = 20
    q = punyo_trajectory(cfg, model, N, 0)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = "forward_differences"
    v, a, tau_g, free_g, Pg = frozen_expectation(all_gravity(model), prob, sp, q)
    _, _, tau_0, free_0, P0 = frozen_expectation(no_gravity(model), prob, sp, q)
    tau, tau_free = tau_g.copy(), free_g.copy()
    tau[:, :HUMANOID], tau_free[:, :HUMANOID] = tau_0[:, :HUMANOID], free_0[:, :HUMANOID]
    # (capsules act: their contact changes tau at most time steps - and their length matters: the spheres at the
    # capsules' centres give another tau)
    acting = np.abs(tau - tau_free).max(axis=1) > 1e-3
    assert np.count_nonzero(acting) >= N // 2, np.count_nonzero(acting)
    tau_spheres = Oracle(as_spheres(no_gravity(model)), prob, sp).eval_traj(q)[2]
    assert np.abs(tau[:, :HUMANOID] - tau_spheres[:, :HUMANOID]).max() > 1e-3
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("v"), v) and same(dev.get("a"), a)
    got = dev.get("tau")
    scale = np.maximum(np.abs(tau).max(axis=1), 1.0)
    err = np.abs(got - tau).max(axis=1)
    print("tau: largest error / scale", (err / scale).max())
    assert np.all(err <= TAU_REL * scale), (err / scale).max()
    dev.eval_partials()
    for k in PARTIALS:
        w = Pg[k].copy()
        w[:, :HUMANOID, :] = P0[k][:, :HUMANOID, :]
        g = dev.get(k)
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), k
        bound = BLOCK_REL * max(np.abs(w[~nan]).max(), 1.0)
        print(k, "largest error", np.abs(g - w)[~nan].max(), "bound", bound)
        assert np.abs(g - w)[~nan].max() <= bound, (k, np.abs(g - w)[~nan].max(), bound)
    dev.close()


# ---- 4. which kernels
EXAMPLE_SHAPES = {"jaco": 6, "jaco_ball": 6, "dual_jaco": 0, "spinner_capsule": 0, "2dof_spinner_capsule": 0}


def _shape(model, cfg):
    prob, sp, _ = make_problem(cfg, model, num_steps=4)
    dev = hip.HipPath(model, prob, sp)
    shape = dev.get_option("fast_shape")
    dev.close()
    return shape


def test_stem_length_one_takes_the_kernels_it_took():
    for name, shape in SHAPES.items():
        assert _shape(load_model(name), load_config(name)) == shape, name
    for name, shape in EXAMPLE_SHAPES.items():
        model, cfg = example(name)
        assert _shape(model, cfg or TWO_DOF_CFG) == shape, name
    model, cfg = punyo()
    assert _shape(model, cfg) == 0
    cfg, _, stems = jaco_chain_and_stems()
    assert _shape(stems[2], cfg) == 0


# ---- 5. launch forms, refusals
def test_batch_equals_single_contexts():
    model, cfg = punyo()
    N, B = 12, 3
    probs, qs = [], []
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.scaling = sp.equality_constraints = False
        prob.q_nom = prob.q_nom + 0.01 * b
        probs.append(prob)
        qs.append(punyo_trajectory(cfg, model, N, b))
    batch = hip.HipPath(model, probs, sp)
    batch.set_q_batch(np.array(qs))
    batch.gn_step()
    arrays = ("v", "a", "tau", "dtau_dqm", "dtau_dqt", "dtau_dqp", "gradient", "H_A", "H_B", "H_C", "step")
    got = {(k, b): batch.get(k, b) for k in arrays for b in range(B)}
    batch.close()
    for b in range(B):
        one = hip.HipPath(model, probs[b], sp)
        one.set_q(qs[b])
        one.gn_step()
        for k in arrays:
            assert same(got[(k, b)], one.get(k)), (k, b)
        one.close()


def solve(model, prob, sp, q_guess):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    return flag, sol, st


def test_resident_loop_equals_stepwise_loop(monkeypatch):
    """test_gpu_trust_region.py::test_resident_loop_equals_stepwise_loop's check (the unconstrained loop, as there), on
    punyo with the example's scaling"""
    model, cfg = punyo()
    prob, sp, q_guess = make_problem(cfg, model, num_steps=20)
    sp.equality_constraints = False
    sp.max_iterations, sp.verbose = 8, False
    monkeypatch.delenv("IDTO_OPT_STEPWISE", raising=False)
    a_flag, a_sol, a_st = solve(model, prob, sp, q_guess)
    monkeypatch.setenv("IDTO_OPT_STEPWISE", "1")
    b_flag, b_sol, b_st = solve(model, prob, sp, q_guess)
    assert a_flag == b_flag
    for series in ("iteration_costs", "trust_region_radii", "trust_ratios", "q_norms", "dq_norms", "dqH_norms",
                   "gradient_norms", "dL_dqs", "h_norms", "merits"):
        x, y = getattr(a_st, series), getattr(b_st, series)
        assert x.size == 8 and np.array_equal(x, y), (series, x, y)
    assert np.array_equal(a_sol.q, b_sol.q) and np.array_equal(a_sol.v, b_sol.v) and np.array_equal(a_sol.tau, b_sol.tau)


@pytest.mark.parametrize("key", sorted(BAD_STEM))
def test_bad_stems_are_refused_by_create(key):
    good, m = bad_stem_model(key)
    prob, sp, _ = make_problem(punyo()[1], good, num_steps=4)
    with pytest.raises(hip.HipError, match=BAD_STEM[key][2]):
        hip.HipPath(m, prob, sp)


# ---- 6. the solve
def test_punyo_solve_as_the_example_runs_it(record_property):
    """punyo.yaml: trust region, scaling, equality constraints on the ball's DoFs, N = 40, 50 iterations"""
    model, cfg = punyo()
    prob, sp, q_guess = make_problem(cfg, model)
    assert prob.num_steps == 40 and sp.max_iterations == 50 and sp.equality_constraints and sp.scaling
    sp.verbose = False
    flag, sol, st = solve(model, prob, sp, q_guess)
    costs = np.array(st.iteration_costs)
    record_property("solve", dict(flag=str(flag), iterations=len(costs), cost_first=float(costs[0]),
                                  cost_last=float(costs[-1]), h_first=float(st.h_norms[0]), h_last=float(st.h_norms[-1]),
                                  ms_per_iteration=float(np.median(st.iteration_times) * 1e3)))
    print("punyo solve:", flag, len(costs), "iterations, cost", costs[0], "->", costs[-1], "h", st.h_norms[0], "->",
          st.h_norms[-1], "ms / iteration", np.median(st.iteration_times) * 1e3)
    assert flag != "kFactorizationFailed"
    assert flag == "kMaxIterationsReached" and len(costs) == 50
    assert np.all(np.isfinite(costs)) and np.all(np.isfinite(sol.q))
    assert costs[-1] < costs[0]


def test_zero_length_all_gravity_solve_tracks_the_oracle():
    """the first iterations follow Oracle.solve within the tolerances of test_gpu_optimizer.py::test_solve_tracks_the_oracle"""
    model, cfg = punyo()
    dev_model, orc_model = zero_length(all_gravity(model)), as_spheres(all_gravity(model))
    prob, sp, q_guess = make_problem(cfg, orc_model)
    sp.max_iterations, sp.verbose, sp.num_threads = 4, False, 1
    ref = Oracle(orc_model, prob, sp).solve(q_guess)
    flag, sol, st = solve(dev_model, prob, sp, q_guess)
    assert len(st.iteration_costs) == 4 and flag == "kMaxIterationsReached"
    rc = ref["stats"]
    assert np.allclose(st.iteration_costs, rc.iteration_costs, rtol=1e-6), (st.iteration_costs, rc.iteration_costs)
    assert np.allclose(st.trust_region_radii, rc.trust_region_radii, rtol=1e-12)
    assert np.allclose(st.h_norms, rc.h_norms, rtol=1e-5, atol=1e-9)
    assert np.abs(sol.q - ref["q"]).max() <= 1e-5 * max(1.0, np.abs(ref["q"]).max())
    assert st.iteration_costs[-1] <= st.iteration_costs[0]
