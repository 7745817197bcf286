"""Capsules on the device (include/idto_model.h, csrc/id_eval.h): each capsule side of a pair becomes a sphere at a
substitute centre, then the sphere / box expressions run unchanged.

* A zero-length capsule is its sphere: every output equals the sphere model's and the oracle's bit for bit.
* The oracle knows no capsules.  A model with real capsules is compared with the oracle evaluating a FROZEN sphere model
  (capsule_ref.frozen_sphere_model): one sphere per pair side at the substitute centre of the configuration being
  evaluated, frozen again at every perturbed configuration of the forward differences."""
import copy
import os

import numpy as np
import pytest

import capsule_ref as cr
from capsule_ref import frozen_expectation  # noqa: F401  (test_gpu_stem.py imports it from here)
from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_gpu_fast_shape import same
from test_model_cross_pairs import dual_jaco, touching_trajectory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")
ARRAYS = ("v", "a", "tau") + PARTIALS + ("gradient", "H_A", "H_B", "H_C")


def example(name):
    cfg = os.path.join(EXAMPLES, name + ".yaml")
    return load_model(os.path.join(EXAMPLES, name + ".model")), (load_config(cfg) if os.path.exists(cfg) else None)


def all_gravity(model):
    m = copy.deepcopy(model)
    m.gravity_enabled = None
    return m.normalize()


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def zero_length_capsules(model, seed):
    """every sphere replaced by a capsule with h = 0 and a random axis"""
    m = copy.deepcopy(model)
    rng = np.random.default_rng(seed)
    for g in range(m.ngeoms):
        if int(m.geom_type[g]) == cr.SPHERE:
            m.geom_type[g] = cr.CAPSULE
            m.geom_size[g] = [m.geom_size[g][0], 0.0, 0.0]
            m.geom_X[g][:9] = random_rotation(rng).ravel()
    return m.normalize()


def device_outputs(model, prob, sp, q):
    dev = hip.HipPath(model, prob, sp)
    shape = dev.get_option("fast_shape")
    dev.set_q(q)
    dev.gn_step()
    out = {k: dev.get(k) for k in ARRAYS}
    dev.close()
    return shape, out


def zero_length_case(name):
    if name == "spinner_sphere":
        cfg, model, N = load_config("spinner"), load_model("spinner_sphere"), 20
        q = synthetic_trajectory(cfg, model, N, seed=0)
        q[:, 1] = np.linspace(1.5, 1.25, N + 1)
    elif name == "hopper":
        cfg, model, N = load_config("hopper"), load_model("hopper"), 20
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
    elif name == "jaco_ball":
        model, cfg = example("jaco_ball")
        model, N = all_gravity(model), 10
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
    else:
        model, cfg = dual_jaco()
        model, N = all_gravity(model), 20
        q = touching_trajectory(model, cfg, N, 0)
    return model, cfg, N, q


@pytest.mark.parametrize("method", ["forward_differences", "central_differences"])
@pytest.mark.parametrize("name", ["spinner_sphere", "hopper", "jaco_ball", "dual_jaco"])
def test_zero_length_capsules_are_spheres(name, method):
    """v, a, tau, the three dtau/dq blocks, g and H of the model whose spheres are capsules with h = 0 (and a random axis)
    == the sphere model's device outputs == the oracle's"""
    model, cfg, N, q = zero_length_case(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = method
    caps = zero_length_capsules(model, seed=3)
    shape_c, got = device_outputs(caps, prob, sp, q)
    assert shape_c == 0
    _, want = device_outputs(model, prob, sp, q)
    for k in ARRAYS:
        assert same(got[k], want[k]), k
    orc = Oracle(model, prob, sp)
    v, a, tau, _ = orc.eval_traj(q)
    assert same(got["v"], v) and same(got["a"], a) and same(got["tau"], tau)
    P = orc.eval_partials(q)
    for k in PARTIALS:
        assert same(got[k], P[k]), k
    g, bands = orc.grad_hess(q)
    assert same(got["gradient"], g)
    assert same(got["H_A"], bands[0]) and same(got["H_B"], bands[1]) and same(got["H_C"], bands[2])


# ---- capsules with length, against the oracle on frozen sphere models
def hopper_capsule_foot():
    """the hopper with its two foot spheres replaced by one capsule between their centres (axis = the segment, the frame
    turned about it)"""
    m = copy.deepcopy(load_model("hopper"))
    c0, c1 = np.asarray(m.geom_X[0][9:], float), np.asarray(m.geom_X[1][9:], float)
    u = (c1 - c0) / np.linalg.norm(c1 - c0)
    assert np.allclose(u, [0, 0, 1])
    ca, sa = np.cos(0.7), np.sin(0.7)
    R = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]])
    m.geom_body = [m.geom_body[0], m.geom_body[2]]
    m.geom_type = [cr.CAPSULE, cr.BOX]
    m.geom_size = [[m.geom_size[0][0], np.linalg.norm(c1 - c0) / 2, 0.0], m.geom_size[2]]
    m.geom_X = [np.concatenate([R.ravel(), (c0 + c1) / 2]), m.geom_X[2]]
    m.pair_a, m.pair_b, m.pair_path = [0], [1], [0]
    return m.normalize()


def dual_jaco_capsule_hand():
    """dual_jaco (every body's weight on) with the left hand's tip sphere a capsule, its axis tilted in the link frame:
    it meets the other arm's spheres through the shared pairs (fd_kernel<8, SHAPE_XCH>)"""
    m = all_gravity(dual_jaco()[0])
    g = 2
    assert int(m.geom_type[g]) == cr.SPHERE and int(m.geom_body[g]) == 6
    c, s = np.cos(0.5), np.sin(0.5)
    m.geom_type[g] = cr.CAPSULE
    m.geom_size[g] = [m.geom_size[g][0], 0.03, 0.0]
    m.geom_X[g][:9] = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]).ravel()
    return m.normalize()


TWO_DOF_CFG = dict(q_init=[1.0, 0.0], v_init=[0.0, 0.0], q_nom_start=[1.0, 0.0], q_nom_end=[1.0, 1.0], q_guess=[1.0, 0.0],
                   Qq=[1, 1], Qv=[0.1, 0.1], R=[0.1, 1e3], Qfq=[10, 10], Qfv=[0.1, 0.1], time_step=0.05, num_steps=20,
                   contact_stiffness=200, dissipation_velocity=0.1, smoothing_factor=0.01, friction_coefficient=0.5,
                   stiction_velocity=0.05)


def frozen_case(name):
    if name == "spinner_capsule":
        model, cfg = example(name)
        N = 40
        q = synthetic_trajectory(cfg, model, N, seed=0)
        q[:, 1] = np.linspace(1.5, 1.25, N + 1)
        q[:, 2] = np.linspace(0.0, 1.2, N + 1)
    elif name == "2dof_spinner_capsule":
        model, _ = example(name)
        cfg, N = TWO_DOF_CFG, 20
        q = synthetic_trajectory(cfg, model, N, seed=1)
        q[:, 0] = np.linspace(1.0, 1.4, N + 1)   # (the two capsules 1 - 4.5 cm into each other)
        q[:, 1] = np.linspace(0.0, 0.3, N + 1)
    elif name == "hopper_capsule_foot":
        cfg, model, N = load_config("hopper"), hopper_capsule_foot(), 20
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
        q[1:, 2] += np.linspace(0.0, 0.4, N)   # (the foot tilts: the lower end changes along the way)
    else:
        model, cfg = dual_jaco_capsule_hand(), dual_jaco()[1]
        N = 20
        q = touching_trajectory(all_gravity(dual_jaco()[0]), cfg, N, 0)
    return model, cfg, N, q


# Tolerances.  The device forms each substitute centre with its own fused operations, the frozen model holds the same
# point as body coordinates that the oracle maps back to the world: the two centres differ by a few ulp of the
# coordinates (~1e-16 m), and tau then by (force per metre) x (that offset) x (lever arm).  TAU_REL bounds that relative
# to the largest tau of the time step.  A difference quotient divides two such errors by dq ~ 1.5e-8,
# i.e. multiplies them by ~1e8: 1e-12 of tau becomes ~1e-4 of tau in a dtau/dq entry, about 1e-6 of the largest entry of
# a block (the blocks' largest entries are the contact stiffness times lever arms, ~1e2 x tau).  BLOCK_REL bounds that.
TAU_REL, BLOCK_REL = 1e-12, 1e-6


@pytest.mark.parametrize("name", ["spinner_capsule", "2dof_spinner_capsule", "hopper_capsule_foot", "dual_jaco_capsule_hand"])
def test_capsules_equal_the_oracle_on_frozen_sphere_models(name):
    model, cfg, N, q = frozen_case(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = "forward_differences"
    v, a, tau, tau_free, P = frozen_expectation(model, prob, sp, q)
    # (the states make the capsules act: their contact changes tau at most time steps)
    acting = np.abs(tau - tau_free).max(axis=1) > 1e-3
    assert np.count_nonzero(acting) >= N // 2, np.count_nonzero(acting)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("v"), v) and same(dev.get("a"), a)
    got = dev.get("tau")
    scale = np.maximum(np.abs(tau).max(axis=1), 1.0)
    err = np.abs(got - tau).max(axis=1)
    assert np.all(err <= TAU_REL * scale), (err / scale).max()
    dev.eval_partials()
    for k in PARTIALS:
        g, w = dev.get(k), P[k]
        nan = np.isnan(w)   # (the oracle's NaN entries: blocks the reference leaves undefined)
        assert np.array_equal(np.isnan(g), nan), k
        bound = BLOCK_REL * max(np.abs(w[~nan]).max(), 1.0)
        assert np.abs(g - w)[~nan].max() <= bound, (k, np.abs(g - w)[~nan].max(), bound)
    dev.close()


# ---- launch forms and the solve on spinner_capsule
def spinner_capsule_problem(N, seed=0):
    model, cfg = example("spinner_capsule")
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    q = synthetic_trajectory(cfg, model, N, seed=seed)
    q[:, 1] = np.linspace(1.5, 1.25, N + 1)
    return model, cfg, prob, sp, q


@pytest.mark.parametrize("reference_solver", [1, 0])
def test_batch_equals_single_contexts(reference_solver):
    """every output of a batch == the single contexts'.  The step too with the reference-order solver.  With the default
    solvers a single small problem without a fast shape factors with the scalar band kernel and a batch with the blocked
    LDL^T: the two steps then differ by the solves' round-off times the condition of H (measured 8e-11 of the step's
    largest entry here), so they are held to 1e-9 of it"""
    model, cfg, _, sp, _ = spinner_capsule_problem(40)
    sp.scaling = sp.equality_constraints = False
    N, B = 40, 3
    probs, qs = [], []
    for b in range(B):
        prob, _, _ = make_problem(cfg, model, num_steps=N)
        prob.q_nom = prob.q_nom + 0.01 * b
        probs.append(prob)
        qs.append(spinner_capsule_problem(N, seed=b)[4])
    batch = hip.HipPath(model, probs, sp)
    assert batch.get_option("fast_shape") == 0
    batch.set_option("reference_solver", reference_solver)
    batch.set_q_batch(np.array(qs))
    batch.gn_step()
    arrays = ARRAYS + ("step",)
    got = {(k, b): batch.get(k, b) for k in arrays for b in range(B)}
    batch.close()
    for b in range(B):
        one = hip.HipPath(model, probs[b], sp)
        one.set_option("reference_solver", reference_solver)
        one.set_q(qs[b])
        one.gn_step()
        for k in ARRAYS:
            assert same(got[(k, b)], one.get(k)), (k, b)
        step = one.get("step")
        if reference_solver:
            assert same(got[("step", b)], step), b
        else:
            assert np.abs(got[("step", b)] - step).max() <= 1e-9 * np.abs(step).max(), b
        one.close()


def solve(model, prob, sp, q_guess):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    return flag, sol, st


def test_resident_loop_equals_stepwise_loop(monkeypatch):
    """test_gpu_trust_region.py::test_resident_loop_equals_stepwise_loop's check, on spinner_capsule"""
    model, cfg = example("spinner_capsule")
    prob, sp, q_guess = make_problem(cfg, model, num_steps=20)
    sp.equality_constraints = False
    sp.max_iterations, sp.verbose = 12, False
    sp.scaling, sp.scaling_method = True, "sqrt"
    monkeypatch.delenv("IDTO_OPT_STEPWISE", raising=False)
    a_flag, a_sol, a_st = solve(model, prob, sp, q_guess)
    monkeypatch.setenv("IDTO_OPT_STEPWISE", "1")
    b_flag, b_sol, b_st = solve(model, prob, sp, q_guess)
    assert a_flag == b_flag
    for series in ("iteration_costs", "trust_region_radii", "trust_ratios", "q_norms", "dq_norms", "dqH_norms",
                   "gradient_norms", "dL_dqs", "h_norms", "merits"):
        x, y = getattr(a_st, series), getattr(b_st, series)
        assert x.size == 12 and np.array_equal(x, y), (series, x, y)
    assert np.array_equal(a_sol.q, b_sol.q) and np.array_equal(a_sol.v, b_sol.v) and np.array_equal(a_sol.tau, b_sol.tau)


def test_spinner_capsule_solve_end_to_end(record_property):
    """the fixture with the spinner example's YAML: max_iters iterations, finite statistics, the cost falls"""
    model, cfg = example("spinner_capsule")
    prob, sp, q_guess = make_problem(cfg, model)
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
