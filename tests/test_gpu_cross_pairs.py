"""Shared pairs on the device: contact pairs between the chains of two paths (include/idto_model.h), evaluated by
fd_kernel<8, SHAPE_XCH> through the exchange area of id_eval<MAXC, true>.

The fixture dual_jaco switches both arms' weight off.  The oracle has one gravity vector, but the arms hang off the world
and contact forces do not depend on g, so the expected arrays are the oracle's with g = 0 on the arms' rows and the
oracle's with g on the box's rows (the argument of test_gpu_gravity_switch.py).  The trajectories are chosen so that the
shared pairs act (test_model_cross_pairs.py checks that with the oracle)."""
import copy
from dataclasses import fields

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import Model, load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_gpu_fast_shape import same
from test_model_cross_pairs import ARMS, drop_pairs, dual_jaco, shared_pairs, touching_trajectory

pytestmark = pytest.mark.gpu

PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")


def no_gravity(model):
    m = copy.deepcopy(model)
    m.gravity = np.zeros(3)
    m.gravity_enabled = None
    return m.normalize()


def all_gravity(model):
    m = copy.deepcopy(model)
    m.gravity_enabled = None
    return m.normalize()


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("method", ["forward_differences", "central_differences", "central_differences4"])
def test_dual_jaco_equals_the_oracle_composition(seed, method):
    model, cfg = dual_jaco()
    N = 20
    q = touching_trajectory(model, cfg, N, seed)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = method
    orc_g, orc_0 = Oracle(model, prob, sp), Oracle(no_gravity(model), prob, sp)
    v, a, tau_g, _ = orc_g.eval_traj(q)
    tau = tau_g.copy()
    tau[:, :ARMS] = orc_0.eval_traj(q)[2][:, :ARMS]
    # (without the shared pairs the arms' rows would differ: the trajectory makes them act)
    tau_cut = Oracle(drop_pairs(no_gravity(model), shared_pairs(model)), prob, sp).eval_traj(q)[2]
    assert not same(tau[:, :ARMS], tau_cut[:, :ARMS])
    Pg, P0 = orc_g.eval_partials(q), orc_0.eval_partials(q)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("tau"), tau)
    assert same(dev.get("v"), v) and same(dev.get("a"), a)
    for t in range(N + 1):
        assert same(dev.get("nplus")[t], orc_g.nplus(q[t]))
    assert dev.get("cost") == orc_g.calc_cost(q, v, tau)
    dev.eval_partials()
    for k in PARTIALS:
        want = Pg[k].copy()
        want[:, :ARMS, :] = P0[k][:, :ARMS, :]
        assert same(dev.get(k), want), k
    assert same(dev.get("tau"), tau)
    dev.close()


def test_all_gravity_dual_jaco_equals_the_oracle():
    """gravity_enabled = None: the oracle applies as it stands - gradient, Hessian bands and the reference-order step"""
    model, cfg = dual_jaco()
    model = all_gravity(model)
    N = 20
    q = touching_trajectory(model, cfg, N, 0)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    orc = Oracle(model, prob, sp)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q(q)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    assert same(dev.get("tau"), orc.eval_traj(q)[2])
    g, bands = orc.grad_hess(q)
    assert same(dev.get("gradient"), g)
    assert same(dev.get("H_A"), bands[0]) and same(dev.get("H_B"), bands[1]) and same(dev.get("H_C"), bands[2])
    _, p = orc.gn_step(q)
    assert same(dev.get("step"), p)
    dev.close()


FEET = (1, 2, 3, 4)   # mini_cheetah: the foot spheres of shank_fl, shank_fr, shank_hl, shank_hr (paths 0-3)


def cheetah_with_foot_pairs():
    """mini_cheetah (K = 4, a floating common body, chains of 3) with a pair between every two feet: shared pairs of
    every two paths next to each path's pairs onto the common body and the ground"""
    m = copy.deepcopy(load_model("mini_cheetah"))
    extra = [(a, b) for i, a in enumerate(FEET) for b in FEET[i + 1:]]
    m.pair_a = np.concatenate([m.pair_a, [a for a, _ in extra]])
    m.pair_b = np.concatenate([m.pair_b, [b for _, b in extra]])
    m.pair_path = np.concatenate([m.pair_path, [int(m.body_path[int(m.geom_body[a])]) for a, _ in extra]])
    return m.normalize()


@pytest.mark.parametrize("method", ["forward_differences", "central_differences"])
def test_cheetah_feet_pairs_equal_the_oracle(method):
    model = cheetah_with_foot_pairs()
    assert len(shared_pairs(model)) == 6
    cfg = load_config("mini_cheetah")
    N = 12
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.smoothing_factor = 0.05   # (the feet are 0.2 - 0.4 m apart: the force reaches ~1.6 m)
    sp.gradients_method = method
    q = synthetic_trajectory(cfg, model, N, seed=4, lower=0.01)
    orc = Oracle(model, prob, sp)
    v, a, tau, cost = orc.eval_traj(q)
    tau_cut = Oracle(drop_pairs(model, shared_pairs(model)), prob, sp).eval_traj(q)[2]
    assert np.abs(tau - tau_cut).max() > 1e-3
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


def test_batch_equals_single_contexts():
    model, cfg = dual_jaco()
    N, B = 20, 3
    probs, qs = [], []
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.scaling = sp.equality_constraints = False
        prob.q_nom = prob.q_nom + 0.01 * b
        probs.append(prob)
        qs.append(touching_trajectory(model, cfg, N, b))
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


class Unvalidated(Model):
    """hands its tables to idto_hip_create without Model.validate (which would refuse them first)"""

    def validate(self):
        pass


def test_a_shared_pair_on_a_third_path_is_refused():
    model = cheetah_with_foot_pairs()
    k = shared_pairs(model)[0]   # feet of paths 0 and 1
    m = Unvalidated(**{f.name: copy.deepcopy(getattr(model, f.name)) for f in fields(model)})
    m.pair_path[k] = 2
    prob, sp, _ = make_problem(load_config("mini_cheetah"), model, num_steps=4)
    with pytest.raises(hip.HipError, match="pair touches a body outside its path"):
        hip.HipPath(m, prob, sp)


def solve(model, prob, sp, q_guess):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    return flag, sol, st


def test_all_gravity_solve_tracks_the_oracle():
    """from a touching guess, 5 iterations, the tolerances of test_gpu_optimizer.py::test_solve_tracks_the_oracle"""
    model, cfg = dual_jaco()
    model = all_gravity(model)
    prob, sp, _ = make_problem(cfg, model)
    sp.max_iterations, sp.verbose, sp.num_threads = 5, False, 1
    # (the guess starts at q_init, as the solver requires, and reaches the touching trajectory over five steps)
    touch = touching_trajectory(model, cfg, prob.num_steps, 1)
    w = np.minimum(1.0, np.arange(prob.num_steps + 1) / 5.0)[:, None]
    q_guess = prob.q_init + w * (touch - prob.q_init)
    ref = Oracle(model, prob, sp).solve(q_guess)
    flag, sol, st = solve(model, prob, sp, q_guess)
    assert len(st.iteration_costs) == 5 and flag == "kMaxIterationsReached"
    rc = ref["stats"]
    assert np.allclose(st.iteration_costs, rc.iteration_costs, rtol=1e-6), (st.iteration_costs, rc.iteration_costs)
    assert np.allclose(st.trust_region_radii, rc.trust_region_radii, rtol=1e-12)
    assert np.allclose(st.h_norms, rc.h_norms, rtol=1e-5, atol=1e-9)
    assert np.abs(sol.q - ref["q"]).max() <= 1e-5 * max(1.0, np.abs(ref["q"]).max())
    assert st.iteration_costs[-1] <= st.iteration_costs[0]


def test_dual_jaco_solve_as_the_example_runs_it(record_property):
    """the fixture's gravity flags and YAML parameters, N = 20, 50 iterations"""
    model, cfg = dual_jaco()
    prob, sp, q_guess = make_problem(cfg, model)
    assert prob.num_steps == 20 and sp.max_iterations == 50
    flag, sol, st = solve(model, prob, sp, q_guess)
    costs = np.array(st.iteration_costs)
    record_property("solve", dict(flag=str(flag), iterations=len(costs), cost_first=float(costs[0]),
                                  cost_last=float(costs[-1]), ms_per_iteration=float(np.median(st.iteration_times) * 1e3)))
    assert flag == "kMaxIterationsReached" and len(costs) == 50
    for k in ("iteration_costs", "trust_region_radii", "q_norms", "dq_norms", "gradient_norms", "dL_dqs", "h_norms",
              "merits", "iteration_times"):
        assert np.all(np.isfinite(np.array(getattr(st, k)))), k
    assert np.all(np.isfinite(sol.q))
    assert costs[-1] <= costs[0]
