"""The per-body gravity switch on the device (idto_model_t::gravity_enabled) and the Jaco example fixtures.

The oracle has one gravity vector.  The arm of a Jaco fixture hangs off the world, so no force of the arm reaches the
object's rows, and contact forces do not depend on g: the expected tau and partials are the oracle's with g = 0 on the
arm's rows and the oracle's with g on the object's rows."""
import copy
import json
import os
from dataclasses import fields

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import Model, iptr, load_model
from idto_amd.optimizer import TrajectoryOptimizer, TrajectoryOptimizerSolution, TrajectoryOptimizerStats
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_gpu_fast_shape import ARRAYS, outputs, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
ARM_ROWS = slice(0, 7)
PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")


def example(name):
    return load_model(os.path.join(EXAMPLES, name + ".model")), load_config(os.path.join(EXAMPLES, name + ".yaml"))


def no_gravity(model):
    m = copy.deepcopy(model)
    m.gravity = np.zeros(3)
    m.gravity_enabled = None
    return m.normalize()


@pytest.mark.parametrize("name,N", [("jaco", 40), ("jaco_ball", 10)])
@pytest.mark.parametrize("seed", [0, 5])
@pytest.mark.parametrize("method", ["forward_differences", "central_differences", "central_differences4"])
def test_jaco_equals_the_oracle_composition(name, N, seed, method):
    model, cfg = example(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = method
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.0)
    orc_g, orc_0 = Oracle(model, prob, sp), Oracle(no_gravity(model), prob, sp)
    v, _, tau_g, _ = orc_g.eval_traj(q)
    tau_0 = orc_0.eval_traj(q)[2]
    tau = tau_g.copy()
    tau[:, ARM_ROWS] = tau_0[:, ARM_ROWS]
    assert not same(tau, tau_g)   # (the arm's weight is there in the oracle's own tau)
    Pg, P0 = orc_g.eval_partials(q), orc_0.eval_partials(q)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.eval_tau()
    assert same(dev.get("tau"), tau)
    assert dev.get("cost") == orc_g.calc_cost(q, v, tau)
    dev.eval_partials()
    for k in PARTIALS:
        want = Pg[k].copy()
        want[:, ARM_ROWS, :] = P0[k][:, ARM_ROWS, :]
        assert same(dev.get(k), want), k
    assert same(dev.get("tau"), tau)
    dev.close()


@pytest.mark.parametrize("name,N", [("jaco", 40), ("jaco_ball", 10)])
@pytest.mark.parametrize("method", [0, 1])
def test_jaco_fast_shape_gives_the_generic_bits(name, N, method):
    model, cfg = example(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=3, lower=0.0)
    shape, fast = outputs(model, prob, sp, q, 1, method)
    assert shape == 6
    _, generic = outputs(model, prob, sp, q, 0, method)
    for k in fast:
        assert same(fast[k], generic[k]), k


def solve(model, prob, sp, q_guess):
    opt = TrajectoryOptimizer(model, prob, sp)
    sol, st = TrajectoryOptimizerSolution(), TrajectoryOptimizerStats()
    flag = opt.Solve(q_guess, sol, st)
    opt.close()
    return flag, sol, st


STATS_ROWS = ("iteration_costs", "trust_region_radii", "q_norms", "dq_norms", "dqH_norms", "trust_ratios",
              "gradient_norms", "dL_dqs", "h_norms", "merits", "linesearch_iterations", "linesearch_alphas")


def stats_rows(st):
    return {k: np.array(getattr(st, k)) for k in STATS_ROWS}


def all_off(model):
    m = copy.deepcopy(model)
    m.gravity_enabled = np.zeros(m.nbodies, dtype=np.int32)
    return m.normalize()


@pytest.mark.parametrize("name,N", [("hopper", 20), ("mini_cheetah", 12)])
def test_every_body_off_equals_zero_gravity(name, N):
    cfg, model = load_config(name), load_model(name)
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=1, lower=0.01)
    for fast in (1, 0):
        s_off, off = outputs(all_off(model), prob, sp, q, fast)
        s_zero, zero = outputs(no_gravity(model), prob, sp, q, fast)
        assert s_off == 0 and s_zero != 0   # (shapes 1 - 5 are for models whose every body has gravity)
        for k in ARRAYS + ("tau_only", "cost"):
            assert same(off[k], zero[k]), k
    prob, sp, q_guess = make_problem(cfg, model)
    sp.max_iterations = 5
    _, _, st_off = solve(all_off(model), prob, sp, q_guess)
    _, _, st_zero = solve(no_gravity(model), prob, sp, q_guess)
    a, b = stats_rows(st_off), stats_rows(st_zero)
    for k in STATS_ROWS:
        assert same(a[k], b[k]), k


class ExplicitOnes(Model):
    """to_c() hands an explicit all-ones array instead of NULL"""

    def to_c(self):
        m, keep = super().to_c()
        keep["gravity_enabled_explicit"] = np.ones(self.nbodies, dtype=np.int32)
        m.gravity_enabled = iptr(keep["gravity_enabled_explicit"])
        return m, keep


def explicit_ones(model):
    return ExplicitOnes(**{f.name: copy.deepcopy(getattr(model, f.name)) for f in fields(model)}).normalize()


@pytest.mark.parametrize("name,N", [("acrobot", 40), ("spinner", 40), ("hopper", 20), ("mini_cheetah", 12),
                                    ("allegro_hand", 8)])
def test_all_on_equals_null(name, N):
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=2, lower=0.0)
    s_null, null = outputs(model, prob, sp, q, 1)
    s_ones, ones = outputs(explicit_ones(model), prob, sp, q, 1)
    assert s_null == s_ones != 0
    for k in null:
        assert same(null[k], ones[k]), k
    # the whole solve (the small models' one-launch iteration, the resident trust-region loop) on the default YAML
    prob, sp, q_guess = make_problem(cfg, model)
    sp.max_iterations = 4
    _, _, st_null = solve(model, prob, sp, q_guess)
    _, _, st_ones = solve(explicit_ones(model), prob, sp, q_guess)
    a, b = stats_rows(st_null), stats_rows(st_ones)
    for k in STATS_ROWS:
        assert same(a[k], b[k]), k


@pytest.mark.parametrize("name", ["jaco", "jaco_ball"])
def test_jaco_solve_end_to_end(name, record_property):
    model, cfg = example(name)
    prob, sp, q_guess = make_problem(cfg, model)
    assert sp.equality_constraints
    flag, sol, st = solve(model, prob, sp, q_guess)
    costs = np.array(st.iteration_costs)
    h = np.array(st.h_norms)
    times = np.array(st.iteration_times)
    rec = dict(model=name, N=prob.num_steps, flag=str(flag), iterations=len(costs), cost_first=float(costs[0]),
               cost_last=float(costs[-1]), h_first=float(h[0]), h_last=float(h[-1]),
               ms_per_iteration=float(np.median(times) * 1e3), solve_time_s=float(st.solve_time),
               max_cost_rise=float(np.max(np.diff(costs))))
    record_property("solve", rec)
    print("jaco solve:", json.dumps(rec))
    assert len(costs) > 1 and np.all(np.isfinite(costs)) and np.all(np.isfinite(h))
    # (iteration_costs changes only when a step is accepted.  With the enforced constraints a step is accepted on the
    # merit function, not on the cost: jaco_ball's cost rises by up to 4.6e-5 on an accepted step while h falls, so the
    # cost is held to an overall fall here, not to a monotone one)
    assert costs[-1] < 0.1 * costs[0], (costs[0], costs[-1])
    # the constraint violation falls by more than an order of magnitude (jaco: 21 -> 1.2 in 50 iterations, jaco_ball:
    # 6.2 -> 3e-5)
    assert h[-1] < 0.1 * h[0], (h[0], h[-1])
