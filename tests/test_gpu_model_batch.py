"""A batch whose problems have models, gravity and contact parameters of their own (idto_hip_set_model_batch,
HipPath.set_model_batch): entry b of the batch must come out bit-identical (==) to the same problem in a single-problem
context created with model b and contact parameters b - through every kernel fd_launch can select - and different from
the base model's entry, so that an implementation that ignores the records fails.

Shapes: N = 3, the shortest horizon at which the bands A, B and C all receive terms from three records (as
tests/test_gpu_fd_tail.py), B = 3 so that a wrong stride and a swapped index both show; variants sit at b = 1 and 2,
b = 0 keeps the base model."""
import copy
import os

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_gpu_batch import ARRAYS, _same
from test_model_stem import punyo_trajectory

pytestmark = pytest.mark.gpu

EXAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "examples")
N, B = 3, 3
FREE_TABLES = ("X_PF", "axis", "mass", "com", "inertia", "damping", "geom_X", "geom_size")
CONTACT = ("contact_stiffness", "dissipation_velocity", "stiction_velocity", "friction_coefficient", "smoothing_factor")
# the models the oracle evaluates as they are (no capsule, shared pair, stem or gravity switch)
ORACLE_MODELS = ("pendulum", "acrobot", "hopper", "mini_cheetah", "allegro_hand", "spinner")


# (the one-body pendulum has no example configuration: the generic kernel for chains of up to two bodies, <2, 0>)
PENDULUM_CFG = dict(q_init=[0.3], v_init=[0.1], q_nom_start=[0.3], q_nom_end=[1.0], q_guess=[0.8], Qq=[1.0], Qv=[0.1], R=[0.1],
                    Qfq=[10.0], Qfv=[0.1], time_step=0.05, num_steps=20)


def _load(name):
    if name == "pendulum":
        return load_model(name), PENDULUM_CFG
    if os.path.exists(os.path.join(EXAMPLES, name + ".model")):
        return load_model(os.path.join(EXAMPLES, name + ".model")), load_config(os.path.join(EXAMPLES, name + ".yaml"))
    return load_model(name), load_config(name)


def _variant(model, sp, seed, only=None):
    """model and parameters with every free table, gravity and the five contact parameters (only: that one alone) a few
    percent off, from a seeded generator"""
    rng = np.random.default_rng(seed)
    m, p = copy.deepcopy(model), copy.deepcopy(sp)

    def off(a):
        a = np.asarray(a, float)
        return a * (1.0 + 0.06 * (rng.random(a.shape) - 0.5))
    for f in FREE_TABLES:
        new = off(getattr(m, f))   # (drawn whether used or not: a field's variant is the same alone and among the others)
        if f == "geom_X" and m.ngeoms:   # a world-fixed box keeps its identity rotation: the pair checks ask for it
            fixed = np.asarray(m.geom_body) < 0
            new[fixed, :9] = np.asarray(m.geom_X, float)[fixed, :9]
        if f == "damping":   # (the examples' joints have none: a factor would leave the zeros)
            new = new + 0.01 * (1.0 + rng.random(new.shape))
        if f == "X_PF":   # ... and a floating joint its identity frame (Model.validate)
            floating = np.asarray(m.jtype) == 3
            new[floating] = np.asarray(m.X_PF, float)[floating]
        if only in (None, f):
            setattr(m, f, new)
    g = off(m.gravity) + np.array([0.2, -0.1, 0.0])   # (a slope)
    if only in (None, "gravity"):
        m.gravity = g
    for k in CONTACT:
        val = float(off(getattr(p, k)))
        if only in (None, k):
            setattr(p, k, val)
    return m.normalize(), p


def _case(name, n=N, nb=B):
    model, cfg = _load(name)
    probs, qs, sp = [], [], None
    for b in range(nb):
        prob, sp, _ = make_problem(cfg, model, num_steps=n)
        sp.scaling = False
        sp.equality_constraints = False
        prob.q_nom = prob.q_nom + 0.01 * b
        prob.v_init = prob.v_init + 0.05 * np.random.default_rng(100 + b).normal(size=model.nv)
        probs.append(prob)
        # held to contact, as tests/test_gpu_batch.py holds its trajectories
        qs.append(punyo_trajectory(cfg, model, n, b) if name == "punyo" else synthetic_trajectory(cfg, model, n, seed=b, lower=0.01))
    return model, probs, sp, np.array(qs)


def _outputs(dev, nb=None):
    """the cost after eval_tau, then every array of ARRAYS after gn_step: of a single context, or of each of the nb
    problems of a batch"""
    dev.eval_tau()
    costs = [dev.get("cost", b) for b in range(nb)] if nb else [dev.get("cost")]
    dev.gn_step()
    out = [dict({arr: dev.get(arr, b if nb else None) for arr in ARRAYS}, cost=costs[b]) for b in range(nb or 1)]
    return out if nb else out[0]


def _single(model, prob, sp, q, options):
    one = hip.HipPath(model, prob, sp)
    for k, v in options.items():
        one.set_option(k, v)
    one.set_q(q)
    out = _outputs(one)
    one.close()
    return out


def _equal(got, want, what):
    for k in want:
        assert _same(got[k], want[k]), (what, k)


def _differ(a, b):
    return not _same(a, b)


# one model per kernel fd_launch can select: the tree shapes 1 .. 6, the capsule spinner (no shape: <3, 0>), SHAPE_XCH,
# SHAPE_STEM, and the generic <2, 0>, <3, 0>, <4, 0>, <8, 0>
KERNELS = [("acrobot", 1), ("hopper", 1), ("mini_cheetah", 1), ("allegro_hand", 1), ("spinner", 1), ("jaco", 1),
           ("spinner_capsule", 1), ("dual_jaco", 1), ("punyo", 1),
           ("pendulum", 1), ("hopper", 0), ("mini_cheetah", 0), ("allegro_hand", 0), ("jaco", 0)]


@pytest.mark.parametrize("reference_solver", [0, 1])
@pytest.mark.parametrize("name,fd_fast", KERNELS)
def test_every_instantiation_reads_its_problems_record(name, fd_fast, reference_solver):
    model, probs, sp, qs = _case(name)
    options = {"reference_solver": reference_solver, "fd_fast": fd_fast}
    models, sps = [model], [sp]
    for b in range(1, B):
        m, p = _variant(model, sp, 1000 + b)
        models.append(m); sps.append(p)
    batch = hip.HipPath(model, probs, sp)
    for k, v in options.items():
        batch.set_option(k, v)
    assert batch.get_option("model_batch") == 0
    for b in range(1, B):
        batch.set_model_batch(b, models[b], sps[b])
    assert batch.get_option("model_batch") == 1
    batch.set_q_batch(qs)
    got = _outputs(batch, B)
    assert batch.solver_status_batch() == [False] * B
    if name in ("spinner", "acrobot"):
        assert batch.get_option("last_assembly") != 5   # gn_small stages the context's one model: it declined
    for b in range(B):
        _equal(got[b], _single(models[b], probs[b], sps[b], qs[b], options), (name, b))
    # the variants act: entries 1 and 2 are not what the base model gives their problems
    for b in range(1, B):
        assert _differ(got[b]["tau"], _single(model, probs[b], sp, qs[b], options)["tau"]), (name, b)
    # the last entry against the oracle on its model (reference-order solver: bit-exact step)
    if name in ORACLE_MODELS:
        g, p = Oracle(models[B - 1], probs[B - 1], sps[B - 1]).gn_step(qs[B - 1])
        assert _same(got[B - 1]["gradient"], g)
        if reference_solver:
            assert _same(got[B - 1]["step"], p)
    # contact acts: a variant that differs in the smoothing factor alone moves tau
    if model.npairs and reference_solver == 0:
        smooth = copy.deepcopy(sp)
        smooth.smoothing_factor = sp.smoothing_factor * 1.05
        batch.set_model_batch(1, None, smooth)
        batch.eval_tau()
        assert _differ(batch.get("tau", 1), _single(model, probs[1], sp, qs[1], options)["tau"]), name
        assert _same(batch.get("tau", 1), _single(model, probs[1], smooth, qs[1], options)["tau"]), name
    batch.close()


def test_each_free_field_alone():
    """one variant per free table, one for gravity, one per contact parameter: each entry == its single context and != the
    base model's - a field that stayed shared shows"""
    fields = list(FREE_TABLES) + ["gravity"] + list(CONTACT)
    model, probs, sp, qs = _case("hopper", nb=len(fields))
    batch = hip.HipPath(model, probs, sp)
    variants = [_variant(model, sp, 2000 + i, only=f) for i, f in enumerate(fields)]
    for b, (m, p) in enumerate(variants):
        batch.set_model_batch(b, m, p)
    batch.set_q_batch(qs)
    got = _outputs(batch, len(fields))
    for b, (m, p) in enumerate(variants):
        _equal(got[b], _single(m, probs[b], p, qs[b], {}), fields[b])
        assert _differ(got[b]["tau"], _single(model, probs[b], sp, qs[b], {})["tau"]), fields[b]
    batch.close()


@pytest.mark.parametrize("gradients_method", ["forward_differences", "central_differences", "central_differences4"])
def test_the_three_difference_schemes(gradients_method):
    model, probs, sp, qs = _case("hopper")
    sp.gradients_method = gradients_method
    models, sps = [model], [sp]
    for b in range(1, B):
        m, p = _variant(model, sp, 3000 + b)
        models.append(m); sps.append(p)
    batch = hip.HipPath(model, probs, sp)
    for b in range(1, B):
        batch.set_model_batch(b, models[b], sps[b])
    batch.set_q_batch(qs)
    got = _outputs(batch, B)
    for b in range(B):
        _equal(got[b], _single(models[b], probs[b], sps[b], qs[b], {}), (gradients_method, b))
    assert _differ(batch.get("dtau_dqt", 1), _single(model, probs[1], sp, qs[1], {})["dtau_dqt"])
    g, _ = Oracle(models[B - 1], probs[B - 1], sps[B - 1]).gn_step(qs[B - 1])
    assert _same(batch.get("gradient", B - 1), g)
    batch.close()


def test_replacing_a_record_moves_that_problem_only():
    model, probs, sp, qs = _case("mini_cheetah")
    m1, p1 = _variant(model, sp, 4001)
    m2, p2 = _variant(model, sp, 4002)
    batch = hip.HipPath(model, probs, sp)
    batch.set_model_batch(1, m1, p1)
    batch.set_q_batch(qs)
    batch.gn_step()
    first = [{arr: batch.get(arr, b) for arr in ARRAYS} for b in range(B)]
    batch.set_model_batch(2, m2, p2)
    batch.gn_step()
    second = [{arr: batch.get(arr, b) for arr in ARRAYS} for b in range(B)]
    for b in (0, 1):
        _equal(second[b], first[b], b)
    assert _differ(second[2]["tau"], first[2]["tau"]) and _differ(second[2]["step"], first[2]["step"])
    _equal(second[2], {k: v for k, v in _single(m2, probs[2], p2, qs[2], {}).items() if k != "cost"}, "replaced")
    batch.set_model_batch(2, model, sp)   # the base model back: the first outputs, bit for bit
    batch.gn_step()
    for b in range(B):
        _equal({arr: batch.get(arr, b) for arr in ARRAYS}, first[b], ("restored", b))
    batch.close()


@pytest.mark.parametrize("name,n", [("hopper", N), ("spinner", N), ("spinner", 16)])
def test_shared_model_batches_are_untouched(name, n):
    """a context that never gets the call reports model_batch 0 and runs the launches it always ran; one whose problems
    were all given the base model explicitly computes the same, through the per-problem kernels.  (spinner, 16 steps:
    the shortest horizon at which the shared-model batch takes its step in one workgroup, gn_small - the batch with
    records declines it and factorises with the block kernels: everything up to the step is compared.)"""
    model, probs, sp, qs = _case(name, n=n)
    plain = hip.HipPath(model, probs, sp)
    plain.set_q_batch(qs)
    want = _outputs(plain, B)
    assert plain.get_option("model_batch") == 0
    if n == 16:
        assert plain.get_option("last_assembly") == 5   # (the shared-model batch keeps its single-workgroup step)
    plain.close()
    explicit = hip.HipPath(model, probs, sp)
    for b in range(B):
        explicit.set_model_batch(b, model, sp)
    assert explicit.get_option("model_batch") == 1
    explicit.set_q_batch(qs)
    got = _outputs(explicit, B)
    assert explicit.get_option("last_assembly") != 5
    for b in range(B):
        _equal(got[b], {k: v for k, v in want[b].items() if n != 16 or k != "step"}, (name, b))
    explicit.close()


def test_refusals_at_the_c_abi(monkeypatch):
    """a topology mismatch, a context of one problem and the constraints' child-context route are refused by name, before
    any device work"""
    model, probs, sp, qs = _case("hopper")
    batch = hip.HipPath(model, probs, sp)
    batch.set_q_batch(qs)
    batch.gn_step()
    before = [batch.get("step", b) for b in range(B)]
    bad = copy.deepcopy(model)
    bad.actuated = 1 - np.asarray(bad.actuated)
    with pytest.raises(hip.HipError, match="model of problem 1 differs from the batch's model in actuated"):
        batch.set_model_batch(1, bad.normalize(), sp)
    bad = copy.deepcopy(model)
    bad.jtype = np.array(bad.jtype)
    bad.jtype[-1] = 1 - int(bad.jtype[-1])   # revolute <-> prismatic
    with pytest.raises(hip.HipError, match="model of problem 2 differs from the batch's model in jtype"):
        batch.set_model_batch(2, bad.normalize(), sp)
    with pytest.raises(hip.HipError, match="differs from the batch's model in nbodies"):
        batch.set_model_batch(1, load_model("acrobot"), sp)
    with pytest.raises(hip.HipError, match="outside the batch"):
        batch.set_model_batch(B, model, sp)
    # nothing was switched, nothing moved
    assert batch.get_option("model_batch") == 0
    batch.gn_step()
    assert all(_same(batch.get("step", b), before[b]) for b in range(B))
    batch.close()
    one = hip.HipPath(model, probs[0], sp)
    with pytest.raises(hip.HipError, match="context of one problem"):
        one.set_model_batch(0, model, sp)
    one.close()
    # the constraints' child-context route (option con_kkt 0) builds single contexts from the ONE model
    monkeypatch.setenv("IDTO_CON_KKT", "0")
    batch = hip.HipPath(model, probs, sp)
    batch.set_model_batch(1, *_variant(model, sp, 5001))
    batch.set_q_batch(qs)
    dofs = list(model.unactuated_dofs)
    assert dofs
    with pytest.raises(hip.HipError, match="child-context route"):
        batch.tr_solve_batch_constrained(2, 2, True, False, np.full(B, 0.1), 1e5, dofs)
    batch.close()
    # ... the banded KKT route serves such a batch: rows == the single contexts' with model b
    monkeypatch.setenv("IDTO_CON_KKT", "1")
    model, probs, sp, qs = _case("hopper", n=8)
    batch = hip.HipPath(model, probs, sp)
    m1, p1 = _variant(model, sp, 5001)
    batch.set_model_batch(1, m1, p1)
    batch.set_q_batch(qs)
    rows, delta = batch.tr_solve_batch_constrained(4, 2, True, False, np.full(B, 0.1), 1e5, dofs)
    cols = [c for c in range(17) if c != 10]   # (column 10 is the device clock)
    for b, (m, p) in enumerate([(model, sp), (m1, p1), (model, sp)]):
        dev = hip.HipPath(m, probs[b], p)
        dev.set_q(qs[b])
        dev.eval_tau()
        r0, d = dev.tr_solve(4, 2, True, False, 0.1, 1e5, constrained_dofs=dofs)
        assert np.array_equal(rows[b][:, cols], r0[:, cols]) and delta[b] == d, b
        assert _same(batch.get("q", b), dev.get("q")), b
        dev.close()
    batch.close()


# ---- the loops: TrajectoryOptimizer.solve_batch(models=..., contacts=...)

def _loop_case(name, iters, linesearch=False):
    import test_gpu_solve_batch as sb
    model, probs, sp, qs = sb._problems(name, max_iterations=iters)
    if linesearch:   # Armijo, scaling off, constraints off: what the device's linesearch loop serves
        sp.method, sp.linesearch_method, sp.scaling, sp.equality_constraints = "linesearch", "armijo", False, False
    models, sps = [None], [None]
    for b in range(1, sb.B):
        m, p = _variant(model, sp, 6000 + b)
        models.append(m); sps.append(p)
    return sb, model, probs, sp, qs, models, sps


@pytest.mark.parametrize("name,iters", [("hopper", 6), ("mini_cheetah", 4)])
@pytest.mark.parametrize("linesearch", [False, True])
def test_every_entry_of_the_loops_equals_its_own_optimizer(name, iters, linesearch):
    """the horizons and iteration counts of tests/test_gpu_solve_batch.py::test_every_entry_equals_its_single_solve; the
    trust region with the YAML's enforced constraints (hopper), and method = linesearch"""
    from idto_amd.optimizer import TrajectoryOptimizer
    sb, model, probs, sp, qs, models, sps = _loop_case(name, iters, linesearch)
    singles = [sb._solve_alone(models[b] or model, probs[b], sps[b] or sp, qs[b]) for b in range(sb.B)]
    if name == "hopper" and not linesearch:
        assert sp.equality_constraints and model.unactuated_dofs
    opt = TrajectoryOptimizer(model, probs[0], sp)
    res = opt.solve_batch(qs, probs, models=models, contacts=sps)
    assert res.batch_route
    for b in range(sb.B):
        sb._assert_entry_equals(res, b, singles[b], (name, linesearch))
    # the variants act: entries 1 and 2 are not what the shared-model batch gives
    plain = opt.solve_batch(qs, probs)
    for b in range(1, sb.B):
        assert _differ(plain.solutions[b].q, res.solutions[b].q), b
    sb._assert_entry_equals(plain, 0, singles[0], "shared")
    # a second call reuses the batch's context: the records are uploaded per call
    again = opt.solve_batch(qs, probs, models=models[::-1], contacts=sps[::-1])
    sb._assert_entry_equals(again, 1, singles[1], "again")
    assert _differ(again.solutions[2].q, res.solutions[2].q)
    opt.close()


def test_refusals_of_solve_batch(monkeypatch):
    """each raises before device work, with its name in the message"""
    from idto_amd.optimizer import TrajectoryOptimizer
    sb, model, probs, sp, qs, models, sps = _loop_case("hopper", 3)
    opt = TrajectoryOptimizer(model, probs[0], sp)
    bad = copy.deepcopy(model)
    bad.actuated = 1 - np.asarray(bad.actuated)
    with pytest.raises(RuntimeError, match="model of problem 1 differs from the batch's model in actuated"):
        opt.solve_batch(qs, probs, models=[None, bad.normalize(), None])
    with pytest.raises(RuntimeError, match="B < 2"):
        opt.solve_batch(qs[:1], probs[:1], models=models[1:2])
    dense = copy.deepcopy(probs)
    dense[1].Qq = dense[1].Qq.copy()
    dense[1].Qq[0, 1] = dense[1].Qq[1, 0] = 1e-3
    with pytest.raises(RuntimeError, match="dense weights"):
        opt.solve_batch(qs, dense, models=models, contacts=sps)
    assert opt.solve_batch(qs, dense).batch_route is False   # (the shared-model batch keeps its entry-by-entry route)
    opt.close()
    monkeypatch.setenv("IDTO_CON_KKT", "0")
    opt = TrajectoryOptimizer(model, probs[0], sp)
    with pytest.raises(RuntimeError, match="child-context constraint route"):
        opt.solve_batch(qs, probs, models=models, contacts=sps)
    opt.close()
