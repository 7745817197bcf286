"""Independent goldens for the example models as they are (tests/golden/examples/kane_*.json, traj_*.json): capsules with
length, the per-body gravity switch, pairs shared between two chains, a stem below the common body.

The fixtures come from tools/make_golden.py examples and tools/make_golden_traj.py <name>: Kane's virtual power with
numerical Jacobians of position-level kinematics, no recursion, no force propagation, the capsule rules written from the
text of include/idto_model.h with another closest-point method than the kernels' (tools/golden_examples.py).

  * not gpu: the fixtures against the CPU oracle's frozen-sphere composition (capsule_ref.frozen_sphere_model at the
    state; rows of bodies whose weight is switched off from the g = 0 model, the others from the g model) - the
    expectation tests/test_gpu_capsule.py and tests/test_gpu_stem.py hold the device to -, so that a later disagreement
    of the device is the device's; and the conditions on the set of states, recomputed with the oracle: which pairs
    act, that the capsules' length and the gravity switch change tau.  The margins from the conventions that geometry
    does not decide are read from the fixtures.
  * gpu: the device on the fixture models as they are, through eval_tau, through gn_step's own tau (the
    finite-difference launch evaluates the base point with other code), with fd_fast 1 and 0 where there is a fast
    shape, as one batch of six, and at trajectory level with forward and central differences.  Every bound is a number
    stored in the fixture."""
import functools
import glob
import json
import os

import numpy as np
import pytest

import capsule_ref as cr
from idto_amd.problem import make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_golden import _check_traj, _qdot
from test_gpu_capsule import TWO_DOF_CFG, example, frozen_case
from test_model_cross_pairs import MIN_CHANGE, drop_pairs, shared_pairs, touching_trajectory
from test_model_stem import CLASSES, all_gravity, no_gravity, pair_class, punyo_trajectory, zero_length

HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLES = os.path.join(HERE, "golden", "examples")
KANE = ["jaco", "jaco_ball", "dual_jaco", "spinner_capsule", "2dof_spinner_capsule", "punyo"]
TRAJ = ["dual_jaco", "spinner_capsule", "punyo"]
FAST_SHAPE = {"jaco": 6, "jaco_ball": 6, "dual_jaco": 0, "spinner_capsule": 0, "2dof_spinner_capsule": 0, "punyo": 0}
MATTERS = 1e-3   # the capsules' length / the gravity switch "matter" when they change tau by more than this, relative
PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")
BANDS = ("H_A", "H_B", "H_C")


@functools.lru_cache(maxsize=None)
def fixture(kind, name):
    return json.load(open(os.path.join(EXAMPLES, f"{kind}_{name}.json")))


def model_of(name):
    model, cfg = example(name)
    return model, (cfg or TWO_DOF_CFG)


def setup(name, N):
    fix = fixture("kane" if N == 1 else "traj", name)
    assert fix["model_file"] == name + ".model"
    model, cfg = model_of(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    for k, val in fix["contact"].items():
        assert getattr(sp, k) == val, "fixture generated with other contact parameters"
    sp.scaling = sp.equality_constraints = False
    return fix, model, cfg, prob, sp


@functools.lru_cache(maxsize=None)
def helper_trajectory(name, helper, N, seed, lower):
    """the trajectory of the tests' helper that a fixture names as the source of a state"""
    model, cfg = model_of(name)
    if helper == "synthetic_trajectory":
        return synthetic_trajectory(cfg, model, N, seed=seed, lower=lower)
    if helper == "touching_trajectory":
        return touching_trajectory(model, cfg, N, seed)
    if helper == "punyo_trajectory":
        return punyo_trajectory(cfg, model, N, seed)
    assert helper == "frozen_case"
    return frozen_case(name)[3]


def rebuilt(name, source):
    q = helper_trajectory(name, source["helper"], source.get("N"), source.get("seed"), source.get("lower"))
    if "rows" in source:
        return q[source["rows"][0]:source["rows"][1]]
    if "columns" in source:
        q = q.copy()
        for i, start, end in source["columns"]:
            q[:, i] = np.linspace(start, end, q.shape[0])
        return q
    if "t" not in source:
        return q
    qt = q[source["t"]].copy()
    for i, val in source["set"]:
        qt[i] = val
    return qt


def off_dofs(model):
    """DoFs of the bodies whose weight is switched off"""
    nvs = {0: 1, 1: 1, 2: 3, 3: 6}
    return [int(model.vstart[i]) + j for i in range(model.nbodies) if not int(model.gravity_enabled[i])
            for j in range(nvs[int(model.jtype[i])])]


def rel(x, y, scale):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max() / scale)


class Composition:
    """the oracle on the sphere model frozen at one state, composed by rows from g and g = 0"""

    def __init__(self, model, prob, sp, q):
        self.prob, self.sp = prob, sp
        self.off = off_dofs(model)
        poses = Oracle(cr.without_geometry(model), prob, sp).body_poses(q)
        self.frozen = cr.frozen_sphere_model(model, poses)

    def tau(self, q, v, a, model=None, switch=True):
        m = self.frozen if model is None else model
        tau = Oracle(all_gravity(m), self.prob, self.sp).inverse_dynamics(q, v, a)
        if switch and self.off:
            tau[self.off] = Oracle(no_gravity(m), self.prob, self.sp).inverse_dynamics(q, v, a)[self.off]
        return tau


# ---- not gpu
def test_fixtures_exist():
    assert sorted(glob.glob(os.path.join(EXAMPLES, "kane_*.json"))) == sorted(
        os.path.join(EXAMPLES, f"kane_{n}.json") for n in KANE)
    assert sorted(glob.glob(os.path.join(EXAMPLES, "traj_*.json"))) == sorted(
        os.path.join(EXAMPLES, f"traj_{n}.json") for n in TRAJ)
    limit = os.path.getsize(os.path.join(HERE, "golden", "traj_allegro_hand.json"))
    for path in glob.glob(os.path.join(EXAMPLES, "*.json")):
        assert os.path.getsize(path) <= limit, path


@pytest.mark.parametrize("name", KANE)
def test_oracle_composition_matches_independent_kane_dynamics(name):
    """every state: q is the helper's, the oracle's frozen-sphere composition gives the fixture's tau within
    tolerance_rel, and the conditions on the set hold when recomputed with the oracle"""
    fix, model, cfg, prob, sp = setup(name, 1)
    assert fix["tolerance_rel"] == 1e-7 and len(fix["states"]) == 6
    capsules = any(int(t) == cr.CAPSULE and model.geom_size[g][1] > 0 for g, t in enumerate(model.geom_type))
    switch, shared = bool(off_dofs(model)), shared_pairs(model)
    assert capsules == (name in ("spinner_capsule", "2dof_spinner_capsule", "punyo"))
    assert switch == (name in ("jaco", "jaco_ball", "dual_jaco", "punyo")) and bool(shared) == (name in ("dual_jaco", "punyo"))
    count = dict(none=0, length=0, gravity=0, shared=0, stem=0)
    classes, worst = set(), 0.0
    for st in fix["states"]:
        q, v, a, want = (np.array(st[k]) for k in ("q", "v", "a", "tau"))
        assert np.array_equal(q, rebuilt(name, st["source"])), st["source"]
        scale = max(np.abs(want).max(), np.abs(st["tau_contact"]).max())
        comp = Composition(model, prob, sp, q)
        tau = comp.tau(q, v, a)
        worst = max(worst, rel(tau, want, scale))
        assert rel(tau, want, scale) <= fix["tolerance_rel"], (st["source"], rel(tau, want, scale))
        orc = Oracle(comp.frozen, prob, sp)
        acting = int(np.count_nonzero(orc.signed_distances(q)[0] <= orc.contact_threshold)) if model.npairs else 0
        assert acting == st["acting_pairs"]
        count["none"] += acting == 0
        if capsules:   # the same model with h = 0: the spheres at the capsules' centres
            count["length"] += rel(tau, comp.tau(q, v, a, cr.frozen_sphere_model(zero_length(model), Oracle(
                cr.without_geometry(model), prob, sp).body_poses(q))), scale) > MATTERS
        if switch:
            count["gravity"] += rel(tau, comp.tau(q, v, a, switch=False), scale) > MATTERS
        if name == "dual_jaco":
            count["shared"] += np.abs(tau - comp.tau(q, v, a, drop_pairs(comp.frozen, shared))).max() > MIN_CHANGE
        if name == "punyo":
            for c in CLASSES:
                ks = [k for k in range(model.npairs) if pair_class(model, k) == c]
                if np.abs(tau - comp.tau(q, v, a, drop_pairs(comp.frozen, ks))).max() > MIN_CHANGE:
                    classes.add(c)
                    count["stem"] += c == "ball-waist"   # (the waist: the one stem body below the torso with geometry)
    print(name, "largest |oracle composition - golden| / scale:", worst)
    assert count["none"] >= 1, "no state without contact"
    assert not capsules or count["length"] >= 3, count
    assert not switch or count["gravity"] >= 3, count
    assert name != "dual_jaco" or count["shared"] >= 3, count
    assert name != "punyo" or (classes == set(CLASSES) and count["stem"] >= 2), (classes, count)
    _margins_hold(fix)


def _margins_hold(fix):
    m = fix["margins"]
    assert m["min_capsule_box_dz"] == 1e-3 and m["min_capsule_capsule_sin2"] == 1e-3
    assert m["capsule_box_dz"] is None or m["capsule_box_dz"] >= 1e-3
    assert m["capsule_capsule_sin2"] is None or m["capsule_capsule_sin2"] >= 1e-3


def assemble(prob, q, v, tau, P, Np):
    """gradient and Hessian bands from tau and its partials by the block formulas of the reference
    (optimizer/trajectory_optimizer.cc:1046-1080, 1103-1161), dense numpy blocks [t, row, col]"""
    N, nq, dt = prob.num_steps, q.shape[1], prob.time_step
    Qq, Qv, R = (2 * dt * np.asarray(x, float) for x in (prob.Qq, prob.Qv, prob.R))
    Qfq, Qfv = 2 * np.asarray(prob.Qf_q, float), 2 * np.asarray(prob.Qf_v, float)
    Pp, T, M = (np.nan_to_num(P[k]) for k in PARTIALS)
    V, W = [n / dt for n in Np], [-n / dt for n in Np]
    eq, ev = q - prob.q_nom, v - prob.v_nom
    g = np.zeros((N + 1, nq))
    A, B, C = np.zeros((N + 1, nq, nq)), np.zeros((N + 1, nq, nq)), np.zeros((N + 1, nq, nq))
    C[0] = np.eye(nq)
    for t in range(1, N):
        Qn = Qfv if t == N - 1 else Qv
        g[t] = Qq @ eq[t] + V[t].T @ Qv @ ev[t] + W[t + 1].T @ Qn @ ev[t + 1] + Pp[t - 1].T @ R @ tau[t - 1] + T[t].T @ R @ tau[t]
        C[t] = Qq + V[t].T @ Qv @ V[t] + Pp[t - 1].T @ R @ Pp[t - 1] + T[t].T @ R @ T[t] + W[t + 1].T @ Qn @ W[t + 1]
        if t < N - 1:
            g[t] += M[t + 1].T @ R @ tau[t + 1]
            C[t] += M[t + 1].T @ R @ M[t + 1]
            B[t + 1] = Pp[t].T @ R @ T[t] + T[t + 1].T @ R @ M[t + 1] + V[t + 1].T @ Qv @ W[t + 1]
            A[t + 2] = Pp[t + 1].T @ R @ M[t + 1]
        else:
            B[N] = Pp[N - 1].T @ R @ T[N - 1] + V[N].T @ Qfv @ W[N]
    g[N] = Pp[N - 1].T @ R @ tau[N - 1] + Qfq @ eq[N] + V[N].T @ Qfv @ ev[N]
    C[N] = Qfq + V[N].T @ Qfv @ V[N] + Pp[N - 1].T @ R @ Pp[N - 1]
    return g, [A, B, C]


@functools.lru_cache(maxsize=None)
def frozen_trajectory_expectation(name):
    """tau, the three partial blocks (forward differences), gradient and H bands of a traj fixture's trajectory: the
    oracle's frozen-sphere expectation (capsule_ref.frozen_expectation), composed by rows from g and g = 0 as
    tests/test_gpu_stem.py composes punyo's"""
    fix, model, cfg, prob, sp = setup(name, 3)
    sp.gradients_method = "forward_differences"
    q = np.array(fix["q"])
    v, a, tau, _, P = cr.frozen_expectation(all_gravity(model), prob, sp, q)
    off = off_dofs(model)
    if off:
        _, _, tau0, _, P0 = cr.frozen_expectation(no_gravity(model), prob, sp, q)
        tau[:, off] = tau0[:, off]
        for k in PARTIALS:
            P[k][:, off, :] = P0[k][:, off, :]
    base = Oracle(cr.without_geometry(model), prob, sp)
    g, bands = assemble(prob, q, v, tau, P, [base.nplus(q[t]) for t in range(prob.num_steps + 1)])
    return tau, P, g, bands


def observed_differences(name):
    """per array: largest |oracle expectation - golden| relative to the golden's largest entry (_check_traj's measure)"""
    fix = fixture("traj", name)
    tau, P, g, bands = frozen_trajectory_expectation(name)
    got = dict(tau=tau, gradient=g, **P, **dict(zip(BANDS, bands)))
    out = {}
    for key in ("tau",) + PARTIALS + ("gradient",) + BANDS:
        want = np.asarray(fix[key], float)
        out[key] = float(np.abs(np.nan_to_num(got[key]).reshape(want.shape) - want).max() / np.abs(want).max())
    return out


def tolerance_rule(observed):
    """5 x the largest observed difference of the derivatives, rounded up to one significant digit, at least 5e-6"""
    x = 5 * max(val for key, val in observed.items() if key != "tau")
    e = 10.0 ** np.floor(np.log10(x))
    return max(5e-6, float(np.ceil(x / e - 1e-9) * e))


@pytest.mark.parametrize("name", TRAJ)
def test_oracle_frozen_expectation_matches_independent_trajectory_derivatives(name):
    fix, model, cfg, prob, sp = setup(name, 3)
    q = np.array(fix["q"])
    assert fix["num_steps"] == 3 and np.array_equal(q, rebuilt(name, fix["source"]))
    _margins_hold(fix)
    # pairs in penetration, of the kinds the fixture is there for
    inside = set()
    for t in range(1, 4):
        frozen = cr.frozen_sphere_model(model, Oracle(cr.without_geometry(model), prob, sp).body_poses(q[t]))
        inside |= set(np.flatnonzero(Oracle(frozen, prob, sp).signed_distances(q[t])[0] < 0).tolist())
    assert inside == set(fix["penetrating_pairs"]) and inside
    if name == "dual_jaco":
        assert inside & set(shared_pairs(model))
    if name == "punyo":
        assert {"arm-ball", "ball-waist"} <= {pair_class(model, k) for k in inside}
    observed = observed_differences(name)
    print(name, "observed |oracle expectation - golden|, relative:", observed, "tolerance", fix["tolerance_derivatives"])
    assert fix["tolerance_tau"] == 1e-11
    assert 5e-6 <= fix["tolerance_derivatives"] <= 1e-4
    assert fix["tolerance_derivatives"] == tolerance_rule(fix["observed_derivatives"])
    for key, val in observed.items():   # (what tools/measure_golden_examples.py stored is what the oracle gives here)
        if key != "tau":
            assert val <= 1.01 * fix["observed_derivatives"][key] + 1e-12, key
    tau, P, g, bands = frozen_trajectory_expectation(name)
    _check_traj(fix, tau, P, g, bands)


# ---- gpu
def one_step_problem(model, prob, st):
    """the one-step trajectory whose (v_1, a_0) are the state's (v, a): tau_0 = ID(q, v, a)"""
    import copy
    q, v, a = (np.array(st[k]) for k in ("q", "v", "a"))
    q0 = q - prob.time_step * _qdot(model, q, v)
    p = copy.deepcopy(prob)
    p.q_init, p.v_init = q0.copy(), v - prob.time_step * a
    return p, np.stack([q0, q])


def check_state(st, tol, tau, v, a, what):
    want = np.array(st["tau"])
    scale = max(np.abs(want).max(), np.abs(st["tau_contact"]).max())
    assert np.abs(v - np.array(st["v"])).max() < 1e-12 and np.abs(a - np.array(st["a"])).max() < 1e-10, what
    err = np.abs(tau - want).max()
    print(what, "|tau - golden| / scale", err / scale)
    assert err <= tol * scale, (what, err / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_fast", [(n, 1) for n in KANE] + [("jaco", 0), ("jaco_ball", 0)])
def test_hip_matches_independent_kane_dynamics(name, fd_fast):
    """eval_tau and gn_step's own tau of the fixture model as it is, for each of the six states; for the models with a
    fast shape (id_fast.h) also with fd_fast 0, the generic id_eval"""
    from idto_amd import hip
    fix, model, cfg, prob, sp = setup(name, 1)
    for i, st in enumerate(fix["states"]):
        p, q = one_step_problem(model, prob, st)
        dev = hip.HipPath(model, p, sp)
        dev.set_option("fd_fast", fd_fast)
        assert dev.get_option("fast_shape") == FAST_SHAPE[name]
        dev.set_q(q)
        for launch in ("gn_step", "eval_tau"):   # (gn_step first: on a fresh context its tau is nobody else's)
            getattr(dev, launch)()
            check_state(st, fix["tolerance_rel"], dev.get("tau")[0], dev.get("v")[1], dev.get("a")[0], (name, i, launch))
        dev.close()


@pytest.mark.gpu
def test_hip_batch_of_six_matches_independent_kane_dynamics():
    """dual_jaco's six states as the six problems of one batch: the shared pairs' records are exchanged through LDS per
    problem, and six problems put more than one on a compute unit"""
    from idto_amd import hip
    fix, model, cfg, prob, sp = setup("dual_jaco", 1)
    probs, qs = zip(*[one_step_problem(model, prob, st) for st in fix["states"]])
    dev = hip.HipPath(model, list(probs), sp)
    assert dev.get_option("fast_shape") == 0
    dev.set_q_batch(np.array(qs))
    for launch in ("gn_step", "eval_tau"):
        getattr(dev, launch)()
        for b, st in enumerate(fix["states"]):
            check_state(st, fix["tolerance_rel"], dev.get("tau", b).reshape(1, -1)[0], dev.get("v", b).reshape(2, -1)[1],
                        dev.get("a", b).reshape(1, -1)[0], ("dual_jaco", b, launch))
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["forward_differences", "central_differences"])
@pytest.mark.parametrize("name", TRAJ)
def test_hip_matches_independent_trajectory_derivatives(name, method):
    from idto_amd import hip
    fix, model, cfg, prob, sp = setup(name, 3)
    sp.gradients_method = method
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == FAST_SHAPE[name]
    dev.set_q(np.array(fix["q"]))
    dev.gn_step()
    P = {k: dev.get(k) for k in PARTIALS}
    _check_traj(fix, dev.get("tau"), P, dev.get("gradient"), [dev.get(k) for k in BANDS])
    dev.close()
