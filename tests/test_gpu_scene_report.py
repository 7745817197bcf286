"""The scene report on the device (include/idto_hip.h idto_hip_scene_report; csrc/scene_report.h): body poses and spatial
velocities, per-pair signed distance, witness points, velocities and forces, and the generalised force of contact.

Geometry and the force law are held with == to the CPU oracle (the expressions are id_eval's, bit-exact against it: DESIGN.md
section 3.2), the batch, the per-problem records and the plants' records with == to contexts created with that model.  The
identity tau_contact = ID(pairless model) - ID(model) holds to rounding: its bar is tests/test_scene_report_host.py's
IDENTITY_TOL, 100 times what the host emulation of the same text shows on the CPU.  States: plant_cases.states(name) - three
per model, the first with an active contact - unless said otherwise.  Nothing here provokes a device fault.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import plant_cases as pc
import scene_fixtures as sf
import test_contact_regions as tcr
from idto_amd import hip
from oracle_lib import Oracle
from test_scene_report_host import IDENTITY_TOL

pytestmark = pytest.mark.gpu

MODELS = pc.MODELS + ["punyo"]
H = 1e-3


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def _x(name):
    return np.array([np.concatenate([q, v]) for q, v, _ in pc.states(name)])


def _context(name, B=1, model=None, sp=None):
    dev_model = model if model is not None else pc.case(name)[0]
    prob, sp0 = pc.problem(name)
    return hip.HipPath(dev_model, [prob] * B if B > 1 else prob, sp if sp is not None else sp0)


def _report(name, x, model=None, sp=None, **kw):
    dev = _context(name, 1, model, sp)
    try:
        return dev.scene_report(x, **kw)
    finally:
        dev.close()


def _trace(fn):
    """fn(), and the host trace's marks while it ran"""
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    L.idto_hip_trace_enable(1)
    try:
        out = fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        L.idto_hip_trace_dump(buf, len(buf))
        L.idto_hip_trace_enable(0)
    return out, buf.value.decode()


def _ascending_sum(rows):
    """[..., npairs, nv] -> [..., nv]: pair after pair from +0"""
    out = np.zeros(rows.shape[:-2] + rows.shape[-1:])
    for k in range(rows.shape[-2]):
        out = out + rows[..., k, :]
    return out


# ---- 1. geometry against the oracle
@pytest.mark.parametrize("name", MODELS)
def test_geometry_equals_the_oracle(name):
    orc, x = pc.oracle(name), _x(name)
    nq = pc.case(name)[1].nq
    rep = _report(name, x)
    assert rep.X_WB.shape == (3, pc.case(name)[0].nbodies, 12) and rep.phi.shape == (3, pc.case(name)[0].npairs)
    for s in range(3):
        assert _same(rep.X_WB[s], orc.body_poses(x[s, :nq])), (name, s)
        phi, n, Ca, Cb = orc.signed_distances(x[s, :nq])
        assert _same(rep.phi[s], phi) and _same(rep.normal[s], n) and _same(rep.Ca[s], Ca) and _same(rep.Cb[s], Cb), (name, s)
        assert _same(rep.active[s], phi <= orc.contact_threshold)
        assert _same(rep.pairs[s][:, 19], np.zeros(len(phi)))
        off = ~rep.active[s]
        assert not np.any(rep.fn[s][off]) and not np.any(rep.force[s][off])
    if pc.case(name)[0].npairs:
        assert rep.active[0].any() and np.abs(rep.force[0]).max() > 0


# ---- 2. the directed states, all of a model in ONE call per role order
@pytest.mark.parametrize("role", tcr.ROLES)
@pytest.mark.parametrize("name", tcr.MODELS)
def test_directed_states_equal_the_oracle_and_meet_the_labels(name, role):
    fix, model, prob, sp = tcr.setup(name, role)
    orc = Oracle(model, prob, sp)
    x = np.array([np.concatenate([st["q"], st["v"]]) for st in fix["states"]])
    assert len(x) == {"allegro_hand": 56, "mini_cheetah": 19, "hopper": 13}[name]
    dev = hip.HipPath(model, prob, sp)
    rep = dev.scene_report(x, pair_rows=True)
    dev.close()
    for i, st in enumerate(fix["states"]):
        q = np.array(st["q"])
        assert _same(rep.X_WB[i], orc.body_poses(q)), (i, st["aim"])
        phi, n, Ca, Cb = orc.signed_distances(q)
        assert _same(rep.phi[i], phi) and _same(rep.normal[i], n) and _same(rep.Ca[i], Ca) and _same(rep.Cb[i], Cb), (i, st["aim"])
        assert _same(rep.active[i], phi <= orc.contact_threshold)
        for k, lab in enumerate(st["pairs"]):
            if lab["kind"] == "far":
                assert not rep.active[i, k]
                continue
            assert bool(rep.active[i, k]) == lab["active"], (i, st["aim"], k)
            diffs = [abs(rep.phi[i, k] - lab["phi"])]
            if "n" in lab:
                diffs += [np.abs(a - b).max() for a, b in zip((rep.normal[i, k], rep.Ca[i, k], rep.Cb[i, k]), tcr.in_role(lab, role))]
            assert max(diffs) <= tcr.GEOMETRY_TOL, (i, st["aim"], k, diffs)
            if lab["dissipation"] == "zero":   # s >= 2: active, and an exactly zero force
                assert rep.active[i, k] and rep.fn[i, k] == 0.0 and not np.any(rep.force[i, k])
    assert _same(_ascending_sum(rep.tau_pairs), rep.tau_contact)


# ---- 2, 3. the independent fixtures of tests/golden/scene, at the bars of the host emulation (tests/scene_fixtures.py)
def _meets_the_fixture(label, role="stored"):
    model, prob, sp, x, _ = sf.case(label, role)
    dev = hip.HipPath(model, prob, sp)
    rep = dev.scene_report(x)   # (all states of the set in ONE call)
    dev.close()
    worst = sf.differences(label, rep.bodies, rep.pairs, rep.tau_contact, role=role)
    for key in sf.QUANTITIES:
        print(label, role, key, "largest relative difference from the fixture", worst[key], "bar", sf.BARS[key])
    for key in sf.QUANTITIES:
        assert worst[key] <= sf.BARS[key], (label, role, key, worst[key], sf.BARS[key])
    return rep


@pytest.mark.parametrize("role", tcr.ROLES)
@pytest.mark.parametrize("name", tcr.MODELS)
def test_directed_states_meet_the_independent_fixtures(name, role):
    _meets_the_fixture("regions_" + name, role)


@pytest.mark.parametrize("label", sf.AS_THEY_ARE)
def test_example_fixtures_as_they_are_meet_the_independent_fixtures(label):
    """capsules with length, shared pairs, the stem and the per-body gravity switch, which the oracle cannot express"""
    rep = _meets_the_fixture(label)
    assert rep.active.any()


# ---- 4. the generalised force
def _pairless(model):
    m = copy.deepcopy(model)
    m.pair_a, m.pair_b, m.pair_path = m.pair_a[:0], m.pair_b[:0], m.pair_path[:0]
    m = m.normalize()
    assert m.npairs == 0 and m.ngeoms == model.ngeoms
    return m


@pytest.mark.parametrize("name", MODELS)
def test_generalised_force_meets_the_oracles_two_inverse_dynamics(name):
    dev_model, orc_model, _ = pc.case(name)
    orc, x = pc.oracle(name), _x(name)
    nq, nv = orc_model.nq, orc_model.nv
    pairless = _pairless(orc_model)
    prob, sp = pc.problem(name, model=pairless)
    bare = Oracle(pairless, prob, sp)
    rep = _report(name, x, pair_rows=True)
    assert _same(_ascending_sum(rep.tau_pairs), rep.tau_contact)
    for s in range(3):
        q, v, zero = x[s, :nq], x[s, nq:], np.zeros(nv)
        without, with_ = bare.inverse_dynamics(q, v, zero), orc.inverse_dynamics(q, v, zero)
        scale = max(1.0, np.abs(without).max(), np.abs(with_).max())
        err = np.abs(rep.tau_contact[s] - (without - with_)).max() / scale
        print(name, s, "|tau_contact - (ID without pairs - ID with pairs)| / scale", err)
        assert err <= IDENTITY_TOL, (name, s, err)
        assert not np.any(rep.tau_pairs[s][~rep.active[s]])
    if orc_model.npairs:
        assert np.abs(rep.tau_contact[0]).max() > 0


# ---- 5. a batch, per-problem records, the plants' records
def _variants(name):
    """(model, parameters) per problem: the case's; another contact stiffness; another radius of its first sphere"""
    model, (_, sp) = pc.case(name)[0], pc.problem(name)
    stiff = copy.deepcopy(sp)
    stiff.contact_stiffness = 1.5 * sp.contact_stiffness
    wide = copy.deepcopy(model)
    g = int(np.flatnonzero(np.asarray(wide.geom_type) == 0)[0])
    size = np.array(wide.geom_size, dtype=float)
    size[g, 0] *= 1.25
    wide.geom_size = size
    return [(model, sp), (model, stiff), (wide.normalize(), sp)]


@pytest.mark.parametrize("name", ["hopper", "mini_cheetah"])
def test_batch_and_per_problem_models_equal_single_contexts(name):
    x = _x(name)
    xb = np.array([x, x[::-1], x])
    var = _variants(name)
    solo = [_report(name, xb[b], pair_rows=True) for b in range(3)]
    dev = _context(name, 3)
    rep = dev.scene_report(xb, pair_rows=True)
    for b in range(3):
        assert _same(rep.bodies[b], solo[b].bodies) and _same(rep.pairs[b], solo[b].pairs), (name, b)
        assert _same(rep.tau_contact[b], solo[b].tau_contact) and _same(rep.tau_pairs[b], solo[b].tau_pairs), (name, b)
    dev.set_model_batch(1, None, var[1][1])
    dev.set_model_batch(2, var[2][0], None)
    rep2 = dev.scene_report(xb, pair_rows=True)
    dev.close()
    own = [_report(name, xb[b], model=var[b][0], sp=var[b][1], pair_rows=True) for b in range(3)]
    for b in range(3):
        assert _same(rep2.bodies[b], own[b].bodies) and _same(rep2.pairs[b], own[b].pairs), (name, b)
        assert _same(rep2.tau_contact[b], own[b].tau_contact) and _same(rep2.tau_pairs[b], own[b].tau_pairs), (name, b)
    # the variants are seen: the stiffness in the force alone, the radius in the distance
    assert _same(rep2.bodies, rep.bodies) and _same(rep2.pairs[0], rep.pairs[0])
    assert _same(rep2.phi[1], rep.phi[1]) and not _same(rep2.force[1], rep.force[1])
    assert not _same(rep2.phi[2], rep.phi[2])


def test_plants_models_and_recorded_rows():
    name = "hopper"
    x, var = _x(name), _variants(name)
    nq = pc.case(name)[1].nq
    xb = np.array([x, x[::-1], x])
    dev = _context(name, 3)
    dev.plant_begin(H)
    dev.plant_set_model(1, None, var[1][1])
    dev.plant_set_model(2, var[2][0], None)
    rep = dev.scene_report(xb, models=hip.SCENE_MODELS_PLANTS, pair_rows=True)
    base = dev.scene_report(xb, pair_rows=True)   # (the context's own model is untouched by the plants')
    own = [_report(name, xb[b], model=var[b][0], sp=var[b][1], pair_rows=True) for b in range(3)]
    plain = [_report(name, xb[b], pair_rows=True) for b in range(3)]
    for b in range(3):
        assert _same(rep.bodies[b], own[b].bodies) and _same(rep.pairs[b], own[b].pairs) and _same(rep.tau_pairs[b], own[b].tau_pairs), b
        assert _same(base.pairs[b], plain[b].pairs) and _same(base.tau_contact[b], plain[b].tau_contact), b
    # the rows that a step of 3 substeps recorded, reported with the plants' physics == the same numbers passed by hand, a
    # state at a time, to a context created with that plant's model
    tau = np.array([t for _, _, t in pc.states(name)])
    dev.plant_set_state(np.zeros(3), xb[:, 0])
    rec, status = dev.plant_step(3, tau, record_every=1)
    assert status.tolist() == [[0, 3]] * 3 and rec.shape == (3, 3, x.shape[1])
    got = dev.scene_report(rec, models=hip.SCENE_MODELS_PLANTS, pair_rows=True)
    dev.close()
    for b in range(3):
        one = _context(name, 1, var[b][0], var[b][1])
        for s in range(3):
            by_hand = one.scene_report(np.array([[float(v) for v in rec[b, s]]]), pair_rows=True)
            assert _same(got.bodies[b, s], by_hand.bodies[0]) and _same(got.pairs[b, s], by_hand.pairs[0]), (b, s)
            assert _same(got.tau_contact[b, s], by_hand.tau_contact[0]) and _same(got.tau_pairs[b, s], by_hand.tau_pairs[0]), (b, s)
        one.close()
    assert np.all(np.isfinite(got.bodies)) and nq > 0


# ---- 6. refusals, each with its own text and no device work; the context's state is untouched
def test_refusals_come_before_any_device_work():
    name = "hopper"
    x = _x(name)
    dev = _context(name, 1)
    L, h = hip.lib(), dev.h
    nb, npairs, bd, pdn = dev.scene_sizes()
    assert (nb, npairs, bd, pdn) == (pc.case(name)[0].nbodies, pc.case(name)[0].npairs, 18, 20)
    bodies = np.zeros((3, nb, bd))
    xc = np.ascontiguousarray(x)
    bad = xc.copy()
    bad[1, 4] = np.inf
    nan = xc.copy()
    nan[2, 0] = np.nan
    cases = [((3, None, 0, hip.dptr(bodies), None, None, None), "x[batch][nstates][nq + nv] is required"),
             ((0, hip.dptr(xc), 0, hip.dptr(bodies), None, None, None), "nstates must be >= 1"),
             ((3, hip.dptr(xc), 0, None, None, None, None), "every output is NULL"),
             ((3, hip.dptr(bad), 0, hip.dptr(bodies), None, None, None), "x is not finite at problem 0, state 1, index 4"),
             ((3, hip.dptr(nan), 0, hip.dptr(bodies), None, None, None), "x is not finite at problem 0, state 2, index 0"),
             ((3, hip.dptr(xc), 2, hip.dptr(bodies), None, None, None), "models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS"),
             ((3, hip.dptr(xc), 1, hip.dptr(bodies), None, None, None), "call idto_hip_plant_begin on the context first")]
    texts = []
    for args, text in cases:
        rc, trace = _trace(lambda: L.idto_hip_scene_report(h, *args))
        err = L.idto_hip_last_error().decode()
        assert rc == -1 and err.startswith("scene_report: ") and text in err, (args[0], args[2], err)
        assert trace == "", trace
        texts.append(err)
    assert len(set(texts)) == len(texts) and not np.any(bodies)
    # forward dynamics alone makes the plants' storage without beginning a plant: still refused
    dev.forward_dynamics(xc[:1], np.zeros((1, dev.nv)))
    assert L.idto_hip_scene_report(h, 3, hip.dptr(xc), 1, hip.dptr(bodies), None, None, None) == -1
    # one output alone is enough, and one wait
    rc, trace = _trace(lambda: L.idto_hip_scene_report(h, 3, hip.dptr(xc), 0, hip.dptr(bodies), None, None, None))
    assert rc == 0 and trace.count("waited for the device") == 1 and "scene_report: waited for the device" in trace
    assert _same(bodies, dev.scene_report(xc).bodies)
    dev.close()


def test_a_report_between_two_steps_changes_nothing():
    from idto_amd.problem import load_config, make_problem, synthetic_trajectory
    from idto_amd.model import load_model
    name, N = "hopper", 6
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
    outs = []
    for with_report in (False, True):
        dev = hip.HipPath(model, prob, sp)
        dev.set_q(q)
        dev.gn_step()
        first = [np.array(dev.get(k)) for k in ("gradient", "step", "tau", "cost")]
        if with_report:
            v = dev.get("v")
            rep = dev.scene_report(np.hstack([q, v]))
            assert np.all(np.isfinite(rep.bodies)) and rep.bodies.shape[0] == N + 1
        dev.set_q(q + 0.1 * dev.get("step").reshape(q.shape))
        dev.gn_step()
        outs.append(first + [np.array(dev.get(k)) for k in ("q", "v", "tau", "gradient", "step", "cost", "H_A", "H_B", "H_C")])
        dev.close()
    for a, b in zip(*outs):
        assert _same(a, b)


# ---- 7. the optimizer level: TrajectoryOptimizer.scene_report, and libidto_opt.so's C-ABI
def test_optimizer_level_report_equals_the_context_level():
    from idto_amd import optimizer
    from idto_amd.model import dptr, load_model
    from idto_amd.problem import load_config, make_problem
    cfg, model = load_config("hopper"), load_model("hopper")
    prob, sp, q_guess = make_problem(cfg, model, num_steps=8)
    sp.max_iterations = 2
    sp.verbose = False
    opt = optimizer.TrajectoryOptimizer(model, prob, sp)
    sol, stats = optimizer.TrajectoryOptimizerSolution(), optimizer.TrajectoryOptimizerStats()
    opt.Solve(q_guess, sol, stats)
    assert sol.q.shape == (9, model.nq) and sol.v.shape == (9, model.nv)
    rep, trace = _trace(lambda: opt.scene_report(sol, pair_rows=True))
    assert trace.count("waited for the device") == 1, trace
    by_qv = opt.scene_report(sol.q, sol.v, pair_rows=True)
    # the C-ABI itself, one output at a time
    L = optimizer.lib()
    sizes = [C.c_int() for _ in range(4)]
    assert L.idto_opt_scene_sizes(opt._h, *[C.byref(s) for s in sizes]) == 0
    assert [s.value for s in sizes] == [model.nbodies, model.npairs, 18, 20]
    pairs = np.zeros((9, model.npairs, 20))
    q, v = np.ascontiguousarray(sol.q), np.ascontiguousarray(sol.v)
    assert L.idto_opt_scene_report(opt._h, 9, dptr(q), dptr(v), None, dptr(pairs), None, None) == 0
    assert L.idto_opt_scene_report(opt._h, 9, dptr(q), dptr(v), None, None, None, None) != 0
    assert "every output is NULL" in L.idto_opt_last_error().decode()
    opt.close()
    dev = hip.HipPath(model, prob, sp)
    ref = dev.scene_report(np.hstack([sol.q, sol.v]), pair_rows=True)
    dev.close()
    for got in (rep, by_qv):
        assert _same(got.bodies, ref.bodies) and _same(got.pairs, ref.pairs)
        assert _same(got.tau_contact, ref.tau_contact) and _same(got.tau_pairs, ref.tau_pairs)
    assert _same(pairs, ref.pairs)
    assert _same(rep.X_WB[0][:, 9:], Oracle(model, prob, sp).body_poses(sol.q[0])[:, 9:])
