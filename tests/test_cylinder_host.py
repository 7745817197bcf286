"""The cylinder branch of csrc/id_eval.h on the host - no GPU, nothing loaded into Python: the device text compiled by g++
with the address and undefined-behaviour sanitizers, in three stand-alone programs.

* tests/cpp/cylinder_host_check.cc calls signed_distance itself on every directed state of tests/cylinder_cases.py, in
  both role orders, in the cylinder's own frame and in a rotated one (an exact signed permutation for the states that
  need c bit for bit, a general rotation for the others).
* tests/cpp/scene_report_host_check.cc (scene_block_body over the lane emulation) reports phi, n, Ca, Cb of the directed
  states placed on the two small models; its own lines hold every active pair's force to contact_pair with ==.
* tests/cpp/id_eval_host_check.cc (id_eval over the lane emulation) gives tau of the same states, held to the oracle on
  cylinder_ref.frozen_model.

Geometry is compared with tests/cylinder_ref.py, the numpy restatement of include/idto_model.h.  The device reaches the
rule through a substitute sphere or box, numpy evaluates it term by term: the two agree to rounding, not bit for bit.
GEOMETRY_MEASURED is the largest |difference| of phi, n, Ca, Cb [m, or 1 for n] that these tests print over all their
states, measured on the CPU; GEOMETRY_TOL is 100 times that (the convention of tests/test_contact_regions.py).

TAU_REL: tests/test_gpu_capsule.py's derivation holds unchanged - the substitute point differs from the frozen model's
by a few ulp of the coordinates, times the stiffness, times the lever arm, relative to the state's largest tau."""
import os

import numpy as np
import pytest

import cylinder_cases as cc
import cylinder_ref as cyl
import lane_emu as le
from idto_amd.problem import make_problem

GEOMETRY_MEASURED = 2.218e-14   # (scene_block_body, both role orders; signed_distance itself: 2.721e-15)
GEOMETRY_TOL = 100 * GEOMETRY_MEASURED
TAU_REL = 1e-12
FIELDS = (("phi", 1, 2), ("n", 2, 5), ("Ca", 5, 8), ("Cb", 8, 11))   # columns of a scene report's pair row


def geometry_error(got, want):
    """largest |difference| over phi, n, Ca, Cb; got: a pair row's [phi, n, Ca, Cb] as 10 doubles"""
    ref = np.concatenate([[want["phi"]], want["n"], want["Ca"], want["Cb"]])
    return float(np.abs(np.asarray(got) - ref).max())


# ---- signed_distance itself
P_EXACT = np.array([0.5, -0.25, 1.0])
P_GENERAL = np.array([0.3, -0.2, 0.7])


def queries():
    """[(label, line of the query file, cylinder_ref's result)]"""
    out = []
    for state, (c, exact) in cc.STATES.items():
        frames = [("own", np.eye(3)), ("rotated", cc.R_EXACT if exact else cc.R_GENERAL)]
        for frame, RX in frames:
            p = P_EXACT if exact else P_GENERAL
            x = p + RX @ np.array(c)   # (exact states: dyadic coordinates and a signed permutation - every term exact)
            if exact:
                assert np.array_equal(RX.T @ (x - p), np.array(c)), state
            for rho in (0.03, 0.0):
                sph = [cyl.SPHERE] + list(np.eye(3).ravel()) + list(x) + [rho, 0.0, 0.0]
                cy = [cyl.CYLINDER] + list(RX.ravel()) + list(p) + [cc.R_DIRECTED, cc.H_DIRECTED, 0.0]
                for role in cc.ROLES:
                    sides = sph + cy if role == "sphere_first" else cy + sph
                    want = cyl.sphere_cylinder(x, rho, p, RX, cc.R_DIRECTED, cc.H_DIRECTED, role == "sphere_first")
                    assert want["region"] == cc.REGION[state], (state, want["region"])
                    line = " ".join(str(int(v)) if i in (0, 16) else repr(float(v)) for i, v in enumerate(sides))
                    out.append((f"{state}/{frame}/{role}/rho={rho}", line, want))
    return out


def test_signed_distance_meets_the_rule_at_every_directed_state(tmp_path):
    exe = le.build("cylinder_host_check", tmp_path)
    qs = queries()
    assert len(qs) == len(cc.STATES) * 2 * 2 * 2
    path = os.path.join(str(tmp_path), "queries.txt")
    with open(path, "w") as f:
        f.write("\n".join(line for _, line, _ in qs) + "\n")
    rc, lines, err = le.run(exe, [path])
    assert rc == 0 and len(lines) == len(qs), err[-6000:]
    worst = 0.0
    for (label, _, want), line in zip(qs, lines):
        vals = [float(t) for t in line.split()]
        assert vals[0] == 1.0, label
        e = geometry_error(vals[1:], want)
        worst = max(worst, e)
        assert e <= GEOMETRY_TOL, (label, e)
        # the properties of a distance: a unit normal from A to B, witness points |phi| apart along it
        n, Ca, Cb = np.array(vals[2:5]), np.array(vals[5:8]), np.array(vals[8:11])
        assert abs(np.linalg.norm(n) - 1.0) <= 1e-15 * 4, label
        assert abs(np.linalg.norm(Ca - Cb) - abs(vals[1])) <= GEOMETRY_TOL, label
        if abs(vals[1]) > 1e-3:
            assert np.abs((Cb - Ca) / vals[1] - n).max() <= 1e-12, label
    print("signed_distance: largest |difference| from cylinder_ref", worst)


# ---- the directed states placed on the two small models
def directed_cases(role):
    return [(f"{name}_{state}_{role}",) + cc.directed(name, state, role) + (name,) for name, state in cc.directed_labels()]


def sp_of(name, model):
    cfg, _ = cc.base_problem(name)
    return make_problem(cfg, model, num_steps=2)[:2]


@pytest.mark.parametrize("role", cc.ROLES)
def test_scene_block_reports_the_rule_on_the_two_small_models(tmp_path, role):
    exe = le.build("scene_report_host_check", tmp_path)
    cases, paths, want_lines = directed_cases(role), [], []
    for label, model, q, v, a, name in cases:
        prob, sp = sp_of(name, model)
        path = os.path.join(str(tmp_path), label + ".case")
        with open(path, "w") as f:
            f.write(f"label {label}\ndev {le.save_model(model, tmp_path, label)}\norc -\n")
            f.write(f"contact {le.fmt(le.contact_values(sp))}\ndump {path}.dump\nstates 1\n{le.fmt(q)}\n{le.fmt(v)}\n")
        paths.append(path)
    rc, lines, err = le.run(exe, paths)
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    worst, active = 0.0, 0
    for (label, model, q, v, a, name), path in zip(cases, paths):
        nb, npairs = model.nbodies, model.npairs
        raw = np.fromfile(path + ".dump")
        pairs = raw[nb * 18:nb * 18 + npairs * 20].reshape(npairs, 20)
        want = cc.expected_pairs(model, q, name)
        threshold = cyl.Frozen(model, *sp_of(name, model)).base.contact_threshold
        for k in range(npairs):
            e = geometry_error(pairs[k, 1:11], want[k])
            worst = max(worst, e)
            assert e <= GEOMETRY_TOL, (label, k, want[k]["region"], e)
            if abs(want[k]["phi"] - threshold) > GEOMETRY_TOL:
                assert (pairs[k, 0] == 1.0) == (want[k]["phi"] <= threshold), (label, k)
            active += int(pairs[k, 0] == 1.0)
        # (the program's own lines: every active pair's force == contact_pair on the same two bodies, 2 problems)
        n_act = int((pairs[:, 0] == 1.0).sum())
        want_lines += [f"{label} forces {2 * n_act}/{2 * n_act}", f"{label} tau_sum 2/2"]
    assert lines[:-1] == want_lines
    assert active >= len(cases)   # (every placed sphere is within the threshold)
    print("scene_block_body: largest |difference| from cylinder_ref", worst)


@pytest.mark.parametrize("role", cc.ROLES)
def test_id_eval_equals_the_oracle_on_frozen_models(tmp_path, role):
    import test_id_eval_host as tih
    exe = le.build("id_eval_host_check", tmp_path)
    cases, paths, want_lines = directed_cases(role), [], []
    for label, model, q, v, a, name in cases:
        prob, sp = sp_of(name, model)
        fr = cyl.Frozen(model, prob, sp)
        tau = fr.tau(q, v, a)
        tau_free = fr.base.inverse_dynamics(q, v, a)
        assert np.abs(tau - tau_free).max() > 1e-3, label   # (the contact acts)
        golden = [(tau, max(np.abs(tau).max(), 1.0))]
        paths.append(tih.write_case(tmp_path, label, model, None, None, sp, [(q, v, a)], golden))
        want_lines.append(f"{label} 3 golden 1/1")
    rc, lines, err = le.run(exe, paths)
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    assert lines[:-1] == want_lines
    worst = [float(l.rsplit(" ", 1)[1]) for l in err.split("\n") if " golden: worst " in l]
    assert len(worst) == len(cases)
    print("id_eval: largest |tau - frozen oracle| / max(|tau|, 1)", max(worst))
    assert max(worst) <= TAU_REL, max(worst)
