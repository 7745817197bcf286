"""The host emulation of csrc/scene_report.h (tests/cpp/scene_report_host_check.cc over tests/cpp/lane_emu, no GPU) held to
the independent fixtures of tests/golden/scene: body velocities, per-pair geometry, velocities and forces and the generalised
contact force at the 88 directed contact states and at the states of the example fixtures as they are - spinner_capsule
(capsules with length), dual_jaco (shared pairs, the gravity switch), punyo (a stem, capsules).  The bars are
tests/scene_fixtures.py's: 100 times what this emulation shows, capped by the generator's 1e-7; the GPU test holds the device
to the same constants."""
import os

import numpy as np
import pytest

import lane_emu as le
import scene_fixtures as sf


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return le.build("scene_report_host_check", tmp_path_factory.mktemp("scene_fixtures"))


def emulate(exe, out_dir, label, role="stored"):
    """-> (bodies [S, nb, 18], pairs [S, npairs, 20], tau_contact [S, nv]) of the emulated blocks at the set's states"""
    model, prob, sp, x, _ = sf.case(label, role)
    tag = f"{label}_{role}"
    dump = os.path.join(str(out_dir), tag + ".f64")
    orc = le.save_model(model, out_dir, tag + "_orc") if label.startswith("regions_") else "-"
    path = os.path.join(str(out_dir), tag + ".case")
    with open(path, "w") as f:
        f.write(f"label {tag}\ndev {le.save_model(model, out_dir, tag + '_dev')}\norc {orc}\n")
        f.write(f"contact {le.fmt(le.contact_values(sp))}\ndump {dump}\nstates {len(x)}\n")
        for row in x:
            f.write(le.fmt(row) + "\n")
    rc, lines, err = le.run(exe, [path])
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-20:]) + err[-4000:]
    S, nb, npairs, nv = len(x), model.nbodies, model.npairs, model.nv
    flat = np.fromfile(dump)
    assert flat.size == S * (nb * 18 + npairs * 20 + nv + npairs * nv)
    bodies, flat = flat[:S * nb * 18].reshape(S, nb, 18), flat[S * nb * 18:]
    pairs, flat = flat[:S * npairs * 20].reshape(S, npairs, 20), flat[S * npairs * 20:]
    return bodies, pairs, flat[:S * nv].reshape(S, nv)


def check(label, worst):
    for key in sf.QUANTITIES:
        print(label, key, "largest relative difference from the fixture", worst[key], "bar", sf.BARS[key])
    for key in sf.QUANTITIES:
        assert worst[key] <= sf.BARS[key], (label, key, worst[key], sf.BARS[key])


@pytest.mark.parametrize("role", ["stored", "exchanged"])
@pytest.mark.parametrize("name", sf.DIRECTED)
def test_directed_states_meet_the_independent_fixtures(exe, tmp_path, name, role):
    label = "regions_" + name
    check(f"{label} {role}", sf.differences(label, *emulate(exe, tmp_path, label, role), role=role))


@pytest.mark.parametrize("label", sf.AS_THEY_ARE)
def test_example_fixtures_as_they_are_meet_the_independent_fixtures(exe, tmp_path, label):
    model = sf.case(label)[0]
    bodies, pairs, tau = emulate(exe, tmp_path, label)
    assert pairs[:, :, 0].any(), "no active pair in the set"
    check(label, sf.differences(label, bodies, pairs, tau))
    assert len(sf.fixture(label)["states"]) == len(bodies) and model.npairs == pairs.shape[1]


def test_the_bars_come_from_the_measurement():
    assert sf.BARS == {k: min(100 * v, 1e-7) for k, v in sf.MEASURED.items()} and all(v > 0 for v in sf.MEASURED.values())
