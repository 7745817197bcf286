"""Cylinder geometry (IDTO_GEOM_CYLINDER, include/idto_model.h) on the host: the cheetah-on-hills fixture
(tests/golden/cylinder/, tools/convert_models.py convert_cylinder_examples), the .model format in Python and C++,
Model.validate's and idto_hip_create's refusals (made before any device is touched, so they work on a box without a GPU),
the declined fast shape, and the independent Kane fixture (tools/make_golden.py cylinder) against the oracle on
cylinder_ref.frozen_model."""
import copy
import json
import os
import shutil
import subprocess
from dataclasses import fields

import numpy as np
import pytest

import cylinder_cases as cc
import cylinder_ref as cyl
from idto_amd import hip
from idto_amd.model import GEOM_TYPES, Model, load_model
from idto_amd.problem import load_config, make_problem
from oracle_lib import Oracle
from test_model_capsule import PROBE

ROOT = cc.ROOT
FIXTURE = os.path.join(cc.FIXTURES, "mini_cheetah_hills.model")


def test_the_type_code_is_4_and_3_stays_unassigned():
    assert GEOM_TYPES["cylinder"] == 4 and 3 not in GEOM_TYPES.values()
    header = open(os.path.join(ROOT, "include", "idto_model.h")).read()
    assert "IDTO_GEOM_CYLINDER = 4" in header and "3 is reserved" in header


def test_mini_cheetah_hills_fixture():
    m, flat = load_model(FIXTURE), load_model("mini_cheetah")
    assert sorted(os.listdir(cc.FIXTURES)) == ["kane_mini_cheetah_hills.json", "mini_cheetah_hills.model", "mini_cheetah_hills.yaml"]
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "traj_allegro_hand.json"))
    assert all(os.path.getsize(os.path.join(cc.FIXTURES, f)) < limit for f in os.listdir(cc.FIXTURES))
    # the flat-ground cheetah, then two hills on the world: Cylinder(1.0, 25) rolled by pi / 2, at (2 + i, 0, -1 + 0.05)
    assert (m.nbodies, m.nq, m.nv, m.npaths, m.common_body) == (13, 19, 18, 4, 0) and m.body_names == flat.body_names
    ng = flat.ngeoms
    assert m.ngeoms == ng + 2
    for f in ("geom_body", "geom_type", "geom_size", "geom_X"):
        assert np.array_equal(getattr(m, f)[:ng], getattr(flat, f)), f
    roll = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], float)
    for i, g in enumerate((ng, ng + 1)):
        assert int(m.geom_type[g]) == cyl.CYLINDER and int(m.geom_body[g]) == -1
        assert np.array_equal(m.geom_size[g], [1.0, 12.5, 0.0])
        assert np.abs(m.geom_X[g][:9].reshape(3, 3) - roll).max() <= 1e-15
        assert np.array_equal(m.geom_X[g][9:], [2.0 + 1.0 * i, 0.0, -1.0 + 0.05])
    # the pairs: the flat cheetah's, and every sphere of the cheetah against every hill; the torso's box against a hill
    # is dropped
    pairs = list(zip(m.pair_a.tolist(), m.pair_b.tolist(), m.pair_path.tolist()))
    spheres = [g for g in range(ng) if int(m.geom_type[g]) == cyl.SPHERE]
    assert len(spheres) == 4
    flat_pairs = set(zip(flat.pair_a.tolist(), flat.pair_b.tolist(), flat.pair_path.tolist()))
    hill_pairs = {(s, h, int(m.body_path[int(m.geom_body[s])])) for s in spheres for h in (ng, ng + 1)}
    assert set(pairs) == flat_pairs | hill_pairs and len(pairs) == len(flat_pairs) + 8
    assert pairs == sorted(pairs, key=lambda p: (p[0], p[1]))
    box = [g for g in range(ng) if int(m.geom_type[g]) == cyl.BOX and int(m.geom_body[g]) >= 0]
    assert not any((b, h) == (pa, pb) for b in box for h in (ng, ng + 1) for pa, pb, _ in pairs)
    cfg, ref = load_config(os.path.join(cc.FIXTURES, "mini_cheetah_hills.yaml")), load_config("mini_cheetah")
    assert cfg["model"] == "mini_cheetah_hills" and "examples/mini_cheetah/mini_cheetah.yaml" in cfg["source"]
    assert {k: v for k, v in cfg.items() if k not in ("model", "source")} == \
        {k: v for k, v in ref.items() if k not in ("model", "source")}


def test_fixture_re_saves_to_identical_bytes(tmp_path):
    assert " type cylinder size " in open(FIXTURE).read()
    out = tmp_path / "x.model"
    load_model(FIXTURE).save(str(out))
    assert out.read_bytes() == open(FIXTURE, "rb").read()


def test_the_cpp_loader_reads_the_same_tables(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    src, exe = tmp_path / "probe.cc", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe), FIXTURE], text=True).strip().split("\n")
    m = load_model(FIXTURE)
    geoms = [l.split() for l in lines if not l.startswith("pair")]
    pairs = [l.split()[1:] for l in lines if l.startswith("pair")]
    assert len(geoms) == m.ngeoms
    for g, row in enumerate(geoms):
        assert (int(row[0]), int(row[1])) == (int(m.geom_body[g]), int(m.geom_type[g]))
        assert np.array_equal([float(x) for x in row[2:5]], m.geom_size[g])
        assert np.array_equal([float(x) for x in row[5:]], m.geom_X[g])
    assert pairs == [[str(int(m.pair_a[k])), str(int(m.pair_b[k])), str(int(m.pair_path[k]))] for k in range(m.npairs)]
    bad = tmp_path / "bad.model"
    bad.write_text(open(FIXTURE).read().replace(" type cylinder ", " type cone ", 1))
    done = subprocess.run([str(exe), str(bad)], capture_output=True, text=True)
    assert done.returncode != 0 and "unknown geometry type" in done.stderr


# ---- refusals: Model.validate, and idto_hip_create before it touches a device
class Unvalidated(Model):
    def validate(self):
        pass


def _good():
    """the hopper with a cylinder for its ground (geometry 2), a capsule and a sphere on its foot, one pair: sphere-cylinder"""
    m = cc.hopper_on_cylinder()
    m = copy.deepcopy(m)
    m.pair_a, m.pair_b, m.pair_path = m.pair_a[1:], m.pair_b[1:], m.pair_path[1:]
    return m.normalize()


def _set_type(g, t, size=None):
    def change(m):
        m.geom_type[g] = t
        if size is not None:
            m.geom_size[g] = size
    return change


def _second_cylinder(m):
    m.geom_type[1], m.geom_size[1] = cyl.CYLINDER, [0.03, 0.1, 0.0]


BAD = {
    "zero radius": (lambda m: m.geom_size.__setitem__(2, [0.0, 2.0, 0.0]), "cylinder size"),
    "negative radius": (lambda m: m.geom_size.__setitem__(2, [-0.5, 2.0, 0.0]), "cylinder size"),
    "zero H": (lambda m: m.geom_size.__setitem__(2, [0.5, 0.0, 0.0]), "cylinder size"),
    "negative H": (lambda m: m.geom_size.__setitem__(2, [0.5, -2.0, 0.0]), "cylinder size"),
    "nan size": (lambda m: m.geom_size.__setitem__(2, [0.5, np.nan, 0.0]), "cylinder size"),
    "inf size": (lambda m: m.geom_size.__setitem__(2, [np.inf, 2.0, 0.0]), "cylinder size"),
    "against a box": (_set_type(1, cyl.BOX, [0.03, 0.03, 0.03]), "cylinder contact pairs need a sphere on the other side"),
    "against a capsule": (_set_type(1, GEOM_TYPES["capsule"], [0.03, 0.1, 0.0]),
                          "cylinder contact pairs need a sphere on the other side"),
    "against a cylinder": (_second_cylinder, "cylinder contact pairs need a sphere on the other side"),
    "code 3": (_set_type(2, 3), "unknown geometry type"),
    "code 5": (_set_type(2, 5), "unknown geometry type"),
}


def _bad_model(key):
    good = _good()
    m = Unvalidated(**{f.name: copy.deepcopy(getattr(good, f.name)) for f in fields(good)})
    BAD[key][0](m)
    return good, m


@pytest.mark.parametrize("key", sorted(BAD))
def test_bad_cylinder_models_are_refused_by_name(key):
    good, m = _bad_model(key)
    prob, sp, _ = make_problem(load_config("hopper"), good, num_steps=4)
    with pytest.raises(hip.HipError, match=BAD[key][1]):
        hip.HipPath(m, prob, sp)
    checked = copy.deepcopy(good)
    for f in ("geom_type", "geom_size", "geom_body", "geom_X"):
        setattr(checked, f, copy.deepcopy(getattr(m, f)))
    with pytest.raises(AssertionError, match=BAD[key][1].replace("geometry type", "type")):
        Model.validate(checked)


def test_a_good_cylinder_model_passes_the_geometry_checks():
    good = _good()
    prob, sp, _ = make_problem(load_config("hopper"), good, num_steps=4)
    try:
        dev = hip.HipPath(good, prob, sp)
        assert dev.get_option("fast_shape") == 0
        dev.close()
    except hip.HipError as e:   # (a box without a GPU)
        assert "no HIP device" in str(e)


FAST_PROBE = r"""
#include <cstdio>
#include <string>
#include "host/model_tables.h"
#include "idto/model_file.h"
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const idto::ModelFile mf = idto::ModelFile::Load(argv[i]);
    const idto_model_t m = mf.c_model();
    idto_host::ModelTables t;
    std::string err;
    if (idto_host::BuildModelTables(&m, &t, &err)) { std::printf("refused %s\n", err.c_str()); continue; }
    std::printf("fast_shape %d capsules %d cylinders %d\n", t.fast_shape, (int)t.capsules, (int)t.cylinders);
  }
  return 0;
}
"""


def test_a_cylinder_clears_the_fast_shape(tmp_path):
    """BuildModelTables (host only): the flat cheetah and the hopper have shapes 3 and 2; with a cylinder, 0"""
    cxx = shutil.which("g++") or shutil.which("c++")
    src, exe = tmp_path / "probe.cc", tmp_path / "probe"
    src.write_text(FAST_PROBE)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "idto_amd", "csrc")]
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off"] + inc + [str(src), os.path.join(
        ROOT, "idto_amd", "csrc", "host", "model_tables.cc"), "-o", str(exe)])
    hop = tmp_path / "hopper_on_cylinder.model"
    cc.hopper_on_cylinder().save(str(hop))
    models = [os.path.join(ROOT, "idto_amd", "models", "mini_cheetah.model"), FIXTURE,
              os.path.join(ROOT, "idto_amd", "models", "hopper.model"), str(hop)]
    lines = subprocess.check_output([str(exe)] + models, text=True).strip().split("\n")
    assert lines == ["fast_shape 3 capsules 0 cylinders 0", "fast_shape 0 capsules 0 cylinders 1",
                     "fast_shape 2 capsules 0 cylinders 0", "fast_shape 0 capsules 0 cylinders 1"]


# ---- the independent Kane fixture against the oracle on the frozen model
def test_the_oracle_on_frozen_models_reproduces_the_kane_fixture():
    """the tolerance of tests/test_golden_examples.py for its Kane fixtures: tolerance_rel = 1e-7 of
    max(|tau|, |tau_contact|)"""
    fix = json.load(open(os.path.join(cc.FIXTURES, "kane_mini_cheetah_hills.json")))
    assert fix["tolerance_rel"] == 1e-7 and len(fix["states"]) == 6
    model, cfg = cc.hills()
    prob, sp, _ = make_problem(cfg, model, num_steps=1)
    for k, val in fix["contact"].items():
        assert getattr(sp, k) == val, "fixture generated with other contact parameters"
    fr = cyl.Frozen(model, prob, sp)
    hill = np.array([cyl.CYLINDER in (int(model.geom_type[int(a)]), int(model.geom_type[int(b)]))
                     for a, b in zip(model.pair_a, model.pair_b)])
    worst, kinds, rim_radius = 0.0, set(), set()
    for st in fix["states"]:
        q, v, a, want = (np.array(st[k]) for k in ("q", "v", "a", "tau"))
        scale = max(np.abs(want).max(), np.abs(st["tau_contact"]).max())
        err = np.abs(fr.tau(q, v, a) - want).max() / scale
        worst = max(worst, err)
        assert err <= fix["tolerance_rel"], (st["source"], err)
        frozen = cyl.frozen_model(model, fr.base.body_poses(q))
        orc = Oracle(frozen, prob, sp)
        near = orc.signed_distances(q)[0] <= orc.contact_threshold
        assert int(near.sum()) == st["acting_pairs"], st["source"]
        assert int((near & hill).sum()) == st["hill_pairs_acting"] and int((near & ~hill).sum()) == st["ground_pairs_acting"]
        kinds.add((bool((near & hill).any()), bool((near & ~hill).any())))
    print("largest |oracle on the frozen model - golden| / scale:", worst)
    assert {(False, False), (False, True), (True, True)} <= kinds   # the air, the ground alone, a hill and the ground


def test_the_oracle_and_the_model_checks_accept_a_sphere_of_radius_0():
    """the rim's substitute (cylinder_ref.frozen_model): Model.validate passes it and the oracle evaluates it as the point it is"""
    model, q, v, a = cc.directed("hopper", "rim", "sphere_first")
    prob, sp = make_problem(load_config("hopper"), model, num_steps=2)[:2]
    fr = cyl.Frozen(model, prob, sp)
    frozen = cyl.frozen_model(model, fr.base.body_poses(q))
    assert int(frozen.geom_type[1]) == cyl.SPHERE and frozen.geom_size[1][0] == 0.0
    phi = Oracle(frozen, prob, sp).signed_distances(q)[0]
    want = cc.expected_pairs(model, q, "hopper")
    assert want[0]["region"] == "rim" and abs(phi[0] - want[0]["phi"]) <= 1e-15
    assert np.all(np.isfinite(fr.tau(q, v, a)))


# ---- the trajectories of the device's frozen-oracle comparison (tests/test_gpu_cylinder.py): the conditions, without a GPU
@pytest.mark.parametrize("name", sorted(cc.FROZEN))
def test_the_cylinders_act_along_the_frozen_oracle_trajectories(name):
    """by the frozen oracle alone: the cylinder pairs change tau by more than 1e-3 at N / 2 time steps or more; on the
    cheetah a hill pair and a ground pair are within the threshold together at some step"""
    model, prob, sp, q, N = cc.frozen_case(name)
    v, a, tau, tau_no_cyl, P = cyl.frozen_expectation(model, prob, sp, q)
    n_act = int(np.count_nonzero(np.abs(tau - tau_no_cyl).max(axis=1) > 1e-3))
    print(name, "time steps at which the cylinder pairs act:", n_act, "of", N)
    assert n_act >= N // 2, n_act
    assert np.all(np.isfinite(tau))
    if name == "mini_cheetah_hills":
        assert cc.hill_and_ground_together(model, prob, sp, q)
