"""Capsule geometry (IDTO_GEOM_CAPSULE, include/idto_model.h) on the host: the capsule spinner fixtures
(tests/golden/examples/, tools/convert_models.py) against their independent readings (world_*.json there,
tools/make_model_fixture.py), the .model format in Python and C++, Model.validate and idto_hip_create's refusals (made
before any device is touched), and the test-side closest-point rules (capsule_ref.py) against brute force."""
import copy
import json
import os
import shutil
import subprocess
from dataclasses import fields

import numpy as np
import pytest

import capsule_ref as cr
from idto_amd import hip
from idto_amd.model import Model, load_model
from idto_amd.problem import load_config, make_problem
from test_golden import _neutral_fk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
NAMES = ["spinner_capsule", "2dof_spinner_capsule"]


def example(name):
    return load_model(os.path.join(EXAMPLES, name + ".model"))


def test_spinner_capsule_fixture():
    m = example("spinner_capsule")
    assert (m.nbodies, m.nq, m.nv) == (3, 3, 3) and m.body_names == ["finger_one", "finger_two", "spinner"]
    assert [int(t) for t in m.geom_type] == [cr.SPHERE] * 11 + [cr.CAPSULE]
    assert int(m.geom_body[11]) == 2 and np.array_equal(m.geom_size[11], [0.25, 0.4, 0.0])
    assert m.npairs == 11 and all(int(m.pair_b[k]) == 11 for k in range(11))
    cfg, ref = load_config(os.path.join(EXAMPLES, "spinner_capsule.yaml")), load_config("spinner")
    assert cfg["model"] == "spinner_capsule" and "examples/spinner/spinner.yaml" in cfg["source"]
    assert {k: v for k, v in cfg.items() if k not in ("model", "source")} == \
        {k: v for k, v in ref.items() if k not in ("model", "source")}
    assert make_problem(cfg, m)[0].num_steps == 40


def test_2dof_spinner_capsule_fixture():
    m = example("2dof_spinner_capsule")
    assert (m.nbodies, m.nq, m.nv) == (2, 2, 2) and m.body_names == ["finger_two", "spinner"]
    assert [int(t) for t in m.geom_type] == [cr.CAPSULE, cr.CAPSULE]
    assert np.array_equal(m.geom_size, [[0.05, 0.45, 0.0], [0.25, 0.4, 0.0]])
    assert m.npairs == 1 and (int(m.pair_a[0]), int(m.pair_b[0])) == (0, 1)
    assert not os.path.exists(os.path.join(EXAMPLES, "2dof_spinner_capsule.yaml"))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_re_saves_to_identical_bytes(name, tmp_path):
    src = os.path.join(EXAMPLES, name + ".model")
    assert " type capsule size " in open(src).read()
    out = tmp_path / "x.model"
    example(name).save(str(out))
    assert out.read_bytes() == open(src, "rb").read()


PROBE = r"""
#include <cstdio>
#include "idto_model.h"
#include "idto/model_file.h"
int main(int argc, char** argv) {
  const idto::ModelFile mf = idto::ModelFile::Load(argv[1]);
  const idto_model_t m = mf.c_model();
  for (int g = 0; g < m.ngeoms; ++g) {
    std::printf("%d %d", m.geom_body[g], m.geom_type[g]);
    for (int i = 0; i < 3; ++i) std::printf(" %.17g", m.geom_size[3 * g + i]);
    for (int i = 0; i < 12; ++i) std::printf(" %.17g", m.geom_X[12 * g + i]);
    std::printf("\n");
  }
  for (int k = 0; k < m.npairs; ++k) std::printf("pair %d %d %d\n", m.pair_a[k], m.pair_b[k], m.pair_path[k]);
  return 0;
}
"""


@pytest.mark.parametrize("name", NAMES)
def test_the_cpp_loader_reads_the_same_tables(name, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    src, exe = tmp_path / "probe.cc", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe), os.path.join(EXAMPLES, name + ".model")], text=True).strip().split("\n")
    m = example(name)
    geoms = [l.split() for l in lines if not l.startswith("pair")]
    pairs = [l.split()[1:] for l in lines if l.startswith("pair")]
    assert len(geoms) == m.ngeoms
    for g, row in enumerate(geoms):
        assert (int(row[0]), int(row[1])) == (int(m.geom_body[g]), int(m.geom_type[g]))
        assert np.array_equal([float(x) for x in row[2:5]], m.geom_size[g])
        assert np.array_equal([float(x) for x in row[5:]], m.geom_X[g])
    assert pairs == [[str(int(m.pair_a[k])), str(int(m.pair_b[k])), str(int(m.pair_path[k]))] for k in range(m.npairs)]


@pytest.mark.parametrize("name", NAMES)
def test_converted_geometry_matches_the_independent_reading(name):
    """world pose, axis and size of every collision primitive at the neutral configuration"""
    fix = json.load(open(os.path.join(EXAMPLES, f"world_{name}.json")))
    m = example(name)
    X = _neutral_fk(m)
    want = [g for L in fix["links"].values() for g in L["geoms"]]
    assert len(want) == m.ngeoms
    for gi in range(m.ngeoms):
        gb, xg = int(m.geom_body[gi]), np.asarray(m.geom_X[gi], float)
        XG = np.eye(4)
        XG[:3, :3], XG[:3, 3] = xg[:9].reshape(3, 3), xg[9:]
        XWG = (X[gb] if gb >= 0 else np.eye(4)) @ XG
        kind = {cr.SPHERE: "sphere", cr.CAPSULE: "capsule"}[int(m.geom_type[gi])]
        best = min((w for w in want if w["type"] == kind),
                   key=lambda w: np.linalg.norm(np.asarray(w["X_WG"])[:3, 3] - XWG[:3, 3]))
        W = np.asarray(best["X_WG"])
        assert np.abs(W[:3, 3] - XWG[:3, 3]).max() <= 1e-12, gi
        assert abs(m.geom_size[gi][0] - best["size"][0]) <= 1e-15
        if kind == "capsule":   # the axis (sign included: it names the -h end) and half the length
            assert np.abs(W[:3, 2] - XWG[:3, 2]).max() <= 1e-12, gi
            assert abs(m.geom_size[gi][1] - best["size"][1] / 2) <= 1e-15 and m.geom_size[gi][2] == 0


# ---- refusals: Model.validate, and idto_hip_create before it touches a device
class Unvalidated(Model):
    def validate(self):
        pass


BAD = {
    "unknown type": (lambda m: m.geom_type.__setitem__(0, 3), "unknown geometry type"),
    "zero radius": (lambda m: m.geom_size.__setitem__(0, [0.0, 0.1, 0.0]), "capsule size"),
    "negative h": (lambda m: m.geom_size.__setitem__(0, [0.03, -0.1, 0.0]), "capsule size"),
    "nan size": (lambda m: m.geom_size.__setitem__(0, [0.03, np.nan, 0.0]), "capsule size"),
    "inf size": (lambda m: m.geom_size.__setitem__(0, [np.inf, 0.1, 0.0]), "capsule size"),
    "moving box": (lambda m: m.geom_body.__setitem__(2, 0), "capsule-box"),
    "rotated box": (lambda m: m.geom_X.__setitem__(2, np.concatenate([[np.cos(.1), -np.sin(.1), 0, np.sin(.1), np.cos(.1), 0,
                                                                        0, 0, 1], m.geom_X[2][9:]])), "capsule-box"),
}


def _bad_model(key):
    good = load_model("hopper")
    good.geom_type = np.array([cr.CAPSULE, cr.SPHERE, cr.BOX], dtype=np.int32)
    good.geom_size = np.array(good.geom_size)
    good.geom_size[0] = [0.03, 0.1, 0.0]
    good = good.normalize()
    m = Unvalidated(**{f.name: copy.deepcopy(getattr(good, f.name)) for f in fields(good)})
    BAD[key][0](m)
    return good, m


@pytest.mark.parametrize("key", sorted(BAD))
def test_bad_capsule_models_are_refused(key):
    good, m = _bad_model(key)
    prob, sp, _ = make_problem(load_config("hopper"), good, num_steps=4)
    with pytest.raises(hip.HipError, match=BAD[key][1]):
        hip.HipPath(m, prob, sp)
    checked = copy.deepcopy(good)
    for f in ("geom_type", "geom_size", "geom_body", "geom_X"):
        setattr(checked, f, copy.deepcopy(getattr(m, f)))
    with pytest.raises(AssertionError):
        Model.validate(checked)


def test_a_good_capsule_model_passes_the_geometry_checks():
    good, _ = _bad_model("unknown type")
    prob, sp, _ = make_problem(load_config("hopper"), good, num_steps=4)
    try:
        hip.HipPath(good, prob, sp).close()
    except hip.HipError as e:   # (a box without a GPU)
        assert "no HIP device" in str(e)


# ---- the closest-point rules against brute force
def seg(p, u, h, n):
    s = np.linspace(-h, h, n)
    return p + s[:, None] * u


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def rot_about_y(a):
    return np.array([np.sin(a), 0.0, np.cos(a)])


SEGMENTS = {   # p1, u1, h1, p2, u2, h2
    "crossing": ([0, 0, 0], [1, 0, 0], 1.0, [0.2, 0.1, 0], [0, 1, 0], 1.0),
    "skew": ([0, 0, 0], unit([1, 0.2, 0]), 0.8, [0.1, -0.3, 0.5], unit([0.3, 1, 0.4]), 0.6),
    "end caps": ([0, 0, 0], [0, 0, 1], 0.5, [0.3, 0.1, 1.2], unit([1, 1, 0]), 0.4),
    "near parallel, general branch": ([0, 0, 0], [0, 0, 1], 1.0, [0.3, 0, 0.5], rot_about_y(1e-4), 1.0),
    "near parallel, parallel rule": ([0, 0, 0], [0, 0, 1], 1.0, [0.3, 0, 0.5], rot_about_y(1e-6), 1.0),
    "parallel overlapping": ([0, 0, 0], [0, 0, 1], 1.0, [0.3, 0, 0.5], [0, 0, 1], 1.0),
    "anti-parallel overlapping": ([0, 0, 0], [0, 0, 1], 1.0, [0.3, 0, 0.5], [0, 0, -1], 1.0),
    "parallel disjoint": ([0, 0, 0], [0, 0, 1], 1.0, [0.1, 0, 3.0], [0, 0, 1], 1.0),
}


@pytest.mark.parametrize("case", sorted(SEGMENTS))
def test_capsule_capsule_rule_against_brute_force(case):
    p1, u1, h1, p2, u2, h2 = [np.asarray(x, float) if not isinstance(x, float) else x for x in SEGMENTS[case]]
    c1, c2 = cr.capsule_capsule(p1, u1, h1, p2, u2, h2)
    for c, p, u, h in ((c1, p1, u1, h1), (c2, p2, u2, h2)):   # on the segments
        assert np.linalg.norm(np.cross(c - p, u)) <= 1e-12 and abs(np.dot(c - p, u)) <= h + 1e-12
    n = 801
    A, B = seg(p1, u1, h1, n), seg(p2, u2, h2, n)
    d = np.linalg.norm(A[:, None, :] - B[None, :, :], axis=2)
    i, j = np.unravel_index(np.argmin(d), d.shape)
    res = (2 * h1 + 2 * h2) / (n - 1)   # a grid point lies within res / 2 of any point of each segment
    dist = np.linalg.norm(c1 - c2)
    # (below the threshold the rule treats the segments as parallel: off by at most the angle, <= sqrt(PARALLEL), times
    # the lengths)
    slack = (h1 + h2) * np.sqrt(cr.PARALLEL) if 1 - np.dot(u1, u2) ** 2 <= cr.PARALLEL else 0.0
    assert dist <= d[i, j] + 1e-12 + slack and d[i, j] <= dist + res
    if "parallel" not in case:   # (a unique minimiser: the points themselves)
        assert np.linalg.norm(c1 - A[i]) <= 10 * res and np.linalg.norm(c2 - B[j]) <= 10 * res
    if case in ("parallel overlapping", "anti-parallel overlapping"):   # the middle of the overlap, z in [-0.5, 1]
        assert np.allclose(c1, [0, 0, 0.25]) and np.allclose(c2, [0.3, 0, 0.25])
    if case == "parallel disjoint":
        assert np.allclose(c1, [0, 0, 1]) and np.allclose(c2, [0.1, 0, 2])


@pytest.mark.parametrize("x", [[0.3, 0.2, 0.1], [0.1, -0.2, 2.0], [0.0, 0.5, -3.0], [1.0, 1.0, 0.7]])
def test_sphere_capsule_rule_against_brute_force(x):
    x, p, u, h = np.asarray(x, float), np.array([0.1, 0.0, 0.2]), unit([0.2, 0.3, 1.0]), 0.8
    c = cr.sphere_capsule(x, p, u, h)
    S = seg(p, u, h, 4001)
    k = np.argmin(np.linalg.norm(S - x, axis=1))
    assert np.linalg.norm(c - S[k]) <= 2 * h / 4000 and np.linalg.norm(x - c) <= np.linalg.norm(x - S[k]) + 1e-12


def test_capsule_box_rule_takes_the_lower_end_and_the_minus_h_end_on_a_tie():
    p, h = np.array([0.0, 0.0, 1.0]), 0.5
    for u in (unit([0.3, 0, 1]), unit([0.3, 0, -1]), unit([1, 0.2, 0.4])):
        S = seg(p, u, h, 1001)
        assert np.array_equal(cr.capsule_box(p, u, h), S[np.argmin(S[:, 2])] if S[0, 2] != S[-1, 2] else S[0]) or \
            np.allclose(cr.capsule_box(p, u, h), S[np.argmin(S[:, 2])])
    u = np.array([1.0, 0.0, 0.0])   # horizontal: a tie
    assert np.array_equal(cr.capsule_box(p, u, h), p - u * h)


def test_zero_length_rules_return_the_centre_itself():
    rng = np.random.default_rng(0)
    for _ in range(50):
        p, q, x = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        u, w = unit(rng.normal(size=3)), unit(rng.normal(size=3))
        assert cr.sphere_capsule(x, p, u, 0.0) is p
        assert cr.capsule_box(p, u, 0.0) is p
        c1, c2 = cr.capsule_capsule(p, u, 0.0, q, w, 0.0)
        assert c1 is p and c2 is q
