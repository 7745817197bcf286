"""A stem of bodies below the common body (include/idto_model.h), and the punyo fixture.

The common body - the one body where the tree branches - may sit on up to IDTO_MAX_STEM - 1 ancestors.  The CPU oracle
walks any tree with parent[i] < i and treats a body between the world and the common body as an ordinary body, so it needs
no change; what this file pins is the contract (Model.validate, idto_hip_create's refusals - made before a device is
touched -, the .model file in Python and C++), the fixture against an independent reading of the SDF, and the oracle on
stem models as a guard on the yardstick itself: a chain described as a stem gives the same bits, and the trajectories the
GPU tests use make a pair of every class act."""
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
from idto_amd.model import MAX_STEM, Model, load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_golden import _composite, _neutral_fk
from test_model_cross_pairs import drop_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
HUMANOID = 14       # punyo: bodies / DoFs 0-13 are the humanoid's, body 14 (DoFs 14-19) is the ball
MIN_CHANGE = 1e-3   # a class of pairs counts as acting when dropping it changes tau by more than this
PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")
CLASSES = ["arm-ball", "arm-ground", "ball-ground", "ball-torso", "ball-waist", "ground-torso"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def punyo():
    return load_model(os.path.join(EXAMPLES, "punyo.model")), load_config(os.path.join(EXAMPLES, "punyo.yaml"))


def all_gravity(model):
    m = copy.deepcopy(model)
    m.gravity_enabled = None
    return m.normalize()


def no_gravity(model):
    m = copy.deepcopy(model)
    m.gravity = np.zeros(3)
    m.gravity_enabled = None
    return m.normalize()


def zero_length(model):
    """every capsule with h = 0: on the device its sphere, bit for bit"""
    m = copy.deepcopy(model)
    for g in range(m.ngeoms):
        if int(m.geom_type[g]) == cr.CAPSULE:
            m.geom_size[g] = [m.geom_size[g][0], 0.0, 0.0]
    return m.normalize()


def as_spheres(model):
    """every capsule replaced by the sphere of its radius at its centre: what the oracle evaluates"""
    m = copy.deepcopy(model)
    for g in range(m.ngeoms):
        if int(m.geom_type[g]) == cr.CAPSULE:
            m.geom_type[g] = cr.SPHERE
            m.geom_size[g] = [m.geom_size[g][0], 0.0, 0.0]
    return m.normalize()


def pair_class(model, k):
    """punyo: which two of waist / torso (with the head) / arm / ball / ground pair k joins"""
    names = []
    for g in (int(model.pair_a[k]), int(model.pair_b[k])):
        b = int(model.geom_body[g])
        names.append("ground" if b < 0 else "ball" if b == HUMANOID else "waist" if b == 0 else "torso" if b == 3 else "arm")
    return "-".join(sorted(names))


def punyo_trajectory(cfg, model, N, seed):
    """The example's interpolation with noise, the humanoid lowered by 0.2 - 0.3 m on its column (torso and arms reach
    the ground) and the ball brought to 0.30 - 0.27 m in front of the waist: a pair of each of the six classes acts
    (test_punyo_trajectory_makes_every_class_of_pairs_act)."""
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.02)
    q[:, 0] = np.linspace(-0.20, -0.30, N + 1)
    q[:, 19] = np.linspace(0.30, 0.27, N + 1)
    return q


def restem(model, common, npaths=None):
    """The same tree with `common` as the common body (-1: none): every body below it becomes the stem, the chains are
    numbered in body order, and pair_path follows tools/convert_models.py's rules."""
    m = copy.deepcopy(model)
    m.common_body = common
    stem, b = set(), common
    while b >= 0:
        stem.add(b)
        b = int(m.parent[b])
    path, nxt = [-1] * m.nbodies, 0
    for i in range(m.nbodies):
        if i in stem:
            continue
        par = int(m.parent[i])
        if par < 0 or par == common:
            path[i] = nxt
            nxt += 1
        else:
            path[i] = path[par]
    m.body_path = path
    m.npaths = npaths or max(1, 1 << (nxt - 1).bit_length())
    pp = []
    for k in range(m.npairs):
        bodies = [int(m.geom_body[int(g)]) for g in (m.pair_a[k], m.pair_b[k])]
        chains = [path[b] for b in bodies if b >= 0 and path[b] >= 0]
        pp.append(chains[0] if chains else 0)
    for s in stem - {common}:   # (the pairs of one stem body: one path - that of the chain bodies it meets)
        mine = [k for k in range(m.npairs) if s in (int(m.geom_body[int(m.pair_a[k])]), int(m.geom_body[int(m.pair_b[k])]))]
        met = {pp[k] for k in mine if any(path[int(m.geom_body[int(g)])] >= 0 for g in (m.pair_a[k], m.pair_b[k])
                                         if int(m.geom_body[int(g)]) >= 0)}
        assert len(met) <= 1
        for k in mine:
            pp[k] = min(met) if met else 0
    m.pair_path = pp
    return m.normalize()


def jaco_chain_and_stems():
    """jaco (every body's weight on) as one chain off the world beside the box, and with its second / third arm link as
    the common body: a stem of 2 / 3, the rest of the arm one chain off the common body"""
    arm = all_gravity(load_model(os.path.join(EXAMPLES, "jaco.model")))
    cfg = load_config(os.path.join(EXAMPLES, "jaco.yaml"))
    return cfg, restem(arm, -1), {2: restem(arm, 1, npaths=2), 3: restem(arm, 2, npaths=2)}


def hopper_on_a_planar_stem():
    """the hopper with its leg as the common body: the stem's first body has the planar joint (attached to the world, as
    the rule for planar and floating joints wants it), the foot is a chain of one off the common body"""
    chain, cfg = load_model("hopper"), load_config("hopper")
    return cfg, chain, restem(chain, 1)


def synthetic_stem_model():
    """punyo's spheres, every body's weight on, with IDTO_MAX_STEM stem bodies of which the third (not adjacent to the
    world) carries two spheres: each against the ground and against the ball (a chain body) - four pairs on one stem
    body, all in the ball's path -, and the common body touched from three paths (the ball's, and both upper arms' through
    pairs that the fixture filters)."""
    m = as_spheres(all_gravity(punyo()[0]))
    assert m.stem == [0, 1, 2, 3] and len(m.stem) == MAX_STEM
    ball, ground, arm_l, arm_r = 13, 14, 7, 10
    assert int(m.geom_body[ball]) == HUMANOID and int(m.geom_body[ground]) == -1
    assert (int(m.geom_body[arm_l]), int(m.geom_body[arm_r])) == (5, 10)
    eye = list(np.eye(3).ravel())
    m.geom_body = np.concatenate([m.geom_body, [2, 2]])
    m.geom_type = np.concatenate([m.geom_type, [cr.SPHERE, cr.SPHERE]])
    m.geom_size = np.concatenate([m.geom_size, [[0.09, 0, 0], [0.06, 0, 0]]])
    m.geom_X = np.concatenate([m.geom_X, [eye + [0.0, 0.05, 0.0], eye + [0.05, 0.12, -0.05]]])
    extra = [(ball, 15, 2), (ground, 15, 2), (ball, 16, 2), (ground, 16, 2), (2, arm_l, 0), (3, arm_l, 0), (1, arm_r, 1)]
    m.pair_a = np.concatenate([m.pair_a, [e[0] for e in extra]])
    m.pair_b = np.concatenate([m.pair_b, [e[1] for e in extra]])
    m.pair_path = np.concatenate([m.pair_path, [e[2] for e in extra]])
    return m.normalize()


# ---- 1. the fixture
def test_punyo_fixture():
    m, cfg = punyo()
    assert (m.nbodies, m.nq, m.nv) == (15, 21, 20)
    arm = lambda s: [f"glue_torso_arm{s}", f"arm_{s}", f"glue_arm_forearm{s}", f"forearm_{s}", f"hand_{s}"]
    assert m.body_names == ["waist", "glue_torso_waist1", "glue_torso_waist2", "torso"] + arm("L") + arm("R") + ["ball"]
    assert list(m.parent) == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 3, 9, 10, 11, 12, -1]
    assert list(m.jtype) == [1] + [0] * 13 + [3]
    assert m.common_body == 3 and m.stem == [0, 1, 2, 3] and m.npaths == 4
    assert list(m.body_path) == [-1] * 4 + [0] * 5 + [1] * 5 + [2]
    assert list(m.gravity_enabled) == [0] * 14 + [1]
    assert m.ngeoms == 15
    assert [int(t) for t in m.geom_type] == [cr.CAPSULE] * 9 + [cr.SPHERE] + [cr.CAPSULE] * 2 + [cr.SPHERE] * 2 + [cr.BOX]
    assert [int(b) for b in m.geom_body] == [0] + [3] * 6 + [5, 7, 8, 10, 12, 13, 14, -1]
    assert m.npairs == 26
    count = {c: sum(pair_class(m, k) == c for k in range(m.npairs)) for c in CLASSES}
    assert count == {"ball-waist": 1, "ball-torso": 6, "ground-torso": 6, "arm-ball": 6, "arm-ground": 6, "ball-ground": 1}
    # the one pair on the stem names the ball's path; the arms' pairs with the ball are shared pairs
    k = next(k for k in range(m.npairs) if pair_class(m, k) == "ball-waist")
    assert int(m.pair_path[k]) == 2
    assert list(m.actuated) == [1] * 14 + [0] * 6 and m.unactuated_dofs == list(range(14, 20))
    assert not np.any(m.damping)
    # the default inertia of an <inertial> without <inertia>: the unit tensor (waist: one link, its frame the body's)
    assert np.array_equal(m.inertia[0], [1, 1, 1, 0, 0, 0]) and m.mass[0] == 12
    assert cfg["num_steps"] == 40 and cfg["time_step"] == 0.05 and cfg["max_iters"] == 50
    assert cfg["method"] == "trust_region" and cfg["scaling"] is True and cfg["equality_constraints"] is True
    assert cfg["gradients_method"] == "forward_differences" and cfg["contact_stiffness"] == 500
    prob, sp, q_guess = make_problem(cfg, m)
    assert prob.num_steps == 40 and q_guess.shape == (41, 21) and sp.equality_constraints


def test_model_file_round_trip(tmp_path):
    src = os.path.join(EXAMPLES, "punyo.model")
    out = tmp_path / "punyo.model"
    load_model(src).save(str(out))
    assert out.read_bytes() == open(src, "rb").read()


PROBE = r"""
#include <cstdio>
#include "idto_model.h"
#include "idto/model_file.h"
int main(int argc, char** argv) {
  const idto::ModelFile mf = idto::ModelFile::Load(argv[1]);
  const idto_model_t m = mf.c_model();
  std::printf("%d %d %d %d %d %d %d\n", m.nbodies, m.nq, m.nv, m.npaths, m.common_body, m.ngeoms, m.npairs);
  for (int i = 0; i < m.nbodies; ++i) {
    std::printf("%d %d %d %d %d", m.parent[i], m.jtype[i], m.body_path[i], m.qstart[i], m.gravity_enabled ? m.gravity_enabled[i] : 1);
    for (int e = 0; e < 12; ++e) std::printf(" %.17g", m.X_PF[12 * i + e]);
    std::printf("\n");
  }
  for (int k = 0; k < m.npairs; ++k) std::printf("%d %d %d\n", m.pair_a[k], m.pair_b[k], m.pair_path[k]);
  return 0;
}
"""


def test_the_cpp_loader_reads_the_same_tables(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    src, exe = tmp_path / "probe.cc", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe), os.path.join(EXAMPLES, "punyo.model")], text=True).strip().split("\n")
    m = punyo()[0]
    assert [int(x) for x in lines[0].split()] == [15, 21, 20, 4, 3, 15, 26]
    for i in range(m.nbodies):
        row = lines[1 + i].split()
        assert [int(x) for x in row[:5]] == [int(m.parent[i]), int(m.jtype[i]), int(m.body_path[i]), int(m.qstart[i]),
                                             int(m.gravity_enabled[i])]
        assert np.array_equal([float(x) for x in row[5:]], m.X_PF[i])
    pairs = [[int(x) for x in l.split()] for l in lines[1 + m.nbodies:]]
    assert pairs == [[int(m.pair_a[k]), int(m.pair_b[k]), int(m.pair_path[k])] for k in range(m.npairs)]


# ---- 2. against the independent reading of the SDF (tools/make_model_fixture.py): joint poses, default inertia
def test_converted_model_matches_the_independent_reading():
    fix = json.load(open(os.path.join(EXAMPLES, "world_punyo.json")))
    m = punyo()[0]
    X = _neutral_fk(m)
    links = fix["links"]

    def root_of(link):
        while links[link].get("welded_to") not in (None, "world"):
            link = links[link]["welded_to"]
        return "world" if links[link].get("welded_to") == "world" else link

    groups = {}
    for ln in links:
        groups.setdefault(root_of(ln), []).append(ln)
    assert groups["world"] == ["base"] and sorted(groups["torso"]) == ["glue_torso_neck", "head", "torso"]
    names = list(m.body_names)
    assert sorted(names) == sorted(g for g in groups if g != "world")
    for b, bn in enumerate(names):
        mass, c, I = _composite([(links[l]["mass"], links[l]["com_W"], links[l]["I_W"]) for l in groups[bn]])
        R, p = X[b][:3, :3], X[b][:3, 3]
        Ib = np.asarray(m.inertia[b], float)
        IB = np.array([[Ib[0], Ib[3], Ib[4]], [Ib[3], Ib[1], Ib[5]], [Ib[4], Ib[5], Ib[2]]])
        assert abs(m.mass[b] - mass) <= 1e-12 * mass, bn
        assert np.abs(p + R @ np.asarray(m.com[b], float) - c).max() <= 1e-12, bn
        assert np.abs(R @ IB @ R.T - I).max() <= 1e-12 * max(1.0, np.abs(I).max()), bn
    # every movable joint: the axis in the world, sign included (two joint frames are turned by pi: the axis of
    # shoulderR_joint2 points to -y, that of elbowR_joint2 too), and for a revolute joint the axis line
    assert len(fix["joints"]) == 14
    for j in fix["joints"]:
        b = names.index(j["child"])
        a_model = X[b][:3, :3] @ np.asarray(m.axis[b], float)
        a_fix = np.asarray(j["axis_W"]) / np.linalg.norm(j["axis_W"])
        assert np.abs(a_model - a_fix).max() <= 1e-4, (j["name"], a_model, a_fix)   # (the file writes pi as 3.1416)
        assert int(m.jtype[b]) == (1 if j["type"] == "prismatic" else 0)
        if j["type"] == "revolute":
            assert np.linalg.norm(np.cross(np.asarray(j["anchor_W"]) - X[b][:3, 3], a_fix)) <= 1e-9, j["name"]
    turned = {j["name"]: j["axis_W"] for j in fix["joints"]}
    assert turned["shoulderR_joint2"][1] < -0.99 and turned["elbowR_joint2"][1] < -0.99 and turned["shoulderL_joint2"][1] > 0.99
    # collision primitives: place, size, and a capsule's axis
    want = list(fix["world_geoms"]) + [g for L in links.values() for g in L["geoms"]]
    assert len(want) == m.ngeoms
    kinds = {cr.SPHERE: "sphere", cr.CAPSULE: "capsule", cr.BOX: "box"}
    for gi in range(m.ngeoms):
        gb, xg = int(m.geom_body[gi]), np.asarray(m.geom_X[gi], float)
        XG = np.eye(4)
        XG[:3, :3], XG[:3, 3] = xg[:9].reshape(3, 3), xg[9:]
        XWG = (X[gb] if gb >= 0 else np.eye(4)) @ XG
        kind = kinds[int(m.geom_type[gi])]
        best = min((w for w in want if w["type"] == kind),
                   key=lambda w: (np.linalg.norm(np.asarray(w["X_WG"])[:3, 3] - XWG[:3, 3]),
                                  abs(w["size"][0] - m.geom_size[gi][0])))
        W = np.asarray(best["X_WG"])
        assert np.abs(W[:3, 3] - XWG[:3, 3]).max() <= 1e-12, gi
        if kind == "box":
            assert np.array_equal(np.asarray(best["size"]) / 2, m.geom_size[gi])
        else:
            assert abs(m.geom_size[gi][0] - best["size"][0]) <= 1e-15
        if kind == "capsule":
            assert np.abs(W[:3, 2] - XWG[:3, 2]).max() <= 1e-12, gi
            assert abs(m.geom_size[gi][1] - best["size"][1] / 2) <= 1e-15 and m.geom_size[gi][2] == 0


# ---- 3. refusals: Model.validate, and idto_hip_create before it touches a device
class Unvalidated(Model):
    def validate(self):
        pass


def _append_pair(m, ga, gb, path):
    m.pair_a = np.concatenate([m.pair_a, [ga]]).astype(np.int32)
    m.pair_b = np.concatenate([m.pair_b, [gb]]).astype(np.int32)
    m.pair_path = np.concatenate([m.pair_path, [path]]).astype(np.int32)


# edit of the punyo fixture -> (Model.validate's message, idto_hip_create's message)
BAD_STEM = {
    "a stem of five": (lambda m: setattr(m, "common_body", 4), "longer than MAX_STEM", "longer than IDTO_MAX_STEM"),
    "a second child": (lambda m: m.parent.__setitem__(4, 2), "second child", "second child"),
    "a path on a stem body": (lambda m: m.body_path.__setitem__(1, 0), "must have path -1", "must have body_path -1"),
    "two paths on one stem body": (lambda m: _append_pair(m, 0, 14, 0), "different paths", "different paths"),
    "a pair inside the stem": (lambda m: _append_pair(m, 0, 1, 2), "joins two stem bodies", "between two stem bodies"),
}


def bad_stem_model(key):
    good = punyo()[0]
    m = Unvalidated(**{f.name: copy.deepcopy(getattr(good, f.name)) for f in fields(good)})
    BAD_STEM[key][0](m)
    return good, m


@pytest.mark.parametrize("key", sorted(BAD_STEM))
def test_bad_stems_are_refused(key):
    good, m = bad_stem_model(key)
    with pytest.raises(AssertionError, match=BAD_STEM[key][1]):
        Model.validate(m)
    prob, sp, _ = make_problem(punyo()[1], good, num_steps=4)
    with pytest.raises(hip.HipError, match=BAD_STEM[key][2]):
        hip.HipPath(m, prob, sp)


def test_the_good_stem_passes_the_checks():
    good, cfg = punyo()
    good.validate()
    prob, sp, _ = make_problem(cfg, good, num_steps=4)
    try:
        hip.HipPath(good, prob, sp).close()
    except hip.HipError as e:   # (a box without a GPU)
        assert "no HIP device" in str(e)


def test_stem_length_one_is_todays_contract():
    for name in ("mini_cheetah", "allegro_hand"):
        m = load_model(name)
        assert m.stem == [m.common_body]
    assert load_model("hopper").stem == []


# ---- 4. the oracle on stem models
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_gives_a_chain_described_as_a_stem_the_same_bits(seed):
    cfg, chain, stems = jaco_chain_and_stems()
    assert chain.common_body == -1 and chain.npaths == 2 and list(chain.body_path) == [0] * 7 + [1]
    N = 10
    q = synthetic_trajectory(cfg, chain, N, seed=seed, lower=0.02)
    prob, sp, _ = make_problem(cfg, chain, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    want = Oracle(chain, prob, sp)
    tau = want.eval_traj(q)[2]
    # (contact acts: without the pairs tau differs by tens of N m)
    assert np.abs(tau - Oracle(cr.without_geometry(chain), prob, sp).eval_traj(q)[2]).max() > 10.0
    P = want.eval_partials(q)
    for ns, m in stems.items():
        assert len(m.stem) == ns and m.common_body == ns - 1
        assert list(m.body_path) == [-1] * ns + [0] * (7 - ns) + [1]
        got = Oracle(m, prob, sp)
        assert same(got.eval_traj(q)[2], tau), ns
        assert same(got.mass_matrix(q[3]), want.mass_matrix(q[3])), ns
        Pg = got.eval_partials(q)
        for k in PARTIALS:
            assert same(Pg[k], P[k]), (ns, k)


def test_oracle_gives_a_stem_that_starts_with_a_planar_joint_the_chains_bits():
    cfg, chain, stem = hopper_on_a_planar_stem()
    assert stem.stem == [0, 1] and list(stem.body_path) == [-1, -1, 0] and int(stem.jtype[0]) == 2
    N = 10
    q = synthetic_trajectory(cfg, chain, N, seed=0, lower=0.01)
    prob, sp, _ = make_problem(cfg, chain, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    want, got = Oracle(chain, prob, sp), Oracle(stem, prob, sp)
    tau = want.eval_traj(q)[2]
    assert np.abs(tau - Oracle(cr.without_geometry(chain), prob, sp).eval_traj(q)[2]).max() > MIN_CHANGE
    assert same(got.eval_traj(q)[2], tau)
    P, Pg = want.eval_partials(q), got.eval_partials(q)
    for k in PARTIALS:
        assert same(Pg[k], P[k]), k


@pytest.mark.parametrize("seed", [0, 1])
def test_punyo_trajectory_makes_every_class_of_pairs_act(seed):
    """on the trajectory the GPU tests use, at N = 40: a pair of each of the six classes is inside the contact threshold,
    and dropping the class changes the oracle's tau by more than MIN_CHANGE; the mass matrix is symmetric"""
    model, cfg = punyo()
    m = as_spheres(all_gravity(model))
    N = 40
    q = punyo_trajectory(cfg, m, N, seed)
    prob, sp, _ = make_problem(cfg, m, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    orc = Oracle(m, prob, sp)
    inside = set()
    for t in range(N + 1):
        phi = orc.signed_distances(q[t])[0]
        inside |= {pair_class(m, k) for k in range(m.npairs) if phi[k] <= orc.contact_threshold}
    assert inside == set(CLASSES)
    tau = orc.eval_traj(q)[2]
    for c in CLASSES:
        cut = Oracle(drop_pairs(m, [k for k in range(m.npairs) if pair_class(m, k) == c]), prob, sp).eval_traj(q)[2]
        assert np.abs(tau - cut).max() > MIN_CHANGE, c
    for t in (0, N // 2, N):
        M = orc.mass_matrix(q[t])
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
        assert np.all(np.linalg.eigvalsh(0.5 * (M + M.T)) > 0)


def test_synthetic_stem_model_loads_its_stem():
    """the model of the GPU tests: four pairs on the third stem body, in one path; the common body touched from three paths;
    and the oracle feels them"""
    m = synthetic_stem_model()
    on_glue = [k for k in range(m.npairs) if 2 in (int(m.geom_body[int(m.pair_a[k])]), int(m.geom_body[int(m.pair_b[k])]))]
    assert len(on_glue) == 4 and {int(m.pair_path[k]) for k in on_glue} == {2}
    on_torso = [k for k in range(m.npairs) if 3 in (int(m.geom_body[int(m.pair_a[k])]), int(m.geom_body[int(m.pair_b[k])]))]
    assert {int(m.pair_path[k]) for k in on_torso} == {0, 1, 2}
    cfg = punyo()[1]
    N = 8
    q = punyo_trajectory(cfg, m, N, 0)
    prob, sp, _ = make_problem(cfg, m, num_steps=N)
    tau = Oracle(m, prob, sp).eval_traj(q)[2]
    for ks in (on_glue, [m.npairs - 3, m.npairs - 2], [m.npairs - 1]):
        assert np.abs(tau - Oracle(drop_pairs(m, ks), prob, sp).eval_traj(q)[2]).max() > MIN_CHANGE
