"""idto_hip_create's refusals of a model (idto_amd/csrc/host/model_tables.cc): all of them are made on the host's tables
before a device is asked for, so each has a case here that needs no GPU - one edit of a good fixture, handed over without
Model.validate, and the library's own message expected.  (The stem's and the capsule's rules: test_model_stem.py,
test_model_capsule.py.)  A good model of every fixture family gets past all of them: it reaches the device check."""
import copy
import os
from dataclasses import fields

import pytest

import capsule_ref as cr
from idto_amd import hip
from idto_amd.model import MAX_CHAIN, Model, load_model
from idto_amd.problem import load_config, make_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
BUILT_IN = ["acrobot", "allegro_hand", "hopper", "mini_cheetah", "spinner"]
FIXTURES = ["dual_jaco", "jaco", "jaco_ball", "punyo", "spinner_capsule"]
PLANAR = 2


class Unvalidated(Model):
    """hands its tables to idto_hip_create without Model.validate (which would refuse them first)"""

    def validate(self):
        pass


def fixture(name):
    if name in BUILT_IN:
        return load_model(name), load_config(name)
    return load_model(os.path.join(EXAMPLES, name + ".model")), load_config(os.path.join(EXAMPLES, name + ".yaml"))


def bodies_of(m, k):
    return [int(m.geom_body[int(g)]) for g in (m.pair_a[k], m.pair_b[k])]


def chain_pair(m):
    """a pair that touches a chain body, and that body"""
    for k in range(m.npairs):
        for b in bodies_of(m, k):
            if b >= 0 and int(m.body_path[b]) >= 0:
                return k, b
    raise AssertionError("no pair on a chain body")


def box_box_pair(m):
    return next(k for k in range(m.npairs) if int(m.geom_type[int(m.pair_a[k])]) == int(m.geom_type[int(m.pair_b[k])]) == cr.BOX)


def not_a_power_of_two(m):
    m.npaths = 3


def planar_joint_on_a_body(m):
    assert int(m.jtype[0]) == PLANAR and m.common_body == -1
    m.parent[0] = 1


def gravity_flag_two(m):
    assert not m.gravity_enabled.all()   # (so that the array is handed over: all ones is passed as NULL)
    m.gravity_enabled[0] = 2


def body_on_a_path_that_is_not_there(m):
    m.body_path[1] = m.npaths


def all_chains_on_one_path(m):
    assert sum(int(p) >= 0 for p in m.body_path) > MAX_CHAIN
    m.body_path[m.body_path >= 0] = 0


def shank_on_the_hip(m):
    assert list(m.parent[1:4]) == [0, 1, 2] and list(m.body_path[1:4]) == [0, 0, 0]
    m.parent[3] = 1


def pair_on_a_path_that_is_not_there(m):
    m.pair_path[0] = m.npaths


def pair_on_another_path(m):
    k, b = chain_pair(m)
    assert all(x < 0 or x == b or int(m.body_path[x]) < 0 for x in bodies_of(m, k))   # (not a shared pair)
    m.pair_path[k] = (int(m.body_path[b]) + 1) % m.npaths


def box_box_the_other_way_round(m):
    k = box_box_pair(m)
    m.pair_a[k], m.pair_b[k] = int(m.pair_b[k]), int(m.pair_a[k])


def pair_of_a_geometry_that_is_not_there(m):
    m.pair_a[0] = m.ngeoms


def common_body_that_is_not_there(m):
    m.common_body = m.nbodies


def common_body_its_own_parent(m):
    assert m.common_body == 0
    m.parent[0] = 0


def geometry_on_a_body_that_is_not_there(m):
    m.geom_body[int(m.pair_a[0])] = m.nbodies


# case -> (fixture, its one edit, idto_hip_create's message)
BAD = {
    "npaths": ("mini_cheetah", not_a_power_of_two, "npaths must be a power of two <= 8"),
    "planar joint": ("hopper", planar_joint_on_a_body, "planar and floating joints must be attached to the world"),
    "gravity flag": ("jaco", gravity_flag_two, "gravity_enabled entries must be 0 or 1"),
    "body path": ("acrobot", body_on_a_path_that_is_not_there, "body without a valid path"),
    "long chain": ("dual_jaco", all_chains_on_one_path, "chain longer than IDTO_MAX_CHAIN"),
    "not a star": ("mini_cheetah", shank_on_the_hip, "model is not a star decomposition"),
    "pair path": ("hopper", pair_on_a_path_that_is_not_there, "pair without a valid path"),
    "pair outside its path": ("mini_cheetah", pair_on_another_path, "pair touches a body outside its path"),
    "box-box": ("mini_cheetah", box_box_the_other_way_round, "box-box contact pairs must be"),
    "pair geometry": ("hopper", pair_of_a_geometry_that_is_not_there, "pair geometry index out of range"),
    "common body": ("acrobot", common_body_that_is_not_there, "common body out of range"),
    "body numbering": ("mini_cheetah", common_body_its_own_parent, "bodies must be numbered so that parent"),
    "geometry body": ("hopper", geometry_on_a_body_that_is_not_there, "geometry body out of range"),
    "geometry body, stem": ("punyo", geometry_on_a_body_that_is_not_there, "geometry body out of range"),
}


def bad_model(key):
    name, edit, _ = BAD[key]
    good, cfg = fixture(name)
    m = Unvalidated(**{f.name: copy.deepcopy(getattr(good, f.name)) for f in fields(good)})
    edit(m)
    return good, cfg, m


@pytest.mark.parametrize("key", sorted(BAD))
def test_bad_models_are_refused(key):
    good, cfg, m = bad_model(key)
    prob, sp, _ = make_problem(cfg, good, num_steps=4)
    with pytest.raises(hip.HipError, match=BAD[key][2]):
        hip.HipPath(m, prob, sp)


@pytest.mark.parametrize("name", BUILT_IN + FIXTURES)
def test_good_models_reach_the_device_check(name):
    good, cfg = fixture(name)
    prob, sp, _ = make_problem(cfg, good, num_steps=4)
    try:
        hip.HipPath(good, prob, sp).close()
    except hip.HipError as e:   # (a box without a GPU)
        assert "no HIP device" in str(e)

