"""Directed contact states: every region of a box and every branch of the force law (tests/golden/contact/regions_*.json).

The contact code exists three times - oracle/rigid_body.h (SignedDistance, ContactForces), csrc/id_eval.h, csrc/id_fast.h -
and the seeded trajectories that hold the copies together visit a few of its branches (no edge, no corner,
no negative face, no inside centre leaving through x or y, never the linear force law).  The fixtures here come from
`python tools/make_golden.py contact`: one-state problems aimed at one branch each, every pair labelled from the independent
generator's own arithmetic (Kane's virtual power, numerical Jacobians; tools/golden_examples.py contact_labels) and kept
clear of every branch boundary it is not aimed at by the margins stored in the file.

This file (no GPU): the fixtures cover the REQUIRED labels stated below; the CPU oracle meets their tau at the stored
1e-7 and their (phi, n, Ca, Cb) at GEOMETRY_TOL, in the stored role order and with pair_a and pair_b exchanged; and
tests/contact_census.py, reading the oracle's outputs alone, gives every pair the generator's geometric labels.
tests/test_gpu_contact_regions.py holds the device to the same fixtures and, bit for bit, to the oracle."""
import copy
import functools
import json
import os

import numpy as np
import pytest

import contact_census as cc
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem
from oracle_lib import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ["allegro_hand", "mini_cheetah", "hopper"]
ROLES = ["stored", "exchanged"]
BOX = 1

FACES = ["+x", "-x", "+y", "-y", "+z", "-z"]
EDGES = ["+x+y", "+x-y", "-x+y", "-x-y", "+x+z", "+x-z", "-x+z", "-x-z", "+y+z", "+y-z", "-y+z", "-y-z"]
CORNERS = [a + b + c for a in ("+x", "-x") for b in ("+y", "-y") for c in ("+z", "-z")]
INSIDE = ["in+x", "in-x", "in+y", "in-y", "in+z", "in-z"]
TIES = ["dx==dy", "dy==dz"]
ALLEGRO_LINEAR = ["+x", "-y", "+z", "+x+y", "-x-z", "+y-z", "+x-y+z", "-x+y-z"]
ALLEGRO_AIMS = ["palm exponent just below 37", "palm exponent just above 37", "palm phi just below the threshold",
                "palm phi just above the threshold"]
# the least margins a fixture may have been generated with (tools/golden_examples.py MIN_* / AIM_*): what double
# rounding can move is 1e-16 relative, many orders below each
MARGIN_BOUNDS = dict(clamp=1e-6, axis_gap=1e-6, phi=1e-6, phi_aimed=1e-8, exponent=1e-3, exponent_aimed=1e-6, s=1e-3,
                     vertex_dz=1e-6, centres=0.02)
# |oracle - fixture| of phi, n, Ca, Cb: the largest difference over all states, pairs and both role orders was measured
# as 1.11e-15 m (a few ulp of the cheetah's coordinates; the two sides round the same
# few operations differently); the bar is 100 times that
GEOMETRY_MEASURED = 1.11e-15
GEOMETRY_TOL = 100 * GEOMETRY_MEASURED


@functools.lru_cache(maxsize=None)
def fixture(name):
    """the fixture with a state's pairs as a list over all pairs of the model: a stored pair's omitted labels filled in
    from `pair_defaults` ("-": the label does not apply); a pair that is not stored is FAR - inactive, phi beyond
    threshold + reach, which test_oracle_signed_distances_match_the_generator asks of the oracle"""
    fix = json.load(open(os.path.join(HERE, "golden", "contact", f"regions_{name}.json")))
    assert fix["pair_defaults"] == dict(region="-", tie="-", force="-", dissipation="-", friction="-")
    npairs = load_model(fix["config"]).npairs
    far = dict(fix["pair_defaults"], kind="far", active=False, phi=np.inf)
    for st in fix["states"]:
        assert all(0 <= int(k) < npairs for k in st["pairs"])
        st["pairs"] = [dict(fix["pair_defaults"], **st["pairs"][str(k)]) if str(k) in st["pairs"] else far
                       for k in range(npairs)]
    return fix


def exchanged_roles(model):
    """pair_a and pair_b exchanged for every sphere-sphere and sphere-box pair; box-box keeps its order, because
    host/model_tables.cc BuildPairLists accepts it only as (box on a moving body, world-fixed box).  No shape refuses the
    exchange of the other kinds: GatherFastRecords derives `cia` from the slots of the two bodies."""
    m = copy.deepcopy(model)
    for k in range(m.npairs):
        ga, gb = int(m.pair_a[k]), int(m.pair_b[k])
        if not (int(m.geom_type[ga]) == BOX and int(m.geom_type[gb]) == BOX):
            m.pair_a[k], m.pair_b[k] = gb, ga
    return m.normalize()


@functools.lru_cache(maxsize=None)
def setup(name, role="stored"):
    """(fixture, model with the fixture's geometry edits in the role order, one-step problem, solver parameters)"""
    fix = fixture(name)
    model = copy.deepcopy(load_model(fix["config"]))
    for e in fix["geom_edits"]:
        model.geom_size[e["geom"]] = e["size"]
        model.geom_X[e["geom"]] = e["X_BG"]
    model = model.normalize()
    if role == "exchanged":
        model = exchanged_roles(model)
    prob, sp, _ = make_problem(load_config(fix["config"]), model, num_steps=1)
    for k, val in fix["contact"].items():
        assert getattr(sp, k) == val, "fixture generated with other contact parameters"
    sp.scaling = sp.equality_constraints = False
    return fix, model, prob, sp


def in_role(lab, role):
    """(n, Ca, Cb) of a stored pair as the role order sees them: box-box pairs keep theirs"""
    if role == "stored" or lab["kind"] == "box-box":
        return np.array(lab["n"]), np.array(lab["Ca"]), np.array(lab["Cb"])
    return -np.array(lab["n"]), np.array(lab["Cb"]), np.array(lab["Ca"])


def box_regions(fix, pairs, where=lambda lab: True):
    """regions of the pairs `pairs` over all states where they come within force_phi of the box"""
    return {st["pairs"][k]["region"] for st in fix["states"] for k in pairs
            if st["pairs"][k]["active"] and st["pairs"][k]["phi"] <= fix["force_phi"] and where(st["pairs"][k])}


def test_fixtures_are_small_and_keep_their_margins():
    for name in MODELS:
        path = os.path.join(HERE, "golden", "contact", f"regions_{name}.json")
        assert os.path.getsize(path) < 256 * 1024
        fix = fixture(name)
        assert fix["tolerance_rel"] == 1e-7 and fix["generator"] == "tools/make_golden.py contact"
        assert fix["margins"]["bound"] == MARGIN_BOUNDS
        for key, least in fix["margins"]["least"].items():
            assert least is None or least >= MARGIN_BOUNDS[key], (name, key, least)


def test_allegro_fixture_covers_the_required_labels():
    """palm box (world-fixed, rotated, role A; pair 0) against the ball on the floating common body, and the ball against
    the finger spheres (pairs 1-19)"""
    fix, model, _, _ = setup("allegro_hand")
    palm = [st["pairs"][0] for st in fix["states"]]
    # all 26 outside regions in the softplus branch; three faces, three edges and two corners, with every axis in both
    # signs, also in the linear one
    assert box_regions(fix, [0], lambda lab: lab["force"] == "softplus") >= set(FACES + EDGES + CORNERS)
    assert box_regions(fix, [0], lambda lab: lab["force"] == "linear") >= set(ALLEGRO_LINEAR + INSIDE)
    assert box_regions(fix, [0]) == set(FACES + EDGES + CORNERS + INSIDE)
    assert {lab["tie"] for lab in palm} == {"-"} | set(TIES)
    for tie, axis in zip(TIES, "xy"):   # `<=` resolves a tie towards the earlier axis
        assert {lab["region"][:2] + lab["region"][3:] for lab in palm if lab["tie"] == tie} == {"in" + axis}
    by_aim = {st["aim"]: st["pairs"][0] for st in fix["states"]}
    assert set(ALLEGRO_AIMS) <= set(by_aim)
    sigma = fix["contact"]["smoothing_factor"]
    below, above = by_aim[ALLEGRO_AIMS[0]], by_aim[ALLEGRO_AIMS[1]]
    assert below["force"] == "softplus" and 0 < 37 + below["phi"] / sigma < 1e-4
    assert above["force"] == "linear" and 0 < -above["phi"] / sigma - 37 < 1e-4
    below, above = by_aim[ALLEGRO_AIMS[2]], by_aim[ALLEGRO_AIMS[3]]
    assert below["active"] and 0 < fix["threshold"] - below["phi"] < 1e-6
    assert not above["active"] and 0 < above["phi"] - fix["threshold"] < 1e-6
    assert {lab["dissipation"] for lab in palm} == {"approach", "separate", "zero", "-"}
    assert {lab["friction"] for lab in palm} >= {"none", "stick", "slip"}
    for st in fix["states"]:   # s >= 2: the pair is active and the ball feels nothing from it
        if st["aim"].startswith("palm separating, s >= 2"):
            assert st["pairs"][0]["active"] and st["pairs"][0]["dissipation"] == "zero"
    radius = lambda k: float(model.geom_size[int(model.pair_a[k])][0])
    got = {(radius(k), st["pairs"][k]["force"]) for st in fix["states"] for k in range(1, model.npairs)}
    assert got >= {(r, f) for r in (0.015, 0.012) for f in ("softplus", "linear", "-")}
    assert float(model.geom_size[20][0]) == 0.06


def test_cheetah_fixture_covers_the_required_labels():
    """body box on the floating common body (role A; pairs 0-3 against the four feet), pair 4 the body on the ground,
    pairs 5-8 the feet on the ground"""
    fix = fixture("mini_cheetah")
    got = box_regions(fix, range(4))
    assert got >= set(FACES)
    assert len(got & set(EDGES)) >= 4 and len(got & set(CORNERS)) >= 2
    assert len({r[-1] for r in got & set(INSIDE)}) >= 2
    near = lambda st, k: st["pairs"][k]["phi"] <= fix["force_phi"]
    assert len({k for st in fix["states"] for k in range(4) if near(st, k)}) >= 3           # paths
    assert any(near(st, k) and st["pairs"][5 + k]["phi"] < 0 for st in fix["states"] for k in range(4))
    assert any(st["pairs"][4]["phi"] < 0 and st["pairs"][4]["active"] for st in fix["states"])
    for st in fix["states"]:   # tilted, and turning
        assert abs(st["q"][0]) < np.cos(0.1) and np.abs(st["v"][:3]).max() > 0


def test_hopper_fixture_covers_the_required_labels():
    """the foot spheres (role A) against a small ground box rotated about two axes"""
    fix, model, _, _ = setup("hopper")
    R = np.array(fix["geom_edits"][0]["X_BG"][:9]).reshape(3, 3)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.abs(R).max() < np.cos(0.3)   # no box axis is a world axis
    got = box_regions(fix, [0, 1])
    assert len(got & set(FACES)) >= 2 and len(got & set(EDGES)) >= 2
    assert len(got & set(CORNERS)) >= 1 and len(got & set(INSIDE)) >= 1


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("name", MODELS)
def test_oracle_matches_independent_kane_dynamics(name, role):
    fix, model, prob, sp = setup(name, role)
    orc = Oracle(model, prob, sp)
    worst = 0.0
    for i, st in enumerate(fix["states"]):
        q, v, a = (np.array(st[k]) for k in ("q", "v", "a"))
        want = np.array(st["tau"])
        scale = max(np.abs(want).max(), np.abs(st["tau_contact"]).max())
        err = np.abs(orc.inverse_dynamics(q, v, a) - want).max() / scale
        worst = max(worst, err)
        assert err <= fix["tolerance_rel"], (i, st["aim"], err)
    print(name, role, "worst |tau - golden| / scale", worst)


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("name", MODELS)
def test_oracle_signed_distances_match_the_generator(name, role):
    fix, model, prob, sp = setup(name, role)
    orc = Oracle(model, prob, sp)
    assert abs(orc.contact_threshold - fix["threshold"]) <= 1e-15
    worst = 0.0
    for i, st in enumerate(fix["states"]):
        phi, n, Ca, Cb = orc.signed_distances(np.array(st["q"]))
        for k, lab in enumerate(st["pairs"]):
            if lab["kind"] == "far":
                assert phi[k] > fix["threshold"] + fix["reach"], (i, st["aim"], k, phi[k])
                continue
            assert lab["phi"] <= fix["threshold"] + fix["reach"]
            diffs = [abs(phi[k] - lab["phi"])]
            # (witness points: of every pair with a box, and of the sphere-sphere pair a state is aimed at)
            assert ("n" in lab) == (lab["kind"] != "sphere-sphere" or k == st["aimed_pair"])
            if "n" in lab:
                diffs += [np.abs(x - y).max() for x, y in zip((n[k], Ca[k], Cb[k]), in_role(lab, role))]
            worst = max(worst, max(diffs))
            assert max(diffs) <= GEOMETRY_TOL, (i, st["aim"], k, diffs)
    print(name, role, "worst |oracle - generator| of phi, n, Ca, Cb", worst)


@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("name", MODELS)
def test_census_gives_the_generators_labels(name, role):
    fix, model, prob, sp = setup(name, role)
    orc = Oracle(model, prob, sp)
    for i, st in enumerate(fix["states"]):
        got = cc.classify(model, orc, np.array(st["q"]))
        for k, (mine, lab) in enumerate(zip(got, st["pairs"])):
            for key in ("active", "force") if lab["kind"] == "far" else ("kind", "region", "active", "force"):
                assert mine[key] == lab[key], (i, st["aim"], k, key, mine[key], lab[key])


def test_fixtures_reach_what_the_parity_trajectories_reach_and_more():
    """the census of tests/test_gpu_parity.py's contact cases (DESIGN.md §8.1 records its table): the sphere-box regions
    and force branches those trajectories visit are a strict subset of the fixtures'"""
    import test_gpu_parity as tp
    table = {}
    for case in tp.CASES:
        model, prob, sp, q = tp.setup(*case)
        if model.npairs:
            cc.census(model, Oracle(model, prob, sp), q[1:], table)
    assert sum(table.values()) == sum(model_npairs * N for model_npairs, N in
                                      ((tp.setup(*c)[0].npairs, c[1]) for c in tp.CASES))
    seen = {(key[2], key[4]) for key in table if key[0].startswith("sphere-box") and key[3]}
    mine = {(lab["region"], lab["force"]) for name in MODELS for st in fixture(name)["states"] for lab in st["pairs"]
            if lab["kind"] == "sphere-box" and lab["active"]}
    assert seen < mine, seen - mine
    for row in sorted(table.items(), key=str):
        print(row)
