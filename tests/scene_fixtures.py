"""Shared by tests/test_scene_fixtures.py (the host emulation, no GPU) and tests/test_gpu_scene_report.py (the device): the
independent fixtures of tests/golden/scene (`python tools/make_golden.py scene`: Kane's virtual power and numerical
Jacobians, no code shared with the oracle or the kernels), the models and states they belong to, and how a scene report
is held to them.

A difference is measured per quantity, relative to the largest entry of that quantity in the state (1 where the state's
entries are all zero).  MEASURED is the largest difference that the host emulation of csrc/scene_report.h shows on the CPU
over all six sets (tests/test_scene_fixtures.py prints it); the bar is 100 times that, capped by the generator's own stored bar
of 1e-7 - what its numerical derivatives are good for."""
import functools
import json
import os

import numpy as np

import test_contact_regions as tcr
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "scene")
EXAMPLES = os.path.join(HERE, "golden", "examples")
DIRECTED = ["allegro_hand", "mini_cheetah", "hopper"]
AS_THEY_ARE = ["spinner_capsule", "dual_jaco", "punyo"]
QUANTITIES = ["w", "v", "phi", "n", "Ca", "Cb", "vn", "vt", "fn", "fB", "tau_contact"]
GENERATOR_BAR = 1e-7
# the largest relative difference of the host emulation per quantity, over the six sets
# (the fixtures keep whole doubles: what is left is the generator's numerical derivatives)
MEASURED = dict(w=3.06e-12, v=1.33e-12, phi=1.66e-14, n=1.78e-15, Ca=6.12e-16, Cb=8.65e-16, vn=2.12e-11, vt=5.88e-12,
                fn=1.11e-11, fB=1.12e-11, tau_contact=1.12e-11)
BARS = {k: min(100 * val, GENERATOR_BAR) for k, val in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def fixture(label):
    """the set's index (<label>.json) with its numbers (<label>.f64: little-endian float64, state after state - per body w, v;
    per stored pair the entries of the index's "pair"; tau_contact) put back into the states: bodies [{w, v}], pairs {index:
    {active, phi, n, ...}}, tau_contact"""
    path = os.path.join(SCENE, label)
    fix = json.load(open(path + ".json"))
    flat = np.fromfile(path + ".f64", dtype="<f8")
    for ext in (".json", ".f64"):
        assert os.path.getsize(path + ext) <= 115064, path + ext   # (the largest fixture of tests/golden/contact)
    assert fix["tolerance_rel"] == GENERATOR_BAR and fix["generator"] == "tools/make_golden.py scene"
    assert fix["body"] == [["w", 3], ["v", 3]] and [k for k, _ in fix["pair"]] == QUANTITIES[2:10] and flat.size == fix["doubles"]
    assert [st["state"] for st in fix["states"]] == list(range(len(fix["states"])))
    at = 0

    def take(n):
        nonlocal at
        at += n
        return flat[at - n:at]

    for st in fix["states"]:
        st["bodies"] = [dict(w=take(3), v=take(3)) for _ in range(fix["nbodies"])]
        labs = {}
        for k, active in zip(st["pairs"], st["active"]):
            labs[str(k)] = dict(active=active, **{key: (take(n) if n > 1 else float(take(1)[0])) for key, n in fix["pair"]})
        st["pairs"], st["tau_contact"] = labs, take(fix["nv"])
    assert at == flat.size
    return fix


@functools.lru_cache(maxsize=None)
def case(label, role="stored"):
    """-> (model, problem, solver parameters, x [S, nq + nv], which pairs keep their order under the exchanged role)"""
    if label.startswith("regions_"):
        fix, model, prob, sp = tcr.setup(label[len("regions_"):], role)
        states = fix["states"]
        keeps = [int(model.geom_type[int(a)]) == tcr.BOX and int(model.geom_type[int(b)]) == tcr.BOX
                 for a, b in zip(model.pair_a, model.pair_b)]
    else:
        assert role == "stored"
        kane = json.load(open(os.path.join(EXAMPLES, f"kane_{label}.json")))
        model = load_model(os.path.join(EXAMPLES, label + ".model"))
        prob, sp, _ = make_problem(load_config(os.path.join(EXAMPLES, label + ".yaml")), model, num_steps=1)
        for k, val in kane["contact"].items():
            assert getattr(sp, k) == val, "fixture generated with other contact parameters"
        states, keeps = kane["states"], [True] * model.npairs
    x = np.array([np.concatenate([st["q"], st["v"]]) for st in states])
    assert len(x) == len(fixture(label)["states"])
    return model, prob, sp, x, keeps


def _rel(got, want):
    want = np.asarray(want, dtype=float)
    scale = np.abs(want).max() if want.size and np.abs(want).max() > 0 else 1.0
    return float(np.abs(np.asarray(got, dtype=float) - want).max() / scale) if want.size else 0.0


def differences(label, bodies, pairs, tau_contact, role="stored"):
    """bodies [S, nb, 18], pairs [S, npairs, 20], tau_contact [S, nv] of a report at case(label, role)'s states -> {quantity:
    the largest relative difference from the fixture}; asserts the active flags and that a pair the fixture does not store
    is inactive.  Exchanged role: a pair that changed its order has n, vt and the force negated and Ca, Cb exchanged."""
    fix, keeps = fixture(label), case(label, role)[4]
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for i, st in enumerate(fix["states"]):
        got = dict(w=bodies[i][:, 12:15], v=bodies[i][:, 15:18], tau_contact=tau_contact[i])
        want = dict(w=[b["w"] for b in st["bodies"]], v=[b["v"] for b in st["bodies"]], tau_contact=st["tau_contact"])
        stored = sorted(int(k) for k in st["pairs"])
        for k in range(pairs.shape[1]):
            if k not in stored:
                assert pairs[i, k, 0] == 0.0 and pairs[i, k, 1] > fix["threshold"] + fix["reach"], (label, i, k)
        flip = np.array([1.0 if (role == "stored" or keeps[k]) else -1.0 for k in stored])[:, None]
        rec = pairs[i][stored] if stored else np.zeros((0, 20))
        labs = [st["pairs"][str(k)] for k in stored]
        assert [bool(r[0]) for r in rec] == [lab["active"] for lab in labs], (label, i)
        a_side, b_side = rec[:, 5:8], rec[:, 8:11]
        swap = (flip < 0)
        got.update(phi=rec[:, 1], n=rec[:, 2:5] * flip, Ca=np.where(swap, b_side, a_side), Cb=np.where(swap, a_side, b_side),
                   vn=rec[:, 11], vt=rec[:, 12:15] * flip, fn=rec[:, 15], fB=rec[:, 16:19] * flip)
        for key in ("phi", "n", "Ca", "Cb", "vn", "vt", "fn", "fB"):
            want[key] = [lab[key] for lab in labs]
        for key in QUANTITIES:
            worst[key] = max(worst[key], _rel(got[key], want[key]))
    return worst
