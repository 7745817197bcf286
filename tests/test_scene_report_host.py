"""csrc/scene_report.h on the host, as a whole block: the device text compiled by g++ over tests/cpp/lane_emu (a lane is an OS
thread, __syncthreads a barrier) - no GPU, nothing loaded into Python.

tests/cpp/scene_report_host_check.cc runs scene_block_body on the grid (states, 2 problems) inside exactly the LDS bytes that
the host would request (scene_lds_doubles): everything behind them is poisoned for the address sanitizer, everything inside
starts as NaN.  The bar is == throughout: every body's R, p, w, v against oracle::Dynamics::Kinematics; every pair's phi, n,
Ca, Cb against oracle::SignedDistance and its active flag against phi <= threshold; every active pair's f and moments
against contact_pair (csrc/id_eval.h) on the same two BodyStates - which ties scene_pair, the restatement, to contact_pair
bit for bit -; the per-body sums of those wrenches, in the order of DESIGN.md section 3.2, against
oracle::Dynamics::ContactForces; tau_contact against the ascending sum of tau_pairs.  It runs once under the address and
undefined-behaviour sanitizers and once under the thread sanitizer (a missing barrier is a data race).

The identity tau_contact = ID(pairless model) - ID(model) at (q, v, 0) holds to rounding, not bit for bit: the report
projects each pair's force joint by joint, inverse dynamics projects the bodies' summed wrenches.  The program prints the
largest |difference| / max(1, |tau|_inf) per model; IDENTITY_MEASURED is the largest value it printed over all the cases
below, IDENTITY_TOL 100 times that (the convention of GEOMETRY_TOL in tests/test_contact_regions.py)."""
import functools
import os
import re

import numpy as np
import pytest

import lane_emu as le
import plant_cases as pc
import test_contact_regions as tcr
import test_id_eval_host as tih
from oracle_lib import Oracle
from idto_amd.problem import make_problem

IDENTITY_MEASURED = 2.904e-16   # (mini_cheetah's states of tests/plant_cases.py; the directed states: at most 2.785e-16)
IDENTITY_TOL = 100 * IDENTITY_MEASURED

MODELS = pc.MODELS + ["punyo", "hopper_planar_stem"]
REGIONS = [f"{name}_{role}" for name in tcr.MODELS for role in tcr.ROLES]


@functools.lru_cache(maxsize=None)
def case(label):
    """-> (device model, oracle model, solver parameters, [(q, v)])"""
    if label in REGIONS:
        name, role = label.rsplit("_", 1)
        fix, model, prob, sp = tcr.setup(name, role)
        return model, model, sp, [(np.array(st["q"]), np.array(st["v"])) for st in fix["states"]]
    c = tih.case(label)
    return c["dev"], c["orc"], c["sp"], [(q, v) for q, v, _ in c["states"]]


@functools.lru_cache(maxsize=None)
def active_pairs(label):
    """how many (state, pair) are within the threshold, by the oracle"""
    dev, orc_model, sp, states = case(label)
    if not orc_model.npairs:
        return 0
    orc = _oracle(label)
    return int(sum((orc.signed_distances(q)[0] <= orc.contact_threshold).sum() for q, _ in states))


@functools.lru_cache(maxsize=None)
def _oracle(label):
    dev, orc_model, sp, states = case(label)
    if label in REGIONS:
        name, role = label.rsplit("_", 1)
        return Oracle(orc_model, tcr.setup(name, role)[2], sp)
    if label == "hopper_planar_stem":
        from test_model_stem import hopper_on_a_planar_stem
        cfg = hopper_on_a_planar_stem()[0]
        return Oracle(orc_model, make_problem(cfg, orc_model, num_steps=3)[0], sp)
    return pc.oracle(label)


def write_case(out_dir, label, dump=None):
    dev, orc, sp, states = case(label)
    path = os.path.join(str(out_dir), label + ".case")
    with open(path, "w") as f:
        f.write(f"label {label}\ndev {le.save_model(dev, out_dir, label + '_dev')}\norc {le.save_model(orc, out_dir, label + '_orc')}\n")
        f.write(f"contact {le.fmt(le.contact_values(sp))}\ndump {dump or '-'}\nstates {len(states)}\n")
        for q, v in states:
            f.write(f"{le.fmt(q)}\n{le.fmt(v)}\n")
    return path


def expected_lines(label):
    dev, orc, sp, states = case(label)
    S, nb, npairs, act = len(states), dev.nbodies, dev.npairs, active_pairs(label)
    sums = 2 * S if npairs else 0
    return [f"{label} bodies {2 * S * nb}/{2 * S * nb}", f"{label} pairs {2 * S * npairs}/{2 * S * npairs}",
            f"{label} forces {2 * act}/{2 * act}", f"{label} body_sums {sums}/{sums}", f"{label} tau_sum {2 * S}/{2 * S}"]


def run_and_compare(exe, out_dir, labels):
    """-> {label: the identity's figure}"""
    paths = [write_case(out_dir, label) for label in labels]
    rc, lines, err = le.run(exe, paths)
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    identity = {m.group(1): float(m.group(2)) for m in (re.match(r"(\S+) identity (\S+)$", l) for l in lines) if m}
    assert [l for l in lines[:-1] if " identity " not in l] == [w for label in labels for w in expected_lines(label)]
    assert sorted(identity) == sorted(labels)
    return identity, err


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return le.build("scene_report_host_check", tmp_path_factory.mktemp("scene_report_host"))


def check_identity(identity):
    for label, value in identity.items():
        print(label, "largest |tau_contact - (ID without pairs - ID with pairs)| / max(1, |tau|_inf):", value)
        assert value <= IDENTITY_TOL, (label, value)


def test_models_equal_the_oracle_and_contact_pair(exe, tmp_path):
    """the six models of tests/plant_cases.py, punyo with zero-length capsules against the oracle's spheres (a stem of three
    bodies, shared pairs) and the hopper on a planar stem; the first state of each model with pairs has an active contact"""
    for label in MODELS:
        if case(label)[0].npairs:
            assert active_pairs(label) > 0, label
    identity, _ = run_and_compare(exe, tmp_path, MODELS)
    check_identity(identity)


@pytest.mark.parametrize("role", tcr.ROLES)
def test_directed_contact_states_equal_the_oracle_and_contact_pair(exe, tmp_path, role):
    """the 88 states of tests/golden/contact/regions_*.json - each aimed at one box region or force-law branch - in the stored
    role order and with pair_a and pair_b exchanged"""
    labels = [f"{name}_{role}" for name in tcr.MODELS]
    assert sum(len(case(label)[3]) for label in labels) == 88
    identity, _ = run_and_compare(exe, tmp_path, labels)
    check_identity(identity)


def test_thread_sanitizer_finds_no_race(tmp_path):
    """the same program and cases under the thread sanitizer: the bodies' records, the pairs' rows and the DoF sums are
    separated by __syncthreads() alone; a missing one is a data race of the emulation's threads.  Any report fails."""
    reason = le.tsan_unavailable(tmp_path)
    if reason:
        pytest.skip(reason)
    exe = le.build("scene_report_host_check", tmp_path, le.TSAN)
    labels = MODELS + [f"{name}_stored" for name in tcr.MODELS]
    paths = [write_case(tmp_path, label) for label in labels]
    rc, lines, err = le.run(exe, paths)
    assert le.unexpected_tsan_reports(err) == [] and "ThreadSanitizer" not in err, err[-6000:]
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-3000:]
