"""csrc/id_eval.h on the host: the device text, unmodified, compiled by g++ over tests/cpp/lane_emu (a lane is an OS
thread, an exchange point a barrier) and held to oracle::Dynamics::InverseDynamics with == - no GPU.

tests/cpp/id_eval_host_check.cc is built here with the address and undefined-behaviour sanitizers (an access beyond the
emulated LDS traps, LDS that nobody wrote reads as NaN) and once more with the thread sanitizer (a missing exchange point is
a data race).  It says whether the C++ TEXT of the generic evaluation is right - indexing, association order, the
exchange area's protocol -; the device compiler, the registers and the launch are below it (lane_emu/hip/hip_runtime.h).

Every instantiation that exists runs: <2>, <3>, <4>, <8>, <8, true> (shared pairs), <8, true, true> (a stem), chosen per
model as fd_launch.hip and plant_launch.hip choose.  Per state `full` and all nv mass-matrix columns in both input layouts
(fd_body's rows, the plant's ramp window), and per group of lanes full -> column -> full on one exchange area that starts as
NaN and is never cleared, several groups side by side in one wavefront.  The program prints a line per (model,
instantiation, mode) with equal/compared; the tests assert the whole set of lines, so that nothing is skipped silently.
"""
import functools
import json
import os

import numpy as np
import pytest

import lane_emu as le
import plant_cases as pc
import test_contact_regions as tcr
from idto_amd.model import load_model
from idto_amd.problem import SolverParameters, load_config, make_problem
from oracle_lib import Oracle
from test_gpu_capsule import TWO_DOF_CFG
from test_model_stem import (all_gravity, as_spheres, hopper_on_a_planar_stem, jaco_chain_and_stems, punyo,
                             synthetic_stem_model, zero_length)

EXAMPLES = pc.EXAMPLES
# the instantiation each model takes (the program prints the one it dispatched to; a change here is a change of dispatch)
INST = {"acrobot": "2", "pendulum": "2", "hopper": "3", "hopper_no_ground": "3", "spinner": "3", "spinner_sphere": "3",
        "free_body": "2", "mini_cheetah": "3", "allegro_hand": "4", "jaco": "8", "jaco_ball": "8", "dual_jaco": "8x",
        "spinner_capsule": "3", "2dof_spinner_capsule": "2", "punyo": "8xs", "synthetic_stem": "8xs", "jaco_stem2": "8xs",
        "jaco_stem3": "8xs", "hopper_planar_stem": "8xs"}
SHIPPED = ["acrobot", "pendulum", "hopper", "hopper_no_ground", "spinner", "spinner_sphere", "free_body", "mini_cheetah",
           "allegro_hand"]
FIXTURES = ["jaco", "jaco_ball", "dual_jaco", "spinner_capsule", "2dof_spinner_capsule", "punyo"]
NO_SPHERE_CONTACT = {"2dof_spinner_capsule"}   # (its contact state: test_fixtures_as_they_are_meet_the_independent_goldens)
CONFIG_OF = {"hopper_no_ground": "hopper", "spinner_sphere": "spinner"}   # (a model without a configuration of its own)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return le.build("id_eval_host_check", tmp_path_factory.mktemp("id_eval_host"))


def _normalized(model, q):
    return pc._normalized(model, q)


def _scan_states(label, orc_model, cfg, sp):
    """plant_cases.states' rule for a model that plant_cases has no case of: the first state has an active contact where
    the model has pairs (asserted), the others are offsets of 0.1 from q_init; v within +-0.5, a within +-2"""
    rng = np.random.default_rng(7100 + len(label))
    q_init = np.asarray(cfg["q_init"], dtype=float) if cfg else np.zeros(orc_model.nq)
    if not cfg:
        q_init[[int(orc_model.qstart[b]) for b in range(orc_model.nbodies) if int(orc_model.jtype[b]) == pc.FLOATING]] = 1.0
    out = []
    if orc_model.npairs:
        prob = make_problem(cfg, orc_model, num_steps=3)[0]
        orc = Oracle(orc_model, prob, sp)
        for t in range(4000):
            amp = (0.05, 0.2, 0.6, 1.2)[t % 4]
            q = _normalized(orc_model, q_init + rng.uniform(-amp, amp, orc_model.nq))
            if -0.03 < orc.signed_distances(q)[0].min() < 0.0:
                out.append(q)
                break
        # (the two spheres at the capsules' centres stay 0.4 m apart at every q: that model's contact runs as it is, below)
        assert bool(out) == (label not in NO_SPHERE_CONTACT), label + ": the scan found no state with an active contact"
    while len(out) < 3:
        out.append(_normalized(orc_model, q_init + rng.uniform(-0.1, 0.1, orc_model.nq)))
    return [(q, rng.uniform(-0.5, 0.5, orc_model.nv), rng.uniform(-2.0, 2.0, orc_model.nv)) for q in out]


@functools.lru_cache(maxsize=None)
def case(label):
    """-> dict(dev, orc, chain, sp, states): the models, the solver parameters (for the contact law) and [(q, v, a)]"""
    chain = None
    if label in pc.MODELS or label == "punyo":
        dev, orc, cfg = pc.case(label)
        sp = pc.problem(label)[1]
        states = pc.states(label)   # (its third vector, an applied torque there, is the acceleration here)
        if orc.npairs:
            assert pc.oracle(label).signed_distances(states[0][0])[0].min() < 0.0
        return dict(dev=dev, orc=orc, chain=None, sp=sp, states=states)
    if label in SHIPPED:
        dev = orc = load_model(label)
        cfg_name = CONFIG_OF.get(label, label)
        cfg = load_config(cfg_name) if os.path.exists(os.path.join(pc.ROOT, "idto_amd", "configs", cfg_name + ".yaml")) else None
    elif label in FIXTURES:   # as plant_cases.case builds punyo: every weight on, zero-length capsules / spheres
        model = load_model(os.path.join(EXAMPLES, label + ".model"))
        path = os.path.join(EXAMPLES, label + ".yaml")
        cfg = load_config(path) if os.path.exists(path) else TWO_DOF_CFG
        dev, orc = zero_length(all_gravity(model)), as_spheres(all_gravity(model))
    elif label == "synthetic_stem":
        dev = orc = synthetic_stem_model()
        cfg = punyo()[1]
    elif label in ("jaco_stem2", "jaco_stem3"):
        cfg, chain, stems = jaco_chain_and_stems()
        dev = orc = stems[int(label[-1])]
    else:
        assert label == "hopper_planar_stem"
        cfg, chain, dev = hopper_on_a_planar_stem()
        orc = dev
    sp = make_problem(cfg, orc, num_steps=3)[1] if cfg else SolverParameters(verbose=False)
    return dict(dev=dev, orc=orc, chain=chain, sp=sp, states=_scan_states(label, orc, cfg, sp))


def write_case(out_dir, label, dev, orc, chain, sp, states, golden=None):
    dev_path = le.save_model(dev, out_dir, label + "_dev")
    orc_path = le.save_model(orc, out_dir, label + "_orc") if orc is not None else "-"
    chain_path = le.save_model(chain, out_dir, label + "_chain") if chain is not None else "-"
    path = os.path.join(str(out_dir), label + ".case")
    with open(path, "w") as f:
        f.write(f"label {label}\ndev {dev_path}\norc {orc_path}\nchain {chain_path}\ncontact {le.fmt(le.contact_values(sp))}\n")
        f.write(f"golden {int(golden is not None)}\nstates {len(states)}\n")
        for k, (q, v, a) in enumerate(states):
            f.write(f"{le.fmt(q)}\n{le.fmt(v)}\n{le.fmt(a)}\n")
            if golden is not None:
                f.write(f"{le.fmt(golden[k][0])}\n{le.fmt([golden[k][1]])}\n")
    return path


def groups(model):
    return max(2, min(64 // model.npaths, 8))


def lines_of(label, inst, model, S, suffix=""):
    nv, G = model.nv, groups(model)
    return [f"{label} {inst} full{suffix} {S}/{S}", f"{label} {inst} columns_fd{suffix} {S * nv}/{S * nv}",
            f"{label} {inst} columns_plant{suffix} {S * nv}/{S * nv}", f"{label} {inst} sequence{suffix} {G}/{G}"]


def expected_lines(label, c, inst=None):
    inst = inst or INST[label]
    S = len(c["states"])
    want = lines_of(label, inst, c["dev"], S) if c["orc"] is not None else []
    if c["chain"] is not None:
        # (the arm as one chain beside the box: two chains off the world whose pairs are shared pairs - <8, true>, not <8>)
        chain_inst = {"jaco_stem2": "8x", "jaco_stem3": "8x", "hopper_planar_stem": "3"}[label]
        want += lines_of(label, inst, c["dev"], S, "==chain" + chain_inst)
    return want


def check(exe, out_dir, labels, cases=None):
    paths, want = [], []
    for label in labels:
        c = cases[label] if cases else case(label)
        paths.append(write_case(out_dir, label, c["dev"], c["orc"], c["chain"], c["sp"], c["states"], c.get("golden")))
        want += c["lines"] if "lines" in c else expected_lines(label, c)
    rc, lines, err = le.run(exe, paths)
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    assert lines[:-1] == want
    return err


# ---- the cases, by group
def test_shipped_models_equal_the_oracle(exe, tmp_path):
    """all nine of idto_amd/models: <2>, <3>, <3> with a common body, <4>"""
    check(exe, tmp_path, SHIPPED)


def test_example_fixtures_equal_the_oracle(exe, tmp_path):
    """the six example fixtures as plant_cases.case builds them (every weight on; zero-length capsules on the device, spheres
    in the oracle): <8>, <8, true>, <8, true, true> among them"""
    check(exe, tmp_path, FIXTURES)


def test_stems_equal_the_oracle_and_their_chain_forms(exe, tmp_path):
    """a stem of IDTO_MAX_STEM with pairs on a stem body; the jaco arm as a stem of 2 and of 3 == the arm as one chain beside
    the box through <8, true>; the hopper on a planar stem == the hopper through <3>"""
    check(exe, tmp_path, ["synthetic_stem", "jaco_stem2", "jaco_stem3", "hopper_planar_stem"])


def as_they_are(name):
    """an example fixture as it is - the per-body gravity switch, capsules with length, which the oracle's one gravity
    vector and spheres cannot express - with the states and tau of tests/golden/examples/kane_<name>.json"""
    fix = json.load(open(os.path.join(EXAMPLES, f"kane_{name}.json")))
    assert fix["tolerance_rel"] == 1e-7
    model = load_model(os.path.join(EXAMPLES, name + ".model"))
    path = os.path.join(EXAMPLES, name + ".yaml")
    sp = make_problem(load_config(path) if os.path.exists(path) else TWO_DOF_CFG, model, num_steps=1)[1]
    for k, val in fix["contact"].items():
        assert getattr(sp, k) == val, "fixture generated with other contact parameters"
    states = [tuple(np.array(st[k]) for k in ("q", "v", "a")) for st in fix["states"]]
    golden = [(np.array(st["tau"]), max(np.abs(st["tau"]).max(), np.abs(st["tau_contact"]).max())) for st in fix["states"]]
    label = name + "_as_it_is"
    return label, dict(dev=model, orc=None, chain=None, sp=sp, states=states, golden=golden,
                       lines=[f"{label} {INST[name]} golden {len(states)}/{len(states)}"])


def test_fixtures_as_they_are_meet_the_independent_goldens(exe, tmp_path):
    """the project's 1e-7 of the scale max(|tau|, |tau_contact|), as tests/test_golden_examples.py holds the oracle's
    composition and the device to the same files"""
    cases = dict(as_they_are(name) for name in FIXTURES)
    err = check(exe, tmp_path, list(cases), cases)
    print(err)


@pytest.mark.parametrize("role", tcr.ROLES)
def test_directed_contact_states_equal_the_oracle(exe, tmp_path, role):
    """every state of tests/golden/contact/regions_*.json - 88, each aimed at one box region or force-law branch - in the
    stored role order and with pair_a and pair_b exchanged"""
    cases, total = {}, 0
    for name in tcr.MODELS:
        fix, model, prob, sp = tcr.setup(name, role)
        states = [tuple(np.array(st[k]) for k in ("q", "v", "a")) for st in fix["states"]]
        total += len(states)
        label = f"{name}_{role}"
        c = dict(dev=model, orc=model, chain=None, sp=sp, states=states)
        c["lines"] = expected_lines(label, c, INST[name])
        cases[label] = c
    assert total == 88
    check(exe, tmp_path, list(cases), cases)


# ---- the thread sanitizer: the same program, the same cases
def test_thread_sanitizer_finds_no_race(tmp_path):
    """a missing wave_exchange_point() in id_eval.h is two lanes on one double of the exchange area with no barrier between
    them: a data race of the emulation's threads.  Any report fails."""
    reason = le.tsan_unavailable(tmp_path)
    if reason:
        pytest.skip(reason)
    exe = le.build("id_eval_host_check", tmp_path, le.TSAN)
    labels = SHIPPED + FIXTURES + ["synthetic_stem", "jaco_stem2", "jaco_stem3", "hopper_planar_stem"]
    paths = []
    for label in labels:
        c = case(label)
        paths.append(write_case(tmp_path, label, c["dev"], c["orc"], c["chain"], c["sp"], c["states"]))
    for name in tcr.MODELS:   # (the exchanged order takes the same exchange points)
        fix, model, prob, sp = tcr.setup(name, "stored")
        states = [tuple(np.array(st[k]) for k in ("q", "v", "a")) for st in fix["states"]]
        paths.append(write_case(tmp_path, name + "_stored", model, model, None, sp, states))
    rc, lines, err = le.run(exe, paths)
    assert le.unexpected_tsan_reports(err) == [] and "ThreadSanitizer" not in err, err[-6000:]
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-3000:]
