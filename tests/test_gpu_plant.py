"""Plants on the device (include/idto_hip.h idto_hip_forward_dynamics, idto_hip_plant_*; csrc/plant.h, csrc/plant_step.h).

The bar is == throughout.  The kernel's evaluations are id_eval's, bit-exact against the oracle;
what it does with them is csrc/plant_step.h, the text that libidto_opt.so exports for the host: so the mass matrix and
the bias equal the oracle's, and the acceleration and every state of a rollout equal the host restatement (oracle physics
plus the exported header functions, step by step).  Neither side contracts a * b + c, and the device's division and
square root are IEEE (tests/test_gpu_kats.py).  The contexts have N = 3; the shapes are the smallest that take every path:
one plant and three, one substep and several, a block that holds a substep's evaluations and one that runs them in rounds.
No test provokes a device fault; the failed-pivot path is covered on the CPU (tests/cpp/plant_step_check.cc).
"""
import copy
import ctypes as C

import numpy as np
import pytest

import plant_cases as pc
from idto_amd import hip
from idto_amd.model import load_model
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

H = 1e-3


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def _context(name, B, model=None, sp=None):
    dev_model = model if model is not None else pc.case(name)[0]
    prob, sp0 = pc.problem(name, model=None)
    return hip.HipPath(dev_model, [prob] * B if B > 1 else prob, sp if sp is not None else sp0)


def _inputs(name, B):
    st = pc.states(name)[:B]
    return (np.array([np.concatenate([q, v]) for q, v, _ in st]), np.array([t for _, _, t in st]))


def _evidence(name, M, bias, refs):
    """what a failing run leaves behind, gathered before anything is asserted: per plant the columns of the mass matrix that
    differ from the oracle's with the largest difference in each, and whether the bias differs -> (the text, nothing differs)"""
    lines, clean = [], True
    for b, (_, M_ref, c_ref) in enumerate(refs):
        cols = {j: float(np.abs(M[b][:, j] - M_ref[:, j]).max()) for j in range(M_ref.shape[1]) if not _same(M[b][:, j], M_ref[:, j])}
        lines.append(f"{name} plant {b}: bias {'differs by %.3e' % np.abs(bias[b] - c_ref).max() if not _same(bias[b], c_ref) else 'equal'}; "
                     f"columns that differ: {', '.join('%d (%.3e)' % kv for kv in cols.items()) or 'none'}")
        clean = clean and not cols and _same(bias[b], c_ref)
    return "\n".join(lines), clean


# ---- forward dynamics: every instantiation (MAXC 2, 3, 3 with a common body, 4; generic 8; XCH; punyo: XCH with a stem, in a
# block of 128 threads and 73,880 B of LDS)
@pytest.mark.parametrize("name", ["acrobot", "hopper", "mini_cheetah", "allegro_hand", "jaco_ball", "dual_jaco", "punyo"])
def test_forward_dynamics_equals_the_oracle(name):
    orc, nq = pc.oracle(name), pc.case(name)[1].nq
    x, tau = _inputs(name, 3)
    dev = _context(name, 3)
    a, M, bias = dev.forward_dynamics(x, tau)
    dev.close()
    refs = [pc.host_fd(orc, x[b, :nq], x[b, nq:], tau[b]) for b in range(3)]
    evidence, clean = _evidence(name, M, bias, refs)
    print(evidence)
    assert clean, evidence
    for b in range(3):
        a_ref, M_ref, c_ref = refs[b]
        assert _same(M[b], M_ref), (name, b, np.abs(M[b] - M_ref).max())
        assert _same(bias[b], c_ref), (name, b, np.abs(bias[b] - c_ref).max())
        assert _same(a[b], a_ref), (name, b, np.abs(a[b] - a_ref).max())
        assert _same(a[b], pc.solve_host(M[b], tau[b], bias[b])[0])


# ---- hold-mode rollouts.  mini_cheetah in a block of 64: (nv + 1) * npaths = 76 lanes, the evaluations go in two rounds
# allegro_hand (MAXC 4), jaco_ball (the generic MAXC 8, which spills vector registers to scratch) and dual_jaco (XCH): every
# instantiation takes several substeps, from the contact state among others
@pytest.mark.parametrize("name,B,S,block", [("hopper", 1, 1, 0), ("hopper", 3, 2, 0), ("mini_cheetah", 3, 5, 0),
                                            ("mini_cheetah", 1, 2, 64), ("acrobot", 3, 5, 0), ("allegro_hand", 3, 3, 0),
                                            ("jaco_ball", 3, 3, 0), ("dual_jaco", 3, 3, 0), ("jaco_ball", 1, 2, 64),
                                            ("punyo", 3, 3, 0)])
def test_hold_rollout_equals_the_host_restatement(name, B, S, block):
    orc, model = pc.oracle(name), pc.case(name)[1]
    nq = model.nq
    x, tau = _inputs(name, B)
    t0 = 0.25 + 0.5 * np.arange(B)
    dev = _context(name, B)
    dev.plant_begin(H, block_threads=block)
    dev.plant_set_state(t0, x)
    rec, status = dev.plant_step(S, tau, record_every=1)
    times, x_end = dev.plant_get_state()
    dev.close()
    assert status.tolist() == [[0, S]] * B
    for b in range(B):
        ref = pc.host_rollout(orc, model, H, x[b, :nq], x[b, nq:], tau[b], S)
        assert _same(rec[b], ref), (name, b, np.abs(rec[b] - ref).max())
        assert _same(x_end[b], ref[-1])
        assert times[b] == t0[b] + S * H
    if B > 1 and name in ("hopper", "mini_cheetah"):   # plant b of the batch == a one-plant context with the same inputs
        for b in range(B):
            solo = _context(name, 1)
            solo.plant_begin(H)
            solo.plant_set_state(t0[b:b + 1], x[b:b + 1])
            rec1, st1 = solo.plant_step(S, tau[b:b + 1], record_every=1)
            solo.close()
            assert _same(rec1[0], rec[b]) and st1.tolist() == [[0, S]]


# ---- above 64 KiB of dynamic LDS: dual_jaco's exchange areas in a block of 128 (65,920 B) and of 256 threads (115,072 B) - its
# default block of 64 asks for 41,344 B.  Such a launch needs the kernel's opt-in (plant_launch.hip plant_set_max_lds)
@pytest.mark.parametrize("block", [128, 256])
def test_blocks_above_64_kib_of_lds_equal_the_oracle_and_the_host_restatement(block):
    name, B, S = "dual_jaco", 3, 3
    orc, model = pc.oracle(name), pc.case(name)[1]
    nq = model.nq
    x, tau = _inputs(name, B)
    t0 = 0.25 + 0.5 * np.arange(B)
    dev = _context(name, B)
    dev.plant_begin(H, block_threads=block)
    a, M, bias = dev.forward_dynamics(x, tau)
    dev.plant_set_state(t0, x)
    rec, status = dev.plant_step(S, tau, record_every=1)
    times, x_end = dev.plant_get_state()
    dev.close()
    refs = [pc.host_fd(orc, x[b, :nq], x[b, nq:], tau[b]) for b in range(B)]
    evidence, clean = _evidence(name, M, bias, refs)
    print(evidence)
    assert clean, evidence
    assert status.tolist() == [[0, S]] * B
    for b in range(B):
        a_ref, M_ref, c_ref = refs[b]
        assert _same(M[b], M_ref) and _same(bias[b], c_ref) and _same(a[b], a_ref), evidence
        ref = pc.host_rollout(orc, model, H, x[b, :nq], x[b, nq:], tau[b], S)
        assert _same(rec[b], ref), (block, b, np.abs(rec[b] - ref).max())
        assert _same(x_end[b], ref[-1]) and times[b] == t0[b] + S * H


def test_record_every_and_enqueue_only():
    """record_every = 2 of 5 substeps: the states behind substeps 2 and 4; a step without outputs is enqueued only and the
    next call's state is the one it left"""
    name, S = "hopper", 5
    x, tau = _inputs(name, 3)
    dev = _context(name, 3)
    dev.plant_begin(H)
    dev.plant_set_state(0.0, x)
    every, _ = dev.plant_step(S, tau, record_every=1)
    dev.plant_set_state(0.0, x)
    some, _ = dev.plant_step(S, tau, record_every=2)
    assert some.shape[1] == 2 and _same(some, every[:, [1, 3]])
    dev.plant_set_state(0.0, x)
    assert dev.plant_step(2, tau, status=False) == (None, None)
    rec, _ = dev.plant_step(3, tau, record_every=3)
    dev.close()
    assert _same(rec[:, 0], every[:, 4])


# ---- per-plant physics
def _hopper_variants():
    base = load_model("hopper")
    prob, sp = pc.problem("hopper")
    out = []
    for b, (m_scale, k_scale, mu) in enumerate([(1.0, 1.0, None), (1.3, 0.5, 0.2), (0.7, 2.0, 1.1)]):
        m, p = copy.deepcopy(base), copy.deepcopy(sp)
        m.mass = np.asarray(m.mass) * m_scale
        m.inertia = np.asarray(m.inertia) * m_scale
        p.contact_stiffness *= k_scale
        if mu is not None:
            p.friction_coefficient = mu
        out.append((m.normalize(), p))
    return prob, out


def test_plants_with_models_of_their_own():
    """three hoppers with different masses, stiffness and friction in the contact state: plant b == a context created with
    model b, and == the host restatement with an oracle of model b; the controller's context keeps its model"""
    prob, variants = _hopper_variants()
    S, nq = 3, variants[0][0].nq
    q, v, tau = pc.states("hopper")[0]
    x = np.tile(np.concatenate([q, v]), (3, 1))
    taus = np.tile(tau, (3, 1))
    dev = hip.HipPath(variants[0][0], [prob] * 3, variants[0][1])
    dev.plant_begin(H)
    for b in (1, 2):
        dev.plant_set_model(b, variants[b][0], variants[b][1])
    dev.plant_set_state(0.0, x)
    rec, status = dev.plant_step(S, taus, record_every=1)
    a, _, _ = dev.forward_dynamics(x, taus)
    assert status.tolist() == [[0, S]] * 3
    assert not _same(rec[1], rec[0]) and not _same(rec[2], rec[0])
    for b in range(3):
        solo = hip.HipPath(variants[b][0], prob, variants[b][1])
        solo.plant_begin(H)
        solo.plant_set_state(0.0, x[:1])
        rec1, _ = solo.plant_step(S, taus[:1], record_every=1)
        solo.close()
        assert _same(rec1[0], rec[b]), b
        orc = Oracle(variants[b][0], prob, variants[b][1])
        assert _same(rec[b], pc.host_rollout(orc, variants[b][0], H, q, v, tau, S)), b
        assert _same(a[b], pc.host_fd(orc, q, v, tau)[0]), b
    # a topology difference is refused with the text of a batch's models
    other = copy.deepcopy(variants[0][0])
    other.jtype = np.asarray(other.jtype).copy()
    other.jtype[-1] = 1 - int(other.jtype[-1])   # revolute <-> prismatic
    with pytest.raises(hip.HipError, match="model of problem 1 differs from the batch's model in"):
        dev.plant_set_model(1, other.normalize(), variants[1][1])
    dev.close()


# ---- status and refusals
def test_a_nan_torque_stops_its_plant_only():
    name, S = "hopper", 3
    x, tau = _inputs(name, 3)
    bad = tau.copy()
    bad[1, 2] = np.nan
    dev = _context(name, 3)
    dev.plant_begin(H)
    dev.plant_set_state(1.0, x)
    rec, status = dev.plant_step(S, bad, record_every=1)
    times, x_end = dev.plant_get_state()
    assert status.tolist() == [[0, S], [2, 0], [0, S]]
    assert _same(x_end[1], x[1]) and times[1] == 1.0
    dev.close()
    for b in (0, 2):
        solo = _context(name, 1)
        solo.plant_begin(H)
        solo.plant_set_state(1.0, x[b:b + 1])
        rec1, _ = solo.plant_step(S, tau[b:b + 1], record_every=1)
        solo.close()
        assert _same(rec1[0], rec[b]) and _same(x_end[b], rec1[0, -1])


def test_refusals_by_name():
    name = "hopper"
    x, tau = _inputs(name, 3)
    dev = _context(name, 3)
    nq, nv = dev.nq, dev.nv
    with pytest.raises(hip.HipError, match="plant_step: call idto_hip_plant_begin"):
        dev.plant_step(1, tau)
    with pytest.raises(hip.HipError, match="plant_set_state: call idto_hip_plant_begin"):
        dev.plant_set_state(0.0, x)
    with pytest.raises(hip.HipError, match="the substep h must be > 0"):
        dev.plant_begin(0.0)
    with pytest.raises(hip.HipError, match="the substep h must be > 0"):
        dev.plant_begin(-1e-3)
    with pytest.raises(hip.HipError, match="mode is IDTO_PLANT_HOLD or IDTO_PLANT_PD_PLUS"):
        dev.plant_begin(H, mode=7)
    with pytest.raises(hip.HipError, match="block_threads is 0, 64, 128, 192 or 256"):
        dev.plant_begin(H, block_threads=96)
    with pytest.raises(hip.HipError, match="PD\\+ needs the stored plans: call idto_hip_mpc_batch_begin"):
        dev.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=np.zeros((1, nq)), Kd=np.zeros((1, nv)))
    dev.mpc_batch_begin(np.zeros(nq, dtype=np.int32), [3, 4])
    with pytest.raises(hip.HipError, match="gains of the wrong size"):
        dev.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=np.zeros((2, nq)), Kd=np.zeros((1, nv)))
    with pytest.raises(hip.HipError, match="a gain in Kp is not finite"):
        dev.plant_begin(H, mode=hip.PLANT_PD_PLUS, Kp=np.full((2, nq), np.inf), Kd=np.zeros((2, nv)))
    dev.plant_begin(H, record_capacity=2)
    with pytest.raises(hip.HipError, match="substeps must be in \\[1, 4096\\]"):
        dev.plant_step(4097, tau)
    with pytest.raises(hip.HipError, match="substeps must be in \\[1, 4096\\]"):
        dev.plant_step(0, tau)
    with pytest.raises(hip.HipError, match="hold mode needs tau_hold"):
        dev.plant_step(1, None)
    with pytest.raises(hip.HipError, match="more recorded states than idto_hip_plant_begin's record_capacity"):
        dev.plant_step(3, tau, record_every=1)
    with pytest.raises(hip.HipError, match="plant index outside the batch"):
        dev.plant_set_model(3)
    dev.close()


def test_a_context_with_child_contexts_is_refused():
    """the child-context route of the constrained batch loop (option con_kkt = 0) makes a context per problem: no plants there"""
    name = "hopper"
    model, _, cfg = pc.case(name)
    from idto_amd.problem import synthetic_trajectory
    dev = _context(name, 3)
    dev.set_q_batch(np.array([synthetic_trajectory(cfg, model, 3, seed=b) for b in range(3)]))
    dev.set_option("con_kkt", 0)
    try:
        dev.tr_solve_batch_constrained(1, 2, True, False, 0.1, 1e5, [0])
    except hip.FactorizationFailed:
        pass
    with pytest.raises(hip.HipError, match="plant_begin: this context has child contexts"):
        dev.plant_begin(H)
    dev.close()


# ---- a context that never begins a plant
OPTIONS = ["reference_solver", "two_sided", "fused", "async_uploads", "nd_min_rows", "nd_recursion", "solver_nd", "solver_pipe",
           "solver_band", "gn_small", "asm_in_solver", "asm_fold", "con_kkt", "kkt_fold", "ls_waves", "tr_small", "tr_fold",
           "kkt_in_asm", "decide_in_solver", "fd_fast", "gradients_method", "last_solver", "last_assembly", "weights_diagonal",
           "solver_timeouts", "ls_solves", "ls_batch_solves", "tr_resident_ok"]


def _gn_step_traced(dev, q):
    L = hip.lib()
    L.idto_hip_trace_dump.argtypes = [C.c_char_p, C.c_int]
    dev.set_q(q)
    L.idto_hip_trace_enable(1)
    try:
        dev.gn_step()
        out = {k: dev.get(k) for k in ("tau", "gradient", "step")}
    finally:
        buf = C.create_string_buffer(1 << 16)
        L.idto_hip_trace_dump(buf, len(buf))
        L.idto_hip_trace_enable(0)
    labels = [line.split(" ", 1)[1] for line in buf.value.decode().splitlines()]
    return out, labels, {k: dev.get_option(k) for k in OPTIONS}


def test_a_context_without_plants_is_what_it_was():
    """the options and a gn_step's trace and results of a context that never begins a plant == those of one that stepped
    plants in between: the plants' storage and launches are the plants' own"""
    from idto_amd.problem import synthetic_trajectory
    name = "mini_cheetah"
    model, _, cfg = pc.case(name)
    q = synthetic_trajectory(cfg, model, 3, seed=0, lower=0.02)
    x, tau = _inputs(name, 1)
    plain, planted = _context(name, 1), _context(name, 1)
    planted.plant_begin(H)
    planted.plant_set_state(0.0, x)
    planted.plant_step(4, tau)
    planted.forward_dynamics(x, tau)
    a, b = _gn_step_traced(plain, q), _gn_step_traced(planted, q)
    plain.close()
    planted.close()
    assert a[1] == b[1] and a[2] == b[2]
    # ... and those of the commit before the plants existed: tests/golden/plant_untouched_context.json, recorded there with
    # this model, horizon and trajectory (last_solver and last_assembly among the options name the launches a gn_step took)
    # (a gn_step emits no host-trace marks, on either commit: the recorded label list is empty, and the comparison of the
    # labels says only that none appeared; what carries information is the options, last_solver and last_assembly included)
    import json
    import os
    golden = json.load(open(os.path.join(pc.ROOT, "tests", "golden", "plant_untouched_context.json")))
    assert (golden["model"], golden["N"]) == (name, 3)
    for labels, options in (a[1:], b[1:]):
        assert labels == golden["labels"] and options == golden["options"]
    for k in a[0]:
        assert _same(a[0][k], b[0][k]), k
