"""The plants' linearisation on the device (include/idto_hip.h idto_hip_plant_linearize; csrc/plant_lin.h, csrc/plant_tangent.h).

The bar is == : the columns are csrc/plant_tangent.h's, the text that tests/cpp/lin_host.cc compiles for the host; their rollouts
are plant_kernel's, which tests/test_gpu_plant.py holds to the host restatement bit for bit (its only rollout tolerance is ==,
so there is no wider one to divide by 2 eps for the models it does not run); the difference is the header's again.  The host
composition (tests/lin_cases.py) is computed once per model and shared.  S = 3 states (mini_cheetah: one), 4 substeps of 1 ms.
The free body's closed form shows that the numbers are right and not merely the same on both sides.
No test provokes a device fault: a failed pivot and an overflowing velocity end a rollout with a status word.
"""
import copy

import numpy as np
import pytest

import lin_cases as lc
from idto_amd import hip
from idto_amd.model import load_model

pytestmark = pytest.mark.gpu

H, SUB = 1e-3, 4


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all(a == b))


def _context(name, B=1, model=None, sp=None):
    dev_model, _, prob, sp0, _, _ = lc.case(name)
    return hip.HipPath(model if model is not None else dev_model, [prob] * B if B > 1 else prob, sp if sp is not None else sp0)


def _report(what, got, ref):
    d = np.abs(np.asarray(got) - np.asarray(ref))
    print(f"{what}: {int((np.asarray(got) != np.asarray(ref)).sum())} of {d.size} entries differ, the largest by {d.max():.3e} (largest entry {np.abs(ref).max():.3e})")


@pytest.mark.parametrize("name,S", [("pendulum", 3), ("acrobot", 3), ("hopper", 3), ("spinner", 3), ("free_body", 3), ("mini_cheetah", 1)])
def test_linearisation_equals_the_host_composition(name, S):
    x, tau = lc.inputs(name, S)
    xn_ref, A_ref, B_ref = lc.host_reference(name, S, H, SUB)
    dev = _context(name)
    xn, A, B, status = dev.plant_linearize(x, tau, H, SUB)
    n, nu = 2 * dev.nv, 1
    assert dev.lin_sizes(S, nu) == (n, 1 + 6 * dev.nv, xn.size, A.size, B.size, S * nu * n, (S + 1) * n * n)
    dev.close()
    for what, got, ref in (("x_next", xn, xn_ref), ("A", A, A_ref), ("B", B, B_ref)):
        _report(f"{name} {what}", got, ref)
    assert status.tolist() == [[0, 0]] * S
    assert _same(xn, xn_ref) and _same(A, A_ref) and _same(B, B_ref)


def test_free_body_closed_form():
    """free_body at rest under gravity with a held force f on the linear dofs: the map of S substeps is affine in (dp, dv_lin, f) -
    v+ = v + S h (g + f / m), p+ = p + S h v + h^2 S (S + 1) / 2 (g + f / m) - so dp+/dp = I, dp+/dv = S h I, dv+/dv = I,
    dv+/df = S h / m I, dp+/df = h^2 S (S + 1) / 2 / m I.  A central difference of an affine map is exact up to round-off, about
    u |x| / eps = 2e-11 |x| per operation over a few dozen operations: 1e-8 relative - to |x|, the size of the entries of x+ that are
    differenced (the largest |x+| among the block's rows), which is what the round-off of x+(+eps) - x+(-eps) scales with.  (Relative
    to the derivative's own entry, 1e-5 for dp+/df, the bound would be 1e-13 absolute: below the 2e-11 of a single operation.)"""
    model = load_model("free_body")
    nv, m = model.nv, float(np.asarray(model.mass)[0])
    x = np.concatenate([[1.0, 0, 0, 0, 0.1, 0.2, 0.8], np.zeros(nv)])
    tau = np.array([0, 0, 0, 0.7, -0.4, 1.9])
    dev = _context("free_body")
    xn, A, B, status = dev.plant_linearize(x[None], tau[None], H, SUB)
    dev.close()
    assert status.tolist() == [[0, 0]]
    A, B, I, xn = A[0], B[0], np.eye(3), xn[0]
    nq = model.nq
    size = {"p": np.abs(xn[4:7]).max(), "v": np.abs(xn[nq + 3:nq + 6]).max()}
    lin_p, lin_v = slice(3, 6), slice(nv + 3, nv + 6)
    blocks = {"dp+/dp": (A[lin_p, lin_p], 1.0), "dp+/dv": (A[lin_p, lin_v], SUB * H), "dv+/dv": (A[lin_v, lin_v], 1.0),
              "dv+/dp": (A[lin_v, lin_p], 0.0), "dv+/df": (B[lin_v, 3:6], SUB * H / m), "dp+/df": (B[lin_p, 3:6], H * H * SUB * (SUB + 1) / 2 / m)}
    for what, (got, entry) in blocks.items():
        print(f"{what}: entry {entry:.6e}, largest error {np.abs(got - entry * I).max():.3e}, |x+| of its rows {size[what[1]]:.3e}")
    for what, (got, entry) in blocks.items():
        assert np.abs(got - entry * I).max() <= 1e-8 * size[what[1]], (what, got)
        # ... and this test's own, tighter figure, worked out for these shapes: an entry of x+ is SUB sums onto the perturbed entry, each
        # rounded once at u |x+| (u = 2^-53; the products h v and h a are 1e-3 of it and smaller: 2 more roundings cover them), in
        # two columns, over 2 eps: 2 (SUB + 2) u |x+| / (2 eps) = 8.8e-11 for the position rows, 3.5e-12 for the velocity rows
        # (measured: at most 1.2e-11 and 6.4e-13)
        assert np.abs(got - entry * I).max() <= 2 * (SUB + 2) * 2.0 ** -53 * size[what[1]] / (2 * hip.LIN_EPS_DEFAULT), (what, got)
    # (no force depends on the position: v+ is the same number in the two columns of a pair, and x - x = 0)
    assert np.all(A[lin_v, lin_p] == 0.0)


def _hopper_variant(scale):
    base, sp = load_model("hopper"), lc.case("hopper")[3]
    m, p = copy.deepcopy(base), copy.deepcopy(sp)
    m.mass = np.asarray(m.mass) * scale
    m.inertia = np.asarray(m.inertia) * scale
    p.contact_stiffness *= 0.5
    p.friction_coefficient = 0.2
    return m.normalize(), p


def _solo(model, sp, x, tau):
    dev = _context("hopper", model=model, sp=sp)
    out = dev.plant_linearize(x, tau, H, SUB)
    dev.close()
    return out


def test_a_batch_with_models_of_its_own():
    """two hoppers, problem 1 heavier with a softer, more slippery ground (set_model_batch): entry b == a context built with model b"""
    x, tau = lc.inputs("hopper", 3)
    base, sp = lc.case("hopper")[0], lc.case("hopper")[3]
    heavy, sp_h = _hopper_variant(1.3)
    dev = _context("hopper", B=2)
    dev.set_model_batch(1, heavy, sp_h)
    xn, A, B, status = dev.plant_linearize(np.array([x, x]), np.array([tau, tau]), H, SUB)
    dev.close()
    assert status.tolist() == [[[0, 0]] * 3] * 2
    assert not _same(A[0], A[1])
    for b, (model, p) in enumerate([(base, sp), (heavy, sp_h)]):
        xn1, A1, B1, _ = _solo(model, p, x, tau)
        assert _same(xn[b], xn1) and _same(A[b], A1) and _same(B[b], B1), b
    assert _same(A[0], lc.host_reference("hopper", 3, H, SUB)[1])


def test_the_plants_models():
    """after plant_begin and plant_set_model(1): SCENE_MODELS_PLANTS linearises plant b's physics, SCENE_MODELS_PROBLEMS still the
    context's; the plants' states are untouched"""
    x, tau = lc.inputs("hopper", 3)
    base, sp = lc.case("hopper")[0], lc.case("hopper")[3]
    heavy, sp_h = _hopper_variant(1.3)
    dev = _context("hopper", B=2)
    with pytest.raises(hip.HipError, match="plant_linearize: the plants' models were asked for: call idto_hip_plant_begin"):
        dev.plant_linearize(np.array([x, x]), np.array([tau, tau]), H, SUB, models=hip.SCENE_MODELS_PLANTS)
    dev.plant_begin(H)
    dev.plant_set_model(1, heavy, sp_h)
    dev.plant_set_state(0.5, x[:2])
    plants = dev.plant_linearize(np.array([x, x]), np.array([tau, tau]), H, SUB, models=hip.SCENE_MODELS_PLANTS)
    problems = dev.plant_linearize(np.array([x, x]), np.array([tau, tau]), H, SUB)
    times, x_now = dev.plant_get_state()
    dev.close()
    assert _same(times, [0.5, 0.5]) and _same(x_now, x[:2])
    ref_base, ref_heavy = _solo(base, sp, x, tau), _solo(heavy, sp_h, x, tau)
    for k in range(3):
        assert _same(plants[k][0], ref_base[k]) and _same(plants[k][1], ref_heavy[k]), k
        assert _same(problems[k][0], ref_base[k]) and _same(problems[k][1], ref_base[k]), k


def test_a_failed_rollout_is_its_states_alone():
    """an overflowing velocity in state 1 of 3 (1e200: its square is not finite) ends that state's nominal rollout with
    PLANT_NONFINITE: status {2, column 0} and NaN for that state, the others as they are without it"""
    name = "acrobot"
    x, tau = lc.inputs(name, 3)
    xn_ref, A_ref, B_ref = lc.host_reference(name, 3, H, SUB)
    bad = x.copy()
    bad[1, -1] = 1e200
    dev = _context(name)
    xn, A, B, status = dev.plant_linearize(bad, tau, H, SUB)
    dev.close()
    assert status.tolist() == [[0, 0], [2, 0], [0, 0]]
    assert np.isnan(xn[1]).all() and np.isnan(A[1]).all() and np.isnan(B[1]).all()
    for s in (0, 2):
        assert _same(xn[s], xn_ref[s]) and _same(A[s], A_ref[s]) and _same(B[s], B_ref[s]), s


def test_a_failed_pivot_is_its_plants_alone():
    """plant 1 with negated masses and inertias (plant_set_model): its mass matrix' first pivot is not > 0 - PLANT_PIVOT in column 0
    of every state of plant 1, NaN there; plant 0 is what it is alone"""
    name = "acrobot"
    x, tau = lc.inputs(name, 3)
    xn_ref, A_ref, B_ref = lc.host_reference(name, 3, H, SUB)
    m = copy.deepcopy(lc.case(name)[0])
    m.mass = -np.asarray(m.mass)
    m.inertia = -np.asarray(m.inertia)
    dev = _context(name, B=2)
    dev.plant_begin(H)
    dev.plant_set_model(1, m.normalize())
    xn, A, B, status = dev.plant_linearize(np.array([x, x]), np.array([tau, tau]), H, SUB, models=hip.SCENE_MODELS_PLANTS)
    dev.close()
    assert status[0].tolist() == [[0, 0]] * 3 and status[1].tolist() == [[1, 0]] * 3
    assert np.isnan(xn[1]).all() and np.isnan(A[1]).all() and np.isnan(B[1]).all()
    assert _same(xn[0], xn_ref) and _same(A[0], A_ref) and _same(B[0], B_ref)


def test_refusals_by_name_leave_the_context_usable():
    name = "acrobot"
    x, tau = lc.inputs(name, 3)
    xn_ref, A_ref, B_ref = lc.host_reference(name, 3, H, SUB)
    dev = _context(name)
    w, nv = dev.nq + dev.nv, dev.nv
    nan_x, inf_tau = x.copy(), tau.copy()
    nan_x[2, 1] = np.nan
    inf_tau[0, 0] = np.inf
    too_many = 65536 // (1 + 6 * nv) + 1
    refused = [
        ("x is not finite at index %d" % (2 * w + 1), lambda: dev.plant_linearize(nan_x, tau, H, SUB)),
        ("tau is not finite at index 0", lambda: dev.plant_linearize(x, inf_tau, H, SUB)),
        (r"substeps must be in \[1, 4096\]", lambda: dev.plant_linearize(x, tau, H, 0)),
        (r"substeps must be in \[1, 4096\]", lambda: dev.plant_linearize(x, tau, H, 4097)),
        ("eps must be > 0 and finite", lambda: dev.plant_linearize(x, tau, H, SUB, eps=0.0)),
        ("eps must be > 0 and finite", lambda: dev.plant_linearize(x, tau, H, SUB, eps=np.inf)),
        ("eps must be > 0 and finite", lambda: dev.plant_linearize(x, tau, H, SUB, eps=np.nan)),
        ("the substep h must be > 0 and finite", lambda: dev.plant_linearize(x, tau, 0.0, SUB)),
        ("the substep h must be > 0 and finite", lambda: dev.plant_linearize(x, tau, -H, SUB)),
        ("the substep h must be > 0 and finite", lambda: dev.plant_linearize(x, tau, np.inf, SUB)),
        ("nstates must be >= 1", lambda: dev.plant_linearize(np.zeros((1, 0, w)), np.zeros((1, 0, nv)), H, SUB)),
        ("columns, more than 65536 in one call", lambda: dev.plant_linearize(np.zeros((1, too_many, w)), np.zeros((1, too_many, nv)), H, SUB)),
        ("models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS", lambda: dev.plant_linearize(x, tau, H, SUB, models=7)),
        ("the plants' models were asked for", lambda: dev.plant_linearize(x, tau, H, SUB, models=hip.SCENE_MODELS_PLANTS)),
    ]
    for text, call in refused:
        with pytest.raises(hip.HipError, match="plant_linearize: .*" + text):
            call()
        xn, A, B, status = dev.plant_linearize(x, tau, H, SUB)
        assert status.tolist() == [[0, 0]] * 3 and _same(xn, xn_ref) and _same(A, A_ref) and _same(B, B_ref), text
    dev.close()
