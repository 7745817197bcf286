"""fd_kernel's lane map without the redundant path lanes (option `fd_dedup`) against the map with every
evaluation on all its paths, on ONE context, where tests/test_gpu_fd_dedup.py leaves it open: mini_cheetah, N = 3 - the
records k = 0, 1, 2 have the v_init row and the NaN and zero fills of the M block.

The comparison is that file's: option 1, then 0, then 1 again; tau, v, a, N+, the slab [M | T | P | tau], the products
(asm_terms), gradient, H_A, H_B, H_C equal value for value, the NaN block equal to the NaN block.
Cases:
  (a) a batch of two whose problems have models of their own (set_model_batch: fd_dedup_models_kernel against
      fd_models_kernel) - a heavier link in one leg of problem 1, other contact parameters, other seeds;
  (b) each of the four legs in turn folded under the body: its body-foot pair - the pair a main lane evaluates itself
      while its helper evaluates the foot-ground pair - is inside the contact threshold in record 2 and outside it before,
      on every path once, the one that adds the body-ground pair among them.  The oracle's signed distances confirm the
      pattern on the CPU before a device is asked, and that no pair lies within 1e-4 of the threshold;
  (c) what a single-path lane copies from the baseline's row: every (leg column, other leg's row) entry of the slab's P
      and T blocks is exactly 0.0 and so is the M block's (T from k = 1, M from k = 2: tests/test_fd_support.py), while
      more than half of the own-leg entries are not zero.
"""
import copy

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

N = 3
ARRAYS = ("tau", "v", "a", "nplus", "slab", "asm_terms")
BANDS = ("gradient", "H_A", "H_B", "H_C")
FOOT_GROUND, BODY_GROUND, BODY_FOOT = (5, 6, 7, 8), (4,), (0, 1, 2, 3)   # pair indices of idto_amd/models/mini_cheetah.model


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _problem(cfg, model):
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = False
    sp.equality_constraints = False
    return prob, sp


def _outputs(dev, set_q, dedup, batch=None):
    dev.set_option("fd_dedup", dedup)
    assert dev.get_option("fd_dedup") == dedup
    set_q(dev)
    dev.eval_partials()
    dev.grad_hess()
    assert dev.get_option("last_assembly") == 1   # the products are fd_kernel's
    assert dev.get_option("last_fd_dedup") == dedup   # ... and the launch was the one asked for
    out = [{a: dev.get(a, b) for a in ARRAYS} for b in (range(batch) if batch else (None,))]
    set_q(dev)
    dev.gn_step()
    for o, b in zip(out, range(batch) if batch else (None,)):
        o.update({a: dev.get(a, b) for a in BANDS})
    return out


def _compare(dev, model, set_q, batch=None):
    """-> the outputs with the lane map; dev is closed"""
    dev.set_option("gn_small", 0)
    dev.set_option("asm_fold", 1)
    on = _outputs(dev, set_q, 1, batch)
    off = _outputs(dev, set_q, 0, batch)
    again = _outputs(dev, set_q, 1, batch)
    dev.close()
    for b, (x, y, z) in enumerate(zip(on, off, again)):
        for a in ARRAYS + BANDS:
            assert _same(x[a], y[a]), (b, a, int(np.sum(~((x[a] == y[a]) | (np.isnan(x[a]) & np.isnan(y[a]))))))
            assert _same(x[a], z[a]), (b, a, "second run")
        stride = x["slab"].size // N   # the M block of record 0
        assert np.all(np.isnan(x["slab"][:model.nq * model.nv])) and np.all(np.isfinite(x["slab"][stride:]))
        assert np.all(np.isfinite(x["tau"])) and np.any(x["tau"] != 0.0)
    return on


def test_batch_of_two_with_models_of_their_own():
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    probs, qs, sp = [], [], None
    for b in range(2):
        prob, sp = _problem(cfg, model)
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, N, seed=30 + b, lower=0.01))
    assert not np.array_equal(qs[0], qs[1])
    heavy = copy.deepcopy(model)
    link = [b for b in range(model.nbodies) if int(model.body_path[b]) == 2][1]   # the middle link of leg 2
    mass = np.asarray(heavy.mass, float).copy()
    mass[link] *= 1.5
    heavy.mass = mass
    heavy = heavy.normalize()
    soft = copy.deepcopy(sp)
    soft.contact_stiffness = 0.7 * sp.contact_stiffness
    soft.friction_coefficient = 0.8 * sp.friction_coefficient
    soft.dissipation_velocity = 1.3 * sp.dissipation_velocity
    dev = hip.HipPath(model, probs, sp)
    assert dev.get_option("fast_shape") == 3 and dev.get_option("fd_dedup") == 1
    dev.set_model_batch(1, heavy, soft)
    assert dev.get_option("model_batch") == 1
    on = _compare(dev, model, lambda d: d.set_q_batch(np.array(qs)), batch=2)
    assert not _same(on[0]["tau"], on[1]["tau"])
    # the record of problem 1 acts: its own model and parameters in a context of its own give its entry, the batch's model does not
    one = hip.HipPath(heavy, probs[1], soft)
    one.set_q(qs[1]); one.eval_partials()
    assert _same(one.get("tau"), on[1]["tau"]) and _same(one.get("slab"), on[1]["slab"])
    one.close()
    base = hip.HipPath(model, probs[1], sp)
    base.set_q(qs[1]); base.eval_partials()
    assert not _same(base.get("tau"), on[1]["tau"])
    base.close()


def folded_leg_trajectory(cfg, model, leg):
    """tests/test_gpu_fd_dedup.py contact_trajectory with leg `leg` in the place of leg 0: the base raised (record 0: nothing
    in contact), lowered with the leg half folded (record 1: feet and body on the ground), lowered further with the leg
    folded under the body (record 2: its foot against the body as well)"""
    q = synthetic_trajectory(cfg, model, N, seed=5, lower=0.0)
    for t, (z, fold) in enumerate(((0.3, 0.0), (-0.2, 1.4), (-0.27, 2.6)), start=1):
        q[t, 6] += z
        q[t, 8 + 3 * leg] += fold
        q[t, 9 + 3 * leg] -= 2 * fold
    return q


@pytest.mark.parametrize("leg", [0, 1, 2, 3])
def test_each_leg_folded_under_the_body(leg):
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    prob, sp = _problem(cfg, model)
    q = folded_leg_trajectory(cfg, model, leg)
    oracle = Oracle(model, prob, sp)
    thr = oracle.contact_threshold
    phi = np.array([oracle.signed_distances(q[k + 1])[0] for k in range(N)])   # [record, pair]
    inside = phi <= thr
    # the leg's own body-foot pair in record 2 and no other body-foot pair anywhere; feet and body on the ground from record 1
    want = np.zeros((N, len(BODY_FOOT)), bool)
    want[2, leg] = True
    assert np.array_equal(inside[:, list(BODY_FOOT)], want), inside.astype(int)
    assert not inside[0].any() and inside[1:, list(FOOT_GROUND + BODY_GROUND)].all(), inside.astype(int)
    # (no pair within the finite-difference step of the threshold: a perturbed evaluation must not switch it)
    assert np.min(np.abs(phi - thr)) > 1e-4
    _compare(hip.HipPath(model, prob, sp), model, lambda d: d.set_q(q))


def _leg_of(model):
    """path of every column of q and of every row / mass column of v: -1 for the common body's (tests/test_fd_support.py)"""
    qleg, vleg = np.full(model.nq, -1), np.full(model.nv, -1)
    for b in range(model.nbodies):
        if b == model.common_body:
            continue
        qleg[int(model.qstart[b])] = vleg[int(model.vstart[b])] = int(model.body_path[b])   # (one revolute joint a body)
    return qleg, vleg


def test_copied_torques_give_exact_zeros():
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    prob, sp = _problem(cfg, model)
    q = synthetic_trajectory(cfg, model, N, seed=3, lower=0.01)
    dev = hip.HipPath(model, prob, sp)
    dev.set_option("fd_dedup", 1)
    dev.set_q(q)
    dev.eval_partials()
    assert dev.get_option("last_fd_dedup") == 1
    slab = np.asarray(dev.get("slab")).reshape(N, -1)
    dev.close()
    nq, nv = model.nq, model.nv
    qleg, vleg = _leg_of(model)
    other = (qleg[:, None] >= 0) & (vleg[None, :] >= 0) & (qleg[:, None] != vleg[None, :])   # [column, row]: the slab's order
    own = (qleg[:, None] >= 0) & (qleg[:, None] == vleg[None, :])
    assert other.sum() == 12 * 9 and own.sum() == 12 * 3
    # (dtau_k/dq_{k+1} for every k; dtau_k/dq_k from k = 1, dtau_k/dq_{k-1} from k = 2: q_0 is fixed)
    for name, block, k0 in (("M", 0, 2), ("T", 1, 1), ("P", 2, 0)):
        blk = slab[k0:, block * nq * nv:(block + 1) * nq * nv].reshape(-1, nq, nv)
        assert np.all(np.isfinite(blk)), name
        assert np.all(blk[:, other] == 0.0), (name, int(np.count_nonzero(blk[:, other])))
        assert np.count_nonzero(blk[:, own]) > 0.5 * blk[:, own].size, name
