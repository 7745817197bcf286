"""fd_kernel's lane map without the redundant path lanes (option `fd_dedup`; fd_dedup_kernel) against the
map with every evaluation on all its paths (`fd_dedup` 0, fd_kernel), on ONE context: mini_cheetah, N = 3 - the records
k = 0, 1, 2 cover the NaN and zero fills of the M block.

Everything the kernel writes, and what gn_step makes of it, must be equal value for value (np.array_equal; the NaN block
equal to the NaN block): tau, v, a, N+, the slab [M | T | P | tau], the products (asm_terms), gradient, H_A, H_B, H_C.
Cases:
  (a) synthetic trajectories, seeds 0 and 1;
  (b) a trajectory on which every kind of pair - foot-ground, body-ground, body-foot - is inside the contact threshold in
      one record and outside it in another: the base raised, then lowered with one leg folded under the body.  The
      oracle's signed distances confirm the pattern on the CPU before a device is asked;
  (c) a constant trajectory, v = a = 0 exactly: inputs that differ in the sign of a zero (id_fast.h InFwd);
  (d) a batch of two problems with different seeds.
hopper has no such lane map: the option changes nothing there.
"""
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


def _setup(name="mini_cheetah"):
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = False
    sp.equality_constraints = False
    return cfg, model, prob, sp


def _outputs(dev, set_q, dedup, batch=None, lane_map=True):
    dev.set_option("fd_dedup", dedup)
    assert dev.get_option("fd_dedup") == dedup
    set_q(dev)
    dev.eval_partials()
    dev.grad_hess()
    assert dev.get_option("last_assembly") == 1   # the products are fd_kernel's
    assert dev.get_option("last_fd_dedup") == (1 if dedup and lane_map else 0)   # ... and the launch was the one asked for
    out = [{a: dev.get(a, b) for a in ARRAYS} for b in (range(batch) if batch else (None,))]
    set_q(dev)
    dev.gn_step()
    for o, b in zip(out, range(batch) if batch else (None,)):
        o.update({a: dev.get(a, b) for a in BANDS})
    return out


def _compare(model, prob, sp, set_q, batch=None, expect_nan=True, lane_map=True):
    dev = hip.HipPath(model, prob, sp)
    dev.set_option("gn_small", 0)
    dev.set_option("asm_fold", 1)
    on = _outputs(dev, set_q, 1, batch, lane_map)
    off = _outputs(dev, set_q, 0, batch, lane_map)
    again = _outputs(dev, set_q, 1, batch, lane_map)
    dev.close()
    for b, (x, y, z) in enumerate(zip(on, off, again)):
        for a in ARRAYS + BANDS:
            assert _same(x[a], y[a]), (b, a, int(np.sum(~((x[a] == y[a]) | (np.isnan(x[a]) & np.isnan(y[a]))))))
            assert _same(x[a], z[a]), (b, a, "second run")
        if expect_nan:   # the M block of record 0
            stride = x["slab"].size // N
            assert np.all(np.isnan(x["slab"][:model.nq * model.nv])) and np.all(np.isfinite(x["slab"][stride:]))
        assert np.all(np.isfinite(x["tau"])) and np.any(x["tau"] != 0.0)
    return on


@pytest.mark.parametrize("seed", [0, 1])
def test_synthetic_trajectories(seed):
    cfg, model, prob, sp = _setup()
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.01)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 3 and dev.get_option("fd_dedup") == 1   # the default
    dev.close()
    _compare(model, prob, sp, lambda d: d.set_q(q))


def contact_trajectory(cfg, model):
    """the base raised (record 0: nothing in contact), lowered with leg 0 half folded (record 1: feet and body on the ground),
    lowered further with leg 0 folded under the body (record 2: its foot against the body as well)"""
    q = synthetic_trajectory(cfg, model, N, seed=5, lower=0.0)
    for t, (z, fold) in enumerate(((0.3, 0.0), (-0.2, 1.4), (-0.27, 2.6)), start=1):
        q[t, 6] += z
        q[t, 8] += fold
        q[t, 9] -= 2 * fold
    return q


def test_every_pair_kind_in_and_out_of_contact():
    cfg, model, prob, sp = _setup()
    q = contact_trajectory(cfg, model)
    oracle = Oracle(model, prob, sp)
    thr = oracle.contact_threshold
    inside = np.array([oracle.signed_distances(q[k + 1])[0] <= thr for k in range(N)])   # [record, pair]
    for kind in (FOOT_GROUND, BODY_GROUND, BODY_FOOT):
        per_record = inside[:, list(kind)].any(axis=1)
        assert per_record.any() and not per_record.all(), (kind, inside.astype(int))
    # (no pair within the finite-difference step of the threshold: a perturbed evaluation must not switch it)
    phi = np.array([oracle.signed_distances(q[k + 1])[0] for k in range(N)])
    assert np.min(np.abs(phi - thr)) > 1e-4
    _compare(model, prob, sp, lambda d: d.set_q(q))


def test_constant_trajectory_zero_velocity_and_acceleration():
    cfg, model, prob, sp = _setup()
    q = np.tile(synthetic_trajectory(cfg, model, N, seed=2, lower=0.01)[1], (N + 1, 1))
    prob.q_init = q[0].copy()
    prob.v_init = np.zeros(model.nv)
    on = _compare(model, prob, sp, lambda d: d.set_q(q))
    assert np.all(on[0]["v"] == 0.0) and np.all(on[0]["a"] == 0.0)


def test_batch_of_two():
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    probs, qs = [], []
    for b in range(2):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.scaling = False
        sp.equality_constraints = False
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, N, seed=20 + b, lower=0.01))
    assert not np.array_equal(qs[0], qs[1])
    _compare(model, probs, sp, lambda d: d.set_q_batch(np.array(qs)), batch=2)


def test_hopper_ignores_the_option():
    cfg, model, prob, sp = _setup("hopper")
    q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == 2
    dev.close()
    _compare(model, prob, sp, lambda d: d.set_q(q), lane_map=False)
