"""The tail of fd_kernel at the small shapes where it can go wrong: the record's copy in LDS and the 3 x 3 tiles of the
assembly products (fd_kernel.h, `terms`), with gP, gT, gM delivered as row nq of the lower-triangle tiles.

Every case is N = 3: the records k = 0, 1, 2 with their rules (T_0 = 0, M_0 and M_1 taken as 0) all occur.  The models
are chosen for the branches of the tile grid, and each test asserts the property it was chosen for:
  mini_cheetah  nq % 3 == 1: two spare rows in the last tile row, even nv, one round of tiles on 256 threads
  allegro_hand  nq % 3 == 2: one spare row, more tiles than threads (two rounds)
  hopper        odd nv: the `nv & 1` tail of the dot product
  spinner       nq % 3 == 0: no spare row, the lower triangles carry one more tile row (gn_small = 0: fd_kernel's path)
"""
import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory

pytestmark = pytest.mark.gpu

N = 3
BANDS = ("gradient", "H_A", "H_B", "H_C")
MODELS = ("mini_cheetah", "allegro_hand", "hopper", "spinner")
TB, THREADS = 3, 256
FAST_SHAPE = {"mini_cheetah": 3, "allegro_hand": 4, "hopper": 2, "spinner": 5}   # model_layout.h: the kernels with the new tail


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _tiles(nq):
    """tiles of the products phase: lower triangles of nbr x nb tiles (row nq rides along), three full nb x nb grids"""
    nb, nbr = -(-nq // TB), nq // TB + 1
    return 3 * (nb * nbr - nb * (nb - 1) // 2) + 3 * nb * nb


def _check_branch(name, model):
    nq, nv = model.nq, model.nv
    if name == "mini_cheetah":
        assert nq % TB == 1 and nv % 2 == 0 and _tiles(nq) <= THREADS
    elif name == "allegro_hand":
        assert nq % TB == 2 and _tiles(nq) > THREADS
    elif name == "hopper":
        assert nv % 2 == 1 and nv > 1
    elif name == "spinner":
        assert nq % TB == 0


def _setup(name, seed=3):
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = False
    sp.equality_constraints = False
    return cfg, model, prob, sp, synthetic_trajectory(cfg, model, N, seed=seed, lower=0.01)


def _dot(Aw, B):
    """out[r, c] = sum_l Aw[l, r] * B[l, c], l ascending from the first product, every product and sum rounded on its own
    (numpy's element-wise operations are IEEE and unfused)"""
    acc = Aw[0][:, None] * B[0][None, :]
    for l in range(1, Aw.shape[0]):
        acc = acc + Aw[l][:, None] * B[l][None, :]
    return acc


@pytest.mark.parametrize("name", MODELS)
def test_asm_terms_against_a_plain_restatement(name):
    cfg, model, prob, sp, q = _setup(name)
    _check_branch(name, model)
    nq, nv = model.nq, model.nv
    dev = hip.HipPath(model, prob, sp)
    assert dev.get_option("fast_shape") == FAST_SHAPE[name]
    dev.set_option("gn_small", 0)
    dev.set_option("asm_fold", 1)
    dev.set_q(q)
    dev.eval_partials()
    dev.grad_hess()
    assert dev.get_option("last_assembly") == 1
    terms = dev.get("asm_terms").reshape(N, -1)
    stride = dev.slab_stride
    slab = dev.get("slab").reshape(N, stride)
    dev.close()

    R = np.asarray(prob.R, float)
    w = np.array([(2.0 * R[r, r]) * float(prob.time_step) for r in range(nv)])   # diagonal of R' = 2 dt R, as uploaded
    bsz, qq = nq * nv, nq * nq
    low = np.tril(np.ones((nq, nq), bool))      # [r, c], r >= c
    for k in range(N):
        blk = lambda j: slab[k, j * bsz:(j + 1) * bsz].reshape(nq, nv).T.copy()   # [l, column]
        M, T, P = blk(0), blk(1), blk(2)
        if k < 2:
            M = np.zeros_like(M)
        if k == 0:
            assert np.all(T == 0.0)
        tau = slab[k, 3 * bsz:3 * bsz + nv]
        X = (P, T, M)
        Xw = [x * w[:, None] for x in X]         # a = X[l][r] * w_l, rounded first
        tw = tau * w
        got = terms[k]
        mat = lambda j: got[j * qq:(j + 1) * qq].reshape(nq, nq).T   # stored at c * nq + r -> [r, c]
        for j in range(3):                       # CP, CT, CM: lower triangles
            want = _dot(Xw[j], X[j])
            assert _same(mat(j)[low], want[low]), (name, k, "C", j)
        for j, (xa, sb) in enumerate(((0, 1), (1, 2), (0, 2))):   # BPT, BTM, APM: all entries
            assert _same(mat(3 + j), _dot(Xw[xa], X[sb])), (name, k, "B/A", j)
        for j in range(3):                       # gP, gT, gM
            want = _dot(tw[:, None], X[j])[0]
            assert _same(got[6 * qq + j * nq:6 * qq + (j + 1) * nq], want), (name, k, "g", j)


def _fold_pair(name, model, prob, sp, set_q, batch=None):
    out = {}
    for fold in (1, 0):
        dev = hip.HipPath(model, prob, sp)
        assert dev.get_option("fast_shape") == FAST_SHAPE[name]
        dev.set_option("gn_small", 0)
        dev.set_option("asm_fold", fold)
        set_q(dev)
        dev.eval_partials()
        dev.grad_hess()
        assert dev.get_option("last_assembly") == (1 if fold else 2)
        out[fold] = [{a: dev.get(a, b) for a in BANDS} for b in (range(batch) if batch else (None,))]
        dev.close()
    for b, (on, off) in enumerate(zip(out[1], out[0])):
        for a in BANDS:
            assert _same(on[a], off[a]), (b, a)


@pytest.mark.parametrize("name,gradients", [(m, "forward_differences") for m in MODELS] +
                         [("mini_cheetah", "central_differences"), ("mini_cheetah", "central_differences4")])
def test_fold_on_equals_fold_off(name, gradients):
    cfg, model, prob, sp, q = _setup(name)
    _check_branch(name, model)
    sp.gradients_method = gradients
    _fold_pair(name, model, prob, sp, lambda dev: dev.set_q(q))


def test_fold_on_equals_fold_off_batch_of_two():
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    probs, qs = [], []
    for b in range(2):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.scaling = False
        sp.equality_constraints = False
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, N, seed=10 + b, lower=0.01))
    assert not np.array_equal(qs[0], qs[1])
    _fold_pair("mini_cheetah", model, probs, sp, lambda dev: dev.set_q_batch(np.array(qs)), batch=2)
