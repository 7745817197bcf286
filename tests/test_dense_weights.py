"""Dense (non-diagonal) cost weights: the expectation the device's dense paths are held to (tests/test_gpu_dense_weights.py)
and the conditions on its inputs, on the CPU.

The example configurations are dominated by R (dtau/dq)^2: with weights derived from the YAMLs' the off-diagonals of Qq, Qv,
Qf_q, Qf_v move H by 1e-13 .. 1e-6 of its largest entry, and no tolerance check would notice a kernel that dropped them.
`balanced_dense_problem` therefore scales each weight by what it contributes to H:

  1. m_k = the largest |entry| of the oracle's bands A, B, C (block C_0 = I excluded) at the trajectory when weight k is the
     identity and the other four are zero (1 where weight k does not enter H at all: Qq and Qv at N = 1, q_0 being fixed);
  2. W_k = S_k / m_k with S_k = I + 0.5 G G^T / n, G standard normal from default_rng(7), drawn in the order of KEYS;
  3. the lower triangle of W_k copied onto the upper one, so that W_k == W_k^T exactly.

  * test_every_dense_weight_matters: conditions on these inputs - the reference alone meets them - so that a wrong use of
    any one weight's off-diagonals shows in H, g and the cost far above round-off;
  * test_oracle_matches_plain_formulas: the oracle's g, bands and cost against tests/test_golden_examples.py assemble()
    (numpy @ on dense blocks) and the plain sum dt e^T W e, fed the oracle's own v, tau, partials and N+."""
import copy
import functools

import numpy as np
import pytest

from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle
from test_golden_examples import BANDS, PARTIALS, assemble

KEYS = ("Qq", "Qv", "R", "Qf_q", "Qf_v")
# the five configurations with the `lower` of tests/test_gpu_solver_accuracy.py CASES
LOWER = {"acrobot": 0.0, "spinner": 0.0, "hopper": 0.01, "mini_cheetah": 0.01, "allegro_hand": 0.0}
HORIZONS = (1, 2, 3, 6)   # i = N only / i = N - 1 with Qf_v, first B / first A, first i < N - 1 / interior rows
CASES = [(name, N) for name in LOWER for N in HORIZONS]
# every entry of g, A, B, C is a sum of at most six triple products with inner dimension <= 23; with balanced weights the
# sum of the absolute terms is a small multiple of the largest entry: (2 x 23 + 6) eps = 1.2e-14, times a margin of ~10
PLAIN_RTOL = 1e-13


def _base(name, N, seed):
    cfg, model = load_config(name), load_model(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    return model, prob, sp, synthetic_trajectory(cfg, model, N, seed=seed, lower=LOWER[name])


@functools.lru_cache(maxsize=None)
def balanced_weights(name, N, seed=1):
    """{k: W_k} of the recipe above (read-only: shared between the tests)"""
    model, prob, sp, q = _base(name, N, seed)
    rng = np.random.default_rng(7)
    out = {}
    for k in KEYS:
        n = np.asarray(getattr(prob, k)).shape[0]
        p = copy.deepcopy(prob)
        for j in KEYS:
            m = np.asarray(getattr(prob, j)).shape[0]
            setattr(p, j, np.eye(m) if j == k else np.zeros((m, m)))
        A, B, C = Oracle(model, p, sp).grad_hess(q)[1][:3]
        m_k = max(np.abs(A).max(), np.abs(B).max(), np.abs(C[1:]).max())
        G = rng.standard_normal((n, n))
        W = (np.eye(n) + 0.5 * G @ G.T / n) / (m_k if m_k > 0 else 1.0)
        W = np.tril(W) + np.tril(W, -1).T
        W.setflags(write=False)
        out[k] = W
    return out


def diagonal_of(W):
    return np.diag(np.diag(W))


def balanced_dense_problem(name, N, seed=1, which=KEYS):
    """(model, prob, sp, q): the configuration at horizon N with the balanced weights; the weights in `which` dense, the
    others the diagonal of their W_k; no scaling, no enforced constraints"""
    model, prob, sp, q = _base(name, N, seed)
    for k, W in balanced_weights(name, N, seed).items():
        setattr(prob, k, W.copy() if k in which else diagonal_of(W))
    return model, prob, sp, q


def plain_cost(prob, q, v, tau):
    """sum_t dt (e_q^T Qq e_q + e_v^T Qv e_v + tau^T R tau) + the terminal terms (TO.cc:147-176)"""
    N, eq, ev = prob.num_steps, q - prob.q_nom, v - prob.v_nom
    run = sum(eq[t] @ prob.Qq @ eq[t] + ev[t] @ prob.Qv @ ev[t] + tau[t] @ prob.R @ tau[t] for t in range(N))
    return prob.time_step * run + eq[N] @ prob.Qf_q @ eq[N] + ev[N] @ prob.Qf_v @ ev[N]


def plain_differences(prob, q, v, tau, P, Np, g, bands, cost):
    """{array: largest |given - plain formula| / the plain array's largest entry} for g, H_A, H_B, H_C, cost"""
    g_p, bands_p = assemble(prob, q, v, tau, P, Np)
    out = {"gradient": np.abs(np.asarray(g).reshape(g_p.shape) - g_p).max() / np.abs(g_p).max()}
    for key, x, y in zip(BANDS, bands, bands_p):
        out[key] = np.abs(x - y).max() / max(np.abs(y).max(), np.finfo(float).tiny)
    c = plain_cost(prob, q, v, tau)
    out["cost"] = abs(cost - c) / abs(c)
    return {k: float(x) for k, x in out.items()}


@functools.lru_cache(maxsize=None)
def oracle_expectation(name, N, which=KEYS):
    """what the oracle gives for balanced_dense_problem(name, N, which=which): computed once, shared, left unchanged"""
    model, prob, sp, q = balanced_dense_problem(name, N, which=which)
    orc = Oracle(model, prob, sp)
    v, a, tau, cost = orc.eval_traj(q)
    g, bands = orc.grad_hess(q)
    out = dict(v=v, a=a, tau=tau, cost=cost, gradient=g.reshape(N + 1, -1), bands=bands[:3], bands5=bands)
    for x in (v, a, tau, out["gradient"], *bands):
        x.setflags(write=False)
    return out


def does_not_enter(k, N):
    """Qq and Qv at N = 1: the only running step is t = 0, where q_0 is fixed (no row of g or H); their cost terms there
    are those of q_init - q_nom_0 (zero in four of the five configurations) and of v_init - v_nom_0 = 0 exactly, so the
    cost cannot be asked to change either"""
    return N == 1 and k in ("Qq", "Qv")


@pytest.mark.parametrize("name,N", CASES)
def test_every_dense_weight_matters(name, N):
    """conditions on the inputs, not measurements: thresholds fixed, the inputs (seed, the 0.5) are what would change"""
    model, prob, sp, q = balanced_dense_problem(name, N)
    for k in KEYS:
        W = getattr(prob, k)
        assert np.array_equal(W, W.T) and np.linalg.eigvalsh(W).min() > 0, k
        assert np.abs(W - diagonal_of(W)).max() > 0, k
    full = oracle_expectation(name, N)
    top = max(np.abs(b).max() for b in full["bands"])
    for k in KEYS:
        one = oracle_expectation(name, N, tuple(j for j in KEYS if j != k))
        dH = max(np.abs(x - y).max() for x, y in zip(full["bands"], one["bands"])) / top
        dg = np.abs(full["gradient"] - one["gradient"]).max() / np.abs(full["gradient"]).max()
        dc = abs(full["cost"] - one["cost"]) / abs(full["cost"])
        print(name, N, k, "off-diagonals change H by %.2e, g by %.2e, the cost by %.2e" % (dH, dg, dc))
        if does_not_enter(k, N):
            assert dH == 0 and dg == 0
            continue
        assert dH >= 5e-3, (k, dH)
        assert dg >= 1e-4, (k, dg)
        assert dc >= 1e-8, (k, dc)


@pytest.mark.parametrize("name,N", CASES)
def test_oracle_matches_plain_formulas(name, N):
    model, prob, sp, q = balanced_dense_problem(name, N)
    sp.gradients_method = "forward_differences"
    orc = Oracle(model, prob, sp)
    want = oracle_expectation(name, N)
    P = orc.eval_partials(q)
    Np = [orc.nplus(q[t]) for t in range(N + 1)]
    seen = plain_differences(prob, q, want["v"], want["tau"], {k: P[k] for k in PARTIALS}, Np, want["gradient"],
                             want["bands"], want["cost"])
    print(name, N, "largest |oracle - plain formulas| / largest entry:", seen)
    for key, val in seen.items():
        assert val <= PLAIN_RTOL, (key, val)
    A, B, C = want["bands"]
    assert all(np.array_equal(C[i], C[i].T) for i in range(N + 1)) and np.array_equal(C[0], np.eye(model.nq))
    assert not B[1].any() and not A[1].any() and (N < 2 or not A[2].any())
