"""csrc/tvlqr_step.h - the Riccati recursion of the time-varying LQR gains and the feedback law, the text that the host and the
device's tvlqr_kernel both compile - on the CPU, through the stand-alone program tests/cpp/lin_host.cc compiled by g++ with the
address and undefined-behaviour sanitizers (tests/lin_cases.py).  Nothing is loaded into Python.

The recursion is held to a numpy restatement of the same formulas (G = R + Bu^T P Bu, K = G^-1 Bu^T P A by Gaussian elimination
without pivoting, P = Q + K^T R K + (A - Bu K)^T P (A - Bu K)) on random stable and unstable time-varying (A_t, B_t), S = 5.  The
tolerance is measured per case: the restatement runs in float64 and in numpy.longdouble, and the gate is GATE times the largest
relative difference between those two - what float64 round-off does to this recursion on this case.  Relative: the largest
absolute difference over all t, over the largest absolute entry, K and P each.
"""
import numpy as np
import pytest

import lin_cases as lc

S = 5
# 100: the scene report's precedent for "a multiple of the reference's own round-off".  Measured on the cases below: the float64
# restatement differs from the longdouble one by 1.06e-16 ... 2.75e-15 relative (largest: n = 12, nu = 6, unstable), the header by
# 1.06e-16 ... 1.55e-15, i.e. at most 1.72 times the restatement's own difference (n = 12, nu = 2, unstable) where 100 are allowed;
# the cost-to-go identity holds to 4.0e-18 ... 2.0e-15.
GATE = 100.0

CASES = [(n, nu, rho) for n, nus in ((2, (1,)), (4, (1, 2)), (12, (1, 2, 6))) for nu in nus for rho in (0.9, 1.3)]


def _spd(rng, n, scale):
    M = rng.uniform(-1, 1, (n, n))
    return scale * (M @ M.T / n + np.eye(n))


def _case(n, nu, rho, seed=0):
    """time-varying A_t of spectral radius rho (0.9 stable, 1.3 unstable), B_t [n, nv], nu actuated columns"""
    rng = np.random.default_rng(1000 * n + 10 * nu + int(10 * rho) + seed)
    nv = n // 2
    A = rng.uniform(-1, 1, (S, n, n))
    for t in range(S):
        A[t] *= rho / np.abs(np.linalg.eigvals(A[t])).max()
    B = rng.uniform(-1, 1, (S, n, nv))
    actuated = np.sort(rng.choice(nv, nu, replace=False))
    return A, B, actuated, _spd(rng, n, 1.0), _spd(rng, nu, 0.1), _spd(rng, n, 10.0)


def _solve(G, F):
    """G^-1 F by Gaussian elimination without pivoting, in G's dtype (numpy.linalg has no longdouble)"""
    G, F = G.copy(), F.copy()
    m = G.shape[0]
    for k in range(m):
        for i in range(k + 1, m):
            l = G[i, k] / G[k, k]
            G[i, k:] -= l * G[k, k:]
            F[i] -= l * F[k]
    for k in range(m - 1, -1, -1):
        F[k] = (F[k] - G[k, k + 1:] @ F[k + 1:]) / G[k, k]
    return F


def restatement(A, B, actuated, Q, R, Qf, dtype):
    A, B, Q, R, Qf = (np.asarray(M, dtype=dtype) for M in (A, B, Q, R, Qf))
    n, nu = A.shape[1], len(actuated)
    K, P = np.zeros((S, nu, n), dtype=dtype), np.zeros((S + 1, n, n), dtype=dtype)
    P[S] = Qf
    for t in range(S - 1, -1, -1):
        Bu = B[t][:, actuated]
        K[t] = _solve(R + Bu.T @ P[t + 1] @ Bu, Bu.T @ P[t + 1] @ A[t])
        Acl = A[t] - Bu @ K[t]
        P[t] = Q + K[t].T @ R @ K[t] + Acl.T @ P[t + 1] @ Acl
    return K, P


def _rel(a, b):
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def exe():
    return lc.sanitized()


@pytest.mark.parametrize("n,nu,rho", CASES)
def test_recursion_against_the_numpy_restatement(exe, n, nu, rho):
    A, B, actuated, Q, R, Qf = _case(n, nu, rho)
    status, K, P = lc.tvlqr(exe, A, B, actuated, Q, R, Qf)
    assert status == 0
    K64, P64 = restatement(A, B, actuated, Q, R, Qf, np.float64)
    Kld, Pld = restatement(A, B, actuated, Q, R, Qf, np.longdouble)
    own = max(_rel(K64, Kld), _rel(P64, Pld))
    got = max(_rel(K, Kld), _rel(P, Pld))
    print(f"n = {n}, nu = {nu}, rho = {rho}: the float64 restatement differs from longdouble by {own:.3e}, the header by {got:.3e}")
    assert own > 0.0, "the two precisions agree exactly: longdouble is no wider than float64 here, the gate measures nothing"
    assert got <= GATE * own, (n, nu, rho, got, own)
    # P_t is symmetric by construction: bit for bit
    for t in range(S + 1):
        assert np.array_equal(P[t], P[t].T), t
    assert np.array_equal(P[S], Qf)


@pytest.mark.parametrize("n,nu,rho", CASES)
def test_cost_to_go_identity(exe, n, nu, rho):
    """the closed loop x_{t+1} = (A_t - Bu_t K_t) x_t, u_t = -K_t x_t from a random x_0, in longdouble with the header's K and P:
    sum_t (x^T Q x + u^T R u) + x_S^T Qf x_S = x_0^T P_0 x_0, to the gate of the case"""
    A, B, actuated, Q, R, Qf = _case(n, nu, rho)
    status, K, P = lc.tvlqr(exe, A, B, actuated, Q, R, Qf)
    assert status == 0
    K64, P64 = restatement(A, B, actuated, Q, R, Qf, np.float64)
    Kld, Pld = restatement(A, B, actuated, Q, R, Qf, np.longdouble)
    own = max(_rel(K64, Kld), _rel(P64, Pld))
    ld = lambda M: np.asarray(M, dtype=np.longdouble)
    x = ld(np.random.default_rng(7 + n + nu).uniform(-1, 1, n))
    x0, cost = x.copy(), np.longdouble(0)
    for t in range(S):
        u = -ld(K[t]) @ x
        cost += x @ ld(Q) @ x + u @ ld(R) @ u
        x = ld(A[t]) @ x + ld(B[t][:, actuated]) @ u
    cost += x @ ld(Qf) @ x
    value = x0 @ ld(P[0]) @ x0
    rel = float(abs(cost - value) / abs(value))
    print(f"n = {n}, nu = {nu}, rho = {rho}: cost-to-go {float(cost):.17g}, x0' P0 x0 {float(value):.17g}, relative difference {rel:.3e} (gate {GATE * own:.3e})")
    assert rel <= GATE * own, (n, nu, rho, rel, own)


def test_a_singular_G_stops_the_recursion_there(exe):
    """R = 0 and Bu_t = 0 at t = 2: G is 0, its first pivot is not > 0 - status 1 + 2, K and P from 2 downward NaN, above untouched"""
    n, nu = 4, 2
    A, B, actuated, Q, R, Qf = _case(n, nu, 0.9)
    R = np.zeros((nu, nu))
    B[2] = 0.0
    status, K, P = lc.tvlqr(exe, A, B, actuated, Q, R, Qf)
    assert status == 1 + 2
    assert np.isnan(K[:3]).all() and np.isnan(P[:3]).all()
    assert np.isfinite(K[3:]).all() and np.isfinite(P[3:]).all()
    # the same weights with every B_t in place: R = 0 alone is no failure (G = Bu^T P Bu is positive definite)
    A2, B2, *_ = _case(n, nu, 0.9)
    assert lc.tvlqr(exe, A2, B2, actuated, Q, R, Qf)[0] == 0


def test_control_law(exe):
    """u = u_nom - K [q (-) q_nom; v - v_nom] on the hopper's tables (no floating joint: the deviation is x - x_nom) against numpy,
    within 4 n eps (|K| |dx|) per row (one left-to-right sum of n products)"""
    from idto_amd.model import load_model
    model = load_model("hopper")
    nq, nv, nu = model.nq, model.nv, 2
    rng = np.random.default_rng(3)
    K = rng.uniform(-5, 5, (nu, 2 * nv))
    x_nom, x, u_nom = rng.uniform(-1, 1, nq + nv), rng.uniform(-1, 1, nq + nv), rng.uniform(-1, 1, nu)
    u = lc.control(exe, model, K, x_nom, u_nom, x)
    dx = x - x_nom
    bound = 4 * 2 * nv * np.finfo(float).eps * (np.abs(K) @ np.abs(dx) + np.abs(u_nom))
    assert np.all(np.abs(u - (u_nom - K @ dx)) <= bound), (u, u_nom - K @ dx)


def test_control_law_with_a_floating_joint(exe):
    """the same law on mini_cheetah's tables (a floating base, qstart != vstart behind it): the deviation's angular part is
    2 vec(q (x) conj(q_nom)), the short way round, the linear part and the joints plain differences - restated in numpy.  The two
    sides form an angular component from four products of entries <= 1 in different orders: each within 8 eps of the exact value,
    16 eps apart; that times |K|, plus the row sum's 4 n eps (|K| |dx| + |u_nom|)."""
    from idto_amd.model import load_model
    model = load_model("mini_cheetah")
    nq, nv, nu = model.nq, model.nv, 12
    assert int(model.jtype[0]) == 3 and int(model.qstart[1]) == 7 and int(model.vstart[1]) == 6
    rng = np.random.default_rng(4)
    K = rng.uniform(-5, 5, (nu, 2 * nv))
    x_nom, x, u_nom = rng.uniform(-1, 1, nq + nv), rng.uniform(-1, 1, nq + nv), rng.uniform(-1, 1, nu)
    for s in (x_nom, x):
        s[:4] /= np.linalg.norm(s[:4])
    for sign in (1.0, -1.0):   # (-q is the same rotation: the d.w < 0 branch gives the same law)
        xs = x.copy()
        xs[:4] *= sign
        a, b = xs[:4], x_nom[:4] * np.array([1.0, -1, -1, -1])
        d = np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])
        dx = np.concatenate([(2.0 if d[0] >= 0 else -2.0) * d[1:], xs[4:nq] - x_nom[4:nq], xs[nq:] - x_nom[nq:]])
        u = lc.control(exe, model, K, x_nom, u_nom, xs)
        eps = np.finfo(float).eps
        bound = 4 * 2 * nv * eps * (np.abs(K) @ np.abs(dx) + np.abs(u_nom)) + 16 * eps * np.abs(K[:, :3]).sum(axis=1)
        assert np.all(np.abs(u - (u_nom - K @ dx)) <= bound), (sign, u, u_nom - K @ dx)
    assert np.abs(dx[:3]).max() > 0.1   # (the deviation is a large rotation: the test is not about a small angle)
