"""The producers' back substitution in closed form (penta_pipe.h pipe_backward), modelled in numpy before any device runs it.

A producer chain of the pipelined solver owns local rows 0 .. nloc-1 and needs x of the two join rows behind them.  Three
tails give its rows once those are known, all from the same un-pivoted block LDL^T factors (U_i = L_ii^T unit upper):
  * row by row:   U_i x_i = Dn rt_i - (Dn Ht_i) x_{i+1} - (Dn Et_i) x_{i+2};
  * recursion:    [Y_i | Z_i | c_i] = U_i^-1 [Dn Ht_i | Dn Et_i | Dn rt_i] ahead of time,  x_i = c_i - Y_i x_{i+1} - Z_i x_{i+2};
  * closed form:  the recursion applied ahead of time to the 2K + 1 right-hand sides [c | 0], with the identity in the
                  two join rows:  T_i = [c_i | 0] - Y_i T_{i+1} - Z_i T_{i+2} = [chat_i | G_i],  x_i = chat_i + G_i [x_nloc ; x_nloc+1].
The model factorises the whole system top-down, substitutes the rows below a nine-row segment row by row (they stand for
the joiner's and the separator's answer) and takes the segment with each tail; the mirrored chain is the same on the
system with its block rows reversed.  Bars: the closed form's componentwise backward error <= 1e-12 (the project's gate
for every tail), its forward error within 1 % of the row-by-row tail's."""
import functools

import numpy as np
import pytest
import scipy.linalg as sl

import oracle_lib as ol
import solver_cases as sc
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory

SEGMENT = 9          # a producer's rows at cheetah N = 40
BWD_BAR = 1e-12
FWD_SLACK = 1.01


def factor(H, n, k):
    """un-pivoted block LDL^T of the block penta-diagonal H (solver_cases.ldlt_padded_numpy without the padding), and the
    forward substitution of nothing yet: returns (Ld, L1, L2, D)"""
    blk = lambda i, j: H[i * k:(i + 1) * k, j * k:(j + 1) * k]
    Ld, L1, L2, D = np.zeros((n, k, k)), np.zeros((n, k, k)), np.zeros((n, k, k)), np.zeros((n, k))
    ut = lambda Lii, M: sl.solve_triangular(Lii, M, lower=True, unit_diagonal=True)
    for i in range(n):
        S = np.tril(blk(i, i)) + np.tril(blk(i, i), -1).T
        if i >= 2:
            L2[i] = ut(Ld[i - 2], blk(i, i - 2).T).T / D[i - 2]
            S -= (L2[i] * D[i - 2]) @ L2[i].T
        if i >= 1:
            M = blk(i, i - 1) - ((L2[i] * D[i - 2]) @ L1[i - 1].T if i >= 2 else 0.0)
            L1[i] = ut(Ld[i - 1], M.T).T / D[i - 1]
            S -= (L1[i] * D[i - 1]) @ L1[i].T
        Ld[i] = np.eye(k)
        for j in range(k):
            D[i, j] = S[j, j]
            Ld[i, j + 1:, j] = S[j + 1:, j] / S[j, j]
            S[j + 1:, j + 1:] -= np.outer(Ld[i, j + 1:, j], S[j + 1:, j])
    assert (D > 0).all()
    return Ld, L1, L2, D


def three_tails(H, b, n, k, nloc=SEGMENT):
    """x of the whole system with rows 0 .. nloc-1 taken row by row, in recursion form and in closed form"""
    Ld, L1, L2, D = factor(H, n, k)
    ut = lambda Lii, M: sl.solve_triangular(Lii, M, lower=True, unit_diagonal=True)
    uinv = lambda i, M: sl.solve_triangular(Ld[i].T, M, lower=False, unit_diagonal=True)
    rhs = b.reshape(n, k)
    y = np.zeros((n + 2, k))
    for i in range(n):
        y[i] = ut(Ld[i], rhs[i] - L1[i] @ y[i - 1] - L2[i] @ y[i - 2])
    Ht = lambda i: L1[i + 1].T if i + 1 < n else np.zeros((k, k))     # Dn Ht_i
    Et = lambda i: L2[i + 2].T if i + 2 < n else np.zeros((k, k))     # Dn Et_i
    x = np.zeros((n + 2, k))
    for i in range(n - 1, nloc - 1, -1):
        x[i] = uinv(i, y[i] / D[i] - Ht(i) @ x[i + 1] - Et(i) @ x[i + 2])
    out = []
    # row by row
    xr = x.copy()
    for i in range(nloc - 1, -1, -1):
        xr[i] = uinv(i, y[i] / D[i] - Ht(i) @ xr[i + 1] - Et(i) @ xr[i + 2])
    out.append(xr[:n].ravel())
    # recursion form
    Y = [uinv(i, Ht(i)) for i in range(nloc)]
    Z = [uinv(i, Et(i)) for i in range(nloc)]
    c = [uinv(i, y[i] / D[i]) for i in range(nloc)]
    xc = x.copy()
    for i in range(nloc - 1, -1, -1):
        xc[i] = c[i] - (Y[i] @ xc[i + 1] + Z[i] @ xc[i + 2])
    out.append(xc[:n].ravel())
    # closed form: T_i = [G_i | chat_i], k x (2k + 1)
    T = {nloc: np.hstack([np.eye(k), np.zeros((k, k + 1))]), nloc + 1: np.hstack([np.zeros((k, k)), np.eye(k), np.zeros((k, 1))])}
    for i in range(nloc - 1, -1, -1):
        T[i] = np.hstack([np.zeros((k, 2 * k)), c[i][:, None]]) - np.hstack([Y[i], Z[i]]) @ np.vstack([T[i + 1], T[i + 2]])
    xf = x.copy()
    xj = np.r_[x[nloc], x[nloc + 1]]
    for i in range(nloc):
        xf[i] = T[i][:, 2 * k] + T[i][:, :2 * k] @ xj
    out.append(xf[:n].ravel())
    return out


def mirrored(H, b, n, k):
    p = (np.arange(n)[::-1, None] * k + np.arange(k)[None, :]).ravel()
    return np.ascontiguousarray(H[np.ix_(p, p)]), b[p], p


@functools.lru_cache(maxsize=None)
def real_system(name, N, seed):
    if name == "jaco":
        from test_gpu_gravity_switch import example
        model, cfg = example(name)
        lower = 0.0
    else:
        cfg, model = load_config(name), load_model(name)
        lower = 0.01
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=lower)
    g, bands = ol.Oracle(model, prob, sp).grad_hess(q)
    k = model.nq
    H, b = ol.penta_make_dense(*bands), -g.ravel()
    assert not H[:k, k:].any() and not b[:k].any()   # block row 0 is the identity: the solver's system starts at row 1
    H, b = np.ascontiguousarray(H[k:, k:]), b[k:].copy()
    x_ref, unc = ol.refined_solution(H, b)
    return H, b, N, k, x_ref, unc


def held(H, b, n, k, x_ref, tag):
    worst = 0.0
    for orient in ("top-down", "mirrored"):
        if orient == "mirrored":
            Hm, bm, p = mirrored(H, b, n, k)
            xs = []
            for xm in three_tails(Hm, bm, n, k):
                x = np.empty_like(xm)
                x[p] = xm
                xs.append(x)
        else:
            xs = three_tails(H, b, n, k)
        (f_row, b_row), (f_rec, b_rec), (f_cl, b_cl) = (sc.errors(H, b, x, x_ref) for x in xs)
        print(f"{tag} {orient}: backward row {b_row:.1e} recursion {b_rec:.1e} closed {b_cl:.1e}; forward {f_row:.4e} {f_rec:.4e} {f_cl:.4e}")
        assert b_cl <= BWD_BAR, (tag, orient, "componentwise backward error", b_cl)
        assert f_cl <= FWD_SLACK * f_row, (tag, orient, "forward error", f_cl, "row by row", f_row)
        worst = max(worst, b_cl)
    return worst


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_closed_form_on_the_cheetah_hessians(seed):
    H, b, n, k, x_ref, _ = real_system("mini_cheetah", 40, seed)
    assert k == 19 and n == 40
    held(H, b, n, k, x_ref, f"cheetah seed {seed}")


def test_closed_form_on_the_jaco_hessian():
    H, b, n, k, x_ref, _ = real_system("jaco", 40, 0)
    assert k == 14
    held(H, b, n, k, x_ref, "jaco")


@pytest.mark.parametrize("k", [9, 16, 19, 20])
def test_closed_form_on_directed_matrices(k):
    c = sc.case(k, 41, 1e12)
    held(c.H, c.b, c.n, c.k, c.x_ref, f"banded_spd k {k}")
