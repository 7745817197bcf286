"""Inputs for the accuracy gate of every instantiated block size of the LDL^T solvers (not a test file).

host/solver_plan.cc SolverBlockSize maps a model's nq = k onto the instantiated block sizes K: 2, 3, 5, 19, 23 exactly, every
other k padded with the identity to 8 / 16 / 24 / 32 (a KKT context: 4 and 29 exactly, 25 .. 30 -> 30).  What is here:
  * revolute_star(k, nu): a model of any nq = k <= 32 for a context of that block size (generic evaluation);
  * star_problem: a ProblemDefinition and a trajectory for it, built directly;
  * banded_spd: block penta-diagonal SPD matrices of a chosen condition number, usable at every k <= 32;
  * ldlt_padded_numpy: what padding must mean - un-pivoted block LDL^T of the blocks embedded in K x K ones, in float64;
  * ldl_fits: which solves the two-workgroup kernel's LDS carve-up admits (32 x 32 blocks do not admit every horizon);
  * case(k, n, cond): one system of the sweep with its extended-precision solution, the same for
    tests/test_solver_cases.py (CPU) and tests/test_gpu_solver_block_sizes.py.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sl

import oracle_lib as ol
from idto_amd.model import Model
from idto_amd.problem import ProblemDefinition, SolverParameters
from test_oracle_penta import from_lower_dense

# k of the sweep per instantiated block size: the lower edge, an example's size, the unpadded case; the exact sizes
# whose production kernels never saw a matrix that is not a Gauss-Newton Hessian
BLOCK_SIZES = {8: (1, 4, 7, 8), 16: (9, 14, 16), 24: (17, 21, 24), 32: (25, 31, 32), 19: (19,), 23: (23,)}
HORIZONS = (3, 9, 10, 11, 24, 41)      # n = N + 1 block rows: one workgroup (3, 9), first two-sided split, odd split, longer
# condition targets per horizon: 1e4, and the largest of 1e12, 1e10, 1e8 at which oracle_lib.refined_solution still knows the
# solution to 1e-15 for every k (rows scaled over six decades within three block rows couple components a factor 1e6
# apart: measured 3e-14 at n = 3 and 3e-15 at n = 9 .. 11 for 1e12, 6e-15 at n = 3 for 1e10)
CONDS = {3: (1e4, 1e8), 9: (1e4, 1e10), 10: (1e4, 1e10), 11: (1e4, 1e10), 24: (1e4, 1e12), 41: (1e4, 1e12)}
# n K > 4096: the single right-hand side no longer stays in LDS (solver_layout.h penta_ldl_layout, bl_size == 0)
LONG = ((25, 129), (21, 171), (14, 257), (7, 513))   # K = 32, 24 (mandatory), 16, 8
LONG_COND = 1e8
SWEEP = [(k, n, c) for ks in BLOCK_SIZES.values() for k in ks for n in HORIZONS for c in CONDS[n]] + [(k, n, LONG_COND) for k, n in LONG]


def solver_block_size(k, kkt=False):
    """host/solver_plan.cc SolverBlockSize"""
    if kkt and k in (4, 29):
        return k
    if kkt and 24 < k <= 30:
        return 30
    return k if k in (2, 3, 5, 19, 23) else 8 if k <= 8 else 16 if k <= 16 else 24 if k <= 24 else 32


def ldl_lds_doubles(n, K, rows=0):
    """solver_layout.h penta_ldl_layout(n, K, 1, rows).end: the LDS of penta_ldl_kernel<K> for one right-hand side"""
    ks, ncr = 4 * ((K + 3) // 4) + 2, 2 * K + 1
    kks = K * ks
    o = (K + ncr) * ks + 2 * kks + 3 * kks + 3 * ks + 3 * ks + 2 * kks + ((K * K + 1) & ~1)
    o += (max(4 * K * K, 3 * K * ks + ks) + 1) & ~1
    o += 2 + 2 * ks + 3 * ks + 2 * kks
    nr = rows if 0 < rows < n else n
    bl = nr * K if n * K <= 4096 else 0
    return o + ((bl + 1) & ~1) + ((nr + 2) * ks if bl else 0)


def ldl_fits(n, K, two_sided):
    """does the two-workgroup kernel's carve-up fit the 160 KiB (host/solver_plan.cc PlanSolve)?  It does not where the
    right-hand side and rt of every local row are to stay in LDS beside 32 x 32 blocks: K = 32 one-sided at n = 28 .. 128,
    two-sided at n = 49 .. 128 - the planner refuses those solves ("right-hand sides do not fit the LDS carve-up")."""
    m = (n - 1) // 2 if two_sided and n >= 10 else 0
    rows = max(m + 2, n - m) + 2 if m > 0 else 0
    return ldl_lds_doubles(n, K, rows) * 8 <= 160 * 1024


def revolute_star(k, nu=0):
    """k revolute bodies in at most 4 chains of at most 8, each chain hanging off the world; no geometry, no pairs, no
    common body.  nu > 0: the first nu joints are unactuated (the others actuated), for the constrained routes."""
    assert 1 <= k <= 32 and 0 <= nu < k
    npaths = 1 if k <= 8 else 2 if k <= 16 else 4
    per = -(-k // npaths)
    assert per <= 8
    i = np.arange(k)
    path = i // per
    parent = np.where(i % per == 0, -1, i - 1)
    X = np.tile(np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.0], (k, 1))
    X[:, 9] = 0.05 + 0.01 * (i % 3)            # small offsets from the parent's frame
    X[:, 10] = 0.02 * path
    X[:, 11] = np.where(parent < 0, 0.1 * path, -0.12 - 0.01 * (i % 4))
    m = Model(name=f"revolute_star_{k}", parent=parent, jtype=np.zeros(k, dtype=int), X_PF=X,
              axis=np.eye(3)[i % 3], mass=0.3 + 0.05 * (i % 5), com=np.c_[0.01 * (i % 2), 0.0 * i, -0.05 - 0.005 * (i % 3)],
              inertia=np.c_[2e-3 + 1e-4 * (i % 4), 2.5e-3 + 1e-4 * (i % 3), 1.5e-3 + 1e-4 * (i % 5), 0.0 * i, 0.0 * i, 0.0 * i],
              damping=np.full(k, 0.05), actuated=(i >= nu).astype(int) if nu else np.ones(k, dtype=int),
              npaths=npaths, common_body=-1, body_path=path, body_names=[f"link{j}" for j in range(k)])
    return m.normalize()


def plain_problem(model, N):
    """identity-like weights around a resting configuration, built directly (no example file)"""
    nq, nv = model.nq, model.nv
    q0 = np.zeros(nq)
    for qs in model.quaternion_starts:
        q0[qs] = 1.0
    return ProblemDefinition(num_steps=N, q_init=q0, v_init=np.zeros(nv), Qq=np.eye(nq), Qv=0.1 * np.eye(nv),
                             Qf_q=10 * np.eye(nq), Qf_v=np.eye(nv), R=0.5 * np.eye(nv), q_nom=np.tile(q0, (N + 1, 1)),
                             v_nom=np.zeros((N + 1, nv)), time_step=0.05)


def star_problem(model, N, seed=0):
    """(ProblemDefinition, SolverParameters, q) for a revolute_star: a swing of every joint with noise on it"""
    nq = model.nq
    rng = np.random.default_rng(100 + seed)
    prob = plain_problem(model, N)
    prob.q_init = 0.2 + 0.05 * np.cos(np.arange(nq))
    prob.q_nom = prob.q_init + np.linspace(0.0, 0.4, N + 1)[:, None] * np.sin(1.0 + np.arange(nq))[None, :]
    prob.v_nom[1:] = np.diff(prob.q_nom, axis=0) / prob.time_step
    q = prob.q_nom + 0.02 * rng.uniform(-1, 1, (N + 1, nq))
    q[0] = prob.q_init
    return prob, SolverParameters(verbose=False), q


def banded_spd(n, k, cond_target, seed):
    """H = L L^T (dense, size n k), L unit lower block-banded with two sub-diagonal blocks, entries uniform in
    +-0.9 / sqrt(3 k), rows scaled by logspace(0, log10(cond_target) / 2): cond(H) within 4x of the target for k = 1 .. 32
    (test_gpu_penta.py's fixed +-0.3 is numerically indefinite from k = 25 on).  Formed block by block - H_ij = sum_m
    L_im L_jm^T for |i - j| <= 2 -, so that what lies outside the band is exactly zero and the long horizons stay cheap."""
    size = n * k
    rng = np.random.default_rng(seed)
    amp = 0.9 / np.sqrt(3 * k)
    scale = np.logspace(0, np.log10(cond_target) / 2, size).reshape(n, k, 1)
    Lb = np.zeros((n, 3, k, k))   # [i][d]: block (i, i - d)
    for i in range(n):
        for d in range(min(i, 2) + 1):
            Lb[i, d] = rng.uniform(-amp, amp, (k, k))
        Lb[i, 0] = np.tril(Lb[i, 0], -1) + np.eye(k)
        Lb[i] *= scale[i]
    H = np.zeros((size, size))
    for i in range(n):
        for j in range(max(0, i - 2), i + 1):
            blk = sum(Lb[i, i - m] @ Lb[j, j - m].T for m in range(max(0, i - 2), j + 1))
            if i == j:
                blk = np.tril(blk) + np.tril(blk, -1).T
            H[i * k:(i + 1) * k, j * k:(j + 1) * k] = blk
            H[j * k:(j + 1) * k, i * k:(i + 1) * k] = blk.T
    return H


def cond_banded(H, k):
    """lambda_max / lambda_min of the symmetric positive definite H of half bandwidth 3 k - 1: all eigenvalues where that
    is cheap, else Lanczos for the largest and shift-and-invert Lanczos (through the band's Cholesky factor) for the smallest"""
    size = H.shape[0]
    if size <= 1400:
        ev = np.linalg.eigvalsh(H)
        return ev[-1] / ev[0] if ev[0] > 0 else np.inf
    import scipy.sparse.linalg as ssl
    w = 3 * k - 1
    ab = np.zeros((w + 1, size))
    for d in range(w + 1):
        ab[d, :size - d] = np.diagonal(H, -d)
    cb = sl.cholesky_banded(ab, lower=True)
    inv = ssl.LinearOperator((size, size), matvec=lambda v: sl.cho_solve_banded((cb, True), v), dtype=np.float64)
    v0 = np.ones(size)
    hi = ssl.eigsh(H, k=1, which="LA", v0=v0, return_eigenvectors=False)[0]
    lo = ssl.eigsh(H, k=1, sigma=0.0, OPinv=inv, which="LM", v0=v0, return_eigenvectors=False)[0]
    return hi / lo


def ldlt_padded_numpy(bands, b, K):
    """H x = b by un-pivoted block LDL^T with row-by-row substitution, float64, the k x k blocks of bands = (A, B, C)
    ([blk, row, col], lower bands, C's lower triangle) embedded in K x K blocks padded with the identity.
    H = L D L^T with block rows [L_i,i-2 | L_i,i-1 | L_ii] (L_ii unit lower) and D_i diagonal:
      L_i,i-2 = A_i L_i-2,i-2^-T D_i-2^-1,   L_i,i-1 = (B_i - L_i,i-2 D_i-2 L_i-1,i-2^T) L_i-1,i-1^-T D_i-1^-1,
      L_ii D_i L_ii^T = C_i - L_i,i-2 D_i-2 L_i,i-2^T - L_i,i-1 D_i-1 L_i,i-1^T.
    Returns (x [n k], the pad components of x [n, K - k] - zero if padding means what it must -, the pivots [n, K])."""
    A, B, C = (np.asarray(v, dtype=np.float64) for v in bands)
    n, k = C.shape[0], C.shape[1]
    assert K >= k

    def pad(M, one):
        P = np.zeros((n, K, K))
        P[:, :k, :k] = M
        if one:
            P[:, np.arange(k, K), np.arange(k, K)] = 1.0
        return P
    A, B, C = pad(A, False), pad(B, False), pad(C, True)
    C = np.tril(C) + np.tril(C, -1).transpose(0, 2, 1)
    rhs = np.zeros((n, K))
    rhs[:, :k] = np.asarray(b, dtype=np.float64).reshape(n, k)
    Ld, L1, L2, D = np.zeros((n, K, K)), np.zeros((n, K, K)), np.zeros((n, K, K)), np.zeros((n, K))
    ut = lambda Lii, M: sl.solve_triangular(Lii, M, lower=True, unit_diagonal=True)   # L_ii^-1 M
    for i in range(n):
        S = C[i].copy()
        if i >= 2:
            L2[i] = ut(Ld[i - 2], A[i].T).T / D[i - 2]
            S -= (L2[i] * D[i - 2]) @ L2[i].T
        if i >= 1:
            M = B[i] - ((L2[i] * D[i - 2]) @ L1[i - 1].T if i >= 2 else 0.0)
            L1[i] = ut(Ld[i - 1], M.T).T / D[i - 1]
            S -= (L1[i] * D[i - 1]) @ L1[i].T
        Ld[i] = np.eye(K)
        for j in range(K):   # scalar LDL^T of the block, no pivoting
            D[i, j] = S[j, j]
            Ld[i, j + 1:, j] = S[j + 1:, j] / S[j, j]
            S[j + 1:, j + 1:] -= np.outer(Ld[i, j + 1:, j], S[j + 1:, j])
    y = np.zeros((n + 2, K))
    for i in range(n):      # forward, row by row (y[-1], y[-2] are the zero rows behind the end)
        y[i] = ut(Ld[i], rhs[i] - L1[i] @ y[i - 1] - L2[i] @ y[i - 2])
    x = np.zeros((n + 2, K))
    for i in range(n - 1, -1, -1):
        r = y[i] / D[i]
        if i + 1 < n:
            r = r - L1[i + 1].T @ x[i + 1]
        if i + 2 < n:
            r = r - L2[i + 2].T @ x[i + 2]
        x[i] = sl.solve_triangular(Ld[i].T, r, lower=False, unit_diagonal=True)
    return x[:n, :k].ravel().copy(), x[:n, k:].copy(), D


def errors(H, b, x, x_ref):
    """(forward error relative to max |x_ref|, componentwise backward error max |H x - b| / (|H| |x| + |b|))"""
    x = np.asarray(x, dtype=np.float64).ravel()
    fwd = np.abs(x - x_ref).max() / np.abs(x_ref).max()
    bwd = (np.abs(H @ x - b) / (np.abs(H) @ np.abs(x) + np.abs(b) + 1e-300)).max()
    return float(fwd), float(bwd)


@functools.lru_cache(maxsize=16)
def case(k, n, cond_target):
    """one system of the sweep: H dense, its bands (A, B, C, D, E), b = H linspace(-3, 12.4) rounded, the
    extended-precision solution of H x = b and its uncertainty, cond(H).  Shared by the tests that follow each other on
    one case; nobody writes to it."""
    H = banded_spd(n, k, cond_target, seed=1000 * k + n)
    bands = from_lower_dense(H, n, k)
    b = H @ np.linspace(-3, 12.4, n * k)
    # (three refinement steps gain more than the nineteen digits there are at LONG_COND; the long horizons' systems of
    # ~3500 unknowns go through the band factorisations: dense ones and dense long-double products cost seconds)
    long = (k, n) in LONG
    x_ref, unc = ol.refined_solution(H, b, steps=3 if long else 6, half_bandwidth=3 * k - 1 if long else None)
    for a in (H, b, x_ref) + tuple(bands):
        a.setflags(write=False)
    return SimpleNamespace(k=k, n=n, K=solver_block_size(k), target=cond_target, H=H, bands=bands, b=b, x_ref=x_ref, unc=unc,
                           cond=float(cond_banded(H, k)))
