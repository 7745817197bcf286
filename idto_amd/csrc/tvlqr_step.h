// tvlqr_step.h — the arithmetic of one backward step of the time-varying LQR recursion about a linearised plant
// (csrc/plant_lin.h tvlqr_kernel; include/idto_hip.h idto_hip_plant_tvlqr) and the feedback law that uses its gains, as pure
// functions of flat arrays.  Plain C++ like plant_step.h: the host includes it as it is, hipcc compiles the same text for the
// device, neither side contracts a * b + c.  Every entry of every product is ONE sum, left to right from its first product -
// a lane each on the device, a loop on the host: no tree reduction anywhere, so both sides produce the same bits.
//
// All matrices are column-major: entry (i, j) of an r x c matrix M at M[j * r + i].  In tangent coordinates (plant_tangent.h),
// n = 2 nv; A is n x n, Bu n x nu (the actuated columns of B), Q, Qf n x n and R nu x nu symmetric.  A step from P = P_{t+1}:
//   PA = P A, PBu = P Bu
//   G  = R + Bu^T PBu (its lower triangle), F = Bu^T PA
//   K  = G^-1 F by plant_step.h's un-pivoted LDL^T, one right-hand side per column of F
//   Acl = A - Bu K, W = P Acl, RK = R K
//   P_t = (Q + K^T RK) + Acl^T W - the Joseph form; entry (i, j), i >= j, is computed and written to (i, j) and (j, i): P_t is
//   symmetric by construction and never symmetrised afterwards.
#pragma once

#include <cstddef>

#include "plant_tangent.h"

namespace idto_plant {

// sum_k a[k * sa] * b[k * sb], k = 0 ... len - 1, left to right from the first product
IDTO_PLANT_HD inline double tvlqr_dot(const double* a, int sa, const double* b, int sb, int len) {
  double s = a[0] * b[0];
  for (int k = 1; k < len; ++k) s = s + a[k * sa] * b[k * sb];
  return s;
}

// (X Y)(i, j) for X r x m and Y m x c
IDTO_PLANT_HD inline double tvlqr_mul(const double* X, int r, const double* Y, int m, int i, int j) { return tvlqr_dot(X + i, r, Y + j * m, 1, m); }
// (X^T Y)(i, j) for X m x r and Y m x c
IDTO_PLANT_HD inline double tvlqr_tmul(const double* X, const double* Y, int m, int i, int j) { return tvlqr_dot(X + i * m, 1, Y + j * m, 1, m); }

IDTO_PLANT_HD inline double tvlqr_G(const double* R, const double* Bu, const double* PBu, int n, int nu, int a, int b) {
  return R[b * nu + a] + tvlqr_tmul(Bu, PBu, n, a, b);
}
IDTO_PLANT_HD inline double tvlqr_Acl(const double* A, const double* Bu, const double* K, int n, int nu, int i, int j) {
  return A[j * n + i] - tvlqr_dot(Bu + i, n, K + j * nu, 1, nu);
}
IDTO_PLANT_HD inline double tvlqr_P(const double* Q, const double* K, const double* RK, const double* Acl, const double* W, int n, int nu, int i, int j) {
  return (Q[j * n + i] + tvlqr_tmul(K, RK, nu, i, j)) + tvlqr_tmul(Acl, W, n, i, j);
}

// The forward substitution of one more right-hand side b through the unit lower factor that plant_ldlt_row left in G
// (multiplier l of row i and pivot k at G[k * nu + i]): the operations plant_ldlt_row applies to ITS right-hand side, in its order
IDTO_PLANT_HD inline void tvlqr_forward(const double* G, int nu, double* b) {
  for (int k = 0; k < nu; ++k)
    for (int i = k + 1; i < nu; ++i) b[i] -= G[k * nu + i] * b[k];
}
// b = D^-1 b, then L^T x = b by plant_ldlt_back_row: plant_ldlt_solve's second half on one right-hand side
IDTO_PLANT_HD inline void tvlqr_back(const double* G, int nu, double* b) {
  for (int i = 0; i < nu; ++i) b[i] = b[i] / G[i * nu + i];
  for (int k = nu - 1; k >= 1; --k) {
    const double xk = b[k];
    for (int i = 0; i < k; ++i) plant_ldlt_back_row(G, nu, b, xk, k, i);
  }
}

// work of tvlqr_step in doubles
IDTO_PLANT_HD inline int tvlqr_step_work(int n, int nu) { return 2 * n * n + 2 * n * nu + nu * nu + nu; }

// The serial form of one step: P [n x n] is P_{t+1} on entry and P_t on return, K [nu x n] the gain.  Returns -1, or the
// index of the first pivot of G that is not > 0 and finite (K and P are then not to be used).
IDTO_PLANT_HD inline int tvlqr_step(int n, int nu, const double* A, const double* Bu, const double* Q, const double* R, double* P, double* K,
                                    double* work) {
  double* PA = work;            // [n x n] P A, then W = P Acl
  double* Acl = PA + n * n;     // [n x n]
  double* PBu = Acl + n * n;   // [n x nu]
  double* RK = PBu + n * nu;    // [nu x n]
  double* G = RK + n * nu;      // [nu x nu]
  double* col = G + nu * nu;    // [nu]
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) PA[j * n + i] = tvlqr_mul(P, n, A, n, i, j);
  for (int j = 0; j < nu; ++j)
    for (int i = 0; i < n; ++i) PBu[j * n + i] = tvlqr_mul(P, n, Bu, n, i, j);
  for (int b = 0; b < nu; ++b)
    for (int a = b; a < nu; ++a) G[b * nu + a] = tvlqr_G(R, Bu, PBu, n, nu, a, b);
  for (int j = 0; j < n; ++j)
    for (int a = 0; a < nu; ++a) K[j * nu + a] = tvlqr_tmul(Bu, PA, n, a, j);
  for (int k = 0; k < nu; ++k) {   // (the factorisation carries column 0 of F as plant_ldlt_row's right-hand side)
    const double d = G[k * nu + k];
    if (!plant_pivot_ok(d)) return k;
    for (int i = k + 1; i < nu; ++i) col[i] = G[k * nu + i];
    for (int i = k + 1; i < nu; ++i) plant_ldlt_row(G, nu, K, col, d, k, i);
  }
  for (int j = 1; j < n; ++j) tvlqr_forward(G, nu, K + j * nu);
  for (int j = 0; j < n; ++j) tvlqr_back(G, nu, K + j * nu);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) Acl[j * n + i] = tvlqr_Acl(A, Bu, K, n, nu, i, j);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) PA[j * n + i] = tvlqr_mul(P, n, Acl, n, i, j);
  for (int j = 0; j < n; ++j)
    for (int a = 0; a < nu; ++a) RK[j * nu + a] = tvlqr_mul(R, nu, K, nu, a, j);
  for (int j = 0; j < n; ++j)   // (P is not read any more: W holds its product)
    for (int i = j; i < n; ++i) { const double p = tvlqr_P(Q, K, RK, Acl, PA, n, nu, i, j); P[j * n + i] = p; P[i * n + j] = p; }
  return -1;
}

// The whole recursion over S linearisations A [S][n x n], B [S][n x nv] with the actuated velocity indices selecting Bu:
// P_out [S + 1][n x n] with P_S = Qf, K_out [S][nu x n].  Returns 0, or 1 + t for the first step t (counting down from S - 1)
// whose G has a pivot that is not > 0 and finite: K_t ... K_0 and P_t ... P_0 are then NaN.  work: tvlqr_step_work(n, nu) + n * n +
// n * nu doubles.
IDTO_PLANT_HD inline int tvlqr_recursion(int S, int nv, int nu, const int* actuated, const double* A, const double* B, const double* Q,
                                         const double* R, const double* Qf, double* K_out, double* P_out, double* work) {
  const int n = 2 * nv;
  double* P = work;             // [n x n]
  double* Bu = P + n * n;       // [n x nu]
  double* step = Bu + n * nu;
  for (int i = 0; i < n * n; ++i) { P[i] = Qf[i]; P_out[(size_t)S * n * n + i] = Qf[i]; }
  for (int t = S - 1; t >= 0; --t) {
    const double* At = A + (size_t)t * n * n;
    for (int c = 0; c < nu; ++c)
      for (int i = 0; i < n; ++i) Bu[c * n + i] = B[(size_t)t * n * nv + (size_t)actuated[c] * n + i];
    double* Kt = K_out + (size_t)t * nu * n;
    if (tvlqr_step(n, nu, At, Bu, Q, R, P, Kt, step) >= 0) {
      const double nan = __builtin_nan("");
      for (int s = t; s >= 0; --s) {
        for (int i = 0; i < nu * n; ++i) K_out[(size_t)s * nu * n + i] = nan;
        for (int i = 0; i < n * n; ++i) P_out[(size_t)s * n * n + i] = nan;
      }
      return 1 + t;
    }
    for (int i = 0; i < n * n; ++i) P_out[(size_t)t * n * n + i] = P[i];
  }
  return 0;
}

// The law u = u_nom - K_t [q (-) q_nom; v - v_nom] (K_t nu x n column-major; jtype, qstart, vstart: the model's tables,
// include/idto_model.h); dx: scratch, n = 2 nv doubles.  Row r of u is one sum, left to right.
IDTO_PLANT_HD inline void tvlqr_control(int nbodies, const int* jtype, const int* qstart, const int* vstart, int nq, int nv, int nu,
                                        const double* K, const double* x_nom, const double* u_nom, const double* x, double* dx, double* u) {
  for (int b = 0; b < nbodies; ++b) tangent_sub(jtype[b], qstart[b], vstart[b], x, x_nom, dx);
  for (int i = 0; i < nv; ++i) dx[nv + i] = x[nq + i] - x_nom[nq + i];
  for (int r = 0; r < nu; ++r) u[r] = u_nom[r] - tvlqr_dot(K + r, nu, dx, 1, 2 * nv);
}

}  // namespace idto_plant
