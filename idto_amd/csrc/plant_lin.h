// plant_lin.h — a plant's linearisation about given states and the time-varying LQR gains along them (include/idto_hip.h
// idto_hip_plant_linearize, idto_hip_plant_tvlqr): x+ ~ f(x*, u*) + A dx + B du in tangent coordinates (plant_tangent.h),
// where f is the plants' own map of `substeps` substeps under a held torque - plant_kernel (plant.h), used as it is.
//
// Per problem b and state s there are P = 1 + 2 * 3 nv COLUMNS, each a plant of its own:
//   column 0                  the nominal (x_s, tau_s)
//   column 1 + 2 k, 2 + 2 k   +eps, -eps along component k of [dtheta (nv); dv (nv); tau (nv)]
// lin_perturb_kernel writes the S * P plant states [t = 0, q, v] and torques (plant_tangent.h lin_perturb_body, a thread per
// column and joint: a position column goes through tangent_add, every other column copies q), plant_kernel rolls them out
// in hold mode, one launch per problem with every workgroup reading the problem's one parameter record, and
// lin_difference_kernel forms
//   column k of [A | B] = [tangent_sub(q+, q-); v+ - v-] / (2 eps),   the divisor formed once,
// a thread per column and joint, nothing accumulated.  status[s] = {0, 0}, or {the code, the column} of the first column
// whose rollout did not end with code 0 (plant.h PLANT_OK): A[s], B[s] and x_next[s] are then NaN.
//
// tvlqr_kernel runs the Riccati recursion of tvlqr_step.h backward over a problem's S linearisations, one workgroup per
// problem, reading A and B from where lin_difference_kernel left them; every matrix of a step lives in LDS (lin_launch.h
// tvlqr_lds_doubles).  An entry of a product is one lane's left-to-right sum (tvlqr_step.h): the same bits as the header
// compiled for the host.  status[b] = 0, or 1 + t for the first step t (counting down) whose G = R + Bu^T P Bu has a pivot
// that is not > 0 and finite - K and P from t downward are then NaN; a state whose linearisation failed arrives as NaN and
// ends the recursion in the same way.
#pragma once

#include <hip/hip_runtime.h>

#include "lin_launch.h"
#include "tvlqr_step.h"

namespace idto_dev {

// grid (S, B)
__global__ void __launch_bounds__(256) lin_perturb_kernel(LinArgs a) {
  const int s = blockIdx.x, b = blockIdx.y, nq = a.nq, nv = a.nv, w = nq + nv;
  const size_t bs = (size_t)b * a.S + s;
  const double* x = a.x + bs * w;
  const double* tau = a.tau + bs * nv;
  for (int item = threadIdx.x; item < a.P * a.nb; item += blockDim.x) {
    const int col = item / a.nb, body = item % a.nb;
    const int jt = a.jtype[body], qs = a.qstart[body], vs = a.vstart[body];
    double* ps = a.pstate + (bs * a.P + col) * (size_t)(1 + w);
    if (body == 0) ps[0] = 0.0;
    idto_plant::lin_perturb_body(jt, qs, vs, nq, nv, col, a.eps, x, tau, ps + 1, ps + 1 + nq, a.ptau + (bs * a.P + col) * (size_t)nv);
  }
}

// grid (S, B)
__global__ void __launch_bounds__(256) lin_difference_kernel(LinArgs a) {
  __shared__ int bad[2];
  const int s = blockIdx.x, b = blockIdx.y, nq = a.nq, nv = a.nv, w = nq + nv, n = 2 * nv;
  const size_t bs = (size_t)b * a.S + s;
  if (threadIdx.x == 0) {
    bad[0] = 0; bad[1] = 0;
    for (int col = 0; col < a.P; ++col) {
      const int code = a.pstatus[2 * (bs * a.P + col)];
      if (code != 0) { bad[0] = code; bad[1] = col; break; }
    }
    a.status[2 * bs] = bad[0]; a.status[2 * bs + 1] = bad[1];
  }
  __syncthreads();
  const bool failed = bad[0] != 0;
  const double nan = __builtin_nan("");
  double* A = a.A + bs * (size_t)n * n;
  double* Bm = a.Bm + bs * (size_t)n * nv;
  const double* nominal = a.pstate + bs * a.P * (size_t)(1 + w) + 1;
  for (int i = threadIdx.x; i < w; i += blockDim.x) a.x_next[bs * w + i] = failed ? nan : nominal[i];
  for (int item = threadIdx.x; item < 3 * nv * a.nb; item += blockDim.x) {
    const int j = item / a.nb, body = item % a.nb;
    const int jt = a.jtype[body], qs = a.qstart[body], vs = a.vstart[body];
    const double* xp = a.pstate + (bs * a.P + 1 + 2 * j) * (size_t)(1 + w) + 1;
    const double* xm = a.pstate + (bs * a.P + 2 + 2 * j) * (size_t)(1 + w) + 1;
    double* dst = j < n ? A + (size_t)j * n : Bm + (size_t)(j - n) * n;
    if (failed) {
      for (int i = 0; i < idto_plant::plant_joint_nv(jt); ++i) { dst[vs + i] = nan; dst[nv + vs + i] = nan; }
    } else {
      idto_plant::lin_difference_body(jt, qs, vs, nq, nv, a.two_eps, xp, xm, dst);
    }
  }
}

// grid (B)
__global__ void __launch_bounds__(256) tvlqr_kernel(TvlqrArgs a) {
  extern __shared__ double lds[];
  using namespace idto_plant;
  const int tid = threadIdx.x, nt = blockDim.x, b = blockIdx.x;
  const int nv = a.nv, n = 2 * nv, nu = a.nu, nn = n * n, S = a.S;
  double* P = lds;            // [n x n]
  double* A = P + nn;         // [n x n]
  double* W = A + nn;         // [n x n] P A, then P Acl
  double* Acl = W + nn;       // [n x n]
  double* Q = Acl + nn;       // [n x n]
  double* Bu = Q + nn;        // [n x nu]
  double* PBu = Bu + n * nu;  // [n x nu]
  double* K = PBu + n * nu;   // [nu x n]
  double* RK = K + n * nu;    // [nu x n]
  double* G = RK + n * nu;    // [nu x nu]
  double* R = G + nu * nu;    // [nu x nu]
  double* col = R + nu * nu;  // [nu]
  double* Kg = a.K + (size_t)b * S * nu * n;
  double* Pg = a.P + (size_t)b * (S + 1) * nn;
  for (int i = tid; i < nn; i += nt) { const double x = a.Qf[i]; P[i] = x; Pg[(size_t)S * nn + i] = x; Q[i] = a.Q[i]; }
  for (int i = tid; i < nu * nu; i += nt) R[i] = a.R[i];
  int failed = -1;
  for (int t = S - 1; t >= 0; --t) {
    const double* At = a.A + ((size_t)b * S + t) * nn;
    const double* Bt = a.Bm + ((size_t)b * S + t) * (size_t)n * nv;
    for (int i = tid; i < nn; i += nt) A[i] = At[i];
    for (int i = tid; i < n * nu; i += nt) Bu[i] = Bt[(size_t)a.actuated[i / n] * n + i % n];
    __syncthreads();
    for (int e = tid; e < nn; e += nt) W[e] = tvlqr_mul(P, n, A, n, e % n, e / n);
    for (int e = tid; e < n * nu; e += nt) PBu[e] = tvlqr_mul(P, n, Bu, n, e % n, e / n);
    __syncthreads();
    for (int e = tid; e < nu * nu; e += nt)
      if (e % nu >= e / nu) G[e] = tvlqr_G(R, Bu, PBu, n, nu, e % nu, e / nu);
    for (int e = tid; e < nu * n; e += nt) K[e] = tvlqr_tmul(Bu, W, n, e % nu, e / nu);
    __syncthreads();
    // ---- G = L D L^T with column 0 of F as plant_ldlt_row's right-hand side: thread = row, as plant_kernel's solve
    for (int k = 0; k < nu; ++k) {
      const double d = G[k * nu + k];
      if (!plant_pivot_ok(d)) { failed = t; break; }   // (every thread reads the same entry behind a barrier: a uniform branch)
      for (int i = k + 1 + tid; i < nu; i += nt) col[i] = G[k * nu + i];
      __syncthreads();
      for (int i = k + 1 + tid; i < nu; i += nt) plant_ldlt_row(G, nu, K, col, d, k, i);
      __syncthreads();
    }
    if (failed >= 0) break;
    for (int j = tid; j < n; j += nt) {   // thread = right-hand side
      if (j > 0) tvlqr_forward(G, nu, K + j * nu);
      tvlqr_back(G, nu, K + j * nu);
    }
    __syncthreads();
    for (int e = tid; e < nu * n; e += nt) { Kg[(size_t)t * nu * n + e] = K[e]; RK[e] = tvlqr_mul(R, nu, K, nu, e % nu, e / nu); }
    for (int e = tid; e < nn; e += nt) Acl[e] = tvlqr_Acl(A, Bu, K, n, nu, e % n, e / n);
    __syncthreads();
    for (int e = tid; e < nn; e += nt) W[e] = tvlqr_mul(P, n, Acl, n, e % n, e / n);
    __syncthreads();
    for (int e = tid; e < nn; e += nt) {   // (P is not read any more: W holds its product)
      const int i = e % n, j = e / n;
      if (i < j) continue;
      const double p = tvlqr_P(Q, K, RK, Acl, W, n, nu, i, j);
      P[j * n + i] = p; P[i * n + j] = p;
      Pg[(size_t)t * nn + j * n + i] = p; Pg[(size_t)t * nn + i * n + j] = p;
    }
    __syncthreads();
  }
  if (failed >= 0) {
    const double nan = __builtin_nan("");
    for (size_t i = tid; i < (size_t)(failed + 1) * nu * n; i += nt) Kg[i] = nan;
    for (size_t i = tid; i < (size_t)(failed + 1) * nn; i += nt) Pg[i] = nan;
  }
  if (tid == 0) a.status[b] = failed >= 0 ? 1 + failed : 0;
}

}  // namespace idto_dev
