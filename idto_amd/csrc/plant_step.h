// plant_step.h — the arithmetic of one substep of a simulated plant (csrc/plant.h plant_kernel; include/idto_hip.h
// idto_hip_plant_*) as pure functions of flat arrays: the un-pivoted LDL^T solve of M a = tau_applied - ID(q, v, 0), the
// PD+ law of the low-level controller (reference examples/pd_plus_controller.cc:39-62), the map N(q) from velocities to
// position rates, and the semi-implicit Euler step.  Plain C++ like mpc_spline.h and ls_decide.h, no HIP type: the host
// includes it as it is, hipcc compiles the same text for the device (`__host__ __device__`), so that a plant stepped on
// either side is the same numbers.  Both sides compile without contraction of a * b + c; every expression below is
// evaluated in the order it is written - do not regroup them.
#pragma once

#include "idto_model.h"

#if defined(__HIPCC__)
#define IDTO_PLANT_HD __host__ __device__
#else
#define IDTO_PLANT_HD
#endif

namespace idto_plant {

// The time of substep s of a launch that begins at t0: one product and one sum, never an accumulation
IDTO_PLANT_HD inline double plant_time(double t0, int s, double h) { return t0 + s * h; }

// x is a finite number (neither NaN nor an infinity), without <cmath>: x - x is 0 exactly for those only
IDTO_PLANT_HD inline bool plant_finite(double x) { return x - x == 0.0; }
IDTO_PLANT_HD inline bool plant_pivot_ok(double d) { return d > 0.0 && plant_finite(d); }

// ---- LDL^T without pivoting of a dense symmetric positive definite matrix of order n, and the solve.
// The matrix is its LOWER triangle, column-major: entry (i, j), i >= j, at A[j * n + i]; the upper triangle is never read.
// Right-looking: for the pivots k = 0, 1, ... in turn, row i > k takes l = A(i, k) / A(k, k), subtracts l * A(j, k) from
// its entries (i, j), k < j <= i, and l * b_k from b_i, and keeps l in (i, k).  `col` is column k below the diagonal as it
// was BEFORE any row of this pivot ran (col[i] = A(i, k)): a row reads the others' entries from there, so that the rows
// of one pivot are independent of each other - one lane per row on the device (the snapshot travels through LDS), a loop
// over the rows on the host - and every entry receives the same operations in the same order, pivot by pivot.
IDTO_PLANT_HD inline void plant_ldlt_row(double* A, int n, double* b, const double* col, double d, int k, int i) {
  const double l = col[i] / d;
  for (int j = k + 1; j <= i; ++j) A[j * n + i] -= l * col[j];
  b[i] -= l * b[k];
  A[k * n + i] = l;
}
// The back substitution L^T x = D^-1 y: every row divides its b_i by its pivot first, then column sweeps k = n - 1, ..., 1 -
// x_k is final when its turn comes, and row i < k subtracts L(k, i) x_k: each x_i's updates in descending order of k
IDTO_PLANT_HD inline void plant_ldlt_back_row(const double* A, int n, double* b, double xk, int k, int i) { b[i] -= A[i * n + k] * xk; }

// The serial form: A is destroyed (L below the diagonal, D on it), b becomes the solution; work: n doubles.
// Returns -1, or the index of the first pivot that is not > 0 and finite (b is then not to be used).
IDTO_PLANT_HD inline int plant_ldlt_solve(double* A, int n, double* b, double* work) {
  for (int k = 0; k < n; ++k) {
    const double d = A[k * n + k];
    if (!plant_pivot_ok(d)) return k;
    for (int i = k + 1; i < n; ++i) work[i] = A[k * n + i];
    for (int i = k + 1; i < n; ++i) plant_ldlt_row(A, n, b, work, d, k, i);
  }
  for (int i = 0; i < n; ++i) b[i] = b[i] / A[i * n + i];
  for (int k = n - 1; k >= 1; --k) {
    const double xk = b[k];
    for (int i = 0; i < k; ++i) plant_ldlt_back_row(A, n, b, xk, k, i);
  }
  return -1;
}

// ---- PD+ (pd_plus_controller.cc:39-62): u = Kp (q_nom - q) + Kd (v_nom - v) [+ u_nom], Kp nu x nq and Kd nu x nv row-major,
// each row summed left to right from its first product; plain subtraction on every position, a quaternion's included,
// as the reference subtracts.  Row r of u:
IDTO_PLANT_HD inline double plant_pd_plus_row(const double* Kp, const double* Kd, int nq, int nv, int r, const double* q,
                                              const double* v, const double* q_nom, const double* v_nom, bool feed_forward,
                                              const double* u_nom) {
  double p = 0.0, d = 0.0;
  for (int c = 0; c < nq; ++c) {
    const double t = Kp[r * nq + c] * (q_nom[c] - q[c]);
    p = (c == 0) ? t : p + t;
  }
  for (int c = 0; c < nv; ++c) {
    const double t = Kd[r * nv + c] * (v_nom[c] - v[c]);
    d = (c == 0) ? t : d + t;
  }
  double u = p + d;
  if (feed_forward) u += u_nom[r];
  return u;
}
// ... and all of u scattered onto the actuated dofs of tau[nv] (the others: 0)
IDTO_PLANT_HD inline void plant_pd_plus(const double* Kp, const double* Kd, int nu, int nq, int nv, const int* actuated_dofs,
                                        const double* q, const double* v, const double* q_nom, const double* v_nom,
                                        bool feed_forward, const double* u_nom, double* tau) {
  for (int j = 0; j < nv; ++j) tau[j] = 0.0;
  for (int r = 0; r < nu; ++r)
    tau[actuated_dofs[r]] = plant_pd_plus_row(Kp, Kd, nq, nv, r, q, v, q_nom, v_nom, feed_forward, u_nom);
}

// ---- qdot = N(q) v for one body's joint (q, v, qdot: the model's whole vectors).  The identity for revolute, prismatic
// and planar joints.  A floating joint (q = [w x y z | p], v = [angular, world frame | linear], include/idto_model.h):
// the quaternion's rate is half the quaternion product [0, omega] q - for a unit quaternion the right inverse of the
// block L(2 q)^T (I - q q^T) / |q| that nplus_block forms - and the position's rate is the linear velocity.
IDTO_PLANT_HD inline void plant_qdot(int jtype, int qs, int vs, const double* q, const double* v, double* qdot) {
  if (jtype == IDTO_JOINT_FLOATING) {
    const double w = q[qs], x = q[qs + 1], y = q[qs + 2], z = q[qs + 3];
    const double ox = v[vs], oy = v[vs + 1], oz = v[vs + 2];
    qdot[qs] = 0.5 * (((-x) * ox - y * oy) - z * oz);
    qdot[qs + 1] = 0.5 * ((w * ox + z * oy) - y * oz);
    qdot[qs + 2] = 0.5 * ((w * oy - z * ox) + x * oz);
    qdot[qs + 3] = 0.5 * ((w * oz + y * ox) - x * oy);
    qdot[qs + 4] = v[vs + 3]; qdot[qs + 5] = v[vs + 4]; qdot[qs + 6] = v[vs + 5];
  } else {
    const int n = (jtype == IDTO_JOINT_PLANAR) ? 3 : 1;
    for (int i = 0; i < n; ++i) qdot[qs + i] = v[vs + i];
  }
}
IDTO_PLANT_HD inline int plant_joint_nv(int jtype) { return jtype == IDTO_JOINT_FLOATING ? 6 : (jtype == IDTO_JOINT_PLANAR ? 3 : 1); }
IDTO_PLANT_HD inline int plant_joint_nq(int jtype) { return jtype == IDTO_JOINT_FLOATING ? 7 : (jtype == IDTO_JOINT_PLANAR ? 3 : 1); }

// ---- one substep of semi-implicit Euler for one body's joint, in place: v+ = v + h a, q+ = q + h N(q) v+ with N at the old
// q, then a floating joint's quaternion divided by its norm sqrt(((w^2 + x^2) + y^2) + z^2) (one correctly rounded IEEE
// operation on both sides).  A body owns its entries of q and v and reads no other's: the bodies are independent (a lane
// each on the device).  qdot: scratch, the size of q.
IDTO_PLANT_HD inline void plant_advance_body(int jtype, int qs, int vs, double h, double* q, double* v, const double* a, double* qdot) {
  const int nvj = plant_joint_nv(jtype), nqj = plant_joint_nq(jtype);
  for (int i = 0; i < nvj; ++i) v[vs + i] = v[vs + i] + h * a[vs + i];
  plant_qdot(jtype, qs, vs, q, v, qdot);
  for (int i = 0; i < nqj; ++i) q[qs + i] = q[qs + i] + h * qdot[qs + i];
  if (jtype == IDTO_JOINT_FLOATING) {
    const double w = q[qs], x = q[qs + 1], y = q[qs + 2], z = q[qs + 3];
    const double nrm = __builtin_sqrt(((w * w + x * x) + y * y) + z * z);
    q[qs] = w / nrm; q[qs + 1] = x / nrm; q[qs + 2] = y / nrm; q[qs + 3] = z / nrm;
  }
}

// ... and for every body of a model in turn (jtype, qstart, vstart: the model's tables, include/idto_model.h)
IDTO_PLANT_HD inline void plant_advance(int nbodies, const int* jtype, const int* qstart, const int* vstart, double h, double* q,
                                        double* v, const double* a, double* qdot) {
  for (int b = 0; b < nbodies; ++b) plant_advance_body(jtype[b], qstart[b], vstart[b], h, q, v, a, qdot);
}

}  // namespace idto_plant
