// plant_tangent.h — tangent coordinates of a plant's state (csrc/plant_lin.h, csrc/tvlqr_step.h; include/idto_hip.h
// idto_hip_plant_linearize, idto_hip_plant_tvlqr).  A state deviation is dx = [dtheta (nv); dv (nv)]: dtheta has a velocity's
// layout, so a floating joint's four quaternion entries are three angular ones (world frame, the convention of plant_qdot's
// [0, omega] q) and every other joint's positions are their own deviations.  Plain C++ like plant_step.h, whose text it
// reuses: the host includes it as it is, hipcc compiles the same text for the device, neither side contracts a * b + c, and
// every expression is evaluated in the order it is written.
#pragma once

#include "plant_step.h"

namespace idto_plant {

// out = q (+) dtheta for one body's joint (q, dtheta, out, qdot: the model's whole vectors; qdot: scratch, the size of q; out may
// not alias q): the position that plant_advance_body makes of q with h = 1 and v+ = dtheta - q + N(q) dtheta by plant_qdot, then a
// floating joint's quaternion divided by its norm; q + dtheta for every other joint.  dtheta = 0 returns q bit for bit where
// the norm expression of q evaluates to 1 (elsewhere within 4 eps: a quotient by 1 +- 2 ulp).
IDTO_PLANT_HD inline void tangent_add(int jtype, int qs, int vs, const double* q, const double* dtheta, double* out, double* qdot) {
  const int nqj = plant_joint_nq(jtype), nvj = plant_joint_nv(jtype);
  for (int i = 0; i < nqj; ++i) out[qs + i] = q[qs + i];
  // (v+ = 0 + 1 * dtheta = dtheta exactly, q+ = q + 1 * qdot: plant_advance_body with a velocity of zero and a = dtheta, h = 1)
  double vplus[6];
  for (int i = 0; i < nvj; ++i) vplus[i] = 0.0;
  plant_advance_body(jtype, qs, 0, 1.0, out, vplus, dtheta + vs, qdot);
}

// out[vs ...] = qa (-) qb for one body's joint, the deviation dtheta with qb (+) dtheta = qa to FIRST order.  Every joint but a
// floating one: qa - qb.  Floating: d = qa (x) conj(qb); the angular part is 2 vec(d), times -1 if d.w < 0 (q and -q are one
// rotation: the short way round), the linear part pa - pb.  2 vec(d) is twice the sine of half the angle where the exact
// logarithm is the angle itself: the error is O(|dtheta|^3) relative to an exact difference of O(|dtheta|), i.e. O(|dtheta|^2)
// relative - 1e-11 at a perturbation of cbrt(2^-52), far below a central difference's own truncation error of the same order
// in eps times the map's third derivative.
IDTO_PLANT_HD inline void tangent_sub(int jtype, int qs, int vs, const double* qa, const double* qb, double* out) {
  if (jtype == IDTO_JOINT_FLOATING) {
    const double aw = qa[qs], ax = qa[qs + 1], ay = qa[qs + 2], az = qa[qs + 3];
    const double bw = qb[qs], bx = qb[qs + 1], by = qb[qs + 2], bz = qb[qs + 3];
    const double dw = ((aw * bw + ax * bx) + ay * by) + az * bz;
    const double dx = ((bw * ax - aw * bx) - ay * bz) + az * by;
    const double dy = ((bw * ay - aw * by) - az * bx) + ax * bz;
    const double dz = ((bw * az - aw * bz) - ax * by) + ay * bx;
    const double s = dw < 0.0 ? -2.0 : 2.0;
    out[vs] = s * dx; out[vs + 1] = s * dy; out[vs + 2] = s * dz;
    for (int i = 0; i < 3; ++i) out[vs + 3 + i] = qa[qs + 4 + i] - qb[qs + 4 + i];
  } else {
    const int n = plant_joint_nv(jtype);
    for (int i = 0; i < n; ++i) out[vs + i] = qa[qs + i] - qb[qs + i];
  }
}

// ---- the columns of a linearisation (csrc/plant_lin.h): per state P = 1 + 2 * 3 nv perturbed copies of (x, tau) = ([q; v], tau) -
// column 0 the nominal, columns 1 + 2 k and 2 + 2 k at +eps and -eps along component k of [dtheta (nv); dv (nv); tau (nv)] -
// and the central difference of what a map made of a pair of them.  A body owns its entries: a lane per column and body on
// the device, loops on the host.
IDTO_PLANT_HD inline int lin_columns(int nv) { return 1 + 2 * 3 * nv; }

// this body's entries of column `col`: q_out, v_out, tau_out are the column's whole vectors.  A position column whose
// component is the body's goes through tangent_add; every other column copies q.
IDTO_PLANT_HD inline void lin_perturb_body(int jtype, int qs, int vs, int nq, int nv, int col, double eps, const double* x, const double* tau,
                                           double* q_out, double* v_out, double* tau_out) {
  const int nqj = plant_joint_nq(jtype), nvj = plant_joint_nv(jtype);
  const int k = (col - 1) / 2, kind = col ? k / nv : -1, comp = col ? k % nv : -1;
  const double e = (col - 1) % 2 == 0 ? eps : -eps;
  if (kind == 0 && comp >= vs && comp < vs + nvj) {
    double ql[7], dl[6], out[7], qdot[7];
    for (int i = 0; i < nqj; ++i) ql[i] = x[qs + i];
    for (int i = 0; i < nvj; ++i) dl[i] = (vs + i == comp) ? e : 0.0;
    tangent_add(jtype, 0, 0, ql, dl, out, qdot);
    for (int i = 0; i < nqj; ++i) q_out[qs + i] = out[i];
  } else {
    for (int i = 0; i < nqj; ++i) q_out[qs + i] = x[qs + i];
  }
  for (int i = 0; i < nvj; ++i) {
    const double v = x[nq + vs + i], t = tau[vs + i];
    v_out[vs + i] = (kind == 1 && vs + i == comp) ? v + e : v;
    tau_out[vs + i] = (kind == 2 && vs + i == comp) ? t + e : t;
  }
}

// this body's rows of a column of [A | B]: dst[n = 2 nv] = [tangent_sub(q+, q-); v+ - v-] / two_eps from the final states xp = [q+; v+]
// and xm = [q-; v-] of the column's pair; two_eps = 2 eps, formed once by the caller
IDTO_PLANT_HD inline void lin_difference_body(int jtype, int qs, int vs, int nq, int nv, double two_eps, const double* xp, const double* xm, double* dst) {
  const int nvj = plant_joint_nv(jtype);
  double d[6];
  tangent_sub(jtype, qs, 0, xp, xm, d);
  for (int i = 0; i < nvj; ++i) {
    dst[vs + i] = d[i] / two_eps;
    dst[nv + vs + i] = (xp[nq + vs + i] - xm[nq + vs + i]) / two_eps;
  }
}

}  // namespace idto_plant
