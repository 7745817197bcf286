// plant.h — plants on the device (include/idto_hip.h idto_hip_forward_dynamics, idto_hip_plant_*): forward dynamics
//   a = M(q)^-1 (tau_applied - ID(q, v, 0))
// from the optimizer's own inverse dynamics with compliant contact (id_eval.h), and semi-implicit Euler substeps of it.
// One workgroup per plant, blockIdx.x the plant: no communication between workgroups, no wait of any kind, and a substep
// loop of a fixed trip count.  The model blob, the state and the applied torque are staged into LDS once; a substep then
// touches global memory only for an optional state record.
//
// A substep at (t, q, v), the arithmetic being csrc/plant_step.h's (the text the host compiles too):
//   1. nv + 1 evaluations on (nv + 1) * npaths lanes, the lanes of one evaluation adjacent as in fd_body's generic branch:
//      evaluation 0 is the bias c = ID(q, v, 0) with `full`, evaluation 1 + j the mass-matrix column M_j = ID(q, 0, e_j)
//      without.  Surplus groups re-run evaluation 0 into a dump row so that the butterflies inside id_eval are complete;
//      (nv + 1) * npaths lanes beyond the block go in rounds.
//   2. M a = tau_applied - c by plant_ldlt_row on wavefront 0, lane = row; the pivot column's snapshot travels through LDS.
//   3. plant_advance_body, a lane of wavefront 0 per body, into a candidate state that is committed only if it is finite.
// The applied torque is either held over the launch or the PD+ law on the plant's stored plan (mpc_batch.h: the MPC
// context's current plane, staged into LDS with the gains): the nominal [q, v, u] at the substep's time is mpc_spline.h's
// evaluation at t - start_time, clamped to the plan's range as the host's Interpolator clamps.  A third controller, the
// time-varying LQR law about a nominal (tvlqr_step.h tvlqr_control), is the compile-time LAW of plant_body: TrackArgs and
// track_kernel below.
// Instantiated: the generic evaluation for chains of up to 2, 3, 4 and 8 bodies, the exchange form id_eval<8, true> for
// models with shared pairs and id_eval<8, true, true> for a stem below the common body.
// Status per plant: 0 ok; 1 a pivot that is not > 0 and finite; 2 a non-finite state or input - each with the substep.  A
// plant that fails stops and keeps the state from before the failing substep.
#pragma once

#include <hip/hip_runtime.h>

#include "id_eval.h"
#include "mpc_spline.h"
#include "plant_sizes.h"
#include "plant_step.h"
#include "tvlqr_step.h"

namespace idto_dev {

enum { PLANT_OK = 0, PLANT_PIVOT = 1, PLANT_NONFINITE = 2 };

struct PlantArgs {
  // the plants' parameter records (model_layout.h model_record_*), mstride bytes apart; the DevContact / DevModel of a record
  // rec_contact / rec_model bytes into it
  const double* records; size_t mstride, rec_contact, rec_model;
  double* state;         // [B][1 + nq + nv]: t, q, v - read at the start, written at the end (steps only)
  const double* tau;     // [B][nv]: the applied torque, held over the launch
  double h; int substeps;
  int record_every; double* record;   // [B][substeps / record_every][nq + nv]: the state behind every record_every-th substep; may be null
  int* status;           // [B][2]: code, substep
  double* tick_out;      // [B][1 + nq + nv], may be null: the final [t, q, v] again, where mpc_shift_kernel reads a tick's inputs
  // forward dynamics only (fd != 0: the launch stops behind the solve and leaves the state alone): a [B][nv], and if not
  // null M [B][nv * nv] column-major and the bias [B][nv]
  int fd; double* a_out; double* M_out; double* bias_out;
  // PD+ (pd != 0; tau is not read): the plans [B][plan_len] of n knots at `breaks` - where the values / knot derivatives of the
  // q, v, u splines lie in a plan: plan_y / plan_m (MpcPlanLayout::y / m) -, the gains Kp [nu][nq] and Kd [nu][nv] row-major
  // and the velocity index of every control component
  int pd, n, nu, feed_forward;
  const double* breaks; const double* plan; size_t plan_len, plan_y[3], plan_m[3];
  const double* Kp; const double* Kd; const int* actuated;
};
// (what PD+ adds to plant_kernel's LDS: plant_sizes.h plant_pd_doubles)

// The time-varying LQR law (LAW; track_kernel below, include/idto_hip.h idto_hip_plant_track): R rollouts per problem, the plant
// blockIdx.x and its problem blockIdx.x / R, of S control steps of m substeps each.  At the start of step t the block stages
// K_t, x*_t and tau*_t into LDS, and wavefront 0 forms tvlqr_step.h's tvlqr_control - a lane per body tangent_sub, a lane per
// velocity v - v*, then a lane per control row ONE sum left to right - into the torque that is held over the step's substeps:
// the map that A_t, B_t linearise.  A launch runs the steps [first_step, first_step + steps); PlantArgs' substeps is S * m, the
// whole rollout's, so that the substep count, the status word and the record's rows (record_every = m) are the rollout's.
struct TrackArgs {
  int R, S, m, first_step, steps, nu;
  const int* actuated;     // [nu] velocity indices
  const double* x_nom;     // [B][S + 1][nq + nv]
  const double* tau_nom;   // [B][S][nv]: every component, the unactuated ones are applied as they are
  const double* K;         // [B][S][nu * n] column-major, n = 2 nv
  double* u_out;           // [B * R][S][nu]
  double* dx_out;          // [B * R][S + 1][n]: row t the deviation in front of step t, row S behind the last
};
// (what the law adds to the LDS, and the dynamic LDS of plant_kernel for a block: plant_sizes.h plant_law_doubles, plant_lds_doubles)

template <int MAXC, bool XCH, bool STEM = false, bool LAW = false>
IDTO_DEV void plant_body(const DevModel& M, const DevContact& cp, const PlantArgs& A, const int b, const TrackArgs* T = nullptr) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nq = M.nq, nv = M.nv, K = M.npaths, E = nv + 1;
  double* q = lds;                 // [nq]
  double* qn = q + nq;             // [nq] the candidate state of a substep
  double* qdot = qn + nq;          // [nq]
  double* v = qdot + nq;           // [nv]
  double* vn = v + nv;             // [nv]
  double* zero = vn + nv;          // [nv] the velocity of the column evaluations, the acceleration of evaluation 0
  double* tau_app = zero + nv;     // [nv]
  double* rhs = tau_app + nv;      // [nv] tau_applied - c, then a
  double* col = rhs + nv;          // [nv] the pivot column's snapshot
  double* edump = col + nv;        // [nv] write-only row of the surplus groups
  double* ramp = edump + nv;       // [2 nv - 1] zeros around a one in the middle: e_j = ramp + (nv - 1 - j)
  double* etau = ramp + (2 * nv - 1);   // [E][nv]: c, then M column-major (entry (i, j) at Mm[j * nv + i]: plant_step.h's layout)
  int* flag = reinterpret_cast<int*>(etau + E * nv);   // [0] a non-finite value was seen, [1] the failed pivot + 1
  double* mblob = etau + E * nv + 2;    // [M.blob_n] the model tables
  double* xch = mblob + M.blob_n;       // (XCH) the exchange areas of the block's concurrent evaluations
  double* Mm = etau + nv;
  // (PD+) behind the exchange areas
  double* plan = xch + (nt / K) * xch_eval_doubles(M.nxb, M.nstem);   // [A.plan_len]
  double* breaks = plan + (A.pd ? A.plan_len : 0);   // [A.n]
  double* Kp = breaks + A.n;                         // [nu][nq]
  double* Kd = Kp + A.nu * nq;                       // [nu][nv]
  double* nom = Kd + A.nu * nv;                      // [nq | nv | nu] the nominal state and control
  int* act = reinterpret_cast<int*>(nom + nq + nv + A.nu);   // [nu]
  // (LAW) in the same place: there is no plan
  double *Kt = nullptr, *xs = nullptr, *taus = nullptr, *dx = nullptr;
  int* lact = nullptr;
  int nu = 0, n = 0, prob = 0;
  if constexpr (LAW) {
    if (A.status[2 * b] != PLANT_OK) return;   // (ended in an earlier launch of the same call: its words and rows stand)
    nu = T->nu; n = 2 * nv; prob = b / T->R;
    Kt = plan;                 // [nu x n] column-major
    xs = Kt + nu * n;          // [nq | nv]
    taus = xs + nq + nv;       // [nv]
    dx = taus + nv;            // [n]
    lact = reinterpret_cast<int*>(dx + n);   // [nu]
    for (int i = tid; i < nu; i += nt) lact[i] = T->actuated[i];
  }

  double* state = A.state + (size_t)b * ((A.fd ? 0 : 1) + nq + nv);
  for (int i = tid; i < M.blob_n; i += nt) mblob[i] = M.blob[i];
  if (A.fd) {   // (forward dynamics: x = [q, v] of the caller, no time)
    for (int i = tid; i < nq; i += nt) q[i] = state[i];
    for (int i = tid; i < nv; i += nt) v[i] = state[nq + i];
  } else {
    for (int i = tid; i < nq; i += nt) q[i] = state[1 + i];
    for (int i = tid; i < nv; i += nt) v[i] = state[1 + nq + i];
  }
  for (int i = tid; i < nv; i += nt) { tau_app[i] = (LAW || A.pd) ? 0.0 : A.tau[(size_t)b * nv + i]; zero[i] = 0.0; }
  const double t0 = A.fd ? 0.0 : state[0];
  if (A.pd) {
    for (size_t i = tid; i < A.plan_len; i += nt) plan[i] = A.plan[(size_t)b * A.plan_len + i];
    for (int i = tid; i < A.n; i += nt) breaks[i] = A.breaks[i];
    for (int i = tid; i < A.nu * nq; i += nt) Kp[i] = A.Kp[i];
    for (int i = tid; i < A.nu * nv; i += nt) Kd[i] = A.Kd[i];
    for (int i = tid; i < A.nu; i += nt) act[i] = A.actuated[i];
  }
  for (int i = tid; i < 2 * nv - 1; i += nt) ramp[i] = (i == nv - 1) ? 1.0 : 0.0;
  if (tid == 0) { flag[0] = 0; flag[1] = 0; }
  __syncthreads();
  const DevModel Ml = rebase_model(M, mblob);
  // the inputs: every later state is checked before it is committed, the torque is held
  for (int i = tid; i < nq + 2 * nv; i += nt) {
    const double x = (i < nq) ? q[i] : ((i < nq + nv) ? v[i - nq] : tau_app[i - nq - nv]);
    if (!idto_plant::plant_finite(x)) flag[0] = 1;
  }
  __syncthreads();
  int code = flag[0] ? PLANT_NONFINITE : PLANT_OK, done = 0;
  int nsub = A.fd ? 1 : A.substeps, s0 = 0;
  if constexpr (LAW) {   // substeps of the rollout, not of the launch
    s0 = T->first_step * T->m; nsub = (T->first_step + T->steps) * T->m; done = s0;
  }
  const int groups = nt / K, xeval = xch_eval_doubles(Ml.nxb, Ml.nstem);
  for (int s = s0; s < nsub && code == PLANT_OK; ++s) {
    if constexpr (LAW) {
      if (s % T->m == 0) {   // a control step begins: tau_app = tau*_t with u_t = tau*_t[act] - K_t dx on the actuated dofs
        const int t = s / T->m;
        const double* Kg = T->K + ((size_t)prob * T->S + t) * (size_t)(nu * n);
        const double* xg = T->x_nom + ((size_t)prob * (T->S + 1) + t) * (size_t)(nq + nv);
        const double* tg = T->tau_nom + ((size_t)prob * T->S + t) * (size_t)nv;
        for (int i = tid; i < nu * n; i += nt) Kt[i] = Kg[i];
        for (int i = tid; i < nq + nv; i += nt) xs[i] = xg[i];
        for (int i = tid; i < nv; i += nt) taus[i] = tg[i];
        __syncthreads();
        if (tid < 64) {   // (q, v are only read here, as the evaluations read them; tau_app and flag[0] are read behind their barrier)
          const int lane = tid;
          for (int body = lane; body < Ml.nb; body += 64) idto_plant::tangent_sub(Ml.jtype[body], Ml.qstart[body], Ml.vstart[body], q, xs, dx);
          if (lane < nv) { dx[nv + lane] = v[lane] - xs[nq + lane]; tau_app[lane] = taus[lane]; }
          wave_exchange_point();
          if (lane < nu) {
            const double u = taus[lact[lane]] - idto_plant::tvlqr_dot(Kt + lane, nu, dx, 1, n);
            if (!idto_plant::plant_finite(u)) flag[0] = 1;
            tau_app[lact[lane]] = u;
            T->u_out[((size_t)b * T->S + t) * (size_t)nu + lane] = u;
          }
          for (int i = lane; i < n; i += 64) T->dx_out[((size_t)b * (T->S + 1) + t) * (size_t)n + i] = dx[i];   // (n = 2 nv: up to 128)
        }
      }
    }
    if (A.pd) {   // the nominal [q, v, u] at this substep's time, a thread per component (read behind the evaluations' barrier)
      const double t = idto_plant::plant_time(t0, s, A.h) - plan[0];
      for (int j = tid; j < nq + nv + A.nu; j += nt) {
        const int sp = j < nq ? 0 : (j < nq + nv ? 1 : 2), c = j - (sp == 0 ? 0 : (sp == 1 ? nq : nq + nv));
        const int dim = sp == 0 ? nq : (sp == 1 ? nv : A.nu);
        nom[j] = idto_spline::spline_value(breaks, A.n, plan + A.plan_y[sp] + c, plan + A.plan_m[sp] + c, dim, t);
      }
    }
    // ---- the evaluations: lane = (evaluation, path)
    for (int e0 = 0; e0 < E; e0 += groups) {
      const int el = e0 + tid / K, path = tid % K;
      const int ee = (el < E) ? el : 0;
      const bool full = ee == 0;
      double* dst = (el < E) ? etau + ee * nv : edump;
      const double* ev = full ? v : zero;
      const double* ea = full ? zero : ramp + (nv - ee);
      if constexpr (XCH) id_eval<MAXC, true, STEM>(Ml, cp, path, full, q, ev, ea, dst, xch + (tid / K) * xeval);
      else id_eval<MAXC>(Ml, cp, path, full, q, ev, ea, dst);
    }
    __syncthreads();
    if (A.fd && A.bias_out)
      for (int i = tid; i < nv; i += nt) A.bias_out[(size_t)b * nv + i] = etau[i];
    if (A.fd && A.M_out) {   // (before the factorisation overwrites it)
      for (int i = tid; i < nv * nv; i += nt) A.M_out[(size_t)b * nv * nv + i] = Mm[i];
      __syncthreads();
    }
    // ---- the solve and the step, on wavefront 0
    if (tid < 64) {
      const int lane = tid;
      if (A.pd) {   // (tau_app is zero off the actuated dofs since the prologue: plant_pd_plus's scatter)
        if (lane < A.nu)
          tau_app[act[lane]] = idto_plant::plant_pd_plus_row(Kp, Kd, nq, nv, lane, q, v, nom, nom + nq, A.feed_forward != 0, nom + nq + nv);
        wave_exchange_point();
      }
      if (lane < nv) rhs[lane] = tau_app[lane] - etau[lane];
      wave_exchange_point();
      int piv = -1;
      for (int k = 0; k < nv; ++k) {
        const double d = Mm[k * nv + k];
        if (!idto_plant::plant_pivot_ok(d)) { piv = k; break; }
        const bool mine = lane > k && lane < nv;
        if (mine) col[lane] = Mm[k * nv + lane];
        wave_exchange_point();
        if (mine) idto_plant::plant_ldlt_row(Mm, nv, rhs, col, d, k, lane);
        wave_exchange_point();
      }
      if (piv >= 0) {
        if (lane == 0) flag[1] = piv + 1;
      } else {
        if (lane < nv) rhs[lane] = rhs[lane] / Mm[lane * nv + lane];
        wave_exchange_point();
        for (int k = nv - 1; k >= 1; --k) {
          const double xk = rhs[k];
          if (lane < k) idto_plant::plant_ldlt_back_row(Mm, nv, rhs, xk, k, lane);
          wave_exchange_point();
        }
        if (!A.fd) {
          for (int body = lane; body < Ml.nb; body += 64) {
            const int jt = Ml.jtype[body], qs = Ml.qstart[body], vs = Ml.vstart[body];
            const int nqj = idto_plant::plant_joint_nq(jt), nvj = idto_plant::plant_joint_nv(jt);
            for (int i = 0; i < nqj; ++i) qn[qs + i] = q[qs + i];
            for (int i = 0; i < nvj; ++i) vn[vs + i] = v[vs + i];
            idto_plant::plant_advance_body(jt, qs, vs, A.h, qn, vn, rhs, qdot);
            bool ok = true;
            for (int i = 0; i < nqj; ++i) ok = ok && idto_plant::plant_finite(qn[qs + i]);
            for (int i = 0; i < nvj; ++i) ok = ok && idto_plant::plant_finite(vn[vs + i]);
            if (!ok) flag[0] = 1;
          }
        }
      }
    }
    __syncthreads();
    if (flag[1]) code = PLANT_PIVOT;
    else if (flag[0]) code = PLANT_NONFINITE;
    if (code != PLANT_OK || A.fd) break;
    // ---- commit
    const bool rec = A.record && A.record_every > 0 && (s + 1) % A.record_every == 0;
    double* out = rec ? A.record + ((size_t)b * (A.substeps / A.record_every) + (size_t)((s + 1) / A.record_every - 1)) * (nq + nv) : nullptr;
    for (int i = tid; i < nq; i += nt) { const double x = qn[i]; q[i] = x; if (rec) out[i] = x; }
    for (int i = tid; i < nv; i += nt) { const double x = vn[i]; v[i] = x; if (rec) out[nq + i] = x; }
    done = s + 1;
    __syncthreads();
  }
  if constexpr (LAW) {
    if (code == PLANT_OK && done == T->S * T->m) {   // the rollout is complete: the last row of dx, against x*_S
      const double* xg = T->x_nom + ((size_t)prob * (T->S + 1) + T->S) * (size_t)(nq + nv);
      for (int i = tid; i < nq + nv; i += nt) xs[i] = xg[i];
      __syncthreads();
      if (tid < 64) {
        const int lane = tid;
        for (int body = lane; body < Ml.nb; body += 64) idto_plant::tangent_sub(Ml.jtype[body], Ml.qstart[body], Ml.vstart[body], q, xs, dx);
        if (lane < nv) dx[nv + lane] = v[lane] - xs[nq + lane];
        wave_exchange_point();
        for (int i = lane; i < n; i += 64) T->dx_out[((size_t)b * (T->S + 1) + T->S) * (size_t)n + i] = dx[i];
      }
    }
  }
  if (A.fd) {
    if (code == PLANT_OK)
      for (int i = tid; i < nv; i += nt) A.a_out[(size_t)b * nv + i] = rhs[i];
  } else {
    double* tick = A.tick_out ? A.tick_out + (size_t)b * (1 + nq + nv) : nullptr;
    const double t_end = idto_plant::plant_time(t0, done - s0, A.h);
    if (tid == 0) { state[0] = t_end; if (tick) tick[0] = t_end; }
    for (int i = tid; i < nq; i += nt) { state[1 + i] = q[i]; if (tick) tick[1 + i] = q[i]; }
    for (int i = tid; i < nv; i += nt) { state[1 + nq + i] = v[i]; if (tick) tick[1 + nq + i] = v[i]; }
  }
  if (tid == 0) { A.status[2 * b] = code; A.status[2 * b + 1] = done; }
}

// The plant's DevModel and DevContact are read from its parameter record through the constant address space, as
// fd_models_kernel reads its problem's (id_eval.h record_at).
template <int MAXC, bool XCH = false, bool STEM = false>
__global__ void __launch_bounds__(256) plant_kernel(PlantArgs A) {
  const RecordPtr rec = record_at(A.records, (size_t)blockIdx.x * A.mstride);
  plant_body<MAXC, XCH, STEM>(*(const DevModel*)(rec + A.rec_model), *(const DevContact*)(rec + A.rec_contact), A, (int)blockIdx.x);
}

// The law's kernel: plant_body with LAW.  The plant is blockIdx.x; its problem blockIdx.x / R selects the parameter record, K,
// x* and tau*.
template <int MAXC, bool XCH = false, bool STEM = false>
__global__ void __launch_bounds__(256) track_kernel(PlantArgs A, TrackArgs T) {
  const RecordPtr rec = record_at(A.records, (size_t)((int)blockIdx.x / T.R) * A.mstride);
  plant_body<MAXC, XCH, STEM, true>(*(const DevModel*)(rec + A.rec_model), *(const DevContact*)(rec + A.rec_contact), A, (int)blockIdx.x, &T);
}

}  // namespace idto_dev
