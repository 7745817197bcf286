// mpc_batch.h — the two ends of a tick of B model-predictive controllers on a batch context (include/idto_hip.h
// idto_hip_mpc_batch_*): in front of the batch trust-region loop the stored plans are time-shifted into the loop's inputs,
// behind it the loop's result is stored as the next plans.  The arithmetic is csrc/mpc_spline.h - the text the host's
// PiecewiseCubic and ModelPredictiveController compile - so that a tick here is the numbers of B single controllers.
//
// A problem's plan is [start_time | y_q | m_q | y_v | m_v | y_u | m_u]: values and knot derivatives [knot][dim] of the
// three splines of StoredTrajectory (n = num_steps + 1 knots; u: the actuated components of tau).  A context keeps two
// planes of B plans: a tick reads the current plane and writes the other one, and the host makes that one current once
// it knows the tick counted (a loop that timed out leaves every plan as it was).
#pragma once

#include <hip/hip_runtime.h>

#include "batch.h"
#include "mpc_spline.h"
#include "trust_region.h"

namespace idto_dev {

struct MpcPlanLayout {
  int n, nq, nv, nu;   // knots; dims of the q, v, u splines
  __host__ __device__ int dim(int s) const { return s == 0 ? nq : (s == 1 ? nv : nu); }
  __host__ __device__ int dims() const { return nq + nv + nu; }
  __host__ __device__ size_t len() const { return 1 + 2 * (size_t)n * dims(); }
  __host__ __device__ size_t y(int s) const { return 1 + 2 * (size_t)n * (s == 0 ? 0 : (s == 1 ? nq : nq + nv)); }
  __host__ __device__ size_t m(int s) const { return y(s) + (size_t)n * dim(s); }
};

// ---- in front of the loop: grid (1, problem), one workgroup per problem (the shift of q_nom reads the old row 0 of every
// position before any thread overwrites it).  tick: [B][1 + nq + nv] = time, q0, v0 of every problem.
struct MpcShiftArgs {
  MpcPlanLayout L;
  const double* breaks;    // [n]: i * time_step
  const int* selector;     // [nq]: q_nom_relative_to_q_init
  double time_step;
  const double* plan;      // [B][L.len()]: the current plane
  const double* tick;
  double* q; double* v_init; double* q_nom;   // problem 0's (arenas pstride bytes apart)
  size_t pstride;
  double* guess_out;       // [B][n * nq]: the guess again, for the host (the loop overwrites q); may be null
};
// (LDS: nq doubles)
__global__ void mpc_shift_kernel(MpcShiftArgs A) {
  extern __shared__ double mpc_old0[];
  const int b = blockIdx.y, n = A.L.n, nq = A.L.nq, nv = A.L.nv;
  const size_t po = (size_t)b * A.pstride;
  const double* plan = A.plan + (size_t)b * A.L.len();
  const double* tick = A.tick + (size_t)b * (1 + nq + nv);
  const double* q0 = tick + 1;
  const double* v0 = tick + 1 + nq;
  double* q = at_problem(A.q, po);
  double* q_nom = at_problem(A.q_nom, po);
  double* v_init = at_problem(A.v_init, po);
  double* guess = A.guess_out ? A.guess_out + (size_t)b * n * nq : nullptr;
  for (int c = threadIdx.x; c < nq; c += blockDim.x) mpc_old0[c] = q_nom[c];
  __syncthreads();
  // UpdateInitialGuess: row i of the guess is the stored q-spline at (time - start_time) + i * time_step; row 0 is q0
  const double start = tick[0] - plan[0];
  const double* yq = plan + A.L.y(0);
  const double* mq = plan + A.L.m(0);
  for (int e = threadIdx.x; e < n * nq; e += blockDim.x) {
    const int i = e / nq, c = e - i * nq;
    const double g = (i == 0) ? q0[c] : idto_spline::spline_value(A.breaks, n, yq + c, mq + c, nq, idto_spline::guess_time(start, i, A.time_step));
    q[e] = g;
    if (guess) guess[e] = g;
    q_nom[e] = idto_spline::nominal_shift(q_nom[e], A.selector[c] != 0, q0[c], mpc_old0[c]);
  }
  for (int c = threadIdx.x; c < nv; c += blockDim.x) v_init[c] = v0[c];
}

// ---- behind the loop (or from plans the host handed in): one thread per (problem, spline of q / v / u, component);
// adjacent threads take adjacent components of [knot][dim].  grid (ceil(dims / block), problem).
struct MpcStoreArgs {
  MpcPlanLayout L;
  const double* breaks;
  const int* actuated;     // [nu]: the velocity index of every control component
  // where problem b's trajectories are: base + b * stride (bytes); tau rows tau_row doubles apart, row control_row(i)
  const double* q; size_t q_stride;
  const double* v; size_t v_stride;
  const double* tau; size_t tau_stride; int tau_row;
  // (behind the loop) v and tau come from the set of fd_kernel outputs that the problem's TRS_CUR names; null: as given
  const double* state; size_t state_stride; long long alt_off;
  // (behind the loop) the statistics rows [B][nrows]: a problem whose flags carry a TR_ELIGIBLE_MASK bit keeps its plan
  const double* rows; int iterations, nrows;
  const double* times; int times_stride;   // the new start_time of problem b: times[b * times_stride]
  const double* plan_old;  // [B][L.len()]: the current plane
  double* plan_new;        // the other plane (may be the same memory as plan_old: a thread reads only what it writes)
  double* work;            // [B][n * dims]: spline_fit's work space
  double* out;             // [B][L.len()] packed for the host; may be null
};
__global__ void mpc_store_kernel(MpcStoreArgs A) {
  const int b = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = A.L.n, nq = A.L.nq, nv = A.L.nv;
  if (j >= A.L.dims()) return;
  const int s = j < nq ? 0 : (j < nq + nv ? 1 : 2);
  const int c = j - (s == 0 ? 0 : (s == 1 ? nq : nq + nv));
  const int dim = A.L.dim(s);
  const size_t len = A.L.len(), yo = A.L.y(s) + c, mo = A.L.m(s) + c;
  const double* pold = A.plan_old + (size_t)b * len;
  double* pnew = A.plan_new + (size_t)b * len;
  double* out = A.out ? A.out + (size_t)b * len : nullptr;
  int flags = 0;
  if (A.rows) {
    const double* r = A.rows + (size_t)b * A.nrows;
    for (int k = 0; k < A.iterations; ++k) flags |= (int)r[(size_t)k * TRR_COUNT + TRR_FLAGS];
  }
  if (flags & TR_ELIGIBLE_MASK) {   // this controller's re-plan failed: its previous plan stays, in both planes
    for (int i = 0; i < n; ++i) {
      const double y = pold[yo + (size_t)i * dim], m = pold[mo + (size_t)i * dim];
      pnew[yo + (size_t)i * dim] = y; pnew[mo + (size_t)i * dim] = m;
      if (out) { out[yo + (size_t)i * dim] = y; out[mo + (size_t)i * dim] = m; }
    }
    if (j == 0) { const double t0 = pold[0]; pnew[0] = t0; if (out) out[0] = t0; }
    return;
  }
  const size_t set = (A.state && A.alt_off != 0 && at_problem(A.state, (size_t)b * A.state_stride)[IDTO_TRS_CUR] != 0.0) ? (size_t)A.alt_off : 0;
  const double* src;
  int stride;
  if (s == 0) { src = at_problem(A.q, (size_t)b * A.q_stride) + c; stride = nq; }
  else if (s == 1) { src = at_problem(A.v, (size_t)b * A.v_stride + set) + c; stride = nv; }
  else { src = at_problem(A.tau, (size_t)b * A.tau_stride + set) + A.actuated[c]; stride = A.tau_row; }
  for (int i = 0; i < n; ++i) {
    const int row = (s == 2) ? idto_spline::control_row(i, n) : i;
    pnew[yo + (size_t)i * dim] = src[(size_t)row * stride];
  }
  double* w = A.work + (size_t)b * n * A.L.dims() + (size_t)n * (s == 0 ? 0 : (s == 1 ? nq : nq + nv)) + c;
  idto_spline::spline_fit(A.breaks, n, pnew + yo, pnew + mo, w, dim);
  if (out)
    for (int i = 0; i < n; ++i) { out[yo + (size_t)i * dim] = pnew[yo + (size_t)i * dim]; out[mo + (size_t)i * dim] = pnew[mo + (size_t)i * dim]; }
  if (j == 0) { const double t0 = A.times[(size_t)b * A.times_stride]; pnew[0] = t0; if (out) out[0] = t0; }
}

}  // namespace idto_dev
