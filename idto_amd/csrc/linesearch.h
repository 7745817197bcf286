// linesearch.h — the cost along a search direction at many step lengths at once (idto_hip_costs_along): what a
// linesearch iteration (reference optimizer/trajectory_optimizer.cc:1852-1977) asks for one step length at a time, each
// a round trip, are independent evaluations known in advance - alpha_j = rho^j - and one of them is only N workgroups.
//   ls_trial_kernel   candidate j's trial point q + alpha_j dq, formed as the host forms it, into candidate j's arena
//   fd_along_kernel   fd_body's tau-only mode with the candidate in blockIdx.y (fd_kernel.h; fd_along_batch_kernel: the
//                     problem of a batch in blockIdx.z)
//   ls_cost_kernel    cost_body (kernels.h) unchanged, one workgroup per candidate
// Nothing of the resident iterate is written: q, its tau, cost, partials, g, H and the step stay as they are.
// Every kernel here takes the problem of a batch from blockIdx.y (fd_along_batch_kernel: blockIdx.z): the context's arrays
// lie pstride bytes apart (batch.h at_problem), the candidate arenas are laid out [problem][candidate], and every problem
// has its own costs, loop state words, scan, rows and work vectors.  With one problem the strides multiply 0.
#pragma once

#include "kernels.h"
#include "ls_decide.h"
#include "ls_fetch.h"

namespace idto_dev {

// A candidate's arena (doubles; arenas lie `stride` doubles apart, a multiple of 8): what fd_kernel's tau-only mode reads
// and writes and cost_body reads.  tau is kept compact, N rows of nv: fd_kernel and cost_body address row t of it as
// slab + t * slab_stride + 3 nv nq, so the launches get slab = tau - 3 nv nq (`slab`, inside the arena: the 3 nv nq
// doubles in front of tau are reserved for that) and slab_stride = nv.
struct LsArena {
  size_t q, v, a, nplus, slab, tau, cost, stride;
};
__host__ __device__ inline LsArena ls_arena(int N, int nq, int nv) {
  LsArena A;
  A.q = 0;
  A.v = A.q + (size_t)(N + 1) * nq;
  A.a = A.v + (size_t)(N + 1) * nv;
  A.nplus = A.a + (size_t)N * nv;
  A.slab = A.nplus + (size_t)(N + 1) * nv * nq;
  A.tau = A.slab + (size_t)3 * nv * nq;
  A.cost = A.tau + (size_t)N * nv;
  A.stride = (A.cost + 1 + 7) & ~(size_t)7;
  return A;
}

struct LsAlphas { double a[64]; };   // (IDTO_LS_MAX_CANDIDATES step lengths, by value: no upload in front of the launch)

// Candidate blockIdx.x's trial point, as the host forms it (host/trajectory_optimizer.cc ArmijoLinesearch:
// step[j] = alpha * dq[j]; AddToQ(step); NormalizeQuaternions): step = fl(alpha dq_i), then fl(q_i + step) - two
// roundings, the unit is compiled without contraction -, then per quaternion n = sqrt(((w w + x x) + y y) + z z) and four
// divisions by n.  quat[]: the quaternions' start indices within one time step.
// (idto_hip_ls_solve) first: the launch's candidates are [first, first + gridDim.x); gate: a device word, not 0.0 = nothing
// to do; alpha_dev: the one step length of the launch, decided on the device
// (a batch) pstride: bytes between the problems' q and dq; pcstride: doubles between the problems' arenas; gstride:
// doubles between the problems' gate / alpha_dev words
__global__ void __launch_bounds__(256)
ls_trial_kernel(int n, int nq, const double* __restrict__ q, const double* __restrict__ dq, LsAlphas alphas,
                const int* __restrict__ quat, int nquat, double* __restrict__ arenas, size_t stride, int first,
                const double* __restrict__ gate, const double* __restrict__ alpha_dev, size_t pstride, size_t pcstride,
                size_t gstride) {
  const size_t pb = blockIdx.y;
  if (gate && gate[pb * gstride] != 0.0) return;
  q = at_problem(q, pb * pstride); dq = at_problem(dq, pb * pstride);
  const int tid = threadIdx.x, nt = blockDim.x, nsteps = n / nq, cand = first + (int)blockIdx.x;
  const double alpha = alpha_dev ? alpha_dev[pb * gstride] : alphas.a[cand];
  double* qc = arenas + pb * pcstride + (size_t)cand * stride;   // (LsArena::q == 0)
  for (int idx = tid; idx < n; idx += nt) {
    const double step = alpha * dq[idx];
    qc[idx] = q[idx] + step;
  }
  if (nquat <= 0) return;
  __syncthreads();
  for (int idx = tid; idx < nsteps * nquat; idx += nt) {
    const int t = idx / nquat, qs = quat[idx - t * nquat];
    double* qq = qc + (size_t)t * nq + qs;
    const double nrm = __builtin_sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    for (int k = 0; k < 4; ++k) qq[k] /= nrm;
  }
}

// L(candidate first + blockIdx.x) into its arena's cost word and into costs[first + blockIdx.x]
// (a batch) the problem's weights and nominal trajectories pstride bytes on, its arenas pcstride doubles, its costs
// costs_stride doubles and its gate word gstride doubles
__global__ void ls_cost_kernel(DevModel M, DevProblem P, double* __restrict__ arenas, LsArena A, int diag,
                               double* __restrict__ costs, int first, const double* __restrict__ gate, size_t pstride,
                               size_t pcstride, size_t costs_stride, size_t gstride) {
  const size_t pb = blockIdx.y;
  if (gate && gate[pb * gstride] != 0.0) return;
  const int cand = first + (int)blockIdx.x;
  double* base = arenas + pb * pcstride + (size_t)cand * A.stride;
  (void)cost_body(M.nq, M.nv, at_problem(P, pb * pstride), base + A.q, base + A.v, base + A.slab, M.nv, base + A.cost, diag,
                  nullptr, costs + pb * costs_stride + cand, TrDecideArgs{});
}

// ---------------------------------------------------------------------------
// The linesearch loop on the device (idto_hip_ls_solve; reference SolveWithLinesearch, optimizer/trajectory_optimizer.cc:
// 2244-2407, with scaling off and no enforced constraints).  Per iteration, behind the launches of the Newton step:
//   ls_prepare_kernel   L' = g.dq, |g|, |dq|, |h|, the throw condition and the early-outs (ls_decide.h ls_begin)
//   per wave of candidates [a, b): ls_trial_kernel, fd_kernel (tau only), ls_cost_kernel - each returns at its first
//                       instruction once the iteration is decided - and ls_scan_kernel, which feeds the wave's costs to the
//                       scan in index order
//   the accepted step   ls_trial_kernel at the decided alpha (backtracking answers alpha / rho, which is not bit for bit a
//                       candidate's), fd_kernel, ls_cost_kernel and ls_finish_kernel: the trust ratio, the statistics row,
//                       q <- q + alpha dq
// No kernel waits for another workgroup: launch order carries every dependency.
// (idto_hip_ls_solve_batch_fetch) The same launches for the problems of a batch side by side, the problem in the grid: every
// problem has its own state words, so its own gate and stop - a problem that has decided, or that carries a flag, idles while
// the others go on -, and ls_gather_batch_kernel packs what goes back to the host (ls_fetch.h).
enum {
  LSS_COST = 0,   // L(q_k)
  LSS_ALPHA,      // the iteration's answer
  LSS_ITERS,
  LSS_LPRIME,
  LSS_GNORM,
  LSS_DQNORM,
  LSS_HNORM,
  LSS_GATE,       // not 0.0: the iteration's waves have nothing left to do
  LSS_STOP,       // not 0.0: the remaining iterations are idle (the flags that stopped the loop)
  LSS_ROWS,       // rows appended so far
  LSS_COUNT = 16
};
enum {   // a row of statistics (idto_hip.h IDTO_LS_ROW)
  LSR_COST = 0, LSR_ALPHA, LSR_ITERS, LSR_RATIO, LSR_QNORM, LSR_DQNORM, LSR_GNORM, LSR_LPRIME, LSR_HNORM, LSR_COST_NEW,
  LSR_CLOCK, LSR_FLAGS, LSR_COUNT
};
enum { LSF_NOT_FINITE = 2, LSF_NOT_DESCENT = 4, LSF_BAD_PIVOT = 32, LSF_LIMIT = 64, LSF_UNDECIDED = 128 };

struct LsLoopArgs {
  int n, nq, nv, N;            // n = (N + 1) nq
  const double *g, *dq;        // the gradient and the Newton step at q_k
  const double *HA, *HB, *HC;  // the Hessian's lower bands (blocks column-major)
  const double* slab; int slab_stride, tau_off;   // tau of q_k: slab + t slab_stride + tau_off
  const int* dofs; int nu;     // the unactuated dofs (|h| of the statistics)
  double* q;                   // the iterate
  double* cost;                // the context's cost word
  double* state;               // [LSS_COUNT]
  idto_ls::LsScan* scan;
  double* rows;                // [iterations][LSR_COUNT]
  double* work;                // [2 n]
  const double* arena;         // the accepted step's arena (q + alpha dq and its cost)
  size_t arena_cost;
  const unsigned* status; unsigned fact_id;   // the solver's status words (host-mapped) and this iteration's factorisation
  int method, max_iters;
  double dt;
  // (a batch: the pointers above are problem 0's) bytes between the problems' context arrays; doubles between their rows,
  // their candidate costs and their arenas.  state, scan and work lie LSS_COUNT, one LsScan and 2 n apart.
  size_t pstride, rows_stride, costs_stride, pcstride;
};

// problem pb's view of the loop's arguments
__device__ inline LsLoopArgs ls_at_problem(LsLoopArgs A, size_t pb) {
  const size_t o = pb * A.pstride;
  A.g = at_problem(A.g, o); A.dq = at_problem(A.dq, o);
  A.HA = at_problem(A.HA, o); A.HB = at_problem(A.HB, o); A.HC = at_problem(A.HC, o);
  A.slab = at_problem(A.slab, o); A.q = at_problem(A.q, o); A.cost = at_problem(A.cost, o);
  A.state += pb * LSS_COUNT; A.scan += pb; A.rows += pb * A.rows_stride; A.work += pb * 2 * (size_t)A.n;
  A.arena += pb * A.pcstride;
  if (A.status) A.status += 2 * pb;   // (the solvers' status words: [2 b] the id of problem b's last failing factorisation)
  return A;
}

__device__ inline void ls_stop_row(const LsLoopArgs& A, int flags) {
  double* S = A.state;
  double* R = A.rows + (size_t)S[LSS_ROWS] * LSR_COUNT;
  for (int i = 0; i < LSR_COUNT; ++i) R[i] = 0.0;
  R[LSR_COST] = S[LSS_COST]; R[LSR_DQNORM] = S[LSS_DQNORM]; R[LSR_GNORM] = S[LSS_GNORM]; R[LSR_LPRIME] = S[LSS_LPRIME];
  R[LSR_HNORM] = S[LSS_HNORM]; R[LSR_CLOCK] = (double)wall_clock64(); R[LSR_FLAGS] = (double)flags;
  S[LSS_ROWS] += 1.0; S[LSS_STOP] = (double)flags; S[LSS_GATE] = 1.0;
}

// The sums are the host's Dot / Norm: one thread each, in index order.
__global__ void __launch_bounds__(256) ls_prepare_kernel(LsLoopArgs A0) {
  const LsLoopArgs A = ls_at_problem(A0, blockIdx.y);
  double* S = A.state;
  if (S[LSS_STOP] != 0.0) return;
  __shared__ double sums[4];
  const int tid = threadIdx.x;
  if (tid == 0) { double s = 0; for (int i = 0; i < A.n; ++i) s += A.g[i] * A.dq[i]; sums[0] = s; }
  if (tid == 64) { double s = 0; for (int i = 0; i < A.n; ++i) s += A.g[i] * A.g[i]; sums[1] = s; }
  if (tid == 128) { double s = 0; for (int i = 0; i < A.n; ++i) s += A.dq[i] * A.dq[i]; sums[2] = s; }
  if (tid == 192) {
    double s = 0;
    for (int t = 0; t < A.N; ++t)
      for (int j = 0; j < A.nu; ++j) {
        const double h = A.slab[(size_t)t * A.slab_stride + A.tau_off + A.dofs[j]];
        s += h * h;
      }
    sums[3] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  S[LSS_LPRIME] = sums[0]; S[LSS_GNORM] = __builtin_sqrt(sums[1]); S[LSS_DQNORM] = __builtin_sqrt(sums[2]);
  S[LSS_HNORM] = __builtin_sqrt(sums[3]);
  int flags = 0;
  if (A.status && A.status[0] == A.fact_id) flags |= LSF_BAD_PIVOT;
  idto_ls::LsScan sc = idto_ls::ls_begin(A.method, S[LSS_COST], sums[0], A.dt, A.max_iters);
  if (!flags && sc.status == idto_ls::LS_NOT_DESCENT) {
    flags |= LSF_NOT_DESCENT;
    if (!(__builtin_fabs(sums[2]) <= 1.7976931348623157e308)) flags |= LSF_NOT_FINITE;
  }
  *A.scan = sc;
  S[LSS_ALPHA] = sc.alpha; S[LSS_ITERS] = (double)sc.ls_iters;
  if (flags) { ls_stop_row(A, flags); return; }
  S[LSS_GATE] = (sc.status != idto_ls::LS_UNDECIDED) ? 1.0 : 0.0;
}

// costs[first .. first + count) into the scan, in index order; last: no wave follows
__global__ void ls_scan_kernel(LsLoopArgs A0, const double* __restrict__ costs, int first, int count, int last) {
  const LsLoopArgs A = ls_at_problem(A0, blockIdx.y);
  costs += (size_t)blockIdx.y * A.costs_stride;
  double* S = A.state;
  if (threadIdx.x != 0 || S[LSS_GATE] != 0.0) return;
  idto_ls::LsScan sc = *A.scan;
  idto_ls::ls_scan(&sc, costs + first, count);
  *A.scan = sc;
  if (sc.status != idto_ls::LS_UNDECIDED) {
    S[LSS_ALPHA] = sc.alpha; S[LSS_ITERS] = (double)sc.ls_iters; S[LSS_GATE] = 1.0;
  } else if (last) {
    ls_stop_row(A, LSF_UNDECIDED);
  }
}

// The accepted step: the trust ratio (CalcTrustRatio, :1979-2035, with scaling off) - H step per element in the order of
// PentaDiagonalMatrix::MultiplyBy (y = 0, then the blocks A_i, B_i, C_i, D_i = B_{i+1}^T, E_i = A_{i+2}^T, columns in order;
// C's upper triangle is the mirror of its lower one), the two dot products by one thread each in index order -, the row,
// q <- q + alpha dq.
__global__ void __launch_bounds__(256) ls_finish_kernel(LsLoopArgs A0) {
  const LsLoopArgs A = ls_at_problem(A0, blockIdx.y);
  double* S = A.state;
  if (S[LSS_STOP] != 0.0) return;
  __shared__ double sums[3];
  const int tid = threadIdx.x, nt = blockDim.x, k = A.nq, nb = A.n / A.nq, kk = k * k;
  const double alpha = S[LSS_ALPHA];
  double* step = A.work;
  double* Hs = A.work + A.n;
  for (int idx = tid; idx < A.n; idx += nt) step[idx] = alpha * A.dq[idx];
  __syncthreads();
  for (int idx = tid; idx < A.n; idx += nt) {
    const int i = idx / k, r = idx - i * k;
    double y = 0.0;
    if (i >= 2) { const double* M = A.HA + (size_t)i * kk; const double* x = step + (size_t)(i - 2) * k; for (int c = 0; c < k; ++c) y += M[c * k + r] * x[c]; }
    if (i >= 1) { const double* M = A.HB + (size_t)i * kk; const double* x = step + (size_t)(i - 1) * k; for (int c = 0; c < k; ++c) y += M[c * k + r] * x[c]; }
    { const double* M = A.HC + (size_t)i * kk; const double* x = step + (size_t)i * k; for (int c = 0; c < k; ++c) y += ((r < c) ? M[r * k + c] : M[c * k + r]) * x[c]; }
    if (i + 1 < nb) { const double* M = A.HB + (size_t)(i + 1) * kk; const double* x = step + (size_t)(i + 1) * k; for (int c = 0; c < k; ++c) y += M[r * k + c] * x[c]; }
    if (i + 2 < nb) { const double* M = A.HA + (size_t)(i + 2) * kk; const double* x = step + (size_t)(i + 2) * k; for (int c = 0; c < k; ++c) y += M[r * k + c] * x[c]; }
    Hs[idx] = y;
  }
  __syncthreads();
  if (tid == 0) { double s = 0; for (int i = 0; i < A.n; ++i) s += A.g[i] * step[i]; sums[0] = s; }
  if (tid == 64) { double s = 0; for (int i = 0; i < A.n; ++i) s += step[i] * Hs[i]; sums[1] = s; }
  if (tid == 128) { double s = 0; for (int i = 0; i < A.n; ++i) s += A.arena[i] * A.arena[i]; sums[2] = s; }
  __syncthreads();
  for (int idx = tid; idx < A.n; idx += nt) A.q[idx] = A.arena[idx];
  if (tid != 0) return;
  const double L = S[LSS_COST], L_new = A.arena[A.arena_cost];
  const double hessian_term = 0.5 * sums[1], gradient_term = sums[0];
  const double predicted = -gradient_term - hessian_term, actual = L - L_new;
  const double eps = 10 * idto_ls::kEps / A.dt / A.dt;
  const double ratio = (predicted < eps && actual < eps) ? 0.5 : actual / predicted;
  const int iters = (int)S[LSS_ITERS];
  const int flags = idto_ls::ls_limit_reached(iters, A.max_iters) ? LSF_LIMIT : 0;
  double* R = A.rows + (size_t)S[LSS_ROWS] * LSR_COUNT;
  R[LSR_COST] = L; R[LSR_ALPHA] = alpha; R[LSR_ITERS] = (double)iters; R[LSR_RATIO] = ratio;
  R[LSR_QNORM] = __builtin_sqrt(sums[2]); R[LSR_DQNORM] = S[LSS_DQNORM]; R[LSR_GNORM] = S[LSS_GNORM];
  R[LSR_LPRIME] = S[LSS_LPRIME]; R[LSR_HNORM] = S[LSS_HNORM]; R[LSR_COST_NEW] = L_new;
  R[LSR_CLOCK] = (double)wall_clock64(); R[LSR_FLAGS] = (double)flags;
  S[LSS_ROWS] += 1.0; S[LSS_COST] = L_new; *A.cost = L_new;
  if (flags) S[LSS_STOP] = (double)flags;
}

// idto_hip_ls_solve_batch_fetch: problem blockIdx.y's [rows | q | v | tau] and its final cost packed into the staging
// buffer (ls_fetch.h) - one launch, one copy to the host behind it.  tau: row t of the slab at slab + t slab_stride + tau_off.
struct LsGatherArgs {
  const double *state, *rows, *q, *v, *slab;
  int N, nv, slab_stride, tau_off;
  size_t pstride, rows_stride;
  idto_fetch::LsFetchLayout L;
  double* out;
};
__global__ void __launch_bounds__(256) ls_gather_batch_kernel(LsGatherArgs G) {
  const size_t pb = blockIdx.y, o = pb * G.pstride;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  using idto_fetch::LsFetchLayout;
  const double* rows = G.rows + pb * G.rows_stride;
  const double* q = at_problem(G.q, o);
  const double* v = at_problem(G.v, o);
  const double* slab = at_problem(G.slab, o);
  double* out = G.out;
  if (tid == 0) out[G.L.final_cost() + pb] = G.state[pb * LSS_COUNT + LSS_COST];
  for (size_t i = tid; i < G.L.nrows; i += nt) out[G.L.rows(pb) + i] = rows[i];
  for (size_t i = tid; i < G.L.cnt[LsFetchLayout::Q]; i += nt) out[G.L.part(pb, LsFetchLayout::Q) + i] = q[i];
  for (size_t i = tid; i < G.L.cnt[LsFetchLayout::V]; i += nt) out[G.L.part(pb, LsFetchLayout::V) + i] = v[i];
  for (size_t i = tid; i < G.L.cnt[LsFetchLayout::TAU]; i += nt) {
    const size_t t = i / (size_t)G.nv, j = i - t * (size_t)G.nv;
    out[G.L.part(pb, LsFetchLayout::TAU) + i] = slab[t * (size_t)G.slab_stride + G.tau_off + j];
  }
}

}  // namespace idto_dev
