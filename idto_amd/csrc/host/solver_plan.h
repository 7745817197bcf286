// solver_plan.h — which kernel factorises a given banded system, with which block size, split, grid and LDS carve-up:
// one decision, made here, as a pure function of (block size, horizon, batch, options).  Host-only C++ (no HIP include):
// idto_hip.hip fills arguments and launches what the plan names; tests/cpp/solver_plan_check.cc sweeps it on the CPU.
#pragma once

#include <cstddef>
#include <string>

namespace idto_host {

// What the decision reads from a context, and nothing else.
struct SolverShape {
  int k = 0, N = 0, batch = 1;   // block size (nq; a KKT context: nq + nu), horizon, problems
  int npos = 0;                  // > 0: a KKT system whose pivots [npos, k) of a block are negative (ldl_npos)
  bool h_assembled = false;      // block row 0 is the identity: the solvers start at row 1
  bool two_sided = true, solver_nd = true, solver_pipe = true;   // the options of the same names
  int solver_band = 1, nd_min_rows = 16, nd_recursion = 1;
  bool has_wst = false;          // the seven-workgroup kernel's W-row buffer exists (SolverBufferCounts: blocks of 21 .. 32)
  int asm_terms_lds = 0, cost_lds = 0;   // LDS of the assembly / the decision, for the launches that carry them
};

struct SolveRequest {
  enum Kind {
    ONE_SIDED,    // the factorisation in one workgroup
    SOLVE,        // nrhs = 1: any kernel; nrhs > 1: the factors alone (two-workgroup kernel), penta_apply_kernel substitutes
    WHOLE_STEP,   // gn_small.h: evaluation, assembly and band solve in one workgroup per problem
  };
  Kind kind = SOLVE;
  int nrhs = 1;
  int step_nq = 0, step_fast_n = 0;   // WHOLE_STEP: the model's nq and the length of its gathered records (gn_small_doubles)
};

// the kernel a plan names = the context's last_solver code (3: the reference LU, 5: the fused launch - not planned here)
enum SolverKind {
  SOLVER_LDL = 1,    // penta_ldl_kernel: one or two workgroups
  SOLVER_ND = 2,     // penta_nd_kernel: nested dissection, seven workgroups
  SOLVER_PIPE = 4,   // penta_pipe_kernel: pipelined chains, five workgroups
  SOLVER_BAND = 6,   // penta_band_kernel: the scalar band factorisation, one workgroup
  SOLVER_SMALL = 7,  // gn_small_kernel: the whole step
};

struct SolverPlan {
  int kind = 0;
  // Geometry of one launch of the banded block LDL^T solver (one right-hand side in the kernel; more
  // go through penta_apply_kernel).
  int r0 = 0, n = 0, k = 0, K = 0, gj_waves = 0, lds = 0, m_split = 0;
  int lds_full = 0;   // the chain code's carve-up with every row of the system (nested dissection, fused launch: their own row counts)
  size_t qq0 = 0;
  // the dissection (SOLVER_ND, SOLVER_PIPE): separator rows s, s+1; join rows j1, j1+1 and j2, j2+1; the longest chain,
  // the local rows its carve-up holds, the recursion-form back substitution's wavefront count (0: row by row)
  int s = 0, j1 = 0, j2 = 0, nloc_max = 0, lds_rows = 0, rec_tail = 0;
  int grid = 0, threads = 0;   // the solver's own workgroups per problem, threads per workgroup
  // a SOLVE with one right-hand side: can this launch also assemble g and the bands (4 (N + 1) more workgroups) and
  // decide on the trust-region loop's trial point (one more)?  With the LDS such a launch asks for.
  bool can_assemble = false, can_decide = false;
  int lds_assemble = 0, lds_decide = 0;
  int lds_small = 0;   // SOLVER_SMALL: doubles of the band solver's carve-up in front of gn_small_kernel's own arrays
  // nrhs > 1: penta_apply_kernel's block size and LDS
  int apply_K = 0, apply_lds = 0;
};

// 0, or -1 with *err: no kernel serves the request (WHOLE_STEP: the step takes the separate launches)
int PlanSolve(const SolverShape& shape, const SolveRequest& request, SolverPlan* plan, std::string* err);

// Rows the fast solver works on.  The assembled Gauss-Newton Hessian has C_0 = I, B_1 = A_2 = 0
// and g_0 = 0 (q_0 is not a decision variable, TO.cc:1093-1165): block row 0 is decoupled, so the
// factorisation starts at row 1 (one block row less on the serial chain of the top workgroup)
// and x_0 = rhs_0.  Bands written into the context behind the API's back get the full system.
inline int SolverFirstRow(bool h_assembled, int N) { return (h_assembled && N >= 2) ? 1 : 0; }
// the factorisation's padded block size (single_rhs_only: the sizes without a penta_apply_kernel count)
int SolverBlockSize(int k, bool single_rhs_only = false);
// penta_apply_kernel: LDS for n block rows of K (the right-hand side of each of its four wavefronts, the chains' exchange)
int ApplyLds(int n, int K);

// Element counts of the solver-only arrays of a context with blocks of K and horizon N (where they lie in the arena of the
// model's context and of the KKT context: host/context_layout.h IDTO_MODEL_ARENA, IDTO_KKT_ARENA).
struct SolverBuffers {
  size_t bands;        // HA | HB | HC in one allocation, two extra zero blocks each (five are reserved)
  size_t factors;      // each of Ust, Hst, Est: padded blocks of 32 x 36
  size_t dinv;         // Dst
  size_t dbg;          // cycle stamps (8 per block row)
  size_t xch_count;    // one producer / joiner pair's exchange: 2 augmented blocks + [2][K] ...
  size_t xch;          // ... two pairs (the nested-dissection kernels)
  size_t flags;
  size_t rowcnt;       // each of the two kernels' per-row release counters: [4][ND_MAXROWS]
  size_t nd_buf;       // nd_layout
  bool has_wst;
  size_t nd_wst;       // the seven-workgroup kernel's W rows, blocks of 21 .. 32 only (else 1)
  size_t apply_t;      // Tst: column-major copies of the factor blocks (penta_apply.h), allocated on first use
};
SolverBuffers SolverBufferCounts(int K, int N);

// The linesearch loop's waves (idto_hip_ls_solve): how many candidate step lengths each launch set evaluates, a pure
// function of (horizon, compute units, method, max_linesearch_iterations).  One candidate is N workgroups of one wavefront:
// the first wave takes as many candidates as give every compute unit one workgroup, every further wave twice its
// predecessor - most linesearches end within the first two waves, and a late one costs launches, not a device full of
// evaluations nobody reads.  Armijo never looks past max_linesearch_iterations candidates; backtracking is not bounded by it
// and gets all kLsMaxCandidates.  override_width > 0 (option "ls_waves"): that many candidates in every wave.
// Returns the number of waves; widths[i] > 0, their sum is the number of candidates, in index order.
constexpr int kLsMaxCandidates = 64;
int PlanLsWaves(int N, int compute_units, int method, int max_linesearch_iterations, int override_width,
                int widths[kLsMaxCandidates]);

}  // namespace idto_host
