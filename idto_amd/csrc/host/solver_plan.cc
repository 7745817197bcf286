// solver_plan.cc — see solver_plan.h.  Plain C++: the layouts come from solver_layout.h, which the kernels include too.
#include "host/solver_plan.h"

#include <algorithm>
#include <cstdlib>

#include "fd_sizes.h"
#include "solver_layout.h"

namespace idto_host {
using namespace idto_dev;

namespace {
constexpr int kMaxLds = kMaxDynamicLds;   // (fd_sizes.h: the one limit of every kernel of the library)

int Fail(std::string* err, const char* what) {
  if (err) *err = what;
  return -1;
}

// Nested dissection (penta_nd.h): seven workgroups - two producer / joiner pairs, two spike
// workgroups, the separator.  Its factors are not what penta_apply_kernel walks, so it serves the
// single-right-hand-side solves only (the Gauss-Newton step).
// separator in the middle; in each half the joiner chain (next to the separator) gets the extra row
struct NdSplit { int s, j1, j2; };
// Pipelined chains (penta_pipe.h): a joiner's block row costs ~1.35x a producer's (its spike wavefronts share the
// SIMDs) and its two join rows come after the producer's hand-over, so the producers take ~57% of the rows that are
// not join rows: both sides then reach the join together (measured at K = 19: 2.56 / 3.45 us per row).
NdSplit nd_split(int n, bool pipe, int K) {
  NdSplit sp;
  sp.s = (n - 2) / 2;
  const int htop = sp.s, hbot = n - sp.s - 2;
  auto producer_rows = [&](int half) {
    if (!pipe) {
      // (seven workgroups.  Measured: producer done at 0.6 + (np + 2) t, joiner at the join at 0.6 + d + (half - np - 2) t'
      // with t = 4.2, t' = 4.53, d = 6.3 us at K = 23 (the joiner publishes every row and starts later) and t = 6.2,
      // t' = 6.3, d = 8.5 at K = 29: both sides meet at np = (half - 2) / 2 + 0.27 resp. - 0.24 rows.  An odd
      // half - 2 (every even n) therefore rounds UP at K = 23 - allegro N = 60: 67.7 / 66.6 us instead of 63.6 / 70.3 -
      // and down at K = 29 - N = 40: 62 / 66 instead of 68 / 59.5.)
      static const int extra = [] { const char* e = std::getenv("IDTO_ND_PRODUCER_EXTRA"); return e ? std::atoi(e) : -1; }();   // (measurement aid)
      const int np = extra >= 0 ? (half - 2) / 2 + extra : (half - 2 + (K > 20 && K <= 24 ? 1 : 0)) / 2;
      return std::max(1, std::min(np, half - 3));
    }
    static const double share = [] { const char* e = std::getenv("IDTO_PIPE_SPLIT"); return e ? std::atof(e) : 0.52; }();   // (measurement aid)
    int np = (int)(share * (half - 2) + 0.6);
    return std::max(1, std::min(np, half - 3));
  };
  sp.j1 = producer_rows(htop);                     // producer P0: rows 0 .. j1-1
  sp.j2 = n - producer_rows(hbot) - 2;             // producer P3: rows j2+2 .. n-1
  return sp;
}
int NdLongestChain(const NdSplit& sp, int n) { return std::max(std::max(sp.s - sp.j1, sp.j2 - sp.s), std::max(sp.j1, n - sp.j2 - 2)); }
// (the chains keep the right-hand side and rt / x of their own rows: joiner nloc, producer nloc + 2 pseudo-rows, + 2 spare)
int NdChainRows(int nloc_max) { return nloc_max + 4; }
int NdLds(const SolverPlan& p, int nloc_max) {
  const int ks = ldl_ks(p.K), NF = 2 * p.K, KP = 4 * ((p.K + 3) / 4);
  const int chain = penta_ldl_layout(p.n, p.K, 1, NdChainRows(nloc_max)).end * (int)sizeof(double);
  const int spike = (3 * NF * ks + 3 * KP * ks + 3 * p.K * p.K + 2 * ks + 4) * (int)sizeof(double);
  const int sep = nd_sep_lds_doubles(p.K) * (int)sizeof(double);
  return std::max(std::max(spike, sep), chain);
}
bool NdPipelined(const SolverShape& c, const SolverPlan& p) { return c.solver_pipe && p.K <= 20; }
bool NdEligible(const SolverShape& c, const SolverPlan& p) {
  // (the 8 x 8 instantiation is unpadded: the KKT systems' - spinner_capsule's 7 + 1 - not a padded H's)
  const bool inst = SolverInstantiated(FAM_ND, p.K) && (p.K != 8 || c.npos > 0) && p.K == p.k;
  // (seven workgroups per problem, one per CU: a batch that would not fit the 256 CUs at once is
  // better served by the two-workgroup form - same work per problem on fewer CUs)
  // (horizons from nd_min_rows block rows on - option "nd_min_rows", 16: the MPC examples plan over 20 steps, and the
  // one-launch iteration that serves shorter systems takes 99 us for the cheetah there against 21 + ~40 of fd_kernel and
  // the pipelined solver.  The seven-workgroup kernel keeps 24: its chains of 4 - 5 rows buy nothing below that.)
  const bool pipe_kernel = NdPipelined(c, p);
  if (!(c.solver_nd && c.two_sided && inst && p.n >= (pipe_kernel ? c.nd_min_rows : std::max(24, c.nd_min_rows)) && 7 * c.batch <= 256)) return false;
  // the joiner chains' per-row tables hold ND_MAXROWS local rows: longer horizons (n >= 127) take the
  // two-workgroup factorisation
  const int nloc_max = NdLongestChain(nd_split(p.n, pipe_kernel, p.K), p.n);
  return nloc_max <= ND_MAXROWS && NdLds(p, nloc_max) <= kMaxLds;
}

// The scalar band factorisation (penta_band.h): blocks up to 5 (half width 3 k - 1 <= 14: a lane per diagonal in a row
// of 16), one workgroup per problem, single right-hand side.
bool BandEligible(const SolverShape& c, const SolverPlan& p, bool whole_step = false) {
  // (option solver_band: 0 off, 1 blocks up to 4 - at 5 the pipelined kernel is faster, 41 against 47 us for hopper -, 2 up to 5)
  if (!(c.solver_band > 0 && c.two_sided && p.K == p.k && p.k >= 2 && p.k <= (c.solver_band > 1 ? 5 : 4))) return false;
  const int M = p.n * p.k, W = 3 * p.k;
  // (a batch: two wavefronts per problem shorten ONE problem's solve; with many in flight the five workgroups' work per
  // problem is what counts - 64 spinner problems 554k against 567k it/s, 256: 747k / 782k; acrobot 649k / 619k)
  // (gn_small.h - `whole_step` - is one workgroup per problem for EVERYTHING: there the batch argument points the other
  // way, 64 acrobot problems 650k -> 2.89M it/s)
  if (c.batch > 1 && c.solver_band < 2 && p.k > 2 && !whole_step) return false;
  // (horizons the pipelined kernel would take: shorter ones keep the fused launch / the two-workgroup factorisation)
  return p.n >= c.nd_min_rows && M >= 4 * W && band_layout(M, W).end * (int)sizeof(double) <= kMaxLds;
}

// pipe_layout<K>(n, true).end / pipe_recursion_tail_fits<K> of an instantiated size, 0 / -1 without one
int PipeLdsDoubles(int K, int n) {
  switch (K) {
#define IDTO_X(KM) case KM: return pipe_layout<KM>(n, true).end;
    IDTO_PIPE_KERNELS(IDTO_X)
#undef IDTO_X
  }
  return 0;
}
// (the seven-workgroup kernel's chains take the recursion form from blocks of 21 on: penta_nd.h's RECT)
int RecursionTailFits(int K, int lds_doubles, int nloc_joiner, int nloc_producer) {
  switch (K) {
#define IDTO_X(KM) case KM: return KM > 20 ? pipe_recursion_tail_fits<KM>(lds_doubles, nloc_joiner, nloc_producer) : 0;
    IDTO_ND_KERNELS(IDTO_X)
#undef IDTO_X
  }
  return 0;
}

// gn_small.h: fd + assembly + band solve of a small all-revolute model in ONE workgroup per problem.
// (p: the plan of the system the launch solves - H's, or the KKT context's with blocks of nq + nu)
int SmallLds(const SolverShape& c, const SolveRequest& rq, const SolverPlan& p, int* lds_small) {
  int band = band_layout(p.n * p.k, 3 * p.k).end;
  band += band & 1;
  if (lds_small) *lds_small = band;
  return (band + gn_small_doubles(c.N, rq.step_nq, rq.step_fast_n, p.k)) * (int)sizeof(double);
}
}  // namespace

int SolverBlockSize(int k, bool single_rhs_only) {
  // block sizes of the reference's example models are instantiated exactly, others are padded
  // (30: the factorisation alone - no penta_apply_kernel of that size -, for the KKT systems of kkt.h: allegro's 23 + 6.
  // The 32 x 32 instantiation needs three elimination wavefronts and spills 378 registers.)
  if (single_rhs_only && (k == 29 || k == 4)) return k;   // (exact instantiations for the KKT systems of allegro and spinner)
  if (single_rhs_only && k > 24 && k <= 30) return 30;
  return (k == 2 || k == 3 || k == 5 || k == 19 || k == 23) ? k : (k <= 8 ? 8 : k <= 16 ? 16 : k <= 24 ? 24 : 32);
}

int ApplyLds(int n, int K) { return 4 * (n * K + 4 * 64 + 2) * (int)sizeof(double); }   // (per column: rt of every row, the chains' exchange)

int PlanSolve(const SolverShape& c, const SolveRequest& rq, SolverPlan* p, std::string* err) {
  *p = SolverPlan{};
  const bool one_sided = rq.kind == SolveRequest::ONE_SIDED;
  if (rq.kind == SolveRequest::SOLVE && rq.nrhs < 1) return Fail(err, "nrhs < 1");
  p->r0 = SolverFirstRow(c.h_assembled, c.N);
  p->n = c.N + 1 - p->r0;
  p->k = c.k;
  p->qq0 = (size_t)p->r0 * p->k * p->k;
  if (p->k < 1 || p->k > 32) return Fail(err, "fast solver supports nq <= 32");
  p->K = SolverBlockSize(p->k, c.npos > 0);
  const int per_wave = 64 - p->K, ncr = 2 * p->K + 1;
  p->gj_waves = (ncr + per_wave - 1) / per_wave;
  // two-sided elimination (two workgroups meeting at block rows m, m+1) once the horizon is long
  // enough to pay for the hand-over
  p->m_split = (c.two_sided && !one_sided && p->n >= 10) ? (p->n - 1) / 2 : 0;
  // (a workgroup of the two-sided elimination keeps the right-hand side and rt / x of its own rows only)
  p->lds = penta_ldl_layout(p->n, p->K, 1, ldl_two_sided_rows(p->n, p->m_split, 1)).end * (int)sizeof(double);
  p->lds_full = penta_ldl_layout(p->n, p->K, 1).end * (int)sizeof(double);
  if (p->lds > kMaxLds) return Fail(err, "right-hand sides do not fit the LDS carve-up");
  // the two workgroups must not share a CU (each is one wavefront per SIMD, issue-bound): ask for
  // more than half of the 160 KB LDS so that the dispatcher cannot co-locate them
  if (p->m_split > 0) p->lds = std::max(p->lds, 84 * 1024);
  if (p->lds > kMaxLds) return Fail(err, "LDS carve-up too large");
  p->threads = 256;

  if (rq.kind == SolveRequest::WHOLE_STEP) {
    // What the launch stands in for must be what the two launches would have run: the scalar band factorisation of the
    // assembled system (BandEligible), from row 1 on.
    if (!(c.N >= 2 && BandEligible(c, *p, true) && p->r0 == 1)) return Fail(err, "gn_small: not a system of the scalar band factorisation");
    p->lds = SmallLds(c, rq, *p, &p->lds_small);
    if (p->lds > kMaxLds) return Fail(err, "gn_small: LDS carve-up too large");
    if (!SolverInstantiated(FAM_BAND, 3 * p->k)) return Fail(err, "no penta_band_kernel of this block size");
    p->kind = SOLVER_SMALL; p->grid = 1;
    return 0;
  }

  const bool any_kernel = rq.kind == SolveRequest::SOLVE && rq.nrhs == 1;
  const bool band = any_kernel && BandEligible(c, *p), nd = any_kernel && NdEligible(c, *p);
  if (band) {
    if (!SolverInstantiated(FAM_BAND, 3 * p->k)) return Fail(err, "no penta_band_kernel of this block size");
    p->kind = SOLVER_BAND; p->grid = 1;
    p->lds = band_layout(p->n * p->k, 3 * p->k).end * (int)sizeof(double);
  } else if (nd) {
    const bool pipe = NdPipelined(c, *p);
    const NdSplit sp = nd_split(p->n, pipe, p->K);
    p->s = sp.s; p->j1 = sp.j1; p->j2 = sp.j2;
    p->nloc_max = NdLongestChain(sp, p->n);
    p->lds_rows = NdChainRows(p->nloc_max);
    const int lds = NdLds(*p, p->nloc_max);
    if (pipe) {
      // pipelined chains (penta_pipe.h): five workgroups of eight wavefronts, the joiners carry their spike columns
      if (!SolverInstantiated(FAM_PIPE, p->K)) return Fail(err, "no penta_pipe_kernel of this block size");
      const int sep = nd_sep_lds_doubles(p->K) * (int)sizeof(double);
      p->lds = std::max(PipeLdsDoubles(p->K, p->n) * (int)sizeof(double), sep);
      if (p->lds > kMaxLds) return Fail(err, "pipelined solver: LDS carve-up too large");
      p->kind = SOLVER_PIPE; p->grid = 5; p->threads = 512;
    } else {
      p->kind = SOLVER_ND; p->grid = 7;
      p->lds = lds;
      // back substitution in recursion form (penta_pipe.h chain_recursion_tail) where every row's [Y | Z | c] fits the
      // 160 KB: allegro's 23 x 23 blocks up to N = 60, its 29 x 29 KKT blocks up to N = 40
      if (c.nd_recursion && c.has_wst) {
        const int nj = std::max(p->s - p->j1, p->j2 - p->s), np = std::max(p->j1, p->n - p->j2 - 2);
        if (const int ww = RecursionTailFits(p->K, kMaxLds / (int)sizeof(double), nj, np)) {
          p->rec_tail = ww;
          p->lds = kMaxLds;
        }
      }
    }
  } else {
    if (!SolverInstantiated(FAM_LDL, p->K)) return Fail(err, "no penta_ldl_kernel of this block size");
    p->kind = SOLVER_LDL; p->grid = p->m_split > 0 ? 2 : 1;
  }
  if (any_kernel) {
    // The launches that can carry the assembly are the scalar band kernel's and the pipelined chains' (4 (N + 1)
    // workgroups behind the solver's own, one per CU: 5 problems' worth of solver workgroups must leave room); the one
    // that can also decide on the trial point is a DEC instantiation of the pipelined kernel.
    p->can_assemble = c.solver_pipe && (p->kind == SOLVER_BAND || (p->kind == SOLVER_PIPE && 5 * c.batch <= 64));
    p->can_decide = p->can_assemble && p->kind == SOLVER_PIPE && SolverInstantiated(FAM_PIPE_DEC, p->K) && c.cost_lds <= kMaxLds;
    if (p->can_assemble) p->lds_assemble = std::max(p->lds, c.asm_terms_lds);
    if (p->can_decide) p->lds_decide = std::max(p->lds_assemble, c.cost_lds);
  }
  if (rq.kind == SolveRequest::SOLVE && rq.nrhs > 1) {
    // (several right-hand sides: the factorisation stops after its forward pass, every column incl. the first is
    // substituted by penta_apply_kernel - which walks factors of its own block size)
    p->apply_K = SolverBlockSize(p->k);
    if (p->apply_K != p->K || !SolverInstantiated(FAM_APPLY, p->apply_K)) return Fail(err, "no penta_apply_kernel for the factors of this block size");
    p->apply_lds = ApplyLds(p->n, p->apply_K);
  }
  return 0;
}

SolverBuffers SolverBufferCounts(int K, int N) {
  SolverBuffers b;
  const size_t rows = (size_t)N + 1;
  b.bands = (size_t)3 * (N + 6) * K * K;
  b.factors = rows * 32 * 36;
  b.dinv = rows * 32;
  b.dbg = (size_t)(N + 4) * 8 * 32;
  // exchange buffer of the two-sided solver (one right-hand side): 2 augmented blocks + [2][K]
  b.xch_count = 2 * (size_t)(3 * 32 + 1) * ldl_ks(32) + 2 * 32;
  b.xch = 2 * b.xch_count;   // (two producer / joiner pairs in the nested-dissection kernel)
  b.flags = 16;
  b.rowcnt = 4 * ND_MAXROWS;
  b.nd_buf = (size_t)nd_layout(32).end;
  b.has_wst = K > 20 && K <= 32;
  b.nd_wst = b.has_wst ? 2 * (size_t)ND_MAXROWS * nd_layout(K).frow : 1;
  b.apply_t = 3 * rows * 32 * 36;
  return b;
}

int PlanLsWaves(int N, int compute_units, int method, int max_linesearch_iterations, int override_width,
                int widths[kLsMaxCandidates]) {
  int total = kLsMaxCandidates;
  if (method == 0) total = std::min(kLsMaxCandidates, std::max(1, max_linesearch_iterations));   // (Armijo's do-while: at least one)
  int width = override_width > 0 ? override_width : std::max(1, compute_units / std::max(1, N));
  int count = 0;
  for (int done = 0; done < total; ++count) {
    const int w = std::min(std::min(width, kLsMaxCandidates), total - done);
    widths[count] = w;
    done += w;
    if (override_width <= 0) width *= 2;
  }
  return count;
}

}  // namespace idto_host
