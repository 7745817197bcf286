// context_layout.h — where every per-problem device array of a context lies in its arena: one table per kind of context,
// carved in the table's order (64-byte aligned entries of max(count, 1) elements, the arena stride rounded to 256 bytes).
// The order IS the contract with every kernel that takes a problem at b * pstride: an entry is added where it belongs, none
// is moved (the solvers' exchange buffers were never measured at another placement).  Host-only C++ (no HIP include):
// idto_hip.hip plans, allocates once and points the context's fields with the same tables; tests/cpp/context_layout_check.cc
// holds the plan to tests/golden/context_layout.txt on the CPU.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "idto_hip.h"

// The model's context.  X(field of idto_hip_ctx = the entry's name, element type, count) - U(name, type, count): an entry
// no field points to.  Counts in terms of nq, nv, N, rows = N + 1, bsz = nv nq, qq = nq^2, nvars = rows nq, slab_stride
// and sb = SolverBufferCounts(nq, N) (host/solver_plan.h), all size_t.
// What fd_kernel writes exists twice (batch.h AltSel): the same five entries again, so that the second set has the first
// one's relative offsets and one number - alt_off - leads from any of them to its twin.
#define IDTO_ARENA_SAME(f) f
#define IDTO_ARENA_ALT(f) f##_alt
#define IDTO_ARENA_FD_OUTPUTS(E, S)                                                  \
  E(S(v), double, rows * nv) E(S(a), double, N * nv) E(S(nplus), double, rows * bsz) \
  E(S(slab), double, (N + IDTO_SLAB_PAD) * slab_stride) E(S(terms), double, N * (size_t)asm_terms_stride((int)nq))
#define IDTO_MODEL_ARENA(X, U)                                                                                              \
  /* the problem: one stretch, uploaded with one copy (UploadProblemArrays) */                                              \
  X(d_vinit, double, nv) X(d_qnom, double, rows * nq) X(d_vnom, double, rows * nv)                                          \
  X(d_w[0], double, qq) X(d_w[1], double, nv * nv) X(d_w[2], double, nv * nv) X(d_w[3], double, qq) X(d_w[4], double, nv * nv) \
  X(d_w[5], double, qq) X(d_w[6], double, nv * nv) X(d_w[7], double, nv * nv) X(d_w[8], double, qq) X(d_w[9], double, nv * nv) \
  X(q, double, nvars)                                                                                                       \
  IDTO_ARENA_FD_OUTPUTS(X, IDTO_ARENA_SAME) IDTO_ARENA_FD_OUTPUTS(U, IDTO_ARENA_ALT)                                        \
  /* g and H's three bands in one entry (IDTO_MODEL_BANDS); a second g and H: the trial point's, formed by the solver's     \
     launch while it decides on the point (penta_pipe.h PipeAsm::g2) */                                                     \
  X(g, double, nvars) X(HA, double, sb.bands) X(HA2, double, sb.bands) X(g2, double, nvars)                                 \
  X(step, double, nvars) X(cost, double, 1)                                                                                 \
  X(Kst, double, rows * qq) X(LUst, double, rows * qq) X(Yst, double, rows * qq) X(Zst, double, rows * qq)                  \
  X(pivst, int, nvars)                                                                                                      \
  /* the solvers' own arrays */                                                                                             \
  X(dbg, double, sb.dbg) X(Ust, double, sb.factors) X(Hst, double, sb.factors) X(Est, double, sb.factors)                   \
  X(Dst, double, sb.dinv) X(xch, double, sb.xch) X(nd_rowcnt, unsigned long long, sb.rowcnt) X(nd_buf, double, sb.nd_buf)   \
  X(pipe_rowcnt, unsigned long long, sb.rowcnt) X(nd_wst, double, sb.nd_wst) X(asm_ready, unsigned, 4 * rows)               \
  X(flags, unsigned, sb.flags) X(sync_cnt, unsigned long long, 2)                                                           \
  /* the trust-region loop's */                                                                                             \
  X(tr_D, double, nvars) X(tr_gt, double, nvars) X(tr_w, double, nvars) X(tr_dq, double, nvars) X(q_trial, double, nvars)   \
  X(tr_out, double, 16) X(tr_Dprev, double, nvars) X(tr_part, double, 9 * rows)                                             \
  X(tr_part_ll, double, 2 * (TR_NSUM * rows + 3)) X(tr_part2, double, 2 * rows) X(decide_word, double, 4)                   \
  X(tr_state, double, TRS_COUNT) X(tr_cnt, unsigned long long, 1)                                                           \
  /* the equality-constraint step's outputs (per problem, so that the batched loop finds them at the arena stride):        \
     [H^-1 (g + J^T lambda) | J^T lambda] and the multipliers (nu <= nv; + 4: the blocked dense LDL^T's [min, max | ...]) */ \
  X(con_out, double, 2 * nvars) X(con_lambda, double, N * nv + 4)

// The solver-only context of a KKT system (nq = its block size, nv = 0): what LaunchLdl / FactorStatus touch, in an order
// of its own.
#define IDTO_KKT_ARENA(X, U)                                                                                              \
  X(HA, double, sb.bands) X(g, double, nvars) X(step, double, nvars)                                                      \
  X(Ust, double, sb.factors) X(Hst, double, sb.factors) X(Est, double, sb.factors) X(Dst, double, sb.dinv)                \
  X(dbg, double, sb.dbg) X(xch, double, sb.xch) X(flags, unsigned, sb.flags)                                              \
  X(nd_rowcnt, unsigned long long, sb.rowcnt) X(pipe_rowcnt, unsigned long long, sb.rowcnt) X(nd_buf, double, sb.nd_buf)  \
  X(nd_wst, double, sb.nd_wst)

// Fields that point INTO an entry: X(field, the entry's field, index) - field = entry + index * band doubles, band =
// (N + 6) nq^2: N + 1 blocks and five zero blocks (the solver prefetches rows i + 1, i + 2 without bounds checks, and
// addresses all three bands from HA with 32-bit offsets: hence one entry)
#define IDTO_MODEL_BANDS(X) X(HB, HA, 1) X(HC, HA, 2) X(HB2, HA2, 1) X(HC2, HA2, 2)
#define IDTO_KKT_BANDS(X) X(HB, HA, 1) X(HC, HA, 2)

// Every IDTO_ARR_* id (include/idto_hip.h) of the model's context:
//   A(id, field, public count)   contiguous at `field` (an entry or a band) - counts as above
//   S(id, at, width)             N rows of `width` doubles, `at` into each record of the slab (slab_stride apart)
//   O(id)                        outside the arena plan: the constraint step's, sized by the constraints in force
// IDTO_ARR_DEBUG is the KKT context's dbg instead while option "solver_debug" is 2 (idto_hip.hip DevPtr).
#define IDTO_ARRAYS(A, S, O)                                                                                        \
  A(IDTO_ARR_Q, q, rows * nq) A(IDTO_ARR_V, v, rows * nv) A(IDTO_ARR_A, a, N * nv) S(IDTO_ARR_TAU, 3 * bsz, nv)     \
  A(IDTO_ARR_NPLUS, nplus, rows * bsz) S(IDTO_ARR_DTAU_DQM, 0, bsz) S(IDTO_ARR_DTAU_DQT, bsz, bsz)                  \
  S(IDTO_ARR_DTAU_DQP, 2 * bsz, bsz) A(IDTO_ARR_GRADIENT, g, rows * nq) A(IDTO_ARR_H_A, HA, rows * qq)              \
  A(IDTO_ARR_H_B, HB, rows * qq) A(IDTO_ARR_H_C, HC, rows * qq) A(IDTO_ARR_STEP, step, rows * nq)                   \
  A(IDTO_ARR_COST, cost, 1) A(IDTO_ARR_SLAB, slab, N * slab_stride) A(IDTO_ARR_DEBUG, dbg, (N + 4) * 8 * 32)        \
  A(IDTO_ARR_HBANDS, HA, 3 * (N + 6) * qq) A(IDTO_ARR_TR_DQ, tr_dq, rows * nq) A(IDTO_ARR_TR_W, tr_w, rows * nq)    \
  A(IDTO_ARR_TR_SCALE, tr_D, rows * nq) A(IDTO_ARR_ASM_TERMS, terms, N * (size_t)asm_terms_stride((int)nq))         \
  O(IDTO_ARR_CON_S) O(IDTO_ARR_CON_LAMBDA)

namespace idto_host {

enum ArenaKind { ARENA_MODEL = 0, ARENA_KKT = 1 };

struct ArenaEntry {
  const char* name;
  size_t elem, count, offset;   // bytes of an element, elements (what the table says: at least one is carved), bytes into the arena
};
struct ArenaBand { const char* name; const char* entry; int index; };

struct ArenaPlan {
  std::vector<ArenaEntry> entries;   // in the table's order = the order they are carved in
  std::vector<ArenaBand> bands;
  size_t pstride = 0;                // bytes from one problem's arena to the next
  long long alt_off = 0;             // bytes from an output of fd_kernel to its twin of the second set (the model's context; else 0)
  size_t band = 0;                   // doubles from one band of an H to the next
  bool has_wst = false;              // nd_wst exists (else its entry is a placeholder and the field stays null)
  size_t xch_count = 0, flag_count = 0;
  int slab_stride = 0;               // doubles of a record of the slab: three partials and tau
  // the entry called `name`, or null
  const ArenaEntry* Find(const std::string& name) const;
  // where the field `name` - an entry or a band - begins (bytes into the arena) and how many elements follow it within
  // its entry; false: no such field
  bool Locate(const std::string& name, size_t* offset, size_t* room) const;
};
ArenaPlan PlanArena(ArenaKind kind, int nq, int nv, int N);

// An IDTO_ARR_* id of the model's context
struct ArrayInfo {
  enum Where { UNKNOWN = 0, ENTRY, SLAB_ROWS, OUTSIDE };
  Where where = UNKNOWN;
  const char* field = nullptr;   // ENTRY: the field it lies at
  long count = -1;               // its public element count (OUTSIDE: -1, the context knows)
  size_t at = 0, width = 0;      // SLAB_ROWS: N rows of `width` doubles, `at` doubles into each record
};
ArrayInfo ArrayLookup(int what, int nq, int nv, int N);
// every id of the table, in its order
std::vector<int> ArrayIds();

// Dynamic LDS and block sizes of the launches whose geometry is a pure function of the sizes (fd_kernel's depends on the
// uploaded model and stays with it)
struct LaunchSizes {
  int asm_lds, asm_diag_lds, asm_terms_lds, asm_terms_threads, penta_lds, solve_lds, cost_lds;
  int apply_lds;   // penta_apply_kernel at the factorisation's block size: bounds the horizon, kept by no field
};
LaunchSizes PlanLaunchSizes(int nq, int nv, int N);

}  // namespace idto_host
