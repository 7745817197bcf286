// penta_pipe.h — the forward elimination of a chain of the block LDL^T factorisation (penta_ldl.h) as a
// pipeline of wavefronts that follow each other through LDS, without a products phase.
//
// penta_ldl_body eliminates block row i in the registers of one wavefront, then ALL wavefronts form the next
// row's Schur complement S_{i+1} = C - Et_{i-1}^T Dn Et_{i-1} - Ht_i^T Dn Ht_i on the matrix cores from LDS,
// and the eliminating wavefront loads it back: per block row 2.1k cycles of products + 0.4k of loads + 1.6k of
// stores and barriers next to the 4.1k cycles of the K dependent pivots (profiles/r02_solver_phases.txt).
// Here the update by Ht_i is applied pivot by pivot WHILE row i is eliminated (right-looking):
//
//   wave A (row i)      pivot j: scaled pivot row t_j = [D^-1 U | D^-1 Ht | D^-1 Et | D^-1 rt]_j and d_j -> LDS
//   wave B (row i+1)    holds W_{i+1} = [S | H | E | y] in the same one-column-per-lane register layout and
//                       applies  W_{i+1}[r][c] -= Ht_i[j][r] / d_j * [Ht_i | Et_i | . | rt_i][j][c]  as soon as
//                       row j appears (19 multipliers as LDS broadcasts, one FMA per row)
//   when A has published its last pivot, B holds the complete W_{i+1} and starts eliminating at once; A
//   reloads with the inputs of row i+2 and becomes the follower.
//
// The update by Et_i (two rows ahead, a whole row time of slack) stays a dense block product on the matrix
// cores: helper wavefronts form  G = Et_i^T Dn [Et_i | rt_i | Ft_i]  from the published rows, the follower
// subtracts it half-way through its row.  The same helpers stage the band blocks (HBM -> LDS, column layout)
// and write the factors out for the back substitution - the published rows ARE the row-major, 1/d-scaled
// factors penta_ldl_tail and penta_apply_kernel read.  The chain's critical path per block row is the K pivots
// of wave A plus one LDS hand-over.
//
// Nested dissection (penta_nd.h): the 2K "spike" columns F that couple a joiner chain to the separator are
// carried by a second pair of wavefronts (A', B') in lock-step with the chain - they were a workgroup of their
// own trailing the joiner by a row and a half (9 us at the end of the forward pass).
//
// Reference recursion: optimizer/penta_diagonal_solver.h:124-197 (Factorize), :199-248 (SolveInPlace).
#pragma once

#include "kernels.h"
#include "penta_nd.h"
#include "solver_layout.h"

namespace idto_dev {

// (PipeGeo, pipe_rlo, pipe_mfma_follow, PIPE_HPC / HS / HPN, PipeLds / pipe_layout<K>: solver_layout.h)

// flag words (ints, values = local row + 1)
enum {
  PF_SLOTGEN = 0,    // [3] main wavefront owns ring slot s for row il
  PF_SLOTGEN2 = 3,   // [3] spike wavefront likewise
  PF_ROWDONE = 6,    // [3] all pivots of row il published (main)
  PF_ROWDONE2 = 9,   // [3] (spike)
  PF_STAGED = 12,    // [2] inputs of row il are in stage buffer il & 1
  PF_INITD = 14,     // [2] main wavefront has loaded them
  PF_INITD2 = 16,    // [2] spike wavefront has
  PF_GDONE = 18,     // [2][2] G of row il is in gbuf[il & 1] (two helper wavefronts)
  PF_COPIED = 22,    // [3] factors of the row in ring slot s are written out
  PF_COPIED2 = 25,   // [3] spike columns likewise
  PF_ABORT = 28,     // a bounded wait ran out: everybody stops waiting
  PF_JOINED = 29,    // joiner: the producer's contributions to the two join rows are in the stage buffers
  PF_HIDONE = 30,    // the second follower's (high) rows of row il are in the hand-over buffer (main columns)
  PF_HIDONE2 = 31,   // (spike columns)
  PF_T0 = 40,        // [2] wall clock at the workgroup's start (pipe_giveup)
  PF_COUNT = 32
};

constexpr int PIPE_SPIN_CAP = 1 << 17;            // polls (~150 cycles each with the sleep: ~10 ms) before a wait may give up ...
constexpr long long PIPE_AGE_TICKS = 1000000;      // ... and then only in a workgroup that is older than 10 ms of the 100 MHz wall clock
// (the poll count alone runs out early under clock throttling or a profiler's serialisation and would degrade the context
// for good; a launch takes ~65 us, so a workgroup of that age is stuck.  The age, not the duration of the wait: a start
// time per wait is two more live registers in every wait loop of a register-bound kernel - measured 64.8 against 63.4 us)

// flags and published words are polled: volatile accesses in the LDS address space (a volatile access through a
// generic pointer becomes a flat load with system-scope cache bits)
typedef __attribute__((address_space(3))) volatile int pipe_lds_int;
typedef __attribute__((address_space(3))) volatile double pipe_lds_dbl;

struct PipeCtl {
  pipe_lds_int* f;       // LDS flags
  unsigned* status;      // host-mapped factorisation status
  unsigned fact_id;
};
// A bounded wait that ran out (a partner workgroup is not resident, or a bug) sets PF_ABORT: every other wait of
// the workgroup then gives up early, and the end of pipe_forward reports a failed factorisation.  (No function
// call here: a call site inside the chain wavefronts' row loop makes every live register cross it.)
// every poll is wave-uniform by construction (readfirstlane): scalar branches, no exec-mask loops
__device__ __forceinline__ bool pipe_giveup(const PipeCtl& c, int n) {
  if ((n & 255) != 0) return false;
  if (__builtin_amdgcn_readfirstlane(c.f[PF_ABORT]) != 0) return true;
  if (n >= PIPE_SPIN_CAP) {
    const long long t0 = ((long long)(unsigned)c.f[PF_T0 + 1] << 32) | (unsigned)c.f[PF_T0];   // the workgroup's start (pipe setup)
    if ((long long)wall_clock64() - t0 > PIPE_AGE_TICKS) { c.f[PF_ABORT] = 1; return true; }
  }
  return false;
}
// waits until flag >= target; bounded, see PIPE_SPIN_CAP
__device__ __forceinline__ void pipe_wait(const PipeCtl& c, int flag, int target) {
  int n = 0;
  while (__builtin_amdgcn_readfirstlane(c.f[flag]) < target) {
    __builtin_amdgcn_s_sleep(1);
    if (pipe_giveup(c, ++n)) break;
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// one lane posts flag = value after the wavefront's earlier LDS writes (LDS executes a wavefront's operations
// in order; the fence only keeps the compiler from reordering)
__device__ __forceinline__ void pipe_post(const PipeCtl& c, int flag, int value) {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if ((threadIdx.x & 63) == 0) c.f[flag] = value;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// a bounded wait on a word in global memory (another workgroup's flag, penta_ldl.h spin_wait); false: it gave up
__device__ __forceinline__ bool pipe_wait_global(const PipeCtl& c, const unsigned* f, unsigned epoch, const SpinCtl sc) {
  const bool ok = spin_wait([&] {
    return (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == epoch;
  }, sc);
  if (!ok) c.f[PF_ABORT] = 1;
  (void)__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
  return ok;
}

__device__ __forceinline__ bool pipe_isnan(double v) { return v != v; }
// keeps a per-lane offset opaque to loop-invariant code motion: the chain wavefronts' row loop is one huge
// unrolled body, and every address the compiler hoists out of it (the join rows' exchange buffer alone: 57
// 64-bit pointers) is a register that lives through the pivots
__device__ __forceinline__ int pipe_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// 1 / d: hardware estimate (~2^-23 relative) and ONE cubic step, x (1 + e + e^2) with e = 1 - d x: error e^3 ~ 2^-69,
// three dependent FMAs instead of the four of two Newton steps (the reciprocal chain is on the critical path of
// every pivot)
__device__ __forceinline__ double pipe_rcp(double d) {
#ifdef PIPE_RCP_TWO_NEWTON
  return fast_rcp(d);
#endif
  const double x = __builtin_amdgcn_rcp(d);
  const double e = __builtin_fma(-d, x, 1.0);
  const double p = __builtin_fma(e, e, e);
  return __builtin_fma(x, p, x);
}

// v with lane LANE replaced by the wave-uniform 64-bit pattern (hi, lo): two v_writelane_b32
template <int LANE>
__device__ __forceinline__ double pipe_setlane(double v, int uhi, int ulo) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  wrlane<LANE>(lo, ulo);
  wrlane<LANE>(hi, uhi);
  return __hiloint2double(hi, lo);
}

// ---- wave A, main columns: pivot J of the row held in xr (lane = column of [S | H | E | y]); `rowp` / `rawp` =
// this lane's positions in row 0 of the ring slot, `slot0` = the slot's base.
// penta_ldl_body's pivot step broadcasts the K - J - 1 multipliers with two v_readlane_b32 each and is bound
// by the issue rate of one wavefront (~70 instructions for a middle pivot).  Here the scaled pivot row is
// written to LDS anyway (the followers and the factors need it), and its entries D^-1 U[J][r] ARE the
// multipliers: the wavefront reads them back as LDS broadcasts, two per instruction, and updates
// xr[r] -= (U[J][r] / d_J) * xr[J].  Only the next row goes the fast way (v_readlane), so that the next pivot
// and its reciprocal do not wait for the LDS round trip; the rest of the update runs in its shadow.
// (Multipliers from the upper triangle throughout: L = (D^-1 U)^T exactly, as the back substitution assumes.)
// (One more step of software pipelining: the multipliers read back at pivot J are used at pivot J+1 - `mu_p`,
// `xj_p` are pivot J-1's - so that no instruction of the dependent chain pivot -> reciprocal -> next pivot ever
// waits for an LDS read issued in the same step.  Row J+1 gets pivot J-1's term first, then pivot J's by
// v_readlane, and is complete for the next reciprocal; rows J+2.. get pivot J-1's terms in the chain's shadow.)
// `hook` runs once, at pivot JH, off the dependent chain: the eliminating wavefront takes in the high rows the
// second follower accumulated (pipe_chain_wave).
template <int K, int J, int JH, class Hook>
__device__ __forceinline__ void pipe_pivot(double (&xr)[K], double inv, const double (&mu_p)[K], const double xj_p,
                                           double* __restrict__ rowp, double* __restrict__ rawp,
                                           const double* __restrict__ slot0, const bool is63, Hook hook, double* dbg = nullptr) {
  using G = PipeGeo<K>;
  (void)dbg;
  // Two LDS writes per pivot, in this order and at once: the unscaled parts, then the scaled row whose lane 62 is
  // the "published" word the followers poll.  The fences are compiler barriers (the hardware executes a
  // wavefront's LDS operations in order): without them the compiler pairs the writes of two consecutive pivots
  // into one ds_write2_b64 - a row would go out a pivot late, and the word could overtake the unscaled parts.
  const double xj = xr[J];
  // The dependent chain of the factorisation is  1/d_J -> d_{J+1} -> 1/d_{J+1}.  d_{J+1} = S[J+1][J+1] - U[J][J+1]^2 / d_J
  // sits in lane J+1 and needs nothing but that lane's own registers and 1/d_J: it is formed HERE, before the
  // scaled row, its publication and the broadcast of the next multiplier - all of which then run beside the chain
  // instead of inside it (the same value reaches xr[J+1] the usual way below; the two differ by a rounding).
  double inv_next = 1.0;
  if constexpr (J + 1 < K) {
    if constexpr (J >= 1) xr[J + 1] = __builtin_fma(-mu_p[J + 1], xj_p, xr[J + 1]);   // pivot J-1's term (its multiplier was read a step ago)
    const double dn = __builtin_fma(-(xj * xj), inv, xr[J + 1]);
    inv_next = pipe_rcp(rdlane(dn, J + 1));
  }
  rawp[J * G::RS] = xj;   // (columns of H, E, y: the unscaled pivot row; other lanes: a dump position)
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  double t = xj * inv;
  {
    // lanes 62 / 63 carry no column: 63 publishes 1 / d_J (the factors' Dn, the pivot test), 62 the "published"
    // word - any non-NaN pattern (a NaN reads as "not yet" to the followers), here the high half of a small float
    t = is63 ? inv : t;
    int lo = __double2loint(t), hi = __double2hiint(t);
    wrlane<62>(hi, 0x3f800000);
    t = __hiloint2double(hi, lo);
  }
  rowp[J * G::RS] = t;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  double mu[K];
  if constexpr (J + 2 < K) {   // the multipliers of rows J+2 .. K-1, back from the row just written
    const double2* p2 = reinterpret_cast<const double2*>(slot0 + J * G::RS);
#pragma unroll
    for (int m = (J + 2) / 2; m < (K + 1) / 2; ++m) {
#ifdef PIPE_MULT_READLANE   // (measurement aid, tools/micro/pivot_bench.hip: faster alone on a CU, slower in the kernel)
      double2 v; v.x = rdlane(t, 2 * m < K ? 2 * m : K - 1); v.y = rdlane(t, 2 * m + 1 < K ? 2 * m + 1 : K - 1);
#else
      const double2 v = p2[m];
#endif
      // (an odd J needs only the second half of its first pair, mu[J + 1] goes unused: left to itself the compiler
      // narrows that read to 8 bytes, and every read after it is then 8 bytes off a 16-byte boundary - ds_read2_b64
      // with an address of its own, a v_add_u32 per read on the eliminating wavefront.  The next step "uses" it.)
      mu[2 * m] = v.x;
      if (2 * m + 1 < K) mu[2 * m + 1] = v.y;
    }
  }
  if constexpr (J + 1 < K) {
    const double m1 = rdlane(t, J + 1);
    xr[J + 1] = __builtin_fma(-m1, xj, xr[J + 1]);
  }
  if constexpr (J == JH) hook();
  if constexpr (J >= 1) {
#pragma unroll
    for (int r = J + 2; r < K; ++r) xr[r] = __builtin_fma(-mu_p[r], xj_p, xr[r]);
    if constexpr ((J & 1) == 0 && J + 1 < K) asm volatile("" ::"v"(mu_p[J]));   // (the unused half of pivot J-1's first read, see above)
  }
  // (keep the steps apart: left to itself the scheduler defers a row's updates until the row becomes the pivot
  // row - a chain of dependent FMAs into one accumulator right where the next pivot waits for it)
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (J + 1 < K) pipe_pivot<K, J + 1, JH>(xr, inv_next, mu, xj, rowp, rawp, slot0, is63, hook, dbg);
}

// ---- wave A, spike columns: pivot J of Ft = L^-1 F (lane = spike column, xr = the column's K rows).  The multipliers
// T_J[c] = (D^-1 U)[J][c], c > J, are the MAIN wavefront's published row (`arow`, position c): nothing of this
// wavefront's own goes into them, so they are read AHEAD of their use exactly as pipe_pivot does with its own -
// T_J[J+2 ..] at pivot J for pivot J + 1 (`mu_p`, `xj_p`), and T_J[J+1], the one the next pivot's value waits for, a whole
// pivot earlier (`m1`) - and a pivot here is K - J - 1 FMAs and two stores with ONE FMA on the dependent chain, not an LDS
// round trip followed by the FMAs.  (Rounds 3-5 read them at their use: 125 ns a pivot, 2.4 us a row against the main
// wavefront's 1.9.  The spike chain ran a row behind and set a joiner's pace through the G wavefront, which needs both rows:
// 3.3 us a row.)  `need(J)`: returns once the main wavefront has published pivot J; asked one pivot ahead, for the read of m1.
template <int K, int J, int JH, class Hook, class Need>
__device__ __forceinline__ void pipe_spike_pivot(double (&xr)[K], const double (&mu_p)[K], const double xj_p, const double m1,
                                                 double* __restrict__ rowp, double* __restrict__ fout, const bool store,
                                                 const double* __restrict__ arow, Hook hook, Need need) {
  using G = PipeGeo<K>;
  if constexpr (J == JH) hook();
  if constexpr (J + 2 < K) need(J + 2);   // (pivots J, J + 1 were asked for a step ago)
  const double xj = xr[J];
  if constexpr (J + 1 < K) {
    if constexpr (J >= 1) xr[J + 1] = __builtin_fma(-mu_p[J + 1], xj_p, xr[J + 1]);   // pivot J-1's term
    xr[J + 1] = __builtin_fma(-m1, xj, xr[J + 1]);                                      // pivot J's: the row is complete
  }
  rowp[J * G::RS] = pipe_setlane<63>(xj, 0x3ff00000, 0);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  // (and to HBM for the separator's Q / this chain's own correction: column `lane`, row J; write-through - the
  // separator sits on another XCD - so that the row's release is a drained store queue, not a fence)
  if (store) __hip_atomic_store(fout + J, xj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double mu[K];
  double m1n = 0.0;
  if constexpr (J + 2 < K) {
    const double2* p2 = reinterpret_cast<const double2*>(arow + J * G::RS);
#pragma unroll
    for (int m = (J + 2) / 2; m < (K + 1) / 2; ++m) {
      const double2 v = p2[m];
      mu[2 * m] = v.x;
      if (2 * m + 1 < K) mu[2 * m + 1] = v.y;
    }
    m1n = arow[(J + 1) * G::RS + J + 2];
  }
  if constexpr (J >= 1) {
#pragma unroll
    for (int r = J + 2; r < K; ++r) xr[r] = __builtin_fma(-mu_p[r], xj_p, xr[r]);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (J + 1 < K) pipe_spike_pivot<K, J + 1, JH>(xr, mu, xj, m1n, rowp, fout, store, arow, hook, need);
}

// K uniform multipliers [pos0, pos0 + K) of a published row (pos0 even): LDS broadcast reads, two per instruction
template <int K>
__device__ __forceinline__ void pipe_read_mult(const double* __restrict__ row, int pos0, double (&mu)[K]) {
  const double2* p2 = reinterpret_cast<const double2*>(row + pos0);
#pragma unroll
  for (int m = 0; m < K / 2; ++m) { const double2 v = p2[m]; mu[2 * m] = v.x; mu[2 * m + 1] = v.y; }
  if (K & 1) mu[K - 1] = row[pos0 + K - 1];
}

// waits until row J of a ring slot carries a pivot (main) / the spike wavefront's word, i.e. until the word is no
// quiet NaN (the publisher never writes one: pipe_pivot).  Polls the high half only - one 8-byte LDS write
// lands both halves at once; bounded
__device__ __forceinline__ void pipe_wait_row(const PipeCtl& c, const double* word) {
  pipe_lds_int* hi = (pipe_lds_int*)word + 1;
  int n = 0;
  while ((__builtin_amdgcn_readfirstlane(*hi) & 0x7ff80000) == 0x7ff80000) {
    __builtin_amdgcn_s_sleep(1);
    if (pipe_giveup(c, ++n)) break;
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

struct PipeArgs {
  int n, k;
  const double* HA; const double* HB; const double* HC; const double* b;
  double rhs_sign;
  double* x;
  double* Ust; double* Hst; double* Est; double* Dst;
  double* xch; unsigned* flags; unsigned epoch;
  unsigned* status; unsigned fact_id;
  // nested dissection (spike chains): [Ft | rt] rows for the separator and their release counters
  double* fst; int fstride; unsigned long long* frowcnt;
  double* wst;        // chain_recursion_tail (the seven-workgroup kernel): W_il = U_il^-1 Dn Ft_il of a joiner's rows, laid out like fst
  double* xjoin_ll;   // the pair's two join rows of x, joiner -> producer, epoch in every word (penta_nd.h ll_store)
  double* join_ll;    // the producer's contributions to the join rows, [2][(3K + 1) ks] values in the same form
  // g and the bands assembled by other workgroups of this launch (PipeAsm): [rows][4] words that hold the epoch once
  // part p of block row i is in memory; solver row o is assembly row o + asm_first.  nullptr: they were there before.
  const unsigned* asm_ready; int asm_first, asm_rows;
  double* ts;
  int closed_tail;    // pipe_backward, a producer of the pipelined kernel: its recursion in closed form (pipe_closed_tail)
};

// ---- g and the band blocks formed INSIDE the solver's launch (idto_hip_gn_step): the 4 (N + 1) workgroups behind the
// solver's own (5 of penta_pipe_kernel, 1 of penta_band_kernel) run assemble_terms_kernel's rows (kernels.h assemble_terms_row: same expressions, same bits), store with
// write-through and publish one word per (block row, part); the chains' loads of a row wait for the words of the
// rows it touches and bypass the L2 (another XCD's L2 held the lines first).  What this buys is the launch boundary
// between assembly and solver (~8 us a step); the assembly workgroups are gone long before the chains need
// their compute units' neighbours.
struct PipeAsm {
  int on;                   // 0: the bands are in HBM already
  int nq, nv, rows, first;  // rows = N + 1 block rows; solver row 0 is block row `first`
  DevProblem P;
  const double* q; const double* terms; const double* v_res; const double* nplus;
  double* g; double* HA; double* HB; double* HC;
  AltSel alt;
  unsigned* ready;
  const double* gate;       // idto_hip_tr_solve: a problem whose word is 0 (its step was rejected) keeps g and H, nullptr: assemble
  // (DEC instantiations of penta_pipe_kernel, inside idto_hip_tr_solve) the decision is made IN this launch: one more
  // workgroup - the one behind the assembly's - evaluates the trial point's cost and decides (kernels.h cost_body:
  // cost_kernel's work, whose launch this saves); the assembly's workgroups start cold under it instead of behind it
  int decide;               // 0: `gate` (or nothing) as above
  const double* dq;         // q of the trial point: the cost's, and the assembly's for an accepted step (the copy into the
                            // iterate's array is the deciding workgroup's, not ordered against anybody in this launch)
  const double* dv; const double* dslab; int dslab_stride; double* dcost; int ddiag;
  TrDecideArgs dT; AltSel dalt;   // (the trial point's outputs live in the set the iterate does not occupy)
  double* dword; unsigned depoch; // the decision, the launch's epoch in every word: 1 + accepted + 2 (current set AFTER it)
  // The assembly does not wait for the decision: it forms g and H of the TRIAL point at once into a second set of
  // arrays (same layout), the chains take their system from there once the step is accepted (from g, H as they stand
  // when it is rejected), and the assembly's workgroups form the accepted point's g and H once more into the primary
  // arrays behind the decision - off everybody's critical path - for the kernels that follow.
  double* g2; double* HA2; double* HB2; double* HC2;
  const double* curpre;     // the current-set word as the iteration's tr_iter_kernel found it (the deciding workgroup flips the word itself mid-launch)
};
// does this problem assemble in this launch?  (cur: the set that holds the iterate, where the launch itself decides)
template <bool DEC = false>
__device__ __forceinline__ bool pipe_asm_on(const PipeAsm& F, size_t o, const SpinCtl sc = SpinCtl{nullptr, 0}, int* cur = nullptr) {
  if (!F.on) return false;
  if (DEC && F.decide) {
    double x = 0.0;
    if ((threadIdx.x & 63) == 0) {
      const double* word = at_problem(F.dword, o);
      if (!spin_wait([&] { return tr_ll_try(word, F.depoch, x); }, sc)) x = 1.0;   // (no decision within the bound: nothing is assembled, the timeout is reported)
    }
    const int code = __builtin_amdgcn_readfirstlane((int)x) - 1;
    if (cur) *cur = code >> 1;
    return (code & 1) != 0;
  }
  return !(F.gate && *at_problem(F.gate, o) == 0.0);
}

// the deciding workgroup (PipeAsm::decide): cost_kernel's work for the problem, then the word the others poll
__device__ __forceinline__ void pipe_decide_role(const PipeAsm& F, const size_t pstride) {
  const size_t o = (size_t)blockIdx.y * pstride, w = o + (size_t)alt_offset(F.dalt, o);
  const DevProblem P = at_problem(F.P, o);
  TrDecideArgs T = F.dT;
  T.state = at_problem(T.state, o); T.out = at_problem(T.out, o); T.q = at_problem(T.q, o);
  T.q_trial = at_problem(T.q_trial, o); T.rows += (size_t)blockIdx.y * T.rows_stride;
  T.part2 = at_problem(T.part2, o);
  if (T.lambda) T.lambda = at_problem(T.lambda, o);
  const double cur_old = T.state[TRS_CUR];
  const bool acc = cost_body<4>(F.nq, F.nv, P, at_problem(F.dq, o), at_problem(F.dv, w), at_problem(F.dslab, w), F.dslab_stride,
                             at_problem(F.dcost, o), F.ddiag, nullptr, nullptr, T);
  if (threadIdx.x == 0) {
    const int cur_new = acc ? (cur_old != 0.0 ? 0 : 1) : (cur_old != 0.0 ? 1 : 0);   // (tr_decide: an accepted step's set is the iterate's now)
    tr_ll_store(at_problem(F.dword, o), (double)(1 + (acc ? 1 : 0) + 2 * cur_new), F.depoch);
  }
}

// (first_wg: how many workgroups of the grid's x run the solver - 5 in penta_pipe_kernel, 1 in penta_band_kernel; ts:
// debug stamps or nullptr, in the slot behind the solver's roles)
template <bool DEC = false>
__device__ __forceinline__ void pipe_assemble(double* ts, const unsigned epoch, const size_t pstride, PipeAsm F, const int first_wg,
                                              const SpinCtl sc = SpinCtl{nullptr, 0}) {
  struct { double* ts; unsigned epoch; size_t pstride; } A{ts, epoch, pstride};
  extern __shared__ double lds[];
  const bool decided = DEC && F.decide;
  const int a0 = (int)blockIdx.x - first_wg;
  if (decided && a0 == 0) { pipe_decide_role(F, pstride); return; }   // (the first workgroup behind the chains': dispatched early)
  const int a = decided ? a0 - 1 : a0, i = a >> 2, part = a & 3;
  if (i >= F.rows) return;
  const size_t o = (size_t)blockIdx.y * A.pstride;
  if (!decided && !pipe_asm_on<false>(F, o)) return;
  if (A.ts && threadIdx.x == 0)   // debug stamps of role 5: [0] latest end, [1] latest start of an assembly workgroup (positive doubles order like integers)
    atomicMax(reinterpret_cast<unsigned long long*>(A.ts + first_wg * 64 + 1), (unsigned long long)__double_as_longlong((double)wall_clock64()));
  if (A.ts && a == 4 && threadIdx.x == 0) A.ts[first_wg * 64 + 8] = (double)wall_clock64();
  // (deciding launch: the trial point's records - the set the iterate does NOT occupy as the launch finds the state - and
  // its q; results into the second set of arrays)
  const size_t w = o + (size_t)(decided ? (((*at_problem(F.curpre, o) != 0.0) != (F.dalt.which != 0)) ? F.dalt.off : 0) : alt_offset(F.alt, o));
  const DevProblem P = at_problem(F.P, o);
  const double* qa = at_problem(decided ? F.dq : F.q, o);
  assemble_terms_row<true>(F.nq, F.nv, P, qa, at_problem(F.terms, w), at_problem(F.v_res, w), at_problem(F.nplus, w),
                           at_problem(decided ? F.g2 : F.g, o), at_problem(decided ? F.HA2 : F.HA, o),
                           at_problem(decided ? F.HB2 : F.HB, o), at_problem(decided ? F.HC2 : F.HC, o), i, part, lds);
  if (A.ts && a == 4 && threadIdx.x == 0) A.ts[first_wg * 64 + 9] = (double)wall_clock64();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every write-through store acknowledged ...
  __syncthreads();
  if (A.ts && a == 4 && threadIdx.x == 0) A.ts[first_wg * 64 + 10] = (double)wall_clock64();
  if (threadIdx.x == 0)                              // ... before the word that says so
    __hip_atomic_store(at_problem(F.ready, o) + 4 * i + part, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (A.ts && threadIdx.x == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(A.ts + first_wg * 64), (unsigned long long)__double_as_longlong((double)wall_clock64()));
  if (decided) {
    // behind the decision: an accepted point's g and H once more, into the arrays every later kernel reads (same
    // operands, same code, same bits; nobody in this launch waits for it)
    if (!pipe_asm_on<true>(F, o, sc)) return;
    __syncthreads();
    assemble_terms_row<false>(F.nq, F.nv, P, qa, at_problem(F.terms, w), at_problem(F.v_res, w), at_problem(F.nplus, w),
                              at_problem(F.g, o), at_problem(F.HA, o), at_problem(F.HB, o), at_problem(F.HC, o), i, part, lds);
  }
}

// one wavefront waits for solver rows o_lo .. o_hi (clamped to the system) to be assembled: a lane per word
__device__ __forceinline__ void pipe_rows_ready(const PipeArgs& A, const PipeCtl& c, int o_lo, int o_hi, const SpinCtl sc) {
  if (!A.asm_ready) return;
  const int lane = threadIdx.x & 63;
  o_lo = o_lo < 0 ? 0 : o_lo;
  o_hi = o_hi > A.n - 1 ? A.n - 1 : o_hi;
  const int nw = 4 * (o_hi - o_lo + 1);
  const unsigned* w = A.asm_ready + 4 * (o_lo + A.asm_first) + (lane < nw ? lane : 0);
  const bool ok = spin_wait([&] {
    const bool mine = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.epoch;
    return __builtin_amdgcn_ballot_w64(mine) == __builtin_amdgcn_ballot_w64(true);
  }, sc);
  if (!ok) c.f[PF_ABORT] = 1;
}
// a band entry: through the L2 when it was assembled by this launch
__device__ __forceinline__ double pipe_band(const PipeArgs& A, const double* p) {
  return A.asm_ready ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}

// ---- a chain wavefront.  Three of them take turns: while one ELIMINATES row i (publishing every pivot row), the
// other two FOLLOW it with the Schur update of row i+1, W_{i+1} -= Ht_i^T Dn [Ht_i | Et_i | rt_i], one half of
// W's K rows each: the wavefront that eliminates row i+1 next takes rows 0 .. RLO-1, the one that has just
// eliminated row i-1 takes rows RLO .. K-1 and hands them over through LDS.  (A follower's pivot step is K
// double-precision FMAs per lane at 8 cycles each plus the multiplier reads - slower than the eliminating
// wavefront's step; with one follower per row the chain ran at the follower's pace, 0.8 us behind every row.)
// The high rows are subtracted a few pivots into the elimination (subtractions commute): the hand-over is off the
// critical path.  `spk` (compile time): this wavefront carries the 2K spike columns, else [S | H | E | y].
template <int K>
struct PipeRows {
  static constexpr int RLO = pipe_rlo<K>();   // even: the high rows' multipliers start 16-byte aligned
  static constexpr bool MFMA = pipe_mfma_follow<K>();
  static constexpr int NHI = K - RLO;
  static constexpr int JH = RLO >= 6 ? 4 : (RLO >= 2 ? RLO - 2 : 0);   // pivot at which the eliminating wavefront takes the high rows in
  static constexpr int XS = NHI + (NHI & 1);                          // stride of a column in the hand-over buffer
};

// the follower's loop over the pivot rows of the row before (ring slot at `prow`): acc[r - R0] += mu_r * v for the rows
// [R0, R0 + NR).  Software pipeline: the multipliers of pivot J + 1 are in flight while pivot J's terms are formed,
// and ONE poll tells how many rows have been published (lane l watches row l's word), so a follower that is behind
// does not poll at all.  `mid` runs once half-way.
// how many leading rows of a ring slot are published (main words, and the spike words when `spk`): ONE LDS read -
// lane l watches row l's main word, lane 32 + l its spike word
template <int K, bool spk>
struct PipeWatch {
  pipe_lds_int* w;
  int avail = 0;
  bool spk_wg;   // the workgroup carries spike columns (all eight wavefronts busy)
  __device__ __forceinline__ PipeWatch(const double* slot0, bool spk_wg_) : spk_wg(spk_wg_) {
    using G = PipeGeo<K>;
    const int lane = threadIdx.x & 63;
    w = (pipe_lds_int*)(slot0 + (lane < K ? lane * G::RS + G::od : (spk && lane >= 32 && lane < 32 + K) ? (lane - 32) * G::RS + G::og : G::oz)) + 1;
  }
  // returns once row J is published (bounded)
  __device__ __forceinline__ void need(const PipeCtl& ctl, int J) {
    int n = 0;
    while (J >= avail) {
      const unsigned long long pub = __builtin_amdgcn_ballot_w64((*w & 0x7ff80000) != 0x7ff80000);
      const int a0 = __builtin_ctzll(~pub | (1ull << K)), a1 = __builtin_ctzll(~(pub >> 32) | (1ull << K));
      avail = spk ? (a0 < a1 ? a0 : a1) : a0;
      if (J < avail) break;
      // (a poll is an LDS round trip and the row it waits for ~100 ns away: no nap where the wavefront has its SIMD to
      // itself; in the joiner workgroups two wavefronts share a SIMD, and a spinning follower takes issue slots from
      // the eliminating wavefront next to it - measured: rows 3.3 -> 4.0 us)
      if (spk_wg) __builtin_amdgcn_s_sleep(1);
      if (pipe_giveup(ctl, ++n)) { avail = K; break; }
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  }
};

template <int K, int R0, int NR, bool spk, bool SPKWG, class Mid>
__device__ __forceinline__ void pipe_follow(const PipeCtl& ctl, const double* __restrict__ prow, const int srcp, double (&acc)[NR > 0 ? NR : 1], Mid mid,
                                            double* dbg = nullptr) {
  using G = PipeGeo<K>;
  constexpr int RS = G::RS;
  static_assert((R0 & 1) == 0, "multiplier pairs");
  const int lane = threadIdx.x & 63;
  double mu[2][NR > 0 ? NR + 1 : 1], vv[2];
  (void)lane;
  PipeWatch<K, spk> watch(prow, SPKWG);
  auto need = [&](int J) { watch.need(ctl, J); };
  auto load = [&](int J, double (&m)[NR > 0 ? NR + 1 : 1], double& v) {
    const double2* p2 = reinterpret_cast<const double2*>(prow + J * RS + G::oH + R0);
#pragma unroll
    for (int q = 0; q < (NR + 1) / 2; ++q) { const double2 t2 = p2[q]; m[2 * q] = t2.x; m[2 * q + 1] = t2.y; }
    v = prow[J * RS + srcp];   // (unscaled: oRH / oRE / oRy; spike rows are published unscaled)
  };
  need(0);
  load(0, mu[0], vv[0]);
#pragma unroll
  for (int J = 0; J < K; ++J) {
    if (J + 1 < K) { need(J + 1); load(J + 1, mu[(J + 1) & 1], vv[(J + 1) & 1]); }
    if (J == (K + 1) / 2) mid();
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = __builtin_fma(mu[J & 1][r], vv[J & 1], acc[r]);
    if ((J == 4 || J == 9 || J == 14 || J == K - 1) && dbg) dbg[J == K - 1 ? 3 : J / 5] = (double)wall_clock64();   // (option "solver_debug")
  }
}

// The low follower on the matrix cores (K >= 17).  xr[r] -= sum_J (Ht[J][r] / d_J) * v[J][c] for the 16 rows r of one row
// tile and this lane's column c, where v = [Ht | Et | rt] unscaled (main wavefront: positions oRH ..., contiguous) or the
// spike row Ft (oF ...).  k-step sq = pivots 4 sq .. 4 sq + 3 of the ring slot, as soon as they are published: A operand
// the scaled rows D^-1 Ht (position oH + row; lane (fk, fl) reads row 4 sq + fk, entry fl), B operand three column tiles of
// v; pad rows of the slot are zeros.  What a pivot costs this wavefront: a quarter of (4 LDS reads of 8 bytes with a
// lane's own address + 3 matrix-core instructions) - against 5 broadcast reads of 16 bytes (1 KB of LDS bandwidth
// each) + 1 + 10 FMAs of pipe_follow; a joiner's followers read 35 such broadcasts per pivot, 280 cycles of the LDS
// pipeline against a pivot period of 250 (the solver's forward pass), which is what made a joiner's row 3.3 us
// where the eliminating wavefront needs 2.0.  The K terms of an entry are summed on their own (in the accumulator) and
// subtracted once, as before.  Columns of the tiles that no lane owns (pads, the words next to the spike row) are
// garbage in, garbage out: a column of B only reaches the same column of the product.  `pc`: this lane's product column
// (PIPE_HPC: none - the scratch's zero column).
template <int K, bool spk, bool SPKWG, class Mid>
__device__ __forceinline__ void pipe_follow_mfma(const PipeCtl& ctl, const double* __restrict__ prow, double* __restrict__ hp, const int pc,
                                                 double (&xr)[K], Mid mid, double* dbg = nullptr) {
  using G = PipeGeo<K>;
  using d4 = __attribute__((ext_vector_type(4))) double;
  constexpr int RS = G::RS, SK = (K + 3) / 4, CT = PIPE_HPC / 16, HS = PIPE_HS;
  static_assert(2 * G::KE + 1 <= PIPE_HPC && 2 * K <= PIPE_HPC, "product columns");
  static_assert(G::oRH + PIPE_HPC <= RS && G::oF + PIPE_HPC <= G::oRH, "B operand reads stay inside the row");
  const int lane = threadIdx.x & 63, fl = lane & 15, fk = lane >> 4;
  PipeWatch<K, spk> watch(prow, SPKWG);
  d4 acc[CT];
#pragma unroll
  for (int tc = 0; tc < CT; ++tc) acc[tc] = d4{0.0, 0.0, 0.0, 0.0};
  const double* op = prow + fk * RS + fl;
#pragma unroll
  for (int sq = 0; sq < SK; ++sq) {
    watch.need(ctl, (4 * sq + 3 < K ? 4 * sq + 3 : K - 1));
    const double* row = op + 4 * sq * RS;
    const double a = row[G::oH];
    double b[CT];
#pragma unroll
    for (int tc = 0; tc < CT; ++tc) b[tc] = row[(spk ? G::oF : G::oRH) + 16 * tc];
#pragma unroll
    for (int tc = 0; tc < CT; ++tc) acc[tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[tc], acc[tc], 0, 0, 0);
    if (sq == SK / 2) mid();
    if (dbg && sq >= 1 && sq <= 3) dbg[sq - 1] = (double)wall_clock64();   // (option "solver_debug")
  }
  // tiles -> this lane's column (the wavefront's own scratch: its LDS operations execute in order, no wait in between)
#pragma unroll
  for (int tc = 0; tc < CT; ++tc)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) hp[(16 * tc + fl) * HS + fk + 4 * rg] = acc[tc][rg];
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  const double2* h2 = reinterpret_cast<const double2*>(hp + pc * HS);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double2 v = h2[q];
    xr[2 * q] -= v.x;
    xr[2 * q + 1] -= v.y;
  }
  if (dbg) dbg[3] = (double)wall_clock64();
}

template <int K, bool SPK, bool spk>
__device__ __forceinline__ void pipe_chain_wave(const PipeArgs& A, const ChainCfg& cfg, const PipeLds& L, const PipeCtl& ctl,
                                                const int sigma) {
  extern __shared__ double lds[];
  using G = PipeGeo<K>;
  using R = PipeRows<K>;
  constexpr int ks = ldl_ks(K), RS = G::RS, GS = G::GS, NCS = G::NCX + (SPK ? 2 * K : 0);
  constexpr int RLO = R::RLO, NHI = R::NHI;
  const int lane = threadIdx.x & 63;
  const bool producer = cfg.producer != 0;
  const int nloc = cfg.nloc, m_split = cfg.m_split;
  const int nrows = nloc + (producer ? 2 : 0);
  double* ring = lds + L.ring;
  double* stg = lds + L.stage;
  double* gbuf = lds + L.gbuf;
  double* xhi = lds + L.xhi;
  const double qnan = __builtin_nan("");
  // this lane's column: position in a published row, column in the staging buffer / G / the hand-over buffer,
  // source position of the follower's update (what pivot row j of the row before contributes to this column)
  int pos, scol, gcol, src, rawpos = G::odump + (lane & 7);
  bool has_col = true;
  if (!spk) {
    if (lane < K) { pos = G::oS + lane; scol = lane; gcol = lane; src = G::oRH + lane; }
    else if (lane < 2 * K) { pos = G::oH + lane - K; scol = lane; gcol = -1; src = G::oRE + lane - K; rawpos = G::oRH + lane - K; }
    else if (lane < 3 * K) { pos = G::oE + lane - 2 * K; scol = lane; gcol = -1; src = -1; rawpos = G::oRE + lane - 2 * K; }
    else if (lane == 3 * K) { pos = G::oy; scol = lane; gcol = G::KE; src = G::oRy; rawpos = G::oRy; }
    else { pos = (lane == 62) ? G::od : (lane == 63) ? G::oi : G::odump + (lane & 7); scol = -1; gcol = -1; src = -1; has_col = false; }
  } else {
    if (lane < 2 * K) { pos = G::oF + lane; scol = G::NCX + lane; gcol = G::KE + 2 + lane; src = pos; }
    else { pos = (lane == 63) ? G::og : G::odump + (lane & 7); scol = -1; gcol = -1; src = -1; has_col = false; }
  }
  const int srcp = src >= 0 ? src : G::oz;
  // pipe_follow_mfma: the column of the product [Ht | Et | rt] (positions oRH ... of a row) / Ft that updates this lane's column
  const int hpc = src < 0 ? PIPE_HPC : (spk ? src - G::oF : src - G::oRH);
  const int xcol = has_col ? scol : NCS;   // (lanes without a column: a dump column of the hand-over buffer)
  const int f_slotgen = spk ? PF_SLOTGEN2 : PF_SLOTGEN, f_rowdone = spk ? PF_ROWDONE2 : PF_ROWDONE;
  const int f_initd = spk ? PF_INITD2 : PF_INITD, f_hidone = spk ? PF_HIDONE2 : PF_HIDONE;
  double xr[K];
  double diag0 = 1.0;
  int pending_release = -1;
  (void)pending_release;
  auto publishes = [&](int il) { return il >= 0 && il < nloc; };   // (a producer's pseudo-rows publish nothing)
  // the inputs of row il -> xr (staged by the I/O wavefront)
  auto init_row = [&](int il) {
    if (spk) {
      // coupling of this chain's first two rows to the separator rows (nearest first), see penta_nd.h:
      //   row 0: [coupling(row 0, nearest) | coupling(row 0, farthest)],  row 1: [coupling(row 1, nearest) | 0];
      // every other row's spike block is fill-in and starts from zero.  Straight from the band arrays.
      const int k = A.k, kk = k * k, dHB = (int)(A.HB - A.HA);
      const bool mir = cfg.mirror != 0;
      const int f = lane, ff = f < K ? f : f - K;
      const bool on = lane < 2 * K && (il == 0 || (il == 1 && f < K));
      int off = 0, stride = 0;
      if (on) {
        if (il == 0) { off = mir ? (f < K ? dHB + kk : 2 * kk) + ff : (f < K ? dHB : 0) + ff * k; }
        else { off = mir ? 2 * kk + ff : ff * k; }
        stride = mir ? k : 1;
      }
      const int o = mir ? cfg.base - il : cfg.base + il;
      const double* base = A.HA + (size_t)(o < 0 ? 0 : o) * kk + pipe_opaque(off);
      if (il < 2) pipe_rows_ready(A, ctl, o, o + 2, cfg.spin);   // (the coupling blocks sit in rows o + 1, o + 2 of the band arrays for both directions)
#pragma unroll
      for (int r = 0; r < K; ++r) xr[r] = (il < 2 && on) ? pipe_band(A, base + r * stride) : 0.0;
      return;
    }
    pipe_wait(ctl, PF_STAGED + (il & 1), il + 1);
    if (has_col) {
      const double2* s2 = reinterpret_cast<const double2*>(stg + (il & 1) * G::NCX * GS + scol * GS);
#pragma unroll
      for (int r2 = 0; r2 < K / 2; ++r2) { const double2 v = s2[r2]; xr[2 * r2] = v.x; xr[2 * r2 + 1] = v.y; }
      if (K & 1) xr[K - 1] = stg[(il & 1) * G::NCX * GS + scol * GS + K - 1];
    } else {
#pragma unroll
      for (int r = 0; r < K; ++r) xr[r] = 0.0;
    }
    // the diagonal entry of the band block this lane's pivot starts from (pivot test after the elimination)
    diag0 = (!spk && lane < K) ? stg[(il & 1) * G::NCX * GS + lane * GS + lane] : 1.0;
    if (!spk) pipe_post(ctl, f_initd + (il & 1), il + 1);
  };
  // x[r] -= G[r] for r < nr (rows of this lane's column of G = Et^T Dn [Et | rt | Ft] of row il - 2, gbuf[il & 1])
  auto sub_g = [&](int il, double (&x)[K], int nr) {
    const double2* g2 = reinterpret_cast<const double2*>(gbuf + (il & 1) * G::NGC * GS + gcol * GS);
#pragma unroll
    for (int r2 = 0; r2 < (K + 1) / 2; ++r2) {
      if (2 * r2 < nr) {
        const double2 v = g2[r2];
        x[2 * r2] -= v.x;
        if (2 * r2 + 1 < nr && 2 * r2 + 1 < K) x[2 * r2 + 1] -= v.y;
      }
    }
  };
  // follows row il - 1 with the HIGH rows of row il (which another wavefront will eliminate) and hands them over;
  // `mid`: what this wavefront does for itself half-way (loading its own next row's inputs)
  auto follow_high = [&](int il, auto mid) {
    if (NHI == 0 || il >= nrows || !publishes(il - 1)) { mid(); return; }
    const int pslot = (il + 2) % 3;
    pipe_wait(ctl, PF_SLOTGEN + pslot, il);
    if (spk) pipe_wait(ctl, PF_SLOTGEN2 + pslot, il);
    double acc[NHI > 0 ? NHI : 1];
#pragma unroll
    for (int r = 0; r < NHI; ++r) acc[r] = 0.0;
    pipe_follow<K, RLO, NHI, spk, SPK>(ctl, ring + pslot * G::SLOT, srcp, acc, [&] {
      mid();
      if (il >= 2 && gcol >= 0) {   // this half's share of G (added: the hand-over is subtracted)
        pipe_wait(ctl, PF_GDONE + (il & 1), il - 1);
        const double2* g2 = reinterpret_cast<const double2*>(gbuf + (il & 1) * G::NGC * GS + gcol * GS + RLO);
#pragma unroll
        for (int q = 0; q < (NHI + 1) / 2; ++q) {
          const double2 v = g2[q];
          acc[2 * q] += v.x;
          if (2 * q + 1 < NHI) acc[2 * q + 1] += v.y;
        }
      }
    });
    // (the buffer's previous contents - row il - 1's high rows - were taken in by the wavefront that has just
    // finished eliminating row il - 1)
    double* dst = xhi + xcol * R::XS;
#pragma unroll
    for (int r = 0; r < NHI; ++r) dst[r] = acc[r];
    pipe_post(ctl, f_hidone, il + 1);
  };

  if (sigma == 2) follow_high(1, [] {});   // (row 1's high rows: nobody has eliminated a row before row 0 yet)
  if (sigma < nrows) init_row(sigma);
  for (int il = sigma; il < nrows; il += 3) {
    const bool pseudo = il >= nloc;
    const int slot = il % 3, pslot = (il + 2) % 3;   // ring slots of this row and of the row before
    // option "solver_debug": phases of the fifth row of the chain (slots 8 .. 15 of the role's stamps)
    auto pstamp = [&](int k) { if (!spk && cfg.ts && il == 4 && lane == 0) cfg.ts[8 + k] = (double)wall_clock64(); };
    pstamp(0);
    const bool follow = publishes(il - 1);
    const bool take_high = NHI > 0 && follow;   // the other follower's rows (with their share of G) arrive through the hand-over buffer
    bool subg_done = il < 2;
    auto subg = [&]() {   // the update by Et of two rows before: G from the matrix cores (the rows the other follower does not cover)
      pipe_wait(ctl, PF_GDONE + (il & 1), il - 1);
      if (gcol >= 0) sub_g(il, xr, take_high ? RLO : K);
      subg_done = true;
    };
    // (join rows of a joiner: the producer's Schur-complement contributions were added to the row's inputs by the I/O
    // wavefront when it staged them - no chain wavefront ever waits on another workgroup's memory)
    if (il >= 3 && !pseudo) {
      // this row will be published into the ring slot of row il - 3: that row must have been consumed.  It has
      // long been, and here - before the row to follow has started - the check costs nothing.
      pipe_wait(ctl, PF_COPIED + slot, il - 2);
      pipe_wait(ctl, PF_GDONE + ((il - 3) & 1), il - 2);
    }
    // ---- follower of row il - 1: the LOW rows of this wavefront's own row
    if (follow) {
      pipe_wait(ctl, PF_SLOTGEN + pslot, il);
      if (spk) pipe_wait(ctl, PF_SLOTGEN2 + pslot, il);
      pstamp(2);
      if constexpr (R::MFMA) {
        pipe_follow_mfma<K, spk, SPK>(ctl, ring + pslot * G::SLOT, lds + L.hp + (spk ? PIPE_HPN : 0), hpc, xr,
                                      [&] { pstamp(4); if (!subg_done) subg(); },
                                      (!spk && cfg.ts && il == 4 && lane == 0) ? cfg.ts + 20 : nullptr);
        pstamp(5);
        if (!subg_done) subg();
        pstamp(6);
      } else {
      double acc[RLO];
#pragma unroll
      for (int r = 0; r < RLO; ++r) acc[r] = 0.0;
      pipe_follow<K, 0, RLO, spk, SPK>(ctl, ring + pslot * G::SLOT, srcp, acc, [&] { pstamp(4); if (!subg_done) subg(); },
                                  (!spk && cfg.ts && il == 4 && lane == 0) ? cfg.ts + 20 : nullptr);
      pstamp(5);
      if (!subg_done) subg();
      // (C - G) - sum: the K rank-one terms are summed on their own and subtracted once, as penta_ldl_body's
      // products phase does (subtracting them one by one rounds K times at the magnitude of C)
#pragma unroll
      for (int r = 0; r < RLO; ++r) xr[r] -= acc[r];
      pstamp(6);
      }
    }
    if (!subg_done) subg();
    auto high_rows = [&]() {
      if (!take_high) return;
      pipe_wait(ctl, f_hidone, il + 1);
      const double2* x2 = reinterpret_cast<const double2*>(xhi + xcol * R::XS);
#pragma unroll
      for (int q = 0; q < (NHI + 1) / 2; ++q) {
        const double2 v = x2[q];
        xr[RLO + 2 * q] -= v.x;
        if (2 * q + 1 < NHI) xr[RLO + 2 * q + 1] -= v.y;
      }
    };
    if (!producer && !spk && cfg.two && il >= m_split) {
      // ---- join rows of a joiner: + the producer's contributions (fetch_join, the I/O wavefront)
      pipe_wait(ctl, PF_JOINED, 1);
      const bool first = il == m_split;
      // stage column -> column of the buffer: S, H (first join row only), y
      const int jc = scol < K ? scol : (scol < 2 * K && first) ? scol : scol == 3 * K ? (first ? 2 * K : K) : -1;
      if (has_col && jc >= 0) {
        const double2* s2 = reinterpret_cast<const double2*>(lds + L.jbuf + (first ? 0 : (2 * K + 1) * G::KE) + jc * G::KE);
#pragma unroll
        for (int r2 = 0; r2 < K / 2; ++r2) { const double2 v = s2[r2]; xr[2 * r2] += v.x; xr[2 * r2 + 1] += v.y; }
        if (K & 1) xr[K - 1] += lds[L.jbuf + (first ? 0 : (2 * K + 1) * G::KE) + jc * G::KE + K - 1];
      }
    }
    if (pseudo) {
      // ---- producer: hand the column over (layout of penta_ldl_body's exchange buffer)
      high_rows();
      if (has_col) {   // (write-through, the epoch in every word: no fence, no flag - penta_nd.h ll_store)
        const int wo = pipe_opaque((il - nloc) * K * 64 + lane);   // column `lane` of [S | H | E | y]
#pragma unroll
        for (int r = 0; r < K; ++r) ll_store(A.join_ll + 2 * (wo + r * 64), xr[r], A.epoch);
      }
    } else {
      // ---- eliminate, publishing every pivot row
      double* rowp = ring + slot * G::SLOT + pos;
      if (!spk && cfg.ts && lane == 0 && il < 20) cfg.ts[24 + 2 * il] = (double)wall_clock64();   // option "solver_debug": elimination of row il starts ...
      if (lane < K) ring[slot * G::SLOT + lane * RS + (spk ? G::og : G::od)] = qnan;
      pipe_post(ctl, f_slotgen + slot, il + 1);
      if (!spk) {
        {
          double mu0[K];
#pragma unroll
          for (int r = 0; r < K; ++r) mu0[r] = 0.0;
          // (s_setprio 3 for the eliminating wavefront while it holds the role - VERDICT r3 #3 - was measured and dropped:
          // its K pivots stay at 1.96 us - the wavefront is bound by its own dependent chain and its LDS round trips, not
          // by lost issue slots - and the followers it starves make a joiner's row 3.36 -> 3.80 us:
          // profiles/r04_setprio_experiment.txt)
          pipe_pivot<K, 0, R::JH>(xr, pipe_rcp(rdlane(xr[0], 0)), mu0, 0.0, rowp, ring + slot * G::SLOT + rawpos, ring + slot * G::SLOT,
                                  lane == 63, high_rows, (cfg.ts && il == 3 && lane == 0) ? cfg.ts + 16 : nullptr);
        }
        pipe_post(ctl, f_rowdone + slot, il + 1);
        if (cfg.ts && lane == 0 && il < 20) cfg.ts[25 + 2 * il] = (double)wall_clock64();   // ... and ends
        // factorisation status (the reference reports kFailure from Factorize: penta_diagonal_solver.h:181-185,
        // trajectory_optimizer.cc:2084): every pivot positive, finite, and not cancelled to nothing against the
        // diagonal entry of H it started from (d <= eps H_ll: H is not numerically positive definite)
        const double il_ = (lane < K) ? ring[slot * G::SLOT + lane * RS + G::oi] : 1.0;   // 1 / d: NaN for d = 0 / inf / NaN
        const bool bad = lane < K && !(il_ > 0.0 && il_ * diag0 < 4503599627370496.0);
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) {
          __hip_atomic_store(A.status, A.fact_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_fetch_add(A.status + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if (cfg.ts) cfg.ts[7] = (double)(il + 1);
        }
      } else {
        // spike columns: Ft = L^-1 F with the multipliers D^-1 U the main wavefront publishes; rows go out unscaled
        if (cfg.ts && il == 4 && lane == 0) cfg.ts[16] = (double)wall_clock64();   // option "solver_debug": the spike wavefront's row 4 begins ...
        const double* arow = ring + slot * G::SLOT;
        double* fout = A.fst + (size_t)il * A.fstride + pipe_opaque(lane * ks);
        pipe_wait(ctl, PF_SLOTGEN + slot, il + 1);
        pipe_lds_int* watch = (pipe_lds_int*)(arow + (lane < K ? lane * RS + G::od : G::oz)) + 1;
        int avail = 0;
#pragma unroll
        for (int J = 0; J < K; ++J) {
          if (J == R::JH) high_rows();
          for (int n = 0; J >= avail;) {   // one poll covers every row the main wavefront has published
            avail = __builtin_ctzll(~__builtin_amdgcn_ballot_w64((*watch & 0x7ff80000) != 0x7ff80000) | (1ull << K));
            if (J < avail) break;
            __builtin_amdgcn_s_sleep(1);
            if (pipe_giveup(ctl, ++n)) { avail = K; break; }
          }
          __atomic_signal_fence(__ATOMIC_SEQ_CST);
          rowp[J * RS] = pipe_setlane<63>(xr[J], 0x3ff00000, 0);
          __atomic_signal_fence(__ATOMIC_SEQ_CST);
          if (lane < 2 * K) __hip_atomic_store(fout + J, xr[J], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (J + 1 < K) {
            const double2* p2 = reinterpret_cast<const double2*>(arow + J * RS);
#pragma unroll
            for (int m = (J + 1) / 2; m < (K + 1) / 2; ++m) {
              const double2 v = p2[m];
              if (2 * m > J) xr[2 * m] = __builtin_fma(-v.x, xr[J], xr[2 * m]);
              if (2 * m + 1 < K) xr[2 * m + 1] = __builtin_fma(-v.y, xr[J], xr[2 * m + 1]);
            }
          }
        }
        pipe_post(ctl, f_rowdone + slot, il + 1);
        if (cfg.ts && il == 4 && lane == 0) cfg.ts[17] = (double)wall_clock64();   // ... its last pivot is published ...
        // the row's spike block is in HBM: one of the three releases the separator waits for (the G wavefront adds two
        // with 1 / d and rt)
#ifdef PIPE_DEFER_RELEASE
        if (il + 3 >= nloc) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) __hip_atomic_fetch_add(A.frowcnt + il, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          pending_release = il;
        }
#else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(A.frowcnt + il, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        if (cfg.ts && il == 4 && lane == 0) cfg.ts[18] = (double)wall_clock64();   // ... and released to the separator
      }
    }
    // ---- follower of row il + 1: the HIGH rows of row il + 2 for the wavefront that eliminates it; half-way,
    // this wavefront's own next row's inputs
    bool inited = false;
    follow_high(il + 2, [&] { if (il + 3 < nrows) init_row(il + 3); inited = true; });
    if (!inited && il + 3 < nrows) init_row(il + 3);
    if (spk && cfg.ts && il == 4 && lane == 0) cfg.ts[19] = (double)wall_clock64();   // (the spike wavefront of row 4 has followed row 5)
#ifdef PIPE_DEFER_RELEASE
    if (spk && pending_release >= 0) {   // the stores of that row were issued a row ago: acknowledged by now
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_fetch_add(A.frowcnt + pending_release, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pending_release = -1;
    }
#endif
  }
}

// The forward pass of one chain.  512 threads (no spike columns: waves 0-2 eliminate in turn, 3 = I/O, 4 = G, the rest idle) or
// (SPK: waves 0-2 main columns, 3-5 spike columns, 6 = I/O, 7 = G and the spike rows out).
// On exit (after a block-wide barrier): factors in HBM, rt of every row in lds[L.xall ...], as penta_ldl_tail expects.
template <int K, bool SPK>
__device__ __forceinline__ void pipe_forward(const PipeArgs& A, const ChainCfg& cfg, const PipeLds& L) {
  extern __shared__ double lds[];
  using G = PipeGeo<K>;
  constexpr int ks = ldl_ks(K), KK = K * K, RS = G::RS, GS = G::GS, NCS = G::NCX + (SPK ? 2 * K : 0);
  // (the wavefront index is uniform: tell the compiler, or the chain wavefronts' row loop - which starts at
  // wave & 1 - becomes a divergent loop with every counter in a vector register)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool mirror = cfg.mirror != 0, producer = cfg.producer != 0;
  const int nloc = cfg.nloc, m_split = cfg.m_split;
  const int nrows = nloc + (producer ? 2 : 0);   // + the producer's two pseudo-rows (its contributions to the join rows)
  const int k = A.k, kk = k * k;
  auto orig = [&](int il) { const int o = mirror ? cfg.base - il : cfg.base + il; return o < 0 ? 0 : o; };
  double* ring = lds + L.ring;
  double* stg = lds + L.stage;
  double* gbuf = lds + L.gbuf;
  PipeCtl ctl{(pipe_lds_int*)(lds + L.flags), A.status, A.fact_id};
  const double qnan = __builtin_nan("");

  // ---- setup: what must be exact zeros - the flags, the pad rows of the ring slots (the matrix cores' k-steps read
  // them) and the position `oz` of every row, the rt rows - nothing else (LDS is 150 KB here; everything else is
  // written before it is read)
  for (int idx = tid; idx < 32; idx += blockDim.x) lds[L.flags + idx] = 0.0;
  if (tid == 0) {   // (behind the zero fill: words 40, 41 are idx 20, written by lane 20 of this same wavefront one instruction earlier)
    const long long now = (long long)wall_clock64();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    ctl.f[PF_T0] = (int)(unsigned)now; ctl.f[PF_T0 + 1] = (int)(now >> 32);
  }
  for (int idx = tid; idx < 3 * (G::KR - K) * RS; idx += blockDim.x) {
    const int sl = idx / ((G::KR - K) * RS), e = idx - sl * (G::KR - K) * RS;
    ring[sl * G::SLOT + K * RS + e] = 0.0;
  }
  for (int idx = tid; idx < 3 * K; idx += blockDim.x) ring[(idx / K) * G::SLOT + (idx % K) * RS + G::oz] = 0.0;
  for (int idx = tid; idx < (ND_MAXROWS + 2) * GS; idx += blockDim.x) lds[L.xall + idx] = 0.0;
  if (pipe_mfma_follow<K>())   // pipe_follow_mfma: the scratch's zero column (main, spike)
    for (int idx = tid; idx < (SPK ? 2 : 1) * PIPE_HS; idx += blockDim.x) lds[L.hp + (idx / PIPE_HS) * PIPE_HPN + PIPE_HPC * PIPE_HS + idx % PIPE_HS] = 0.0;
  __syncthreads();
  chain_ts(cfg, 0);

  constexpr int W_SPK0 = 3, W_IO = SPK ? 6 : 3, W_G = 7;   // (G on the SIMD it shares with the I/O or a spike wavefront, not with a main one)

  if (wave < 3) {
    pipe_chain_wave<K, SPK, false>(A, cfg, L, ctl, wave);
  } else if (SPK && wave < W_SPK0 + 3) {
    pipe_chain_wave<K, SPK, true>(A, cfg, L, ctl, wave - W_SPK0);
  } else if (wave == W_IO) {
    // =====================================================================================================
    // I/O wavefront: stages the band blocks of row t + 2 (column layout), writes the factors of row t out
    constexpr int PM = (G::NCX * K + 63) / 64;   // (the spike columns' inputs: only rows 0 and 1, below)
    const int dHB = (int)(A.HB - A.HA), dHC = (int)(A.HC - A.HA);
    // per-lane slots (fixed over the rows): source offset relative to the row's A block (or to its right-hand
    // side), destination in the staging buffer, which part the element belongs to
    int s_off[PM], s_dst[PM];
    unsigned long long mH = 0, mE = 0, mY = 0, mAny = 0;
    static_assert(PM <= 64, "slot masks are 64-bit");
#pragma unroll
    for (int s = 0; s < PM; ++s) {
      const int e = lane + 64 * s;
      const bool valid = e < G::NCX * K;
      const int c = valid ? e / K : 0, r = valid ? e - c * K : 0;
      s_dst[s] = valid ? c * GS + r : 2 * G::NCX * GS;   // (one dump double behind the two staging buffers)
      s_off[s] = 0;
      if (!valid) continue;
      if (c < K) { s_off[s] = dHC + c * k + r; mAny |= 1ull << s; }
      else if (c < 2 * K) { const int cc = c - K; s_off[s] = mirror ? dHB + cc * k + r : dHB + kk + r * k + cc; mH |= 1ull << s; mAny |= 1ull << s; }
      else if (c < 3 * K) { const int cc = c - 2 * K; s_off[s] = mirror ? cc * k + r : 2 * kk + r * k + cc; mE |= 1ull << s; mAny |= 1ull << s; }
      else if (c == 3 * K) { s_off[s] = r; mY |= 1ull << s; mAny |= 1ull << s; }
    }
    auto stage_row = [&](int il) {
      const bool pseudo = il >= nloc;
      const int o = orig(il);
      const double* base = A.HA + (size_t)o * kk;
      const double* bp = A.b + (size_t)o * k;
      double* dst = stg + (il & 1) * G::NCX * GS;
      // join rows of a joiner have no coupling beyond the join, a producer's pseudo-rows have all-zero inputs
      unsigned long long kill = ~mAny;
      if (pseudo) kill = ~0ull;
      else if (!producer && cfg.two) kill |= (il >= m_split ? mE : 0ull) | (il >= m_split + 1 ? mH : 0ull);
      if (!pseudo) pipe_rows_ready(A, ctl, o, mirror ? o : o + 2, cfg.spin);
      if (il == 0 && A.ts && lane == 0) A.ts[7] = (double)wall_clock64();   // (debug: the first row's inputs are assembled)
      double val[PM];
      if (A.asm_ready) {
#pragma unroll
        for (int s = 0; s < PM; ++s) {
          const double* p = (mY >> s & 1) ? bp : base;
          val[s] = __hip_atomic_load(p + s_off[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else {
#pragma unroll
        for (int s = 0; s < PM; ++s) {
          const double* p = (mY >> s & 1) ? bp : base;
          val[s] = p[s_off[s]];
        }
      }
#pragma unroll
      for (int s = 0; s < PM; ++s) {
        double v = (mY >> s & 1) ? A.rhs_sign * val[s] : val[s];
        v = (kill >> s & 1) ? 0.0 : v;
        if (s_dst[s] < 2 * G::NCX * GS) dst[s_dst[s]] = v;
      }
    };
    // The producer's Schur-complement contributions to the joiner's two join rows (its two pseudo-rows; penta_nd.h
    // ll_store: every value carries the epoch, the lanes poll the data itself, all 36 loads of a lane in flight at
    // once) -> LDS, columns [S | H | y] for the join row next to the producer (X0 = pseudo-row 1, and the coupling of
    // the two join rows, H(r, c) += H'(c, r)), [S | y] for the other (X1 = pseudo-row 0).  Source slots: [pseudo
    // row][r][column: 64].  The chain wavefronts pick the values up from LDS after they have followed the row before:
    // none of them ever waits on another workgroup's memory.  One attempt; false: not all there yet.
    auto fetch_join = [&]() {
      constexpr int NV1 = (2 * K + 1) * K, NV2 = (K + 1) * K, PM1 = (NV1 + 63) / 64, PM2 = (NV2 + 63) / 64;
      const unsigned long long* q = reinterpret_cast<const unsigned long long*>(A.join_ll);
      double add[PM1 + PM2];
      bool good = true;
#pragma unroll
      for (int s = 0; s < PM1 + PM2; ++s) {
        const bool one = s < PM1;
        const int v = lane + 64 * (one ? s : s - PM1), c = v / K, r = v - c * K;
        const bool in = v < (one ? NV1 : NV2);
        int src = 0;
        if (one) src = c < K ? K * 64 + r * 64 + c : c < 2 * K ? (c - K) * 64 + K + r : K * 64 + r * 64 + 3 * K;
        else src = c < K ? r * 64 + c : r * 64 + 3 * K;
        src = in ? src : 0;
        const unsigned long long a = __hip_atomic_load(q + 2 * src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long b = __hip_atomic_load(q + 2 * src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add[s] = __longlong_as_double((long long)((a & 0xffffffffull) | (b << 32)));
        good = good && (!in || ((unsigned)(a >> 32) == A.epoch && (unsigned)(b >> 32) == A.epoch));
      }
      if (__builtin_amdgcn_ballot_w64(good) != __builtin_amdgcn_ballot_w64(true)) return false;
      double* jb = lds + L.jbuf;
#pragma unroll
      for (int s = 0; s < PM1 + PM2; ++s) {
        const bool one = s < PM1;
        const int v = lane + 64 * (one ? s : s - PM1), c = v / K, r = v - c * K;
        if (v < (one ? NV1 : NV2)) jb[(one ? 0 : (2 * K + 1) * G::KE) + c * G::KE + r] = add[s];
      }
      return true;
    };
    bool join_done = producer || !cfg.two;
    auto copy_row = [&](int il) {
      const int slot = il % 3, o = orig(il);
      const double* row0 = ring + slot * G::SLOT;
      for (int idx = lane; idx < K * ks; idx += 64) {
        const int r = idx / ks, c = idx - r * ks;
        const double* row = row0 + r * RS;
        const bool in = c < K;
        A.Ust[(size_t)o * K * ks + idx] = (in && r < c) ? row[G::oS + c] : 0.0;
        A.Hst[(size_t)o * K * ks + idx] = in ? row[G::oH + c] : 0.0;
        A.Est[(size_t)o * K * ks + idx] = in ? row[G::oE + c] : 0.0;
      }
      if (lane < K) {
        // (a chain with spike columns: the G wavefront sends 1 / d and rt to HBM as the pivots appear - the separator reads
        // them, and this wavefront's copies of finished rows queue up behind the join)
        if (!SPK) A.Dst[(size_t)o * K + lane] = row0[lane * RS + G::oi];
        lds[L.xall + (il + 2) * ks + lane] = row0[lane * RS + G::oRy];   // rt (unscaled) for the back substitution
      }
    };
    stage_row(0);
    pipe_post(ctl, PF_STAGED + 0, 1);
    if (nrows > 1) { stage_row(1); pipe_post(ctl, PF_STAGED + 1, 2); }
    int copied = 0;   // rows whose factors are written out
    for (int t = 0; t < nrows; ++t) {
      if (t + 2 < nrows) {
        pipe_wait(ctl, PF_INITD + (t & 1), t + 1);
        stage_row(t + 2);
        pipe_post(ctl, PF_STAGED + (t & 1), t + 3);
      }
      // the producer's contributions (fetch_join): a look when the row before the last is staged, the wait proper
      // when the last one is.  From the first look on the factors of finished rows wait their turn (the ring slot of
      // row t is not needed again before row t + 3): the chains want the join data the moment the row before the
      // join has been followed, and copy_row's release fence alone is ~1 us.
      if (!join_done && t + 2 >= m_split) {
        if (cfg.ts && lane == 0 && t + 1 >= m_split) cfg.ts[1] = (double)wall_clock64();
        if (t + 1 >= m_split) { if (!spin_wait(fetch_join, cfg.spin)) ctl.f[PF_ABORT] = 1; join_done = true; }
        else join_done = fetch_join();
        if (join_done) {
          pipe_post(ctl, PF_JOINED, 1);
          if (cfg.ts && lane == 0) cfg.ts[5] = (double)wall_clock64();
        }
      }
      if (!join_done && t + 2 >= m_split) continue;
      for (; copied <= t && copied < nloc; ++copied) {
        pipe_wait(ctl, PF_ROWDONE + copied % 3, copied + 1);
        copy_row(copied);
        pipe_post(ctl, PF_COPIED + copied % 3, copied + 1);
      }
    }
  } else if (wave == W_G) {
    // =====================================================================================================
    // G = Et_t^T Dn [Et_t | rt_t | Ft_t] on the matrix cores: A operand the scaled rows D^-1 Et, B operand the
    // unscaled [Et | rt] (oRE ...) and spike rows (oF ...)
    using d4 = __attribute__((ext_vector_type(4))) double;
    constexpr int SK = (K + 3) / 4, TT = (K + 15) / 16;
    constexpr int NCG = SPK ? G::NGC : G::KE + 1;        // columns of G that exist
    constexpr int CT = (NCG + 15) / 16;
    const int fl = lane & 15, fk = lane >> 4;
    // (a chain with spike columns: this wavefront also hands the separator 1 / d_J and rt_J of every row - lanes 0 .. 3
    // and 4 .. 7, four pivots per k-step - and releases them; the spike wavefront releases the spike block itself)
    const int xr4 = lane & 3;
    const int xpos = (lane >> 2) == 0 ? G::oi : G::oRy;
    for (int t = 0; t < nloc; ++t) {
      const int slot = t % 3;
      const double* row0 = ring + slot * G::SLOT;
      const bool prod = t + 2 < nrows;   // (else nobody is two rows ahead)
      if (!prod && SPK) {
        pipe_wait(ctl, PF_SLOTGEN + slot, t + 1);
        PipeWatch<K, false> watch(row0, true);
        double* xout = (lane >> 2) == 0 ? A.Dst + (size_t)orig(t) * K : A.fst + (size_t)t * A.fstride + 2 * K * ks;
#pragma unroll
        for (int sq = 0; sq < SK; ++sq) {
          watch.need(ctl, (4 * sq + 3 < K ? 4 * sq + 3 : K - 1));
          const int r = 4 * sq + xr4;
          if (lane < 8 && r < K) __hip_atomic_store(xout + r, row0[r * RS + xpos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (prod) {
        // The products run WHILE the row is being eliminated: k-step sq (pivot rows 4 sq .. 4 sq + 3) as soon as
        // those rows are published, so that G is complete a k-step after the row's last pivot and the followers
        // of the row after next can take it in early.
        pipe_wait(ctl, PF_SLOTGEN + slot, t + 1);
        if (SPK) pipe_wait(ctl, PF_SLOTGEN2 + slot, t + 1);
        PipeWatch<K, SPK> watch(row0, true);
        double* xout = !SPK ? nullptr : (lane >> 2) == 0 ? A.Dst + (size_t)orig(t) * K : A.fst + (size_t)t * A.fstride + 2 * K * ks;
        d4 acc[CT][TT];
#pragma unroll
        for (int tc = 0; tc < CT; ++tc)
#pragma unroll
          for (int tr = 0; tr < TT; ++tr) acc[tc][tr] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int sq = 0; sq < SK; ++sq) {
          watch.need(ctl, (4 * sq + 3 < K ? 4 * sq + 3 : K - 1));
          if (SPK) {
            const int r = 4 * sq + xr4;
            if (lane < 8 && r < K) __hip_atomic_store(xout + r, row0[r * RS + xpos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          const double* row = row0 + (4 * sq + fk) * RS;   // (pad rows: zeros)
          double a[TT], bq[CT];
#pragma unroll
          for (int tr = 0; tr < TT; ++tr) a[tr] = row[G::oE + 16 * tr + fl];
#pragma unroll
          for (int tc = 0; tc < CT; ++tc) {
            const int ci = 16 * tc + fl;                                                // column of G
            bq[tc] = row[ci < G::KE + 2 ? G::oRE + ci : G::oF + ci - (G::KE + 2)];       // where its operand sits in a row
          }
#pragma unroll
          for (int tc = 0; tc < CT; ++tc)
#pragma unroll
            for (int tr = 0; tr < TT; ++tr) acc[tc][tr] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tr], bq[tc], acc[tc][tr], 0, 0, 0);
        }
        double* gout = gbuf + (t & 1) * G::NGC * GS;
#pragma unroll
        for (int tc = 0; tc < CT; ++tc)
#pragma unroll
          for (int tr = 0; tr < TT; ++tr)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
              const int r = 16 * tr + fk + 4 * rg, ci = 16 * tc + fl;
              if (r < K && ci < NCG) gout[ci * GS + r] = acc[tc][tr][rg];
            }
        pipe_post(ctl, PF_GDONE + (t & 1), t + 1);
      }
      if (SPK) {   // two of the three releases of the row: a drained store queue
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(A.frowcnt + t, 2ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  if (tid == 0 && ctl.f[PF_ABORT] != 0 && cfg.spin.word) {   // a wait gave up: tell the host (it repeats the solve)
    __hip_atomic_store(cfg.spin.word, cfg.spin.id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_fetch_add(cfg.spin.word + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  chain_ts(cfg, 2);
}

// ---- back substitution of a chain in recursion form.
// penta_ldl_tail solves  U_i x_i = Dn rt_i - (Dn Ht_i) x_{i+1} - (Dn Et_i) x_{i+2}  row after row: K dependent
// (v_readlane, FMA) steps per block row on one wavefront, 0.8 us per row, all of it on the critical path after the
// separator has answered.  But a chain's workgroup is IDLE between the end of its forward pass and that answer
// (10 us for the joiners, 25 us for the producers).  In that time all its wavefronts form, for every row at once,
//   [Y_i | Z_i | c_i | W_i] = U_i^-1 [Dn Ht_i | Dn Et_i | Dn rt_i | Dn Ft_i]
// (K back substitutions with one column per lane, the reference's Y_i, Z_i: optimizer/penta_diagonal_solver.h:160-178),
// so that what remains afterwards is  c_i -= W_i x_sep  (all rows in parallel) and
//   x_i = c_i - Y_i x_{i+1} - Z_i x_{i+2},
// two dense K x K mat-vecs per row with x passed through LDS: ~0.12 us per row.
// LDS (everything the forward pass used is free): per local row [Y | Z] row-major (stride 2 KE), W likewise, c.
// (PipeBack: solver_layout.h)

// v[lane] + v[lane ^ 32] in every lane: one v_permlane32_swap per 32-bit half (a ds_bpermute round trip costs ~100 cycles)
__device__ __forceinline__ double pipe_half_sum(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

template <int K, bool SPK>
__device__ __forceinline__ bool pipe_backward_fits(const PipeLds& L, int nloc) { return nloc * PipeBack<K, SPK>::BS + 4 * PipeBack<K, SPK>::KE + 2 <= L.xall; }

// ---- a producer's recursion in closed form.
// A producer has its [Y_i | Z_i | c_i] ~16 us before the joiner's two join rows of x arrive, and then walks its rows one
// after the other on one wavefront (0.24 us a row).  Everything in that walk but the 2K numbers of the join rows is known
// beforehand: with T_nloc = [I 0 | 0], T_nloc+1 = [0 I | 0] and
//   T_i = [G_i | chat_i] = [0 | c_i] - Y_i T_{i+1} - Z_i T_{i+2}            (the recursion on 2K + 1 right-hand sides)
// every row is x_i = chat_i + G_i [x_nloc ; x_nloc+1].  The T_i are formed in the idle time - nloc dependent products
// [Y_i | Z_i] (K x 2KE) times [T_{i+1} ; T_{i+2}] (2KE x (2KE + 1)) on the matrix cores, a 16 x 16 tile per wavefront,
// a barrier per row - and the arrival of the join rows costs one mat-vec, all rows side by side.
// (The order of every sum is fixed by the tiling: the result does not depend on timing.  PipeClosed: solver_layout.h)
template <int K>
__device__ __forceinline__ bool pipe_closed_fits(const PipeLds& L, int nloc) { return PipeClosed<K>::end(nloc) <= L.xall; }

// (Called from the kernel's body behind pipe_backward, which returns after phase 1 and leaves what this needs to know
// in the LDS, PipeClosed::PAR: as a part of pipe_backward with its arguments in scalar registers, the deciding launch's
// kernel <19, true> spilled 241 .. 249 SGPRs instead of 204 - tools/check_resources.py allows 228 -, although this runs
// behind the forward pass and shares nothing with it; as a function that is called, it rounds the kernels' 36 B of
// scratch up to 48.  This way: 221.)
template <int K>
__device__ __forceinline__ void pipe_closed_tail() {
  extern __shared__ double lds[];
  using B = PipeBack<K, false>;
  using C = PipeClosed<K>;
  using d4 = __attribute__((ext_vector_type(4))) double;
  constexpr int KE = B::KE, YS = B::YS, TS = C::TS, NC = C::NC;
  constexpr int TT = (K + 15) / 16, CT = (NC + 15) / 16, SK = 2 * KE / 4;
  static_assert(2 * K <= 64, "a lane per component of the two join rows");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nt = blockDim.x, nwaves = nt >> 6;
  // (what the caller knows comes through the LDS, PipeClosed::PAR, and stays in vector registers)
  const int xall = pipe_layout<K>(0, false).xall;
  const unsigned long long* par = reinterpret_cast<const unsigned long long*>(lds + xall + C::PAR);
  const int nloc = __builtin_amdgcn_readfirstlane((int)(unsigned)par[5]);
  double* x = reinterpret_cast<double*>(par[0]);
  const double* xjoin_ll = reinterpret_cast<const double*>(par[1]);
  const SpinCtl spin = {reinterpret_cast<unsigned*>(par[2]), (unsigned)(par[4] >> 32)};
  double* ts = reinterpret_cast<double*>(par[3]);
  const unsigned epoch = (unsigned)par[4];
  const int k = (int)(unsigned)(par[5] >> 32), base = (int)(unsigned)par[6], mirror = (int)(unsigned)(par[6] >> 32);
  auto orig = [&](int il) { const int o = mirror ? base - il : base + il; return o < 0 ? 0 : o; };
  double* T = lds + C::base(nloc);
  // the two join rows' slots: the identity
  for (int idx = tid; idx < 2 * C::SLOT; idx += nt) {
    const int h = idx / C::SLOT, r = (idx - h * C::SLOT) / TS, n = idx - h * C::SLOT - r * TS;
    T[nloc * C::SLOT + idx] = (n == h * KE + r) ? 1.0 : 0.0;
  }
  __syncthreads();
  const int fl = lane & 15, fk = lane >> 4;
  for (int il = nloc - 1; il >= 0; --il) {
    const double* yz = lds + il * B::BS + B::oYZ;
    const double* cc = lds + il * B::BS + B::oC;
    double* Ti = T + il * C::SLOT;
    for (int tile = wave; tile < TT * CT; tile += nwaves) {
      const int tr = tile / CT, tc = tile - tr * CT;
      const int ar = 16 * tr + fl < K ? 16 * tr + fl : K - 1;      // (rows past K: a copy of the last row, never stored)
      const int bn = 16 * tc + fl < NC ? 16 * tc + fl : NC - 1;    // (columns past chat likewise)
      double a[SK], b[SK];
#pragma unroll
      for (int sq = 0; sq < SK; ++sq) {
        const int p = 4 * sq + fk, h = p >= KE ? 1 : 0, pr = p - h * KE;   // position in [Y | Z]: row pr of T_{il+1+h}
        a[sq] = yz[ar * YS + p];
        const double t = Ti[(1 + h) * C::SLOT + (pr < K ? pr : K - 1) * TS + bn];
        b[sq] = pr < K ? t : 0.0;   // (the pad column of Y, Z is zero; what it meets must be a number)
      }
      d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int sq = 0; sq < SK; ++sq) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[sq], b[sq], acc, 0, 0, 0);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int r = 16 * tr + fk + 4 * rg, n = 16 * tc + fl;
        if (r < K && n < NC) Ti[r * TS + n] = (n == NC - 1 ? cc[r] : 0.0) - acc[rg];
      }
    }
    __syncthreads();
  }
  if (ts && tid == 0) ts[21] = (double)wall_clock64();
  // ---- the join rows arrive: a thread per (row, component), its row of G and chat in registers before the wait.
  // Every wavefront that has rows polls the 2K words itself (the existing flagged words, the bounded poll) and keeps
  // its own copy in what held rt of the local rows: no barrier behind the arrival.
  if (wave * 64 >= nloc * K) return;
  double* xj = lds + xall + wave * 2 * KE;
  if (lane < 2 * KE) xj[lane] = 0.0;
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  const int idx0 = wave * 64 + lane, idx = idx0 < nloc * K ? idx0 : 0, il = idx / K, r = idx - il * K;
  double g[2 * KE];
  {
    const double2* g2 = reinterpret_cast<const double2*>(T + il * C::SLOT + r * TS);
#pragma unroll
    for (int m = 0; m < KE; ++m) { const double2 v = g2[m]; g[2 * m] = v.x; g[2 * m + 1] = v.y; }
  }
  const double chat = T[il * C::SLOT + r * TS + NC - 1];
  if (lane < 2 * K) {   // local row nloc (next to this chain) is the joiner's second join row
    const int h = lane >= K ? 1 : 0, c = lane - h * K;
    xj[h * KE + c] = ll_load(xjoin_ll + 2 * ((1 - h) * K + c), epoch, spin);
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  if (ts && tid == 0) ts[22] = (double)wall_clock64();
  const double2* x2 = reinterpret_cast<const double2*>(xj);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int m = 0; m < KE; m += 2) {
    const double2 u = x2[m], v = x2[m + 1];
    a0 = __builtin_fma(g[2 * m], u.x, a0); a1 = __builtin_fma(g[2 * m + 1], u.y, a1);
    a2 = __builtin_fma(g[2 * m + 2], v.x, a2); a3 = __builtin_fma(g[2 * m + 3], v.y, a3);
  }
  const double v = chat + ((a0 + a1) + (a2 + a3));
  if (idx0 < nloc * K && r < k) x[(size_t)orig(il) * k + r] = v;
  if (ts && tid == 0) ts[4] = (double)wall_clock64();
}

// WGLOB (the seven-workgroup kernel's chains, 4 wavefronts, K = 23 / 29: 16 rows of [Y | Z | c] are 141 KB): W_il goes
// to global memory (A.wst) instead of the LDS - it is read once, a row per thread, and those loads are issued before the
// wait for the separator, where the row-by-row tail fetched Ft_il.  The spike rows come from another workgroup there
// (cfg.frowcnt counts them in).
template <int K, bool SPK, bool WGLOB = false>
__device__ __forceinline__ void pipe_backward(const PipeArgs& A, const ChainCfg& cfg, const PipeLds& L) {
  extern __shared__ double lds[];
  using B = PipeBack<K, SPK && !WGLOB>;
  constexpr int ks = ldl_ks(K), KE = B::KE, YS = B::YS, KS2 = K * ks;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
  const bool mirror = cfg.mirror != 0, producer = cfg.producer != 0;
  const int nloc = cfg.nloc, m_split = cfg.m_split, k = A.k;
  auto orig = [&](int il) { const int o = mirror ? cfg.base - il : cfg.base + il; return o < 0 ? 0 : o; };
  double* xb = lds + nloc * B::BS;   // [4][KE]: x of the last rows, for the broadcast reads
  // ---- phase 1 (no dependence on other workgroups): the recursion matrices of every row, rows over wavefronts.
  // Two passes ([Y | Z | c], then W): one pass with both solves keeps 2 x 171 multipliers alive in the compiler's eyes.
  // (Branch-free: every lane loads from somewhere and stores somewhere - a dump double behind the x ring for the lanes
  // without a column - or the register allocator loses the row vector to scratch in the exec-mask maze.)
  double* dump = xb + 4 * KE;
  auto solve = [&](const double* Us, double (&xr)[K]) __attribute__((always_inline)) {   // xr <- U^-1 xr, U = I + strictly upper (rows of Us), bottom row first
    constexpr int NP = (K + 1) / 2;
    double2 ub[2][NP];   // the multipliers of a row are read while the row below is applied
    auto loadu = [&](int r, double2 (&u)[NP]) __attribute__((always_inline)) {
      const double2* u2 = reinterpret_cast<const double2*>(Us + r * ks);
#pragma unroll
      for (int m = (r + 1) / 2; m < NP; ++m) u[m] = u2[m];
    };
    if (K >= 2) loadu(K - 2, ub[0]);
#pragma unroll
    for (int q = 0; q < K - 1; ++q) {
      const int r = K - 2 - q;
      if (r >= 1) loadu(r - 1, ub[(q + 1) & 1]);
      asm volatile("" ::: "memory");   // (keeps the reads where they are: left alone the compiler reads all K (K - 1) / 2 multipliers first, 360 registers)
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int m = (r + 1) / 2; m < NP; ++m) {
        const double2 u = ub[q & 1][m];
        if (2 * m > r) a0 = __builtin_fma(u.x, xr[2 * m], a0);
        if (2 * m + 1 < K) a1 = __builtin_fma(u.y, xr[2 * m + 1], a1);
      }
      xr[r] -= a0 + a1;
    }
  };
  // (one list of tasks, [Y | Z | c] of every row, then W of every row, dealt out over the wavefronts: a loop over the
  // rows per pass left six of eight wavefronts idle in every pass's last round - 4 rounds of ~2.4 us for a joiner's
  // 2 x 10 tasks instead of 3)
  // (WGLOB: pass 1 is a row of the PARTNER joiner's - this workgroup is the pair's producer, idle for 40 us after its
  // own forward pass, the joiner for 25 and with three more rows: W_il = U_il^-1 Dn Ft_il from the joiner's factors and
  // the spike workgroup's row, both released through the spike row's counter, into the joiner's wst)
  auto do_pass = [&](const int il, const int pass, const bool stage) __attribute__((always_inline)) {
    const bool partner = WGLOB && pass == 1;
    if (partner) {
      spin_wait([&] { return __hip_atomic_load(cfg.wp_frowcnt + il, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= cfg.frowtarget; }, cfg.spin);
      (void)__hip_atomic_load(cfg.wp_frowcnt + il, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int op = cfg.wp_mirror ? cfg.wp_base - il : cfg.wp_base + il;
    const int o = partner ? (op < 0 ? 0 : op) : orig(il);
    double* slot = lds + il * B::BS;
    // D^-1 U staged where this task's results go (row-major, stride ks): another wavefront may be on the row's other task
    // (a partner's row: in the wavefront's scratch behind the separator's solution)
    double* Us = partner ? lds + L.W + 2 * KE + 2 + wave * KS2 : slot + ((pass && !WGLOB) ? B::oW : B::oYZ);
    constexpr int NU = (KS2 + 63) / 64;
    double uv[NU];   // (all global loads of the task are issued before anything waits for one)
    if (stage) {
#pragma unroll
      for (int t = 0; t < NU; ++t) uv[t] = A.Ust[(size_t)o * KS2 + (lane + 64 * t < KS2 ? lane + 64 * t : 0)];
    }
    const double dinv = (lane < K) ? A.Dst[(size_t)o * K + lane] : 0.0;   // lane r: 1 / d_r
    double xr[K];
    double* dst = dump;
    int dstride = 0;
    if (pass == 0) {   // columns [Dn Ht | Dn Et | Dn rt]; the two pad entries of a row of [Y | Z] (odd K) are cleared on the way
      const double* src = (lane < K) ? A.Hst + (size_t)o * KS2 + lane : A.Est + (size_t)o * KS2 + (lane < 2 * K ? lane - K : 0);
      const double mg = lane < 2 * K ? 1.0 : 0.0, mc = lane == 2 * K ? 1.0 : 0.0;
#pragma unroll
      for (int r = 0; r < K; ++r) xr[r] = src[r * ks] * mg + (rdlane(dinv, r) * lds[L.xall + (il + 2) * ks + r]) * mc;
      if (lane < 2 * K) { dst = slot + B::oYZ + (lane < K ? lane : KE + lane - K); dstride = YS; }
      else if (lane == 2 * K) { dst = slot + B::oC; dstride = 1; }
      else if ((K & 1) && lane <= 2 * K + 2) { dst = slot + B::oYZ + (lane == 2 * K + 1 ? K : KE + K); dstride = YS; }   // (xr = 0 there)
    } else {           // columns Dn Ft (the coupling to the separator)
      const double* fsrc = (WGLOB ? cfg.wp_fst : A.fst) + (size_t)il * A.fstride + (size_t)(lane < 2 * K ? lane : 0) * ks;
      const double mf = lane < 2 * K ? 1.0 : 0.0;
#pragma unroll
      for (int r = 0; r < K; ++r) xr[r] = (rdlane(dinv, r) * fsrc[r]) * mf;
      if (WGLOB) {
        if (lane < 2 * K) { dst = cfg.wp_wst + (size_t)il * A.fstride + (size_t)lane * ks; dstride = 1; }
      } else {
        if (lane < 2 * K) { dst = slot + B::oW + (lane < K ? lane : KE + lane - K); dstride = YS; }
        else if ((K & 1) && lane <= 2 * K + 1) { dst = slot + B::oW + (lane == 2 * K ? K : KE + K); dstride = YS; }
      }
    }
    if (stage) {
#pragma unroll
      for (int t = 0; t < NU; ++t) if (lane + 64 * t < KS2) Us[lane + 64 * t] = uv[t];
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    solve(Us, xr);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (the staged U may sit where the results go)
    if (partner) {
      // a row of W for the joiner: write-through stores, their acknowledgements, then the row's word - the joiner
      // fetches a row as soon as its word is there (one flag for all rows left the whole fetch, 92 loads per thread and
      // ~4 us, behind the last row).  The stores go out lanes side by side (scattered 8-byte write-through stores - a
      // column per lane, as the registers hold it - cost four times as much): a half of the row at a time through the
      // wavefront's scratch, which the substitution no longer needs.
      double* Tw = Us;
      double* wrow_dst = cfg.wp_wst + (size_t)il * A.fstride;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (lane >= half * K && lane < half * K + K) {
#pragma unroll
          for (int r = 0; r < K; ++r) Tw[(lane - half * K) * ks + r] = xr[r];
        }
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
        for (int t = 0; t < NU; ++t)
          if (lane + 64 * t < KS2) __hip_atomic_store(wrow_dst + half * KS2 + lane + 64 * t, Tw[lane + 64 * t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(cfg.wrow + il, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
      for (int r = 0; r < K; ++r) dst[r * dstride] = xr[r];
    }
  };
  if (WGLOB) {
    // A producer's two lists: its own rows (needed when x of the join rows arrives, late) and the partner's W rows
    // (needed BEFORE the separator answers: the joiner fetches them ahead of its wait; each can start once the spike
    // workgroup has published the row).  A partner row that is there goes first, the own rows fill the waits - taken
    // one list after the other, the W rows of the mirrored pair were complete 0.6 us before the separator's answer
    // and their fetch (4 us) then sat on the path.  (As many wavefronts on the partner's rows as there is LDS for
    // their staged D^-1 U: 4 at K = 23, 2 at K = 29 N = 40.)
    const int ws = (cfg.wp_wst && wave < cfg.wp_waves) ? cfg.wp_waves : 0, wn = ws ? cfg.wp_nloc : 0;
    // (the counter of the next partner row is asked BEFORE a row's work and looked at after it - its round trip is
    // ~1 us; lane 0's answer decides for the wavefront: the lanes of one load need not see the same value)
    auto ask = [&](int il) { return il < wn ? __hip_atomic_load(cfg.wp_frowcnt + il, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull; };
    auto there = [&](unsigned long long cnt) { return __builtin_amdgcn_readfirstlane(cnt >= cfg.frowtarget ? 1 : 0); };
    int own = wave, wt = wave;
    int ready = there(ask(wt));
    while (own < nloc || wt < wn) {
      if (wt < wn && (ready || own >= nloc)) {
        const unsigned long long nxt = ask(wt + ws);
        do_pass(wt, 1, true);
        wt += ws;
        ready = there(nxt);
      } else {
        const unsigned long long nxt = ask(wt);
        do_pass(own, 0, true);
        own += nwaves;
        ready = there(nxt);
      }
    }
  } else {
    for (int task = wave; task < (SPK ? 2 : 1) * nloc; task += nwaves) {
      const int pass = task >= nloc ? 1 : 0;
      do_pass(task - pass * nloc, pass, true);
    }
  }
  __syncthreads();
  chain_ts(cfg, 3);
  if (cfg.ts && tid == 0) cfg.ts[6] = (double)wall_clock64();
  if constexpr (!WGLOB && !SPK) {
    if (A.closed_tail) {   // a producer of the pipelined kernel: no row of it waits for another once the join rows are known
      if (tid == 0) {
        unsigned long long* par = reinterpret_cast<unsigned long long*>(lds + L.xall + PipeClosed<K>::PAR);
        par[0] = (unsigned long long)A.x; par[1] = (unsigned long long)A.xjoin_ll; par[2] = (unsigned long long)cfg.spin.word;
        par[3] = (unsigned long long)cfg.ts; par[4] = (unsigned long long)A.epoch | ((unsigned long long)cfg.spin.id << 32);
        par[5] = (unsigned long long)(unsigned)nloc | ((unsigned long long)(unsigned)k << 32);
        par[6] = (unsigned long long)(unsigned)cfg.base | ((unsigned long long)(unsigned)cfg.mirror << 32);
      }
      __syncthreads();
      return;
    }
  }
  // ---- phase 2 (spike chains): once the separator is solved, c_i -= W_i [x_near ; x_far]
  if (WGLOB && cfg.fst) {
    // a thread per (row, component), two of them per thread at most (pipe_recursion_tail_fits); the rows of W are in
    // registers before the wait for the separator.  Each thread waits for the word of ITS row (the producer sets it
    // after the row's stores): the first elements are the early rows, fetched long before the last row exists.
    const int nt = blockDim.x;
    const int pidx = (tid < nloc * K) ? tid : 0, pil = pidx / K, pr = pidx - pil * K;
    const int qidx = (tid + nt < nloc * K) ? tid + nt : 0, qil = qidx / K, qr = qidx - qil * K;
    double f[2 * K], f2[2 * K];
    {
      spin_wait([&] { return __hip_atomic_load(cfg.wrow + pil, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.epoch; }, cfg.spin);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const double* F = A.wst + (size_t)pil * A.fstride + pr;
#pragma unroll
      for (int c = 0; c < 2 * K; ++c) f[c] = F[c * ks];
#pragma unroll
      for (int c = 0; c < 2 * K; ++c) asm volatile("" : "+v"(f[c]));
      if (cfg.ts && tid == 0) cfg.ts[7] = (double)wall_clock64();
      spin_wait([&] { return __hip_atomic_load(cfg.wrow + qil, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.epoch; }, cfg.spin);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const double* F2 = A.wst + (size_t)qil * A.fstride + qr;
#pragma unroll
      for (int c = 0; c < 2 * K; ++c) f2[c] = F2[c * ks];
#pragma unroll
      for (int c = 0; c < 2 * K; ++c) asm volatile("" : "+v"(f2[c]));
    }
    double* xs = lds + L.W;
    if (tid < 2 * KE) {
      const int half = tid / KE, r = tid - half * KE;
      xs[tid] = (r < K) ? ll_load(cfg.xsep_ll + 2 * ((mirror ? half : 1 - half) * K + r), A.epoch, cfg.spin) : 0.0;
    }
    __syncthreads();
    if (tid < nloc * K) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < K; ++c) { a0 = __builtin_fma(f[c], xs[c], a0); a1 = __builtin_fma(f[K + c], xs[KE + c], a1); }
      lds[pil * B::BS + B::oC + pr] -= a0 + a1;
    }
    if (tid + nt < nloc * K) {
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int c = 0; c < K; ++c) { a0 = __builtin_fma(f2[c], xs[c], a0); a1 = __builtin_fma(f2[K + c], xs[KE + c], a1); }
      lds[qil * B::BS + B::oC + qr] -= a0 + a1;
    }
    __syncthreads();
  }
  const int hf = lane >> 5, r_ = lane & 31, rr = r_ < K ? r_ : 0;
  static_assert(K <= 32, "one row per lane of a half-wavefront");
  double M0[KE], M1[KE], c0 = 0.0, c1 = 0.0;
  auto fetch_m = [&](int il, double (&M)[KE]) __attribute__((always_inline)) {
    const double2* y2 = reinterpret_cast<const double2*>(lds + il * B::BS + B::oYZ + rr * YS + hf * KE);
#pragma unroll
    for (int m = 0; m < KE / 2; ++m) { const double2 a = y2[m]; M[2 * m] = a.x; M[2 * m + 1] = a.y; }
  };
  auto fetch = [&](int il, double (&M)[KE], double& c) __attribute__((always_inline)) {
    fetch_m(il, M);
    c = lds[il * B::BS + B::oC + rr];
  };
  // (a joiner of the pipelined kernel: what follows the separator's answer is on the launch's critical path)
  // (the spike chains of penta_pipe_kernel always have their rows of Ft: cfg.fst is set)
  constexpr bool early = !WGLOB && SPK;
  if constexpr (early) {
    double* xs = lds + L.W;
    // what does not depend on x_sep goes in front of the wait for it: the cleared x ring, the first row's matrices
    if (wave == 0) {
      for (int c = lane; c < 4 * KE; c += 64) xb[c] = 0.0;
      if (nloc > 0) fetch_m(nloc - 1, M0);
#pragma unroll
      for (int m = 0; m < KE; ++m) asm volatile("" : "+v"(M0[m]));   // (the reads stay in front of the poll)
    }
    // (the 2K threads that fetch x_sep poll their own entry, which carries the epoch: penta_nd.h ll_store)
    if (tid < 2 * KE) {
      const int half = tid / KE, r = tid - half * KE;
      xs[tid] = (r < K) ? ll_load(cfg.xsep_ll + 2 * ((mirror ? half : 1 - half) * K + r), A.epoch, cfg.spin) : 0.0;   // mirrored chain: nearest = s, else nearest = s + 1
    }
    __syncthreads();
    // one round: a half-wavefront per row (ten rows on eight wavefronts were two), counted from the join end - the
    // two join rows, which the recursion takes first, are wavefront 0's own and are not waited for
    for (int t = 2 * wave + hf; t < nloc; t += 2 * nwaves) {
      const int il = nloc - 1 - t;
      if (r_ < K) {
        const double2* w2 = reinterpret_cast<const double2*>(lds + il * B::BS + B::oW + r_ * YS);
        const double2* x2 = reinterpret_cast<const double2*>(xs);
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int m = 0; m < KE; ++m) { const double2 w = w2[m], x = x2[m]; a0 = __builtin_fma(w.x, x.x, a0); a1 = __builtin_fma(w.y, x.y, a1); }
        lds[il * B::BS + B::oC + r_] -= a0 + a1;
      }
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  }
  // ---- phase 3: the recursion on one wavefront.  Lanes 0..31: row r of Y_il (times x_{il+1}), lanes 32..63: row r of
  // Z_il (times x_{il+2}); the halves meet in one exchange.  The matrix rows are in registers a row ahead (two sets,
  // the loop is unrolled by two); on the dependent chain of a row: x_{il+1} back from LDS (ten broadcast reads), K
  // FMAs in two accumulators, the exchange, x_il to LDS.
  if (wave != 0) {
    if constexpr (early) lds_barrier();   // (their rows of c: wavefront 0 comes here after its first row)
    return;
  }
  if (cfg.ts && tid == 0) cfg.ts[21] = (double)wall_clock64();
  if constexpr (!early) {
    for (int c = lane; c < 4 * KE; c += 64) xb[c] = 0.0;
  }
  if (cfg.two && producer) {
    // x of local rows nloc (next to this chain) and nloc + 1 come from the joiner (its two join rows)
    if (lane < K) {
      xb[(nloc & 3) * KE + lane] = ll_load(A.xjoin_ll + 2 * (K + lane), A.epoch, cfg.spin);
      xb[((nloc + 1) & 3) * KE + lane] = ll_load(A.xjoin_ll + 2 * lane, A.epoch, cfg.spin);
    }
  }
  auto row = [&](int il, const double (&M)[KE], const double c, double (&Mn)[KE], double& cn) __attribute__((always_inline)) {
    const double2* xv = reinterpret_cast<const double2*>(xb + ((il + 1 + hf) & 3) * KE);
    double x[KE];
#pragma unroll
    for (int m = 0; m < KE / 2; ++m) { const double2 a = xv[m]; x[2 * m] = a.x; x[2 * m + 1] = a.y; }
    if (il >= 1) fetch(il - 1, Mn, cn);
    // (pad entries of the rows were cleared when they were written, the pad entries of x are zero)
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int m = 0; m < KE / 2; ++m) { a0 = __builtin_fma(M[2 * m], x[2 * m], a0); a1 = __builtin_fma(M[2 * m + 1], x[2 * m + 1], a1); }
    const double part = a0 + a1;
    const double v = c - pipe_half_sum(part);
    if (lane < K) {
      xb[(il & 3) * KE + lane] = v;
      if (lane < k) A.x[(size_t)orig(il) * k + lane] = v;
      if (cfg.two && !producer && il >= m_split) ll_store(A.xjoin_ll + 2 * ((il - m_split) * K + lane), v, A.epoch);   // a join row: the producer polls it
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
  };
  if constexpr (early) {
    // the first row's matrices are in registers since before the wait, its c and the next row's are this wavefront's
    // own; the barrier stands where the first row of another wavefront's correction is asked for
    if (nloc > 0) c0 = lds[(nloc - 1) * B::BS + B::oC + rr];
    if (cfg.ts && tid == 0) cfg.ts[22] = (double)wall_clock64();
    if (nloc > 0) row(nloc - 1, M0, c0, M1, c1);
    lds_barrier();   // (LDS only: __syncthreads would wait here for the first join row's stores to be acknowledged, 0.36 us)
    for (int il = nloc - 2; il >= 0; il -= 2) {
      row(il, M1, c1, M0, c0);
      if (il >= 1) row(il - 1, M0, c0, M1, c1);
    }
  } else {
    if (nloc > 0) fetch(nloc - 1, M0, c0);
    if (cfg.ts && tid == 0) cfg.ts[22] = (double)wall_clock64();
    for (int il = nloc - 1; il >= 0; il -= 2) {
      row(il, M0, c0, M1, c1);
      if (il >= 1) row(il - 1, M1, c1, M0, c0);
    }
  }
  chain_ts(cfg, 4);
}

// ---- the seven-workgroup kernel's chains (penta_nd.h, K = 23 / 29) take their back substitution in the same form.
// Their forward pass (penta_ldl_body) leaves rt of the local rows at xall_off, in the middle of what the recursion
// matrices will occupy: the rows move to the top of the launch's LDS first.
// (pipe_recursion_tail_fits: solver_layout.h)
template <int K>
__device__ void chain_recursion_tail(int n, int k, double* x, double* Ust, double* Hst, double* Est, double* Dst,
                                     const ChainCfg& cfg, unsigned epoch, int xall_off) {
  extern __shared__ double lds[];
  using B = PipeBack<K, false>;
  constexpr int ks = ldl_ks(K);
  const int tid = threadIdx.x, nloc = cfg.nloc;
  PipeLds L = {};
  L.xall = cfg.lds_doubles - (nloc + 2) * ks;
  L.W = nloc * B::BS + 4 * B::KE + 2;
  {
    double keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) keep[j] = (tid + 256 * j < (nloc + 2) * ks) ? lds[xall_off + tid + 256 * j] : 0.0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) if (tid + 256 * j < (nloc + 2) * ks) lds[L.xall + tid + 256 * j] = keep[j];
    __syncthreads();
  }
  PipeArgs P = {};
  P.n = n; P.k = k; P.x = x; P.Ust = Ust; P.Hst = Hst; P.Est = Est; P.Dst = Dst; P.epoch = epoch;
  P.fst = const_cast<double*>(cfg.fst); P.fstride = cfg.fstride; P.wst = cfg.wst; P.xjoin_ll = cfg.xjoin_ll;
  pipe_backward<K, true, true>(P, cfg, L);
}

// grid (5, batch), 512 threads: blockIdx.x = role, blockIdx.y = problem of the batch
//   0: P0 producer, rows 0 .. j1-1 top-down        1: P3 producer, rows n-1 .. j2+2 bottom-up
//   2: J1 joiner, rows s-1 .. j1+2 then j1+1, j1   3: J2 joiner, rows s+2 .. j2-1 then j2, j2+1   (with their spike columns)
//   4: the separator (penta_nd.h nd_separator)
// Every wait is bounded (PIPE_SPIN_CAP): a workgroup that is not resident with its partners ends with the
// factorisation status set instead of hanging the device.
template <int K, bool DEC = false>
__global__ void __launch_bounds__(512) penta_pipe_kernel(NdArgs A, PipeAsm F) {
  if (blockIdx.x >= 5) {
    pipe_assemble<DEC>(A.ts, A.epoch, A.pstride, F, 5, SpinCtl{A.status + 2 * gridDim.y, A.fact_id});
    return;
  }
  {
    const size_t o = (size_t)blockIdx.y * A.pstride;
    A.HA = at_problem(A.HA, o); A.HB = at_problem(A.HB, o); A.HC = at_problem(A.HC, o); A.b = at_problem(A.b, o);
    A.x = at_problem(A.x, o); A.Ust = at_problem(A.Ust, o); A.Hst = at_problem(A.Hst, o); A.Est = at_problem(A.Est, o);
    A.Dst = at_problem(A.Dst, o); A.xch = at_problem(A.xch, o); A.flags = at_problem(A.flags, o);
    A.rowcnt = at_problem(A.rowcnt, o); A.ndbuf = at_problem(A.ndbuf, o);
    A.spin = SpinCtl{A.status + 2 * gridDim.y, A.fact_id};
    A.status += 2 * blockIdx.y;
  }
  const int role = blockIdx.x;
  if (role == A.debug_skip_role) return;
  // does this launch assemble the system?  (a deciding launch: known once its decision is out - an accepted trial point's
  // g and H stand in the second set of arrays, which the launch's assembly fills without waiting)
  const bool asm_on = pipe_asm_on<DEC>(F, (size_t)blockIdx.y * A.pstride, A.spin);
  if (DEC && F.decide && asm_on) {
    const size_t o = (size_t)blockIdx.y * A.pstride, qq0 = (size_t)F.first * F.nq * F.nq;
    A.HA = at_problem(F.HA2, o) + qq0; A.HB = at_problem(F.HB2, o) + qq0; A.HC = at_problem(F.HC2, o) + qq0;
    A.b = at_problem(F.g2, o) + (size_t)F.first * F.nq;
  }
  if (role == 4) {
    A.asm_ready = asm_on ? at_problem(F.ready, (size_t)blockIdx.y * A.pstride) : nullptr;
    A.asm_first = F.first;
    A.wt_rows = 1;
    nd_separator<K, false>(A);
    return;
  }
  const NdBuf B = nd_layout(K);
  ChainCfg c = {};
  c.two = 1;
  c.dbg_slot = role;
  c.ts = A.ts ? A.ts + role * 64 : nullptr;
  c.spin = A.spin;
  int pair;
  if (role == 0) { c.mirror = 0; c.producer = 1; c.base = 0; c.nloc = A.j1; pair = 0; }
  else if (role == 1) { c.mirror = 1; c.producer = 1; c.base = A.n - 1; c.nloc = A.n - A.j2 - 2; pair = 1; }
  else {
    const int w = role - 2;
    c.mirror = (w == 0); c.producer = 0;
    c.base = (w == 0) ? A.s - 1 : A.s + 2;
    c.m_split = (w == 0) ? A.s - A.j1 - 2 : A.j2 - A.s - 2;
    c.nloc = c.m_split + 2;
    pair = w;
    c.fst = A.ndbuf + B.fst + (size_t)w * ND_MAXROWS * B.frow; c.fstride = B.frow;
    c.frowcnt = A.rowcnt + (2 + w) * ND_MAXROWS; c.frowtarget = (A.rowtarget / A.rowunit) * 3ull;
    c.xsep = A.ndbuf + B.xsep; c.sepflag = A.flags + 4;
    c.xsep_ll = A.ndbuf + B.ll;
  }
  PipeArgs P;
  P.n = A.n; P.k = A.k; P.HA = A.HA; P.HB = A.HB; P.HC = A.HC; P.b = A.b; P.rhs_sign = A.rhs_sign; P.x = A.x;
  P.Ust = A.Ust; P.Hst = A.Hst; P.Est = A.Est; P.Dst = A.Dst;
  P.xch = A.xch + (size_t)pair * A.xch_pair; P.flags = A.flags + 2 * pair; P.epoch = A.epoch;
  P.status = A.status; P.fact_id = A.fact_id;
  P.fst = const_cast<double*>(c.fst); P.fstride = c.fstride;
  P.frowcnt = role >= 2 ? A.rowcnt + (2 + role - 2) * ND_MAXROWS : nullptr;
  P.ts = c.ts;
  P.xjoin_ll = A.ndbuf + B.ll + (1 + pair) * 4 * K;
  P.join_ll = A.ndbuf + B.joinll + (size_t)pair * B.joinll_pair;
  P.asm_ready = asm_on ? at_problem(F.ready, (size_t)blockIdx.y * A.pstride) : nullptr;
  P.asm_first = F.first; P.asm_rows = F.rows;
  P.closed_tail = 0;
  const bool spike = role >= 2;
  const PipeLds L = pipe_layout<K>(A.n, spike);
  if (spike) pipe_forward<K, true>(P, c, L);
  else pipe_forward<K, false>(P, c, L);
  // back substitution: in recursion form when every row's matrices fit the LDS (horizons up to ~45 block rows at
  // K = 19), else row by row from the factors as the two-workgroup kernel does
  // (all four chains take the same form: the join rows change hands in the form's own protocol)
  // Recursion form only where the triangular solves are long (K = 19): multiplying by precomputed U^-1 blocks costs
  // a factor ~cond(U) of backward error (measured 1e-14 componentwise against 1e-16; the forward error is unchanged),
  // which small blocks need not pay - their row-by-row chain is K steps anyway.
  // (debug_pipe_tail: 1 row by row, 2 the recursion walked row after row by the producers too)
  const bool recursion = K > 8 && A.debug_pipe_tail != 1 && pipe_backward_fits<K, true>(pipe_layout<K>(A.n, true), max(A.s - A.j1, A.j2 - A.s)) &&
                         pipe_backward_fits<K, false>(pipe_layout<K>(A.n, false), max(A.j1, A.n - A.j2 - 2));
  if (recursion) {
    // the producers' rows in closed form where both producers' T_i fit behind their [Y | Z | c] (K = 19: up to 9 rows,
    // horizons up to 42 block rows; both or none, as with the form itself) and a thread per (row, component) exists
    const int np = max(A.j1, A.n - A.j2 - 2);
    P.closed_tail = !spike && A.debug_pipe_tail != 2 && pipe_closed_fits<K>(pipe_layout<K>(A.n, false), np) && np * K <= (int)blockDim.x;
    if (spike) pipe_backward<K, true>(P, c, L);
    else pipe_backward<K, false>(P, c, L);
    if (P.closed_tail) pipe_closed_tail<K>();
    return;
  }
  if (threadIdx.x >= 256) return;
  penta_ldl_tail<K, 256>(A.n, A.k, 1, A.x, A.Ust, A.Hst, A.Est, A.Dst, nullptr, c, P.xch, P.flags, A.epoch, L.xall, 1,
                         L.W, c.nloc + (c.producer ? 2 : 0));
}

}  // namespace idto_dev
