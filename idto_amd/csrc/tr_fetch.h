// tr_fetch.h — where everything lies in the staging buffer that the trust-region loop's fetches bring to the host with one copy
// (idto_hip_tr_solve_fetch, idto_hip_tr_solve_batch_fetch, idto_hip_mpc_batch_replan).  Offsets in doubles:
//   batch form:   [best | final_cost[B] | status[B]]  B x [state | rows]  T x [q | v | tau | dq | w]  [guesses | plans]
//                 T = B, or - only_best - 1: the best problem's; guesses, plans: the MPC tick's (mpc_batch.h), else empty
//   single form:  [state | rows] [q | v | tau | dq | w]: no header, one problem, one slot
// Plain C++, no HIP type: the host sizes and unpacks the buffer with it, hipcc compiles the same text for the kernels that pack
// it (trust_region.h tr_gather_kernel, tr_gather_batch_kernel), tests/cpp/tr_fetch_check.cc walks it on the CPU.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#define IDTO_TF_HD __host__ __device__
#else
#define IDTO_TF_HD
#endif
namespace idto_fetch {
struct TrFetchLayout {
  size_t B, nstate, nrows, slots, head;   // problems, state words and statistics doubles of each; trajectory blocks; the header's doubles
  size_t cnt[5], nguess, nplans;          // a trajectory block's parts in order: q, v, tau, dq, w; the hook's parts behind the fetch's own
  enum Part { Q = 0, V = 1, TAU = 2, DQ = 3, W = 4 };
  IDTO_TF_HD static TrFetchLayout Make(int B, int nstate, size_t nrows, int N, int nq, int nv, bool only_best, bool batch_form,
                                       size_t nguess = 0, size_t nplans = 0) {
    const size_t nqa = (size_t)(N + 1) * nq, nva = (size_t)(N + 1) * nv, nta = (size_t)N * nv, b = batch_form ? (size_t)B : 1;
    return TrFetchLayout{b, (size_t)nstate, nrows, (batch_form && !only_best) ? b : 1, batch_form ? 1 + 2 * b : 0, {nqa, nva, nta, nqa, nqa}, nguess, nplans};
  }
  IDTO_TF_HD size_t header() const { return 0; }              // batch form: the best problem's index, ...
  IDTO_TF_HD size_t final_cost() const { return 1; }          // ... B final costs ...
  IDTO_TF_HD size_t status() const { return 1 + B; }          // ... and B status words
  IDTO_TF_HD size_t state(size_t b) const { return head + b * (nstate + nrows); }
  IDTO_TF_HD size_t rows(size_t b) const { return state(b) + nstate; }
  IDTO_TF_HD size_t traj_doubles() const { return cnt[Q] + cnt[V] + cnt[TAU] + cnt[DQ] + cnt[W]; }
  IDTO_TF_HD size_t traj(size_t slot) const { return state(B) + slot * traj_doubles(); }
  IDTO_TF_HD size_t part(size_t slot, int i) const { size_t o = traj(slot); for (int j = 0; j < i; ++j) o += cnt[j]; return o; }
  IDTO_TF_HD size_t fetch_total() const { return traj(slots); }   // without the hook's parts
  IDTO_TF_HD size_t guess() const { return fetch_total(); }
  IDTO_TF_HD size_t plans() const { return guess() + nguess; }
  IDTO_TF_HD size_t total() const { return plans() + nplans; }
};
}  // namespace idto_fetch
