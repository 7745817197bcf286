// ls_fetch.h — where everything lies in the staging buffer that the linesearch loop's fetches bring to the host with one copy
// (idto_hip_ls_solve_fetch, idto_hip_ls_solve_batch_fetch).  Offsets in doubles:
//   batch form:   [final_cost[B]]  B x [rows | q | v | tau]
//   single form:  [rows | q | v | tau]: no header, one problem
// Plain C++, no HIP type: the host sizes and unpacks the buffer with it, hipcc compiles the same text for the kernel that packs
// it (linesearch.h ls_gather_batch_kernel), tests/cpp/ls_fetch_check.cc walks it on the CPU.
#pragma once
#include <cstddef>
#if defined(__HIPCC__)
#define IDTO_LF_HD __host__ __device__
#else
#define IDTO_LF_HD
#endif
namespace idto_fetch {
struct LsFetchLayout {
  size_t B, nrows, head;   // problems, statistics doubles of each, the header's doubles
  size_t cnt[3];           // a problem's trajectory parts in order: q, v, tau
  enum Part { Q = 0, V = 1, TAU = 2 };
  IDTO_LF_HD static LsFetchLayout Make(int B, int iterations, int row_doubles, int N, int nq, int nv, bool batch_form) {
    const size_t b = batch_form ? (size_t)B : 1;
    return LsFetchLayout{b, (size_t)iterations * row_doubles, batch_form ? b : 0,
                         {(size_t)(N + 1) * nq, (size_t)(N + 1) * nv, (size_t)N * nv}};
  }
  IDTO_LF_HD size_t final_cost() const { return 0; }   // batch form: B final costs
  IDTO_LF_HD size_t problem_doubles() const { return nrows + cnt[Q] + cnt[V] + cnt[TAU]; }
  IDTO_LF_HD size_t rows(size_t b) const { return head + b * problem_doubles(); }
  IDTO_LF_HD size_t part(size_t b, int i) const { size_t o = rows(b) + nrows; for (int j = 0; j < i; ++j) o += cnt[j]; return o; }
  IDTO_LF_HD size_t total() const { return rows(B); }
};
}  // namespace idto_fetch
