// context_layout.cc — see context_layout.h
#include "host/context_layout.h"

#include <algorithm>

#include "arena_sizes.h"
#include "host/solver_plan.h"

#define IDTO_STR_(x) #x
#define IDTO_STR(x) IDTO_STR_(x)

namespace idto_host {
using namespace idto_dev;

namespace {
// what the tables' count expressions are written in
struct Sizes {
  size_t nq, nv, N, rows, bsz, qq, nvars, slab_stride;
  SolverBuffers sb;
  Sizes(int nq_, int nv_, int N_)
      : nq((size_t)nq_), nv((size_t)nv_), N((size_t)N_), rows(N + 1), bsz(nv * nq), qq(nq * nq), nvars(rows * nq),
        slab_stride(3 * bsz + nv), sb(SolverBufferCounts(nq_, N_)) {}
};
#define IDTO_SIZES(z)                                                                                                 \
  const size_t nq = z.nq, nv = z.nv, N = z.N, rows = z.rows, bsz = z.bsz, qq = z.qq, nvars = z.nvars, slab_stride = z.slab_stride; \
  const SolverBuffers& sb = z.sb;                                                                                     \
  (void)nq; (void)nv; (void)N; (void)rows; (void)bsz; (void)qq; (void)nvars; (void)slab_stride; (void)sb
}  // namespace

ArenaPlan PlanArena(ArenaKind kind, int nq_, int nv_, int N_) {
  const Sizes z(nq_, nv_, N_);
  IDTO_SIZES(z);
  ArenaPlan p;
  size_t top = 0;
  auto carve = [&](const char* name, size_t count, size_t elem) {
    const size_t o = (top + 63) & ~(size_t)63;
    top = o + std::max<size_t>(count, 1) * elem;
    p.entries.push_back(ArenaEntry{name, elem, count, o});
  };
#define IDTO_X(field, type, count) carve(IDTO_STR(field), count, sizeof(type));
#define IDTO_B(field, entry, index) p.bands.push_back(ArenaBand{#field, #entry, index});
  if (kind == ARENA_MODEL) {
    IDTO_MODEL_ARENA(IDTO_X, IDTO_X)
    IDTO_MODEL_BANDS(IDTO_B)
    p.alt_off = (long long)(p.Find("v_alt")->offset - p.Find("v")->offset);
  } else {
    IDTO_KKT_ARENA(IDTO_X, IDTO_X)
    IDTO_KKT_BANDS(IDTO_B)
  }
#undef IDTO_X
#undef IDTO_B
  p.pstride = (top + 255) & ~(size_t)255;
  p.band = (N + 6) * qq;
  p.has_wst = sb.has_wst;
  p.xch_count = sb.xch_count;
  p.flag_count = sb.flags;
  p.slab_stride = (int)slab_stride;
  return p;
}

const ArenaEntry* ArenaPlan::Find(const std::string& name) const {
  for (const ArenaEntry& e : entries)
    if (name == e.name) return &e;
  return nullptr;
}

bool ArenaPlan::Locate(const std::string& name, size_t* offset, size_t* room) const {
  size_t skip = 0;   // elements of the entry in front of the field
  const ArenaEntry* e = Find(name);
  if (!e)
    for (const ArenaBand& b : bands)
      if (name == b.name) { e = Find(b.entry); skip = (size_t)b.index * band; }
  if (!e || skip > e->count) return false;
  *offset = e->offset + skip * e->elem;
  *room = e->count - skip;
  return true;
}

ArrayInfo ArrayLookup(int what, int nq_, int nv_, int N_) {
  const Sizes z(nq_, nv_, N_);
  IDTO_SIZES(z);
  ArrayInfo r;
  switch (what) {
#define IDTO_A(id, fld, cnt) case id: r.where = ArrayInfo::ENTRY; r.field = #fld; r.count = (long)(cnt); break;
#define IDTO_S(id, off, wid) case id: r.where = ArrayInfo::SLAB_ROWS; r.at = off; r.width = wid; r.count = (long)(N * (wid)); break;
#define IDTO_O(id) case id: r.where = ArrayInfo::OUTSIDE; break;
    IDTO_ARRAYS(IDTO_A, IDTO_S, IDTO_O)
#undef IDTO_A
#undef IDTO_S
#undef IDTO_O
    default: break;
  }
  return r;
}

std::vector<int> ArrayIds() {
#define IDTO_A(id, fld, cnt) id,
#define IDTO_S(id, off, wid) id,
#define IDTO_O(id) id,
  return {IDTO_ARRAYS(IDTO_A, IDTO_S, IDTO_O)};
#undef IDTO_A
#undef IDTO_S
#undef IDTO_O
}

LaunchSizes PlanLaunchSizes(int nq, int nv, int N) {
  const int bsz = nv * nq, qq = nq * nq, n = N + 1, D = (int)sizeof(double);
  LaunchSizes s;
  s.asm_lds = D * (3 * nq + 5 * bsz + 4 * nv + nq + std::max(nq, nv) + bsz + 3 * qq + nq);
  s.asm_diag_lds = D * (14 * ((nv + 1) & ~1) * nq + 2 * bsz + 10 * nv + 6 * nq + 2);
  s.asm_terms_lds = D * (5 * ((nv + 1) & ~1) * nq + 4 * nv + nq + 2);
  // a thread per item of the largest part
  s.asm_terms_threads = std::min(512, std::max(256, (std::max(nq * (nq + 1) / 2 + nq, ((nq + 1) / 2) * nq) + 63) / 64 * 64));
  s.penta_lds = D * (10 * qq + nq * (3 * nq + 1) + (n + 2) * nq + nq) + (int)sizeof(int) * nq + 16;
  s.solve_lds = D * ((n + 2) * nq + nq);
  // (cost_kernel is a single block holding one column of every cost term; penta_apply_kernel keeps the right-hand side
  // of each of its four wavefronts: both bound the horizon as well)
  s.cost_lds = D * ((3 * N + 2) * (1 + std::max(nq, nv)) + 2 * (N + 1) + 2);
  s.apply_lds = ApplyLds(n, SolverBlockSize(nq));
  return s;
}

}  // namespace idto_host
