// solver_plan_check.cc — host/solver_plan.cc on the CPU, no device involved (tests/test_solver_plan.py builds this with
// -fsanitize=address,undefined and runs it):
//   1. the plans of a sweep over (block size, multiplier rows, horizon, batch, assembled, options, request) reproduce
//      tests/golden/solver_plan.txt: one SHA-256 per block size over every row, the examples' rows in clear text, the
//      buffer counts and both contexts' carve offsets;
//   2. every plan of the sweep holds what the kernels assume of it;
//   3. SolverBufferCounts covers the highest index the layouts address.
// usage: solver_plan_check <fixture>            (--print: write the fixture's text to stdout instead of comparing)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "host/context_layout.h"
#include "host/solver_plan.h"
#include "sha256.h"
#include "solver_layout.h"

using namespace idto_host;
using namespace idto_dev;

static const int kBatches[8] = {1, 2, 12, 13, 36, 37, 64, 256};
static const int kLds = 160 * 1024;
static int g_bad = 0;
static std::string g_case;

#define HOLD(cond)                                                                    \
  do {                                                                                \
    if (!(cond) && ++g_bad <= 20) std::printf("BROKEN %s: %s\n", g_case.c_str(), #cond); \
  } while (0)

// options: 0 defaults, 1 two_sided = 0, 2 solver_nd = 0, 3 solver_pipe = 0, 4 / 5 solver_band = 0 / 2, 6 nd_min_rows = 24,
// 7 nd_recursion = 0, 8 what a KKT context is made with (no pipelined kernel, seven workgroups for blocks of 29 and 8)
static SolverShape Shape(int k, int npos, int N, int batch, int ha, int opt) {
  SolverShape c;
  c.k = k; c.N = N; c.batch = batch; c.npos = npos; c.h_assembled = ha != 0;
  c.has_wst = SolverBufferCounts(k, N).has_wst;
  if (npos == 0) {   // (a KKT context carries neither the assembly nor the decision)
    const int nq = k, nv = k;
    c.asm_terms_lds = (int)sizeof(double) * (5 * ((nv + 1) & ~1) * nq + 4 * nv + nq + 2);
    c.cost_lds = (int)sizeof(double) * ((3 * N + 2) * (1 + std::max(nq, nv)) + 2 * (N + 1) + 2);
  }
  switch (opt) {
    case 1: c.two_sided = false; break;
    case 2: c.solver_nd = false; break;
    case 3: c.solver_pipe = false; break;
    case 4: c.solver_band = 0; break;
    case 5: c.solver_band = 2; break;
    case 6: c.nd_min_rows = 24; break;
    case 7: c.nd_recursion = 0; break;
    case 8: c.solver_pipe = false; c.solver_nd = (k == 29 || k == 8); break;
  }
  return c;
}
// requests: 0 one-sided, 1 one right-hand side, 2 three right-hand sides, 3 the whole step
static SolveRequest Request(int req, int k, int npos) {
  SolveRequest r;
  r.kind = req == 0 ? SolveRequest::ONE_SIDED : req == 3 ? SolveRequest::WHOLE_STEP : SolveRequest::SOLVE;
  r.nrhs = req == 2 ? 3 : 1;
  r.step_nq = npos > 0 ? npos : k;
  r.step_fast_n = 34 * r.step_nq + 2;
  return r;
}

// "<case> : <plan>\n" (snprintf is most of the sweep's time: the digits are written by hand)
static char* Put(char* o, long long v) {
  if (v < 0) { *o++ = '-'; v = -v; }
  char d[24];
  int n = 0;
  do { d[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *o++ = d[--n];
  *o++ = ' ';
  return o;
}
static int Format(char* buf, int k, int npos, int N, int batch, int ha, int opt, int req, int rc, const SolverPlan& p) {
  char* o = buf;
  for (int v : {k, npos, N, batch, ha, opt, req}) o = Put(o, v);
  *o++ = ':';
  if (rc) { std::memcpy(o, " err\n", 6); return (int)(o + 5 - buf); }
  // kind K r0 n m_split lds lds_full s j1 j2 nloc_max lds_rows rec_tail grid threads lds_small can_assemble can_decide
  // lds_assemble lds_decide apply_K apply_lds
  *o++ = ' ';
  for (int v : {p.kind, p.K, p.r0, p.n, p.m_split, p.lds, p.lds_full, p.s, p.j1, p.j2, p.nloc_max, p.lds_rows, p.rec_tail, p.grid, p.threads,
                p.lds_small, (int)p.can_assemble, (int)p.can_decide, p.lds_assemble, p.lds_decide, p.apply_K, p.apply_lds})
    o = Put(o, v);
  o[-1] = '\n';
  *o = 0;
  return (int)(o - buf);
}

// what the kernels assume of a plan
static void Hold(const SolverShape& c, const SolverPlan& p) {
  HOLD(p.lds > 0 && p.lds <= kLds && p.lds_assemble <= kLds && p.lds_decide <= kLds && p.apply_lds <= kLds);
  HOLD(p.K >= p.k && p.n == c.N + 1 - p.r0 && p.n >= 1 && p.qq0 == (size_t)p.r0 * p.k * p.k);
  HOLD(p.gj_waves >= 1 && p.gj_waves <= 3);
  switch (p.kind) {
    case SOLVER_LDL:
      HOLD(SolverInstantiated(FAM_LDL, p.K));
      HOLD(p.threads == 256 && p.grid == (p.m_split > 0 ? 2 : 1));
      // (the joiner takes rows 0 .. m + 1, the producer m + 2 .. n - 1 and two pseudo-rows: neither is empty)
      HOLD(p.m_split == 0 || (p.m_split >= 1 && p.n - p.m_split - 2 >= 1));
      HOLD(p.lds >= penta_ldl_layout(p.n, p.K, 1, ldl_two_sided_rows(p.n, p.m_split, 1)).end * (int)sizeof(double));
      break;
    case SOLVER_ND:
    case SOLVER_PIPE: {
      HOLD(SolverInstantiated(p.kind == SOLVER_ND ? FAM_ND : FAM_PIPE, p.K) && p.K == p.k);
      HOLD(p.grid == (p.kind == SOLVER_ND ? 7 : 5) && p.threads == (p.kind == SOLVER_ND ? 256 : 512));
      // producer P0 [0, j1) | join rows j1, j1 + 1 and joiner J1 up to s | separator s, s + 1 | joiner J2 down to its join
      // rows j2, j2 + 1 | producer P3 [j2 + 2, n): a partition of [0, n), every chain with a row of its own
      const int p0 = p.j1, jn1 = p.s - p.j1, jn2 = p.j2 - p.s, p3 = p.n - p.j2 - 2;
      HOLD(p0 >= 1 && jn1 >= 3 && jn2 >= 3 && p3 >= 1);
      HOLD(p0 + jn1 + 2 + jn2 + p3 == p.n && p.j1 + 2 <= p.s && p.s + 2 <= p.j2 && p.j2 + 2 <= p.n);
      HOLD(p.nloc_max == std::max(std::max(jn1, jn2), std::max(p0, p3)) && p.nloc_max <= ND_MAXROWS);
      HOLD(p.lds_rows >= std::max(std::max(jn1, jn2), std::max(p0, p3) + 2));   // (a producer: + its two pseudo-rows)
      HOLD(7 * c.batch <= 256);
      if (p.kind == SOLVER_PIPE) {
        HOLD(p.rec_tail == 0 && p.lds >= nd_sep_lds_doubles(p.K) * (int)sizeof(double));
        HOLD(!p.can_decide || SolverInstantiated(FAM_PIPE_DEC, p.K));
      } else {
        HOLD(p.lds >= penta_ldl_layout(p.n, p.K, 1, p.lds_rows).end * (int)sizeof(double) && p.lds >= nd_sep_lds_doubles(p.K) * (int)sizeof(double));
        HOLD(!p.can_assemble && !p.can_decide);
        if (p.rec_tail) {
          const int all = kLds / (int)sizeof(double), nj = std::max(jn1, jn2), np = std::max(p0, p3);
          const int fits = p.K == 23 ? pipe_recursion_tail_fits<23>(all, nj, np) : p.K == 29 ? pipe_recursion_tail_fits<29>(all, nj, np) : 0;
          HOLD(p.rec_tail == fits && p.lds == kLds && c.has_wst && p.K > 20);
        }
      }
      break;
    }
    case SOLVER_BAND:
    case SOLVER_SMALL:
      HOLD(p.K == p.k && SolverInstantiated(FAM_BAND, 3 * p.k) && p.grid == 1 && p.threads == 256);
      HOLD(p.n * p.k >= 4 * 3 * p.k);   // (band_layout: both chains and the middle rows exist)
      HOLD(p.kind != SOLVER_SMALL || (p.r0 == 1 && p.lds_small >= band_layout(p.n * p.k, 3 * p.k).end));
      break;
    default: HOLD(!"a kind");
  }
  HOLD(!p.can_decide || p.can_assemble);
  HOLD(!p.can_assemble || (p.lds_assemble >= p.lds && p.lds_assemble >= c.asm_terms_lds));
  HOLD(!p.can_decide || (p.lds_decide >= p.lds_assemble && p.lds_decide >= c.cost_lds));
  HOLD(p.apply_K == 0 || (p.apply_K == p.K && SolverInstantiated(FAM_APPLY, p.apply_K) && p.kind == SOLVER_LDL));
}

// 3. the arrays cover what the layouts address
static void HoldBuffers() {
  g_case = "buffers";
  const SolverBuffers b = SolverBufferCounts(32, 40);
  for (int K = 1; K <= 32; ++K) {
    if (!(SolverInstantiated(FAM_ND, K) || SolverInstantiated(FAM_PIPE, K))) continue;
    const SolverBuffers bk = SolverBufferCounts(K, 40);
    HOLD(bk.nd_buf >= (size_t)nd_layout(K).end);
    HOLD(bk.xch_count >= 2 * (size_t)(3 * K + 1) * ldl_ks(K) + 2 * K);
    if (K > 20) {
      // the W rows' arrival words sit behind a pair's exchange block (penta_nd.h: cfg.wrow), one 32-bit word per local row
      const size_t wrow = (size_t)((2 * (3 * K + 1) * ldl_ks(K) + 2 * K + 1) & ~1);
      HOLD(bk.xch_count >= wrow + ND_MAXROWS / 2);
      HOLD(bk.has_wst && bk.nd_wst >= 2 * (size_t)ND_MAXROWS * nd_layout(K).frow);
    }
  }
  HOLD(b.xch == 2 * b.xch_count && b.rowcnt >= 4 * ND_MAXROWS && b.flags >= 5);
#define IDTO_X(K, PD, GW) HOLD(b.factors >= (size_t)41 * K * ldl_ks(K) && b.dinv >= (size_t)41 * K);
  IDTO_LDL_KERNELS(IDTO_X)
#undef IDTO_X
}

static std::string Produce(bool hold) {
  std::string out = "# solver plans of the sweep in tests/cpp/solver_plan_check.cc\n";
  char buf[512];
  SolverPlan p;
  for (int k = 1; k <= 32; ++k) {
    Sha256 h;
    const int nposv[3] = {0, k - 1, std::max(1, k - 6)};
    for (int ip = 0; ip < 3; ++ip)
      for (int N = 1; N <= 140; ++N)
        for (int ib = 0; ib < 8; ++ib)
          for (int ha = 0; ha < 2; ++ha)
            for (int opt = 0; opt < 9; ++opt)
              for (int req = 0; req < 4; ++req) {
                const SolverShape c = Shape(k, nposv[ip], N, kBatches[ib], ha, opt);
                const int rc = PlanSolve(c, Request(req, k, nposv[ip]), &p, nullptr);
                const int len = Format(buf, k, nposv[ip], N, kBatches[ib], ha, opt, req, rc, p);
                h.Update(buf, (size_t)len);
                if (hold && !rc) { g_case.assign(buf, (size_t)len - 1); Hold(c, p); }
              }
    std::snprintf(buf, sizeof buf, "digest %d %s\n", k, h.Hex().c_str());
    out += buf;
  }
  // the examples' own block sizes, H and KKT: acrobot 2 / 3, spinner 3 / 4, hopper 5, jaco 14 / 20, cheetah 19, punyo and
  // dual_jaco 21 (-> 24) / 27 (-> 30), allegro 23 / 29
  static const int ex[][2] = {{2, 0}, {3, 0}, {5, 0}, {14, 0}, {19, 0}, {21, 0}, {23, 0}, {3, 2}, {4, 3}, {20, 14}, {27, 21}, {29, 23}};
  static const int Ns[7] = {10, 16, 20, 24, 40, 60, 127};
  for (auto& e : ex)
    for (int N : Ns)
      for (int batch : {1, 64})
        for (int req = 1; req <= 3; ++req) {
          if (req == 2 && e[1] > 0) continue;
          const int opt = e[1] > 0 ? 8 : 0;
          const int rc = PlanSolve(Shape(e[0], e[1], N, batch, 1, opt), Request(req, e[0], e[1]), &p, nullptr);
          Format(buf, e[0], e[1], N, batch, 1, opt, req, rc, p);
          out += std::string("row ") + buf;
        }
  // the solver-only arrays: the KKT context's carve (offsets in bytes, arena stride), idto_hip_create_batch's from its
  // stamp array on (relative offsets; what lies in front of it does not move them: every array starts 64-byte aligned)
  // (both from host/context_layout.cc's plan, the one the library allocates by)
  for (int K = 1; K <= 32; ++K)
    for (int N : {1, 2, 10, 40, 140}) {
      const ArenaPlan kkt = PlanArena(ARENA_KKT, K, 0, N), mdl = PlanArena(ARENA_MODEL, K, K, N);
      out += "kkt " + std::to_string(K) + " " + std::to_string(N) + " :";
      for (const ArenaEntry& e : kkt.entries) out += " " + std::to_string(e.offset);
      out += " " + std::to_string(kkt.pstride) + "\n";
      // dbg .. flags, and where flags ends
      const ArenaEntry *first = mdl.Find("dbg"), *last = mdl.Find("flags");
      out += "main " + std::to_string(K) + " " + std::to_string(N) + " :";
      for (const ArenaEntry* e = first; e <= last; ++e) out += " " + std::to_string(e->offset - first->offset);
      out += " " + std::to_string(last->offset + last->count * last->elem - first->offset) + "\n";
    }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: solver_plan_check <fixture> | --print\n"); return 2; }
  if (std::strcmp(argv[1], "--print") == 0) { std::fputs(Produce(false).c_str(), stdout); return 0; }
  const std::string got = Produce(true);
  HoldBuffers();
  std::ifstream f(argv[1]);
  const std::string want((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  int diff = 0;
  if (got != want) {
    size_t a = 0, b = 0;
    while (a < got.size() || b < want.size()) {
      const size_t ea = std::min(got.find('\n', a), got.size()), eb = std::min(want.find('\n', b), want.size());
      const std::string la = got.substr(a, ea - a), lb = want.substr(b, eb - b);
      if (la != lb && ++diff <= 10) std::printf("DIFFERS\n  plan:    %s\n  fixture: %s\n", la.c_str(), lb.c_str());
      a = ea + 1; b = eb + 1;
    }
    if (!diff) diff = 1;
  }
  // a size without an instantiation is an error return, never another size's kernel: a KKT context's 8 x 8 blocks have
  // no pipelined kernel, and its exact / 30 x 30 factors no penta_apply_kernel
  {
    g_case = "refusals";
    SolverPlan p; std::string err;
    SolverShape c = Shape(8, 7, 40, 1, 1, 0);
    HOLD(PlanSolve(c, Request(1, 8, 7), &p, &err) == -1 && err.find("penta_pipe_kernel") != std::string::npos);
    c = Shape(29, 23, 40, 1, 1, 8);
    HOLD(PlanSolve(c, Request(2, 29, 23), &p, &err) == -1 && err.find("penta_apply_kernel") != std::string::npos);
    c = Shape(33, 0, 40, 1, 1, 0);
    HOLD(PlanSolve(c, Request(1, 33, 0), &p, &err) == -1 && err.find("nq <= 32") != std::string::npos);
  }
  std::printf("%s: %d lines differ from the fixture, %d conditions broken\n", (diff || g_bad) ? "FAILED" : "ok", diff, g_bad);
  return (diff || g_bad) ? 1 : 0;
}
