// context_layout_check.cc — host/context_layout.cc on the CPU, no device involved (tests/test_context_layout.py builds this
// with -fsanitize=address,undefined and runs it):
//   1. the arena plans of the examples' sizes (every entry's offset in clear text) and of a sweep nq = nv = 1 .. 32 x
//      N in {1, 2, 10, 40, 140} (one SHA-256 per nq), of both kinds of context, reproduce tests/golden/context_layout.txt,
//      recorded from the carve sequences as they stood inside idto_hip_create_batch and MakeKkt;
//   2. every plan of the sweep holds what the kernels assume of an arena;
//   3. every array id lies inside its entry, and the launch sizes are the formulas the kernels were written against.
// usage: context_layout_check <fixture>            (--print: write the fixture's text to stdout instead of comparing)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "arena_sizes.h"
#include "host/context_layout.h"
#include "host/solver_plan.h"
#include "sha256.h"

using namespace idto_host;
using namespace idto_dev;

static int g_bad = 0;
static std::string g_case;

#define HOLD(cond)                                                                    \
  do {                                                                                \
    if (!(cond) && ++g_bad <= 20) std::printf("BROKEN %s: %s\n", g_case.c_str(), #cond); \
  } while (0)

static const int kSweepN[5] = {1, 2, 10, 40, 140};

// "<kind> nq <nq> nv <nv> N <N> : <name> <offset> ... pstride <bytes> alt_off <bytes>\n"
static std::string Line(ArenaKind kind, int nq, int nv, int N, const ArenaPlan& p) {
  std::string s = std::string(kind == ARENA_MODEL ? "model" : "kkt") + " nq " + std::to_string(nq) + " nv " + std::to_string(nv) + " N " +
                  std::to_string(N) + " :";
  for (const ArenaEntry& e : p.entries) s += std::string(" ") + e.name + " " + std::to_string(e.offset);
  s += " pstride " + std::to_string(p.pstride) + " alt_off " + std::to_string(p.alt_off) + "\n";
  return s;
}

// 2. what the kernels assume of an arena
static void HoldPlan(ArenaKind kind, int nq, int nv, int N, const ArenaPlan& p) {
  size_t end = 0;
  for (const ArenaEntry& e : p.entries) {
    HOLD(e.offset % 64 == 0);
    HOLD(e.offset >= end);   // (in order: none overlaps its predecessor)
    end = e.offset + std::max<size_t>(e.count, 1) * e.elem;
    HOLD(end <= p.pstride);
  }
  HOLD(p.pstride % 256 == 0 && p.pstride >= end && p.pstride - end < 256);
  const SolverBuffers sb = SolverBufferCounts(nq, N);
  // the three bands of each H: (N + 6) nq^2 doubles apart inside one entry
  HOLD(p.band == (size_t)(N + 6) * nq * nq);
  for (const char* h : {"HA", "HA2"}) {
    const ArenaEntry* e = p.Find(h);
    if (kind == ARENA_KKT && std::strcmp(h, "HA2") == 0) { HOLD(!e); continue; }
    HOLD(e && e->count == 3 * p.band && e->count == sb.bands && e->elem == sizeof(double));
    if (!e) continue;
    const std::string b = std::string("HB") + (h[2] ? "2" : ""), c = std::string("HC") + (h[2] ? "2" : "");
    size_t ob = 0, oc = 0, rb = 0, rc = 0;
    HOLD(p.Locate(b, &ob, &rb) && p.Locate(c, &oc, &rc));
    HOLD(ob == e->offset + p.band * sizeof(double) && oc == ob + p.band * sizeof(double) && rb == 2 * p.band && rc == p.band);
  }
  // the solvers' arrays have the counts of SolverBufferCounts (a KKT context: of its block size nq + nu, which is its nq)
  const struct { const char* name; size_t count, elem; } solver[] = {
      {"Ust", sb.factors, 8}, {"Hst", sb.factors, 8}, {"Est", sb.factors, 8}, {"Dst", sb.dinv, 8}, {"dbg", sb.dbg, 8}, {"xch", sb.xch, 8},
      {"flags", sb.flags, 4}, {"nd_rowcnt", sb.rowcnt, 8}, {"pipe_rowcnt", sb.rowcnt, 8}, {"nd_buf", sb.nd_buf, 8}, {"nd_wst", sb.nd_wst, 8}};
  for (const auto& s : solver) {
    const ArenaEntry* e = p.Find(s.name);
    HOLD(e && e->count == s.count && e->elem == s.elem);
  }
  HOLD(p.has_wst == sb.has_wst && p.xch_count == sb.xch_count && p.flag_count == sb.flags);
  HOLD(p.Find("g") && p.Find("g")->count == (size_t)(N + 1) * nq && p.Find("step") && p.Find("step")->count == (size_t)(N + 1) * nq);
  if (kind == ARENA_KKT) {
    HOLD(p.entries.size() == 14 && p.alt_off == 0);
    return;
  }
  HOLD(p.slab_stride == 3 * nv * nq + nv);
  // the second set of fd_kernel's outputs: the first set's relative offsets, entry for entry
  HOLD(p.alt_off > 0);
  for (const char* f : {"v", "a", "nplus", "slab", "terms"}) {
    const ArenaEntry *e = p.Find(f), *t = p.Find(std::string(f) + "_alt");
    HOLD(e && t && (long long)(t->offset - e->offset) == p.alt_off && t->count == e->count && t->elem == e->elem);
  }
  // the problem's stretch is one run in the order UploadProblemArrays copies it
  HOLD(std::strcmp(p.entries[0].name, "d_vinit") == 0 && std::strcmp(p.entries[12].name, "d_w[9]") == 0);
  // 3. every array id with an arena entry fits it
  for (int id : ArrayIds()) {
    const ArrayInfo a = ArrayLookup(id, nq, nv, N);
    if (a.where == ArrayInfo::ENTRY) {
      size_t off = 0, room = 0;
      HOLD(p.Locate(a.field, &off, &room) && a.count >= 0 && (size_t)a.count <= std::max<size_t>(room, 1));
    } else if (a.where == ArrayInfo::SLAB_ROWS) {
      HOLD(a.at + a.width <= (size_t)p.slab_stride && a.count == (long)(N * a.width));
      HOLD(p.Find("slab") && (size_t)N * p.slab_stride <= p.Find("slab")->count);
    } else {
      HOLD(a.where == ArrayInfo::OUTSIDE && a.count == -1);
    }
  }
}

// 3. the launch sizes: the formulas once more, as the kernels carve their LDS (kernels.h assemble_kernel,
// assemble_diag_kernel, assemble_terms_kernel, penta_kernel, penta_solve_kernel, cost_kernel; penta_apply.h)
static void HoldLaunchSizes(int nq, int nv, int N) {
  const LaunchSizes s = PlanLaunchSizes(nq, nv, N);
  const int D = 8, n = N + 1, nvp = (nv + 1) & ~1, mx = std::max(nq, nv);
  HOLD(s.asm_lds == D * (3 * nq + 5 * nv * nq + 4 * nv + nq + mx + nv * nq + 3 * nq * nq + nq));
  HOLD(s.asm_diag_lds == D * (14 * nvp * nq + 2 * nv * nq + 10 * nv + 6 * nq + 2));
  HOLD(s.asm_terms_lds == D * (5 * nvp * nq + 4 * nv + nq + 2));
  HOLD(s.asm_terms_threads == std::min(512, std::max(256, (std::max(nq * (nq + 1) / 2 + nq, ((nq + 1) / 2) * nq) + 63) / 64 * 64)));
  HOLD(s.penta_lds == D * (10 * nq * nq + nq * (3 * nq + 1) + (n + 2) * nq + nq) + 4 * nq + 16);
  HOLD(s.solve_lds == D * ((n + 2) * nq + nq));
  HOLD(s.cost_lds == D * ((3 * N + 2) * (1 + mx) + 2 * (N + 1) + 2));
  HOLD(s.apply_lds == ApplyLds(n, SolverBlockSize(nq)));
}

static std::string Produce(bool hold) {
  std::string out = "# arena layouts of tests/cpp/context_layout_check.cc: byte offsets of every entry, in carve order\n"
                    "# (the examples: acrobot 2/2, spinner 3/3, hopper 5/5, jaco 14/13, mini_cheetah 19/18, punyo 21/20, allegro_hand 23/22;\n"
                    "# their KKT contexts: blocks of nq + nu = 3, 4, 8, 20, 25, 27, 29)\n";
  static const int model[][3] = {{2, 2, 40}, {2, 2, 1}, {2, 2, 3}, {3, 3, 40}, {5, 5, 40}, {14, 13, 40}, {19, 18, 20}, {21, 20, 40}, {23, 22, 40}};
  static const int kkt[][2] = {{3, 40}, {3, 1}, {3, 3}, {4, 40}, {8, 40}, {8, 3}, {20, 40}, {25, 20}, {27, 40}, {29, 40}};
  for (auto& m : model) out += Line(ARENA_MODEL, m[0], m[1], m[2], PlanArena(ARENA_MODEL, m[0], m[1], m[2]));
  for (auto& k : kkt) out += Line(ARENA_KKT, k[0], 0, k[1], PlanArena(ARENA_KKT, k[0], 0, k[1]));
  for (int kind = 0; kind < 2; ++kind)
    for (int nq = 1; nq <= 32; ++nq) {
      Sha256 h;
      const int nv = kind == ARENA_MODEL ? nq : 0;
      for (int N : kSweepN) {
        const ArenaPlan p = PlanArena((ArenaKind)kind, nq, nv, N);
        const std::string line = Line((ArenaKind)kind, nq, nv, N, p);
        h.Update(line.data(), line.size());
        if (hold) {
          g_case.assign(line, 0, line.find(" :"));
          HoldPlan((ArenaKind)kind, nq, nv, N, p);
          if (kind == ARENA_MODEL) HoldLaunchSizes(nq, nv, N);
        }
      }
      out += std::string("digest ") + (kind == ARENA_MODEL ? "model " : "kkt ") + std::to_string(nq) + " " + h.Hex() + "\n";
    }
  if (hold)   // (nq != nv: the examples)
    for (auto& m : model) {
      g_case = "example " + std::to_string(m[0]) + " " + std::to_string(m[1]) + " " + std::to_string(m[2]);
      HoldPlan(ARENA_MODEL, m[0], m[1], m[2], PlanArena(ARENA_MODEL, m[0], m[1], m[2]));
      HoldLaunchSizes(m[0], m[1], m[2]);
    }
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: context_layout_check <fixture> | --print\n"); return 2; }
  if (std::strcmp(argv[1], "--print") == 0) { std::fputs(Produce(false).c_str(), stdout); return 0; }
  const std::string got = Produce(true);
  std::ifstream f(argv[1]);
  const std::string want((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  int diff = 0;
  if (got != want) {
    size_t a = 0, b = 0;
    while (a < got.size() || b < want.size()) {
      const size_t ea = std::min(got.find('\n', a), got.size()), eb = std::min(want.find('\n', b), want.size());
      const std::string la = got.substr(a, ea - a), lb = want.substr(b, eb - b);
      if (la != lb && ++diff <= 10) std::printf("DIFFERS\n  plan:    %.300s\n  fixture: %.300s\n", la.c_str(), lb.c_str());
      a = ea + 1; b = eb + 1;
    }
    if (!diff) diff = 1;
  }
  // an id the table does not have
  g_case = "unknown id";
  HOLD(ArrayLookup(23, 2, 2, 3).where == ArrayInfo::UNKNOWN && ArrayLookup(-1, 2, 2, 3).count == -1);
  std::printf("%s: %d lines differ from the fixture, %d conditions broken\n", (diff || g_bad) ? "FAILED" : "ok", diff, g_bad);
  return (diff || g_bad) ? 1 : 0;
}
