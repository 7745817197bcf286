// ls_fetch.h on the CPU: the staging layout of the linesearch loop's fetches walked over its cases.  For each case the
// parts, taken in the documented order, tile [0, total()) with no gap and no overlap; total() equals the closed formulas,
// written out here; a problem's block reads rows, q, v, tau; with one problem the layout is the single fetch's order
// (idto_hip_ls_solve_fetch: rows at 0, then q, v, tau - no header).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ls_fetch.h"

using idto_fetch::LsFetchLayout;

static int g_checks = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Piece { size_t at, count; };

int main() {
  const int Bs[] = {1, 2, 3, 37, 64}, iters[] = {1, 7}, dims[][3] = {{1, 2, 2}, {3, 2, 2}, {4, 7, 6}, {40, 19, 18}};
  const int row = 12;   // (IDTO_LS_ROW; the layout takes it as a number)
  for (int B : Bs)
    for (int it : iters)
      for (int batch_form = 0; batch_form < 2; ++batch_form)
        for (const auto& d : dims) {
          const int N = d[0], nq = d[1], nv = d[2];
          if (!batch_form && B > 1) continue;   // (the single form has one problem, whatever B says: checked below for B = 1)
          const size_t nrows = (size_t)it * row, nqa = (size_t)(N + 1) * nq, nva = (size_t)(N + 1) * nv, nta = (size_t)N * nv;
          const LsFetchLayout L = LsFetchLayout::Make(B, it, row, N, nq, nv, batch_form != 0);
          const size_t P = (size_t)B;
          // (b) the closed formulas
          CHECK(L.B == P && L.nrows == nrows && L.head == (batch_form ? P : 0));
          CHECK(L.problem_doubles() == nrows + nqa + nva + nta);
          CHECK(L.total() == (batch_form ? P : 0) + P * (nrows + nqa + nva + nta));
          // (a) the parts in the documented order
          std::vector<Piece> parts;
          if (batch_form) parts.push_back({L.final_cost(), P});
          const size_t want[3] = {nqa, nva, nta};
          CHECK(LsFetchLayout::Q == 0 && LsFetchLayout::V == 1 && LsFetchLayout::TAU == 2);
          for (size_t b = 0; b < P; ++b) {
            parts.push_back({L.rows(b), nrows});
            CHECK(L.part(b, 0) == L.rows(b) + nrows);
            for (int i = 0; i < 3; ++i) {
              CHECK(L.cnt[i] == want[i]);
              parts.push_back({L.part(b, i), L.cnt[i]});
            }
            CHECK(L.rows(b) + L.problem_doubles() == L.rows(b + 1));
          }
          CHECK(L.rows(P) == L.total());
          size_t at = 0;
          for (const Piece& p : parts) { CHECK(p.at == at); at += p.count; }
          CHECK(at == L.total());
          // every double belongs to exactly one part
          std::vector<unsigned char> seen(L.total(), 0);
          for (const Piece& p : parts)
            for (size_t i = 0; i < p.count; ++i) { CHECK(seen[p.at + i] == 0); seen[p.at + i] = 1; }
          for (unsigned char s : seen) CHECK(s == 1);
          // (c) the single form is the single fetch's order, and a batch of one problem is the same behind its one header word
          if (!batch_form) {
            CHECK(L.rows(0) == 0 && L.part(0, LsFetchLayout::Q) == nrows && L.part(0, LsFetchLayout::V) == nrows + nqa &&
                  L.part(0, LsFetchLayout::TAU) == nrows + nqa + nva && L.total() == nrows + nqa + nva + nta);
            const LsFetchLayout S = LsFetchLayout::Make(5, it, row, N, nq, nv, false);   // (B is ignored without the batch form)
            CHECK(S.B == 1 && S.total() == L.total());
          } else if (B == 1) {
            const LsFetchLayout S = LsFetchLayout::Make(1, it, row, N, nq, nv, false);
            CHECK(L.rows(0) == S.rows(0) + 1);
            for (int i = 0; i < 3; ++i) CHECK(L.part(0, i) == S.part(0, i) + 1);
          }
        }
  std::printf("ok: %d checks\n", g_checks);
  return 0;
}
