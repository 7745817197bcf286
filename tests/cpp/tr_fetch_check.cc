// tr_fetch.h on the CPU: the staging layout of the trust-region fetches walked over its cases.  For each case the parts,
// taken in the documented order, tile [0, total()) with no gap and no overlap; fetch_total() equals the closed formulas,
// written out here; a trajectory block reads q, v, tau, dq, w.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tr_fetch.h"

using idto_fetch::TrFetchLayout;

static int g_checks = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    ++g_checks;                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Piece { size_t at, count; };

int main() {
  const int Bs[] = {1, 2, 3, 37}, iters[] = {1, 7}, dims[][3] = {{3, 2, 2}, {4, 7, 6}, {40, 19, 18}};
  const int nstate = 12, row = 16;   // (any: the layout takes the counts as numbers)
  for (int B : Bs)
    for (int it : iters)
      for (int only_best = 0; only_best < 2; ++only_best)
        for (int hook = 0; hook < 2; ++hook)
          for (const auto& d : dims) {
            const int N = d[0], nq = d[1], nv = d[2];
            const bool batch = B > 1;   // B = 1: the single-problem form (no header, no choice, no hook)
            if (!batch && (only_best || hook)) continue;
            const size_t nrows = (size_t)it * row, nqa = (size_t)(N + 1) * nq, nva = (size_t)(N + 1) * nv, nta = (size_t)N * nv;
            const size_t nguess = hook ? (size_t)B * nqa : 0, nplans = hook ? (size_t)B * 5 * (nq + nv + 1) : 0;
            const TrFetchLayout L = TrFetchLayout::Make(B, nstate, nrows, N, nq, nv, only_best != 0, batch, nguess, nplans);
            const size_t T = batch ? (only_best ? 1 : (size_t)B) : 1;
            // (b) the closed formulas
            if (batch) CHECK(L.fetch_total() == 1 + 2 * (size_t)B + (size_t)B * (nstate + nrows) + T * (3 * nqa + nva + nta));
            else CHECK(L.fetch_total() == nstate + nrows + 3 * nqa + nva + nta);
            CHECK(L.total() == L.fetch_total() + nguess + nplans);
            CHECK(L.slots == T && L.nrows == nrows && L.nstate == (size_t)nstate);
            // (a) the parts in the documented order
            std::vector<Piece> parts;
            if (batch) {
              parts.push_back({L.header(), 1});
              parts.push_back({L.final_cost(), (size_t)B});
              parts.push_back({L.status(), (size_t)B});
            }
            for (int b = 0; b < (batch ? B : 1); ++b) {
              parts.push_back({L.state(b), (size_t)nstate});
              parts.push_back({L.rows(b), nrows});
            }
            // (c) q, v, tau, dq, w
            const size_t want[5] = {nqa, nva, nta, nqa, nqa};
            CHECK(TrFetchLayout::Q == 0 && TrFetchLayout::V == 1 && TrFetchLayout::TAU == 2 && TrFetchLayout::DQ == 3 && TrFetchLayout::W == 4);
            for (size_t t = 0; t < T; ++t) {
              CHECK(L.part(t, 0) == L.traj(t));
              for (int i = 0; i < 5; ++i) {
                CHECK(L.cnt[i] == want[i]);
                parts.push_back({L.part(t, i), L.cnt[i]});
              }
              CHECK(L.traj(t) + L.traj_doubles() == L.traj(t + 1));
            }
            CHECK(L.traj(T) == L.fetch_total());
            parts.push_back({L.guess(), nguess});
            parts.push_back({L.plans(), nplans});
            size_t at = 0;
            for (const Piece& p : parts) { CHECK(p.at == at); at += p.count; }
            CHECK(at == L.total());
            // every double belongs to exactly one part
            std::vector<unsigned char> seen(L.total(), 0);
            for (const Piece& p : parts)
              for (size_t i = 0; i < p.count; ++i) { CHECK(seen[p.at + i] == 0); seen[p.at + i] = 1; }
            for (unsigned char s : seen) CHECK(s == 1);
          }
  std::printf("ok: %d checks\n", g_checks);
  return 0;
}
