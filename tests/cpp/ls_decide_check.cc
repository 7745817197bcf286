// ls_decide_check.cc — csrc/ls_decide.h on the CPU (tests/test_ls_decide.py builds this with
// -fsanitize=address,undefined and runs it):
//   1. both step-length chains against literal doubles;
//   2. the scans against a plain restatement of the two host loops (host/trajectory_optimizer.cc ArmijoLinesearch,
//      BacktrackingLinesearch: the loops as they stand there, with the cost of a step length read from a table) over
//      seeded cost sequences;
//   3. every chunking of the same sequence - one, three, seven candidates at a time, all at once - gives the same answer;
//   4. the edge cases: a NaN cost, equal costs, L' = 0, L' > 0, L' = NaN, the early-outs, Armijo exhausted, backtracking
//      undecided within the 64 candidates a device loop covers;
//   5. host/ls_rows.cc: the device loop's statistics rows into TrajectoryOptimizerStats, flag and errors;
//   6. host/solver_plan.cc PlanLsWaves: every schedule of a sweep over (horizon, compute units, method, limit, override)
//      covers every candidate index exactly once, in order, no wave wider than the cap, and reproduces
//      tests/golden/ls_waves.txt (the examples' schedules in clear text).
// usage: ls_decide_check <fixture>            (--print: write the fixture's text to stdout instead of comparing)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <stdexcept>
#include <utility>
#include <vector>

#include "host/ls_rows.h"
#include "host/solver_plan.h"
#include "ls_decide.h"

using namespace idto_ls;

static int g_bad = 0;
#define HOLD(cond)                                                              \
  do {                                                                          \
    if (!(cond) && ++g_bad <= 20) std::printf("BROKEN line %d: %s\n", __LINE__, #cond); \
  } while (0)

// ---- the host loops, restated: `cost(j)` is the cost at the j-th step length the loop asks for.  A request beyond
// the table throws Beyond (backtracking is not bounded).
struct Beyond {};
struct Table {
  const std::vector<double>& c;
  int asked = 0;
  double operator()() {
    if (asked >= (int)c.size()) throw Beyond{};
    return c[(std::size_t)asked++];
  }
};

static std::pair<double, int> HostArmijo(double L, double L_prime, double dt, int max_iters, Table cost) {
  const double c = 1e-4, rho = 0.8;
  double alpha = 1.0 / rho;
  if (!(L_prime <= 0)) throw std::runtime_error("not a descent direction");
  const double thr = 10 * std::numeric_limits<double>::epsilon() / dt / dt;
  if (std::fabs(L_prime) / std::fabs(L) <= thr) return {1.0, 0};
  int i = 0;
  double L_new;
  do {
    alpha *= rho;
    L_new = cost();
    ++i;
  } while ((L_new > L + c * alpha * L_prime) && (i < max_iters));
  return {alpha, i};
}

static std::pair<double, int> HostBacktracking(double L, double L_prime, Table cost) {
  const double c = 1e-4, rho = 0.8;
  double alpha = 1.0;
  if (!(L_prime <= 0)) throw std::runtime_error("not a descent direction");
  if (std::fabs(L_prime) / std::fabs(L) <= std::sqrt(std::numeric_limits<double>::epsilon())) return {1.0, 0};
  double L_old = cost(), L_new = L_old;
  int i = 0;
  bool armijo_met = false;
  while (!(armijo_met && (L_new > L_old))) {
    L_old = L_new;
    alpha *= rho;
    L_new = cost();
    if (L_new <= L + c * alpha * L_prime) armijo_met = true;
    ++i;
  }
  return {alpha / rho, i};
}

struct Answer {
  int status;
  double alpha;
  int iters;
  bool operator==(const Answer& o) const {
    return status == o.status && iters == o.iters && ((alpha == o.alpha) || (alpha != alpha && o.alpha != o.alpha));
  }
};

// the scan, fed `chunk` candidates at a time (0: all at once)
static Answer Scan(int method, double L, double Lp, double dt, int max_iters, const std::vector<double>& costs, int chunk) {
  LsScan s = ls_begin(method, L, Lp, dt, max_iters);
  const int m = (int)costs.size();
  if (chunk <= 0) chunk = m > 0 ? m : 1;
  for (int at = 0; at < m && s.status == LS_UNDECIDED; at += chunk) {
    HOLD(s.next == at);
    ls_scan(&s, costs.data() + at, std::min(chunk, m - at));
  }
  return {s.status, s.alpha, s.ls_iters};
}

// the host loop's answer in the scan's terms (LS_UNDECIDED: the loop asked for more than the table holds)
static Answer Host(int method, double L, double Lp, double dt, int max_iters, const std::vector<double>& costs) {
  try {
    const auto r = method == kArmijo ? HostArmijo(L, Lp, dt, max_iters, Table{costs}) : HostBacktracking(L, Lp, Table{costs});
    int status = LS_DECIDED;
    if (method == kArmijo && r.second >= 1) {   // exhausted: the loop left on its count, the last cost still too high
      const double last = costs[(std::size_t)r.second - 1];
      if (last > L + 1e-4 * r.first * Lp) status = LS_EXHAUSTED;
    }
    return {status, r.first, r.second};
  } catch (const Beyond&) {
    return {LS_UNDECIDED, 1.0, 0};
  } catch (const std::runtime_error&) {
    return {LS_NOT_DESCENT, 1.0, 0};
  }
}

static void Compare(int method, double L, double Lp, double dt, int max_iters, const std::vector<double>& costs) {
  const Answer host = Host(method, L, Lp, dt, max_iters, costs);
  const int chunks[4] = {1, 3, 7, 0};
  for (int chunk : chunks) {
    const Answer dev = Scan(method, L, Lp, dt, max_iters, costs, chunk);
    if (!(dev == host) && ++g_bad <= 20)
      std::printf("BROKEN method %d L %.17g L' %.17g max %d chunk %d: scan (%d, %.17g, %d) host (%d, %.17g, %d)\n", method, L,
                  Lp, max_iters, chunk, dev.status, dev.alpha, dev.iters, host.status, host.alpha, host.iters);
  }
}

static std::uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double Uniform() {   // xorshift64*, in [0, 1)
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

// ---- 5. the rows
static void CheckRows() {
  using namespace idto::optimizer;
  using namespace idto::optimizer::internal;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // three iterations ran of five, the third reached the limit
  std::vector<double> rows(5 * kLsRow, 0.0);
  for (int k = 0; k < 3; ++k) {
    double* R = rows.data() + k * kLsRow;
    R[0] = 10.0 - k; R[1] = 0.8; R[2] = 2 + k; R[3] = 0.9; R[4] = 3.0; R[5] = 0.5; R[6] = 7.0; R[7] = -1.5; R[8] = 0.25;
    R[9] = 9.0 - k; R[10] = 1e6 + 2000.0 * k; R[11] = k == 2 ? 64.0 : 0.0;
  }
  TrajectoryOptimizerStats<double> st;
  LsRowsResult res;
  LsRowsToStats(rows.data(), 5, 1e-3, LinesearchMethod::kArmijo, &st, &res);
  HOLD(res.outcome == LsRowsOutcome::kDone && res.iterations == 3 && res.flag == SolverFlag::kLinesearchMaxIters);
  HOLD(st.iteration_costs.size() == 3 && st.iteration_costs[1] == 9.0 && st.linesearch_iterations[2] == 4);
  HOLD(st.linesearch_alphas[0] == 0.8 && st.trust_region_radii[0] != st.trust_region_radii[0] && st.q_norms[0] == 3.0);
  HOLD(st.dq_norms[0] == 0.5 && st.dqH_norms[0] == 0.5 && st.trust_ratios[0] == 0.9 && st.gradient_norms[0] == 7.0);
  HOLD(st.dL_dqs[1] == -1.5 / 9.0 && st.h_norms[0] == 0.25 && st.merits[2] == 8.0 && st.solve_time == 1e-3);
  HOLD(st.iteration_times[1] == 2000.0 * 1e-8 && st.iteration_times[0] == 1e-3 - 2 * 2000.0 * 1e-8);
  rows[2 * kLsRow + 11] = 0.0;
  st = TrajectoryOptimizerStats<double>(); LsRowsToStats(rows.data(), 5, 1e-3, LinesearchMethod::kArmijo, &st, &res);
  HOLD(res.outcome == LsRowsOutcome::kDone && res.iterations == 3 && res.flag == SolverFlag::kSuccess);
  // the flags that end a loop: the rows in front are taken
  struct { int flag; LsRowsOutcome outcome; } ends[4] = {{128, LsRowsOutcome::kNeedsHostLoop}, {32, LsRowsOutcome::kFailed},
                                                         {4, LsRowsOutcome::kError}, {4 | 2, LsRowsOutcome::kError}};
  for (const auto& e : ends)
    for (LinesearchMethod m : {LinesearchMethod::kArmijo, LinesearchMethod::kBacktracking}) {
      std::vector<double> r2 = rows;
      for (int i = 0; i < kLsRow; ++i) r2[2 * kLsRow + i] = 0.0;
      r2[2 * kLsRow + 0] = nan; r2[2 * kLsRow + 10] = 1e6 + 4000.0; r2[2 * kLsRow + 11] = e.flag;
      st = TrajectoryOptimizerStats<double>(); LsRowsToStats(r2.data(), 5, 1e-3, m, &st, &res);
      HOLD(res.outcome == e.outcome && res.iterations == 2 && st.iteration_costs.size() == 2);
      if (e.flag == 32) HOLD(res.flag == SolverFlag::kFactorizationFailed && res.error == "idto_hip: factorisation failed in iteration 2");
      if (e.flag & 4)
        HOLD(res.error == (m == LinesearchMethod::kArmijo ? "linesearch: not a descent direction (TO.cc:1951)"
                                                          : "linesearch: not a descent direction (TO.cc:1888)"));
    }
  // a flagged FIRST row without a clock still counts; no row at all is an empty run
  std::vector<double> first(2 * kLsRow, 0.0);
  first[11] = 4.0;
  st = TrajectoryOptimizerStats<double>(); LsRowsToStats(first.data(), 2, 1e-3, LinesearchMethod::kArmijo, &st, &res);
  HOLD(res.outcome == LsRowsOutcome::kError && res.iterations == 0 && st.is_empty());
  first[11] = 0.0;
  st = TrajectoryOptimizerStats<double>(); LsRowsToStats(first.data(), 2, 1e-3, LinesearchMethod::kArmijo, &st, &res);
  HOLD(res.outcome == LsRowsOutcome::kDone && res.iterations == 0 && st.is_empty() && res.flag == SolverFlag::kSuccess);
}

// ---- 6. the waves
static std::string WaveLine(int N, int cus, int method, int max_ls, int over) {
  int w[idto_host::kLsMaxCandidates];
  const int n = idto_host::PlanLsWaves(N, cus, method, max_ls, over, w);
  const int total = method == kArmijo ? std::min(kMaxCandidates, std::max(1, max_ls)) : kMaxCandidates;
  int sum = 0;
  HOLD(n >= 1 && n <= idto_host::kLsMaxCandidates);
  std::ostringstream o;
  o << "N " << N << " cus " << cus << " method " << method << " max " << max_ls << " ls_waves " << over << " :";
  for (int i = 0; i < n && i < idto_host::kLsMaxCandidates; ++i) {
    HOLD(w[i] >= 1 && w[i] <= kMaxCandidates);
    if (over > 0 && i + 1 < n) HOLD(w[i] == over);
    if (over <= 0 && i > 0 && i + 1 < n) HOLD(w[i] == 2 * w[i - 1]);   // (geometrically wider, the last wave takes the rest)
    sum += w[i];   // wave i covers [sum before, sum after): every index once, in order, by construction of the prefix sums
    o << " " << w[i];
  }
  HOLD(sum == total);
  o << "\n";
  return o.str();
}
static std::string Waves() {
  std::string text, all;
  // the examples and the tests' shapes in clear text (an MI355X has 256 compute units)
  const int shapes[7][2] = {{20, 256}, {40, 256}, {50, 256}, {4, 256}, {6, 256}, {140, 256}, {50, 104}};
  for (const auto& sh : shapes)
    for (int method : {kArmijo, kBacktracking})
      for (int max_ls : {8, 50})
        text += WaveLine(sh[0], sh[1], method, max_ls, 0);
  for (int over : {1, 3, 5, 64}) text += WaveLine(4, 256, kArmijo, 50, over);
  // the sweep holds the properties (HOLD above); its text is not recorded
  for (int N = 1; N <= 300; N += (N < 70 ? 1 : 23))
    for (int cus : {1, 64, 104, 256, 304, 1024})
      for (int method : {kArmijo, kBacktracking})
        for (int max_ls : {-1, 0, 1, 2, 7, 8, 50, 63, 64})
          for (int over : {0, 1, 3, 5, 63, 64}) all += WaveLine(N, cus, method, max_ls, over);
  HOLD(!all.empty());
  return text;
}

int main(int argc, char** argv) {
  CheckRows();
  {
    const std::string text = Waves();
    if (argc > 1 && std::strcmp(argv[1], "--print") == 0) {
      std::fputs(text.c_str(), stdout);
      return g_bad ? 1 : 0;
    }
    if (argc < 2) { std::printf("usage: ls_decide_check <fixture> | --print\n"); return 2; }
    std::ifstream f(argv[1]);
    std::stringstream have;
    have << f.rdbuf();
    if (!f || have.str() != text) { ++g_bad; std::printf("BROKEN: the wave schedules differ from %s\n", argv[1]); }
  }
  // 1. the chains
  {
    double a[kMaxCandidates], b[kMaxCandidates];
    ls_alpha_chain(kArmijo, kMaxCandidates, a);
    ls_alpha_chain(kBacktracking, kMaxCandidates, b);
    const double lit[8] = {1.0, 0.8, 0.6400000000000001, 0.5120000000000001, 0.40960000000000013, 0.32768000000000014,
                           0.2621440000000001, 0.2097152000000001};
    for (int j = 0; j < 8; ++j) { HOLD(a[j] == lit[j]); HOLD(b[j] == lit[j]); }
    HOLD(1.0 / 0.8 * 0.8 == 1.0);
    double x = 1.0;
    for (int j = 0; j < kMaxCandidates; ++j) { HOLD(a[j] == x); HOLD(b[j] == x); x *= 0.8; }
    HOLD(a[17] == 0.022517998136852502);
    HOLD(kEps == std::numeric_limits<double>::epsilon());
    HOLD(kSqrtEps == std::sqrt(std::numeric_limits<double>::epsilon()));
  }
  // 2. + 3. seeded sequences: a cost that first rises above L, then falls along the chain, with noise; random limits
  for (int trial = 0; trial < 4000; ++trial) {
    const double L = 1.0 + 99.0 * Uniform();
    const double Lp = -L * (1e-6 + Uniform());
    const int max_iters = 1 + (int)(Uniform() * 20);
    const int len = 1 + (int)(Uniform() * kMaxCandidates);
    const double knee = Uniform() * 0.5, bump = L * Uniform() * 0.3, noise = Uniform() < 0.3 ? 1e-3 * L : 0.0;
    std::vector<double> costs((std::size_t)len);
    double alpha = 1.0;
    for (int j = 0; j < len; ++j) {
      const double over = alpha > knee ? (alpha - knee) * bump * 4 : 0.0;
      costs[(std::size_t)j] = L + alpha * Lp * 0.5 + over + noise * (Uniform() - 0.5);
      alpha *= 0.8;
    }
    Compare(kArmijo, L, Lp, 0.05, max_iters, costs);
    Compare(kBacktracking, L, Lp, 0.05, max_iters, costs);
  }
  // 4. edge cases
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  {
    // a NaN cost is accepted at once by Armijo (NaN > bound is false)
    const Answer a = Scan(kArmijo, 10.0, -1.0, 0.05, 50, {nan, 1.0}, 0);
    HOLD(a.status == LS_DECIDED && a.alpha == 1.0 && a.iters == 1);
    Compare(kArmijo, 10.0, -1.0, 0.05, 50, {11.0, nan, 1.0});
    // ... and by backtracking never meets the condition nor compares greater: the scan runs on
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, {nan, nan, nan, nan});
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, {9.0, nan, 8.0, 8.5});
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, {9.0, 8.0, nan, 8.5, 8.6});
    Compare(kArmijo, 10.0, -1.0, 0.05, 50, {inf, inf, 9.0});
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, {inf, inf, 9.0, 9.5});
  }
  {
    // equal costs: backtracking needs a strict rise, Armijo a cost not above its bound
    std::vector<double> flat(70, 9.0);
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, flat);
    HOLD(Scan(kBacktracking, 10.0, -1.0, 0.05, 4, std::vector<double>(kMaxCandidates, 9.0), 0).status == LS_UNDECIDED);
    Compare(kArmijo, 10.0, -1.0, 0.05, 50, flat);
    std::vector<double> at_L(70, 10.0);   // cost == L: above L + c alpha L' for every alpha
    Compare(kArmijo, 10.0, -1.0, 0.05, 50, at_L);
    const Answer a = Scan(kArmijo, 10.0, -1.0, 0.05, 50, at_L, 7);
    double a50[50];
    ls_alpha_chain(kArmijo, 50, a50);
    HOLD(a.status == LS_EXHAUSTED && a.iters == 50 && a.alpha == a50[49]);
    // the bound itself is accepted (L_new > bound is false)
    const double bound = 10.0 + 1e-4 * 1.0 * -1.0;
    const Answer e = Scan(kArmijo, 10.0, -1.0, 0.05, 50, {bound}, 0);
    HOLD(e.status == LS_DECIDED && e.iters == 1);
  }
  {
    // L' = 0: a descent direction by the host's test, and the early-out of both
    for (int method : {kArmijo, kBacktracking}) {
      const LsScan s = ls_begin(method, 10.0, 0.0, 0.05, 50);
      HOLD(s.status == LS_DECIDED && s.alpha == 1.0 && s.ls_iters == 0);
      Compare(method, 10.0, 0.0, 0.05, 50, {1.0, 2.0});
      Compare(method, 10.0, -0.0, 0.05, 50, {1.0, 2.0});
      // L' > 0, L' = NaN: where the host throws
      HOLD(ls_begin(method, 10.0, 1e-300, 0.05, 50).status == LS_NOT_DESCENT);
      HOLD(ls_begin(method, 10.0, nan, 0.05, 50).status == LS_NOT_DESCENT);
      Compare(method, 10.0, 1.0, 0.05, 50, {1.0, 2.0});
      Compare(method, 10.0, nan, 0.05, 50, {1.0, 2.0});
      LsScan t = ls_begin(method, 10.0, 1.0, 0.05, 50);
      HOLD(ls_feed(&t, 1.0) == LS_NOT_DESCENT && t.next == 0);   // (sticky)
    }
    // the early-outs' thresholds: Armijo 10 eps / dt^2 (dt = 0.05: 8.88e-13), backtracking sqrt(eps) (1.49e-8), both inclusive
    const double thr = 10 * std::numeric_limits<double>::epsilon() / 0.05 / 0.05;
    HOLD(ls_begin(kArmijo, 1.0, -thr, 0.05, 50).status == LS_DECIDED);
    HOLD(ls_begin(kArmijo, 1.0, -std::nextafter(thr, 1.0), 0.05, 50).status == LS_UNDECIDED);
    HOLD(ls_begin(kArmijo, -1.0, -thr, 0.05, 50).status == LS_DECIDED);   // |L|
    HOLD(ls_begin(kBacktracking, 1.0, -kSqrtEps, 0.05, 50).status == LS_DECIDED);
    HOLD(ls_begin(kBacktracking, 1.0, -std::nextafter(kSqrtEps, 1.0), 0.05, 50).status == LS_UNDECIDED);
    HOLD(ls_begin(kBacktracking, 1.0, -1e-10, 0.05, 50).status == LS_DECIDED);
    HOLD(ls_begin(kArmijo, 1.0, -1e-10, 0.05, 50).status == LS_UNDECIDED);
    Compare(kArmijo, 1.0, -1e-10, 0.05, 50, {2.0, 0.5});
    Compare(kBacktracking, 1.0, -1e-10, 0.05, 50, {2.0, 0.5});
    HOLD(ls_begin(kArmijo, 0.0, 0.0, 0.05, 50).status == LS_UNDECIDED);   // 0 / 0 = NaN <= thr is false, as on the host
    Compare(kArmijo, 0.0, 0.0, 0.05, 50, {1.0, -1.0});
  }
  {
    // Armijo exhausted at the limit; at a limit of 1 (and below: the do-while evaluates once) after one candidate
    std::vector<double> high(kMaxCandidates, 11.0);
    for (int max_iters : {0, 1, 2, 8, 50, 64}) {
      Compare(kArmijo, 10.0, -1.0, 0.05, max_iters, high);
      const Answer a = Scan(kArmijo, 10.0, -1.0, 0.05, max_iters, high, 3);
      HOLD(a.status == LS_EXHAUSTED && a.iters == std::max(1, max_iters));
      HOLD(ls_limit_reached(a.iters, max_iters));
    }
    // decided by its cost at exactly the limit: an answer for the scan, a failed linesearch for the solve
    std::vector<double> last_ok = {11.0, 11.0, 11.0, 9.0};
    const Answer a = Scan(kArmijo, 10.0, -1.0, 0.05, 4, last_ok, 1);
    HOLD(a.status == LS_DECIDED && a.iters == 4 && ls_limit_reached(a.iters, 4));
    Compare(kArmijo, 10.0, -1.0, 0.05, 4, last_ok);
    // backtracking runs past the limit (the oracle returns 10 with the limit at 4)
    std::vector<double> down_then_up = {9.9, 9.8, 9.7, 9.6, 9.5, 9.4, 9.3, 9.2, 9.1, 9.0, 9.05};
    const Answer b = Scan(kBacktracking, 10.0, -1.0, 0.05, 4, down_then_up, 3);
    double b12[12];
    ls_alpha_chain(kBacktracking, 12, b12);
    HOLD(b.status == LS_DECIDED && b.iters == 10 && b.alpha == b12[10] / 0.8 && ls_limit_reached(b.iters, 4));
    Compare(kBacktracking, 10.0, -1.0, 0.05, 4, down_then_up);
    // ... and is undecided when the cost still falls at candidate 63
    std::vector<double> falling(kMaxCandidates);
    for (int j = 0; j < kMaxCandidates; ++j) falling[(std::size_t)j] = 9.0 - 0.01 * j;
    HOLD(Scan(kBacktracking, 10.0, -1.0, 0.05, 50, falling, 7).status == LS_UNDECIDED);
    Compare(kBacktracking, 10.0, -1.0, 0.05, 50, falling);
  }
  if (g_bad) {
    std::printf("FAILED: %d checks\n", g_bad);
    return 1;
  }
  std::printf("ok: chains, scans against the host loops, chunkings, edge cases, rows, waves\n");
  return 0;
}
