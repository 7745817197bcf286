// batch_rows_check.cc — stand-alone check of host/batch_rows.cc: one problem's statistics rows of the device loop ->
// TrajectoryOptimizerStats, convergence reason, radius, SolverFlag, on hand-written rows; and the stepwise loop's scalars -
// the dogleg step against a restatement on vectors, the trust ratio and the descent test on hand-computed inputs.  Built
// with the address and undefined-behaviour sanitizers by tests/test_batch_rows.py; prints "ok: <n> checks" and exits 0, or
// the failed checks.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "host/batch_rows.h"

using namespace idto::optimizer;
using idto::optimizer::internal::BatchRowsResult;
using idto::optimizer::internal::RowsOutcome;
using idto::optimizer::internal::RowsToStats;
using idto::optimizer::internal::kTrRow;
using idto::optimizer::internal::CalcDoglegScalars;
using idto::optimizer::internal::CalcTrustRatioScalars;
using idto::optimizer::internal::DoglegScalars;
using idto::optimizer::internal::TrustRatioScalars;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

// row k of a made-up solve: every column a distinct value that names (k, column)
static void FillRow(double* R, int k, bool accepted, double clock, int flags = 0, int reason = 0) {
  for (int c = 0; c < kTrRow; ++c) R[c] = 100.0 * (k + 1) + c;
  R[9] = accepted ? 1.0 : 0.0;
  R[10] = clock;
  R[14] = flags;
  R[16] = reason;
}

static std::vector<double> Rows(int n) { return std::vector<double>((std::size_t)n * kTrRow, 0.0); }

static void CheckPushed(const TrajectoryOptimizerStats<double>& s, const std::vector<double>& rows, int k) {
  const double* R = rows.data() + (std::size_t)k * kTrRow;
  CHECK(s.iteration_costs[k] == R[0]);
  CHECK(s.trust_region_radii[k] == R[1]);
  CHECK(s.trust_ratios[k] == R[2]);
  CHECK(s.q_norms[k] == R[3]);
  CHECK(s.dq_norms[k] == R[4]);
  CHECK(s.dqH_norms[k] == R[5]);
  CHECK(s.gradient_norms[k] == R[6]);
  CHECK(s.dL_dqs[k] == R[7]);
  CHECK(s.h_norms[k] == R[8]);
  CHECK(s.merits[k] == R[15]);
  CHECK(s.linesearch_iterations[k] == 0);
  CHECK(std::isnan(s.linesearch_alphas[k]));
}

// ---- the dogleg point restated on vectors (oracle/traj_opt.h CalcDoglegPoint, TO.cc:2108-2202, without scaling): pU, pH,
// the three branches.  Returns which branch was taken (1 Cauchy point on the boundary, 2 Newton point inside, 3 the leg
// between them) and the step in *dq.  w = H^-1 g comes from the caller.
using V = std::vector<double>;
static double DotV(const V& a, const V& b) { double s = 0; for (std::size_t i = 0; i < a.size(); ++i) s += a[i] * b[i]; return s; }
static V MatVec(const V& H, const V& x) {   // row-major n x n
  const std::size_t n = x.size();
  V y(n, 0.0);
  for (std::size_t r = 0; r < n; ++r) for (std::size_t c = 0; c < n; ++c) y[r] += H[r * n + c] * x[c];
  return y;
}
static V SolveSpd(V H, V b) {   // Gaussian elimination without pivoting (H is symmetric positive definite)
  const std::size_t n = b.size();
  for (std::size_t j = 0; j < n; ++j)
    for (std::size_t r = j + 1; r < n; ++r) {
      const double f = H[r * n + j] / H[j * n + j];
      for (std::size_t c = j; c < n; ++c) H[r * n + c] -= f * H[j * n + c];
      b[r] -= f * b[j];
    }
  for (std::size_t j = n; j-- > 0;) {
    for (std::size_t c = j + 1; c < n; ++c) b[j] -= H[j * n + c] * b[c];
    b[j] /= H[j * n + j];
  }
  return b;
}
static int DoglegOnVectors(const V& H, const V& g, const V& w, double Delta, V* dq) {
  const std::size_t n = g.size();
  const double gHg = DotV(g, MatVec(H, g));
  V pH(n), pU(n), d(n);
  for (std::size_t i = 0; i < n; ++i) pH[i] = -w[i] / Delta;                      // :2139-2149
  const double coef = -(DotV(g, g) / gHg);
  for (std::size_t i = 0; i < n; ++i) pU[i] = coef * g[i] / Delta;                // :2157
  dq->resize(n);
  const double pUn = std::sqrt(DotV(pU, pU));
  if (1.0 <= pUn) {                                                               // :2160-2168
    for (std::size_t i = 0; i < n; ++i) (*dq)[i] = (Delta / pUn) * pU[i];
    return 1;
  }
  if (1.0 >= std::sqrt(DotV(pH, pH))) {                                           // :2171-2178
    for (std::size_t i = 0; i < n; ++i) (*dq)[i] = pH[i] * Delta;
    return 2;
  }
  for (std::size_t i = 0; i < n; ++i) d[i] = pH[i] - pU[i];
  const double a = DotV(d, d), b = 2 * DotV(pU, d), c = DotV(pU, pU) - 1.0;       // :2192-2194
  const double sq = (-b + std::sqrt(b * b - 4 * a * c)) / (2 * a);                // the root in (0, 1)
  for (std::size_t i = 0; i < n; ++i) (*dq)[i] = (pU[i] + sq * d[i]) * Delta;     // :2197
  return 3;
}

int main() {
  SolverParameters sp;
  sp.check_convergence = false;

  {   // every row accepted: all of them count, the loop's final radius is kept, max_iterations reached
    const int n = 4;
    sp.max_iterations = n;
    auto rows = Rows(n);
    for (int k = 0; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, true, 1e6 + 2e5 * k);
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(rows.data(), n, 0.7, 0.01, sp, &st, &r);
    CHECK(r.outcome == RowsOutcome::kDone && r.flag == SolverFlag::kMaxIterationsReached);
    CHECK(r.iterations == n && (int)st.iteration_costs.size() == n && (int)st.merits.size() == n);
    CHECK(r.last_accepted && !r.converged && r.Delta == 0.7 && r.error.empty());
    CHECK(st.solve_time == 0.01 && st.convergence_reason == kNoConvergenceCriteriaSatisfied);
    for (int k = 0; k < n; ++k) CheckPushed(st, rows, k);
    // iteration times: the device clock's differences (100 MHz ticks), the first one takes the rest of the wall time
    for (int k = 1; k < n; ++k) CHECK(st.iteration_times[k] == 2e5 * 1e-8);
    CHECK(std::fabs(st.iteration_times[0] - (0.01 - 3 * 2e-3)) < 1e-15);
    // (a wall time shorter than what the device clock saw: the first iteration's time is clamped at 0)
    TrajectoryOptimizerStats<double> st2;
    RowsToStats(rows.data(), n, 0.7, 1e-3, sp, &st2, &r);
    CHECK(st2.iteration_times[0] == 0.0);
  }
  {   // a rejected last row: it counts, and says so
    const int n = 3;
    sp.max_iterations = n;
    auto rows = Rows(n);
    for (int k = 0; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, k != n - 1, 1e6 + 1e5 * k);
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(rows.data(), n, 0.025, 0.5, sp, &st, &r);
    CHECK(r.outcome == RowsOutcome::kDone && r.flag == SolverFlag::kMaxIterationsReached);
    CHECK(r.iterations == n && !r.last_accepted && r.Delta == 0.025);
    CheckPushed(st, rows, n - 1);
    // a rejected row's reason column is not looked at, criteria on or off
    sp.check_convergence = true;
    rows[(std::size_t)(n - 1) * kTrRow + 16] = 2;
    TrajectoryOptimizerStats<double> st2;
    RowsToStats(rows.data(), n, 0.025, 0.5, sp, &st2, &r);
    CHECK(!r.converged && r.flag == SolverFlag::kMaxIterationsReached && st2.convergence_reason == kNoConvergenceCriteriaSatisfied);
    sp.check_convergence = false;
  }
  {   // a converged row followed by idle rows (zeros: the loop left early): they do not count
    const int n = 8;
    sp.max_iterations = n;
    sp.check_convergence = true;
    auto rows = Rows(n);
    FillRow(&rows[0], 0, true, 1e6);
    FillRow(&rows[kTrRow], 1, false, 1.1e6);
    FillRow(&rows[2 * kTrRow], 2, true, 1.2e6, 0, kCostReductionCriterionSatisfied | kSateCriterionSatisfied);
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(rows.data(), n, 9.0, 0.2, sp, &st, &r);
    CHECK(r.outcome == RowsOutcome::kDone && r.flag == SolverFlag::kSuccess && r.converged && r.last_accepted);
    CHECK(r.iterations == 3 && (int)st.iteration_costs.size() == 3);
    CHECK(r.Delta == rows[2 * kTrRow + 1]);   // (the converged row's own radius: the reference leaves before the update)
    CHECK(st.convergence_reason == (kCostReductionCriterionSatisfied | kSateCriterionSatisfied));
    // ... and idle rows that DID run behind it (flag 16, a clock value) do not count either
    for (int k = 3; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, false, 1.2e6 + 1e5 * k, 16);
    TrajectoryOptimizerStats<double> st2;
    RowsToStats(rows.data(), n, 9.0, 0.2, sp, &st2, &r);
    CHECK(r.flag == SolverFlag::kSuccess && r.converged && r.iterations == 3 && (int)st2.merits.size() == 3);
    // with the criteria off the reason column is ignored
    sp.check_convergence = false;
    TrajectoryOptimizerStats<double> st3;
    RowsToStats(rows.data(), n, 9.0, 0.2, sp, &st3, &r);
    CHECK(!r.converged && r.iterations == n && r.flag == SolverFlag::kMaxIterationsReached && r.Delta == 9.0);
    // criteria on, none met in any row: every row counts
    sp.check_convergence = true;
    for (int k = 0; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, true, 1e6 + 1e5 * k);
    TrajectoryOptimizerStats<double> st4;
    RowsToStats(rows.data(), n, 9.0, 0.2, sp, &st4, &r);
    CHECK(!r.converged && r.iterations == n && r.flag == SolverFlag::kMaxIterationsReached && r.Delta == 9.0);
    sp.check_convergence = false;
  }
  // each flag, in row 2 of 5: the two rows in front of it are taken, the flagged one is not
  struct FlagCase { int flags; RowsOutcome outcome; SolverFlag flag; const char* text; };
  const FlagCase flag_cases[] = {
      {1, RowsOutcome::kFailed, SolverFlag::kFactorizationFailed, "not finite"},
      {2, RowsOutcome::kFailed, SolverFlag::kFactorizationFailed, "not finite"},
      {4, RowsOutcome::kError, SolverFlag::kSuccess, "not a descent direction"},
      {8, RowsOutcome::kNeedsHostLoop, SolverFlag::kSuccess, ""},
      {32, RowsOutcome::kFailed, SolverFlag::kFactorizationFailed, "factorisation failed in iteration 2"},
      {32 | 2, RowsOutcome::kFailed, SolverFlag::kFactorizationFailed, "factorisation failed in iteration 2"},
      {8 | 32, RowsOutcome::kNeedsHostLoop, SolverFlag::kSuccess, ""},   // (a vanished multiplier pivot spoils H's pivots behind it)
  };
  for (const FlagCase& fc : flag_cases) {
    const int n = 5;
    sp.max_iterations = n;
    auto rows = Rows(n);
    for (int k = 0; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, true, 1e6 + 1e5 * k, k >= 2 ? fc.flags : 0);
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(rows.data(), n, 3.0, 0.1, sp, &st, &r);
    CHECK(r.outcome == fc.outcome);
    CHECK(r.iterations == 2 && (int)st.iteration_costs.size() == 2);
    if (fc.outcome == RowsOutcome::kFailed) CHECK(r.flag == fc.flag);
    CHECK(r.error.find(fc.text) != std::string::npos);
    CHECK((fc.outcome == RowsOutcome::kNeedsHostLoop) == r.error.empty());
    if (fc.outcome == RowsOutcome::kNeedsHostLoop) CHECK(r.Delta == rows[2 * kTrRow + 1]);
  }
  {   // flag 16 alone (a criterion held earlier: an idle row) is no failure
    const int n = 2;
    sp.max_iterations = n;
    auto rows = Rows(n);
    FillRow(&rows[0], 0, true, 1e6);
    FillRow(&rows[kTrRow], 1, false, 1.1e6, 16);
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(rows.data(), n, 3.0, 0.1, sp, &st, &r);
    CHECK(r.outcome == RowsOutcome::kDone && r.iterations == 2);
  }
  {   // zero iterations: nothing is read, nothing pushed
    sp.max_iterations = 0;
    TrajectoryOptimizerStats<double> st;
    BatchRowsResult r;
    RowsToStats(nullptr, 0, 0.1, 0.3, sp, &st, &r);
    CHECK(r.outcome == RowsOutcome::kDone && r.iterations == 0 && st.is_empty() && r.Delta == 0.1);
    CHECK(r.flag == SolverFlag::kMaxIterationsReached && st.solve_time == 0.3);   // (k == max_iterations == 0, as Solve reports it)
  }
  {   // (a) was a convergence reason reported at all (the single problem writes its caller's *reason only then) ...
    const int n = 3;
    sp.max_iterations = n;
    auto rows = Rows(n);
    for (int k = 0; k < n; ++k) FillRow(&rows[(std::size_t)k * kTrRow], k, true, 1e6 + 1e5 * k);
    TrajectoryOptimizerStats<double> st, st2, st3;
    BatchRowsResult r;
    sp.check_convergence = false;   // criteria off, accepted rows: none
    RowsToStats(rows.data(), n, 1.0, 0.1, sp, &st, &r);
    CHECK(!r.reason_reported && r.iterations == n);
    // ... and the cost of the iterate behind the last row taken: an accepted row's trial cost (column 13)
    CHECK(r.last_accepted && r.iterate_cost == rows[(std::size_t)(n - 1) * kTrRow + 13]);
    sp.check_convergence = true;    // criteria on, an accepted row (whose reason is "none satisfied"): reported
    RowsToStats(rows.data(), n, 1.0, 0.1, sp, &st2, &r);
    CHECK(r.reason_reported && !r.converged && st2.convergence_reason == kNoConvergenceCriteriaSatisfied);
    for (int k = 0; k < n; ++k) rows[(std::size_t)k * kTrRow + 9] = 0.0;   // criteria on, only rejected rows: none
    RowsToStats(rows.data(), n, 1.0, 0.1, sp, &st3, &r);
    CHECK(!r.reason_reported && r.iterations == n);
    // a rejected last row: the iterate is still q_k, its cost the row's own (column 0)
    CHECK(!r.last_accepted && r.iterate_cost == rows[(std::size_t)(n - 1) * kTrRow + 0]);
    CHECK(rows[(std::size_t)(n - 1) * kTrRow + 0] != rows[(std::size_t)(n - 1) * kTrRow + 13]);
    sp.check_convergence = false;
  }
  {   // (b) the dogleg scalars: dqs = a g + b w against the restatement on vectors, n = 6, random SPD H, three radii so
      // that every branch is taken.  The two sides sum in different orders (nine inner products and scalar algebra here,
      // vector operations there), so they agree to round-off: the largest relative difference max|dqs - dq| / max|dq| over
      // these 60 cases measured 3.15e-16 (x86-64, g++ -O1; printed to stderr); the bound is a decade above that, 3.2e-15.
    const std::size_t n = 6;
    unsigned long long seed = 12345;
    auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    double worst = 0.0;
    int taken[4] = {0, 0, 0, 0};
    for (int trial = 0; trial < 20; ++trial) {
      V A(n * n), H(n * n, 0.0), g(n);
      for (double& x : A) x = rnd();
      for (double& x : g) x = rnd();
      for (std::size_t r = 0; r < n; ++r)
        for (std::size_t c = 0; c < n; ++c) {
          for (std::size_t k = 0; k < n; ++k) H[r * n + c] += A[r * n + k] * A[c * n + k];
          if (r == c) H[r * n + c] += 0.5;
        }
      const V w = SolveSpd(H, g), Hg = MatVec(H, g), Hw = MatVec(H, w);
      const double S[9] = {DotV(g, g), DotV(g, Hg), DotV(w, w), DotV(g, w), DotV(g, Hw), DotV(w, Hw), 0.0, 0.0, 0.0};
      const double lenU = S[0] / S[1] * std::sqrt(S[0]), lenH = std::sqrt(S[2]);   // the Cauchy and the Newton step's lengths
      CHECK(lenU < lenH);
      const double radii[3] = {0.5 * lenU, 0.5 * (lenU + lenH), 2.0 * lenH};
      for (int which = 0; which < 3; ++which) {
        V dq;
        const int branch = DoglegOnVectors(H, g, w, radii[which], &dq);
        const DoglegScalars d = CalcDoglegScalars(S, radii[which]);
        CHECK(branch == (which == 0 ? 1 : which == 1 ? 3 : 2));
        ++taken[branch];
        CHECK(d.finite && d.active == (branch != 2));
        if (branch == 1) CHECK(d.b == 0.0 && d.a < 0.0);
        if (branch == 2) CHECK(d.a == 0.0 && d.b == -1.0);
        if (branch == 3) CHECK(d.a < 0.0 && -1.0 < d.b && d.b < 0.0);
        double diff = 0.0, scale = 0.0;
        for (std::size_t i = 0; i < n; ++i) {
          diff = std::max(diff, std::fabs(d.a * g[i] + d.b * w[i] - dq[i]));
          scale = std::max(scale, std::fabs(dq[i]));
        }
        worst = std::max(worst, diff / scale);
      }
    }
    CHECK(taken[1] == 20 && taken[2] == 20 && taken[3] == 20);
    std::fprintf(stderr, "dogleg scalars against vectors: largest relative difference %.3g\n", worst);
    CHECK(worst <= 3.2e-15);
    // g~.H~g~ = 0: the Cauchy point is not a number - reported, not returned as a step
    const double S0[9] = {1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0};
    CHECK(!CalcDoglegScalars(S0, 1.0).finite);
  }
  {   // (c) the trust ratio (TO.cc:2004-2034) and the descent test (:2517-2531)
    const double eps = std::numeric_limits<double>::epsilon();
    // hand-computed: gradient_term = a gg + b gw = -0.5 * 4 - 1 * 2 = -4, hessian_term = 0.5 (0.25 * 8 + 2 * 0.5 * 1 + 3) = 3,
    // predicted = 4 - 3 = 1, actual = 10 - 9.25 = 0.75 (every figure exact in binary)
    const double S[9] = {4.0, 8.0, 7.0, 2.0, 1.0, 3.0, 0.0, 0.0, 0.0};
    TrustRatioScalars t = CalcTrustRatioScalars(S, -0.5, -1.0, -4.0, 10.0, 9.25, 0.1);
    CHECK(t.predicted == 1.0 && t.actual == 0.75 && t.rho == 0.75 && t.dL_dq == -0.4 && t.descent);
    t = CalcTrustRatioScalars(S, -0.5, -1.0, -4.0, 10.0, 10.5, 0.1);   // the cost went up: a negative ratio
    CHECK(t.actual == -0.5 && t.rho == -0.5);
    // the eps rule (10 epsilon / dt^2 = 2.2e-15 at dt = 1): both terms below it -> 0.5, whatever their quotient
    const double S1[9] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    t = CalcTrustRatioScalars(S1, -1e-15, 0.0, -1e-15, 1.0, 1.0 - eps / 2, 1.0);
    CHECK(t.predicted == 1e-15 && t.actual == eps / 2 && t.rho == 0.5);
    t = CalcTrustRatioScalars(S1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0);   // (0 / 0 otherwise)
    CHECK(t.rho == 0.5);
    t = CalcTrustRatioScalars(S1, -1e-15, 0.0, -1e-15, 1.0, 0.5, 1.0);   // only the prediction is below it: the quotient
    CHECK(t.rho == 0.5 / 1e-15);
    t = CalcTrustRatioScalars(S1, -1.0, 0.0, -1.0, 1.0, 1.0, 1.0);       // only the reduction is below it
    CHECK(t.predicted == 1.0 && t.rho == 0.0);
    // the descent test's boundary: dL_dq < epsilon() passes, dL_dq == epsilon() does not
    CHECK(!CalcTrustRatioScalars(S1, 0.0, 0.0, eps, 1.0, 1.0, 1.0).descent);
    CHECK(CalcTrustRatioScalars(S1, 0.0, 0.0, eps, 1.0, 1.0, 1.0).dL_dq == eps);
    CHECK(CalcTrustRatioScalars(S1, 0.0, 0.0, std::nextafter(eps, 0.0), 1.0, 1.0, 1.0).descent);
    CHECK(!CalcTrustRatioScalars(S1, 0.0, 0.0, std::numeric_limits<double>::quiet_NaN(), 1.0, 1.0, 1.0).descent);
  }
  if (g_failed) { std::printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
  std::printf("ok: %d checks\n", g_checks);
  return 0;
}
