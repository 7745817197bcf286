// batch_rows_check.cc — stand-alone check of host/batch_rows.cc (one problem's statistics rows of the device loop ->
// TrajectoryOptimizerStats, convergence reason, radius, SolverFlag) on hand-written rows.  Built with the address and
// undefined-behaviour sanitizers by tests/test_batch_rows.py; prints "ok: <n> checks" and exits 0, or the failed checks.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "host/batch_rows.h"

using namespace idto::optimizer;
using idto::optimizer::internal::BatchRowsResult;
using idto::optimizer::internal::RowsOutcome;
using idto::optimizer::internal::RowsToStats;
using idto::optimizer::internal::kTrRow;

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
  if (g_failed) { std::printf("%d of %d checks failed\n", g_failed, g_checks); return 1; }
  std::printf("ok: %d checks\n", g_checks);
  return 0;
}
