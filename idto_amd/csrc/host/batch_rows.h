// batch_rows.h — one problem's statistics rows of the device-resident trust-region loop (include/idto_hip.h
// idto_hip_tr_solve: rows[iterations][IDTO_TR_ROW]) turned into what TrajectoryOptimizer hands its caller: the
// TrajectoryOptimizerStats sequence, the convergence reason, the radius to keep and a SolverFlag.  The one translation
// there is: SolveOnDevice makes it for its one problem and throws where this reports, SolveBatch and the MPC batch make it
// per problem - one problem's failure is its own.  Beside it the scalars of the stepwise loop's iteration (dogleg step,
// trust ratio), which the device's tr_conv_dogleg forms with the same expressions.  Host-only (no HIP include):
// tests/cpp/batch_rows_check.cc runs all of it on the CPU under the sanitizers.
#pragma once

#include <string>

#include "idto/optimizer/solver_parameters.h"
#include "idto/optimizer/trajectory_optimizer_solution.h"

namespace idto {
namespace optimizer {
namespace internal {

constexpr int kTrRow = 17;   // IDTO_TR_ROW (static_assert in batch_rows.cc's users that include idto_hip.h)

// (the linesearch loop's rows end the same four ways: ls_rows.h says what each means there)
enum class RowsOutcome {
  kDone,            // `flag` is kSuccess or kMaxIterationsReached
  kNeedsHostLoop,   // row `iterations` carries flag 8 (singular constraint Schur complement): the host loop takes over there
  kFailed,          // flag 32, or 1 | 2: `flag` is kFactorizationFailed, `error` says which
  kError            // flag 4 (the step is not a descent direction, where the reference throws): `error` is set
};

struct BatchRowsResult {
  RowsOutcome outcome = RowsOutcome::kDone;
  int iterations = 0;           // rows taken into the statistics (for kNeedsHostLoop / kFailed / kError: the rows in front of the flagged one)
  bool converged = false;       // a convergence criterion held in the last row taken
  bool last_accepted = true;    // the last row taken was an accepted step
  bool reason_reported = false; // a row taken set stats->convergence_reason (check_convergence and an accepted step)
  double iterate_cost = 0.0;    // the cost of the iterate behind the last row taken: L(q_k + dq) if accepted, else L(q_k)
  double Delta = 0.0;           // the radius to keep (a converged row's own; the flagged row's for kNeedsHostLoop; else Delta_end)
  SolverFlag flag = SolverFlag::kSuccess;
  std::string error;
};

// rows: [iterations][kTrRow], iterations = SolverParameters::max_iterations of the loop that wrote them; rows behind the
// last one that ran (column 10, the device clock, is 0: the loop left early after a converged row) do not count.
// Delta_end: the radius the loop ended with.  total_time: wall time of the whole call in seconds (the first iteration's
// time is what the device clock does not account for).  Appends to `stats`; solve_time is set to total_time.
void RowsToStats(const double* rows, int iterations, double Delta_end, double total_time, const SolverParameters& params,
                 TrajectoryOptimizerStats<double>* stats, BatchRowsResult* out);

// TO.cc:2037-2066; throws std::runtime_error where the reference aborts
double SolveDoglegQuadratic(double a, double b, double c);

// CalcDoglegPoint (TO.cc:2108-2202) on the nine inner products S of idto_hip_tr_prepare (g~.g~, g~.H~g~, w.w, g~.w,
// g~.H~w, w.H~w, q.q, h.h, h.lambda): the step is dqs = a g~ + b w.  finite = false (H~ not positive definite along g~, say):
// a and b are not numbers to step with.
struct DoglegScalars { double a, b; bool active, finite; };
DoglegScalars CalcDoglegScalars(const double* S, double Delta);

// CalcTrustRatio (TO.cc:2004-2034) and the descent test (:2517-2531) for that step: gdqs = g~.dqs as the device summed it,
// cost / cost_trial = L(q_k) / L(q_k + dq).  descent = false is the reference's "not a descent direction" error.
struct TrustRatioScalars { double dL_dq, predicted, actual, rho; bool descent; };
TrustRatioScalars CalcTrustRatioScalars(const double* S, double a, double b, double gdqs, double cost, double cost_trial,
                                        double time_step);

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
