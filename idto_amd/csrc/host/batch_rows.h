// batch_rows.h — one problem's statistics rows of the device-resident trust-region loop (include/idto_hip.h
// idto_hip_tr_solve: rows[iterations][IDTO_TR_ROW]) turned into what TrajectoryOptimizer hands its caller: the
// TrajectoryOptimizerStats sequence, the convergence reason, the radius to keep and a SolverFlag.  This is the translation
// TrajectoryOptimizer::SolveOnDevice makes for its one problem (host/trajectory_optimizer.cc), as a pure function so that
// SolveBatch can make it per problem of a batch: where SolveOnDevice throws, this reports - one problem's failure is its
// own.  Host-only (no HIP include): tests/cpp/batch_rows_check.cc runs it on the CPU under the sanitizers.
#pragma once

#include <string>

#include "idto/optimizer/solver_parameters.h"
#include "idto/optimizer/trajectory_optimizer_solution.h"

namespace idto {
namespace optimizer {
namespace internal {

constexpr int kTrRow = 17;   // IDTO_TR_ROW (static_assert in batch_rows.cc's users that include idto_hip.h)

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
  double Delta = 0.0;           // the radius to keep (a converged row's own; the flagged row's for kNeedsHostLoop; else Delta_end)
  SolverFlag flag = SolverFlag::kSuccess;
  std::string error;
};

// rows: [iterations][kTrRow], iterations = SolverParameters::max_iterations of the loop that wrote them; rows behind the
// last one that ran (column 10, the device clock, is 0: the loop left early after a converged row) do not count.
// Delta_end: the radius the loop ended with.  total_time: wall time of the whole call in seconds (the first iteration's
// time is what the device clock does not account for).  `stats` must be empty; solve_time is set to total_time.
void RowsToStats(const double* rows, int iterations, double Delta_end, double total_time, const SolverParameters& params,
                 TrajectoryOptimizerStats<double>* stats, BatchRowsResult* out);

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
