// ls_rows.h — the statistics rows of the device-resident linesearch loop (include/idto_hip.h idto_hip_ls_solve:
// rows[iterations][IDTO_LS_ROW]) turned into what TrajectoryOptimizer hands its caller: the TrajectoryOptimizerStats
// sequence with the host loop's push_data arguments (SolveWithLinesearch, TO.cc:2373-2385: NaN radii, dqH = dq, merit =
// cost), the SolverFlag, and the errors the host loop raises.  Host-only (no HIP include): tests/cpp/ls_decide_check.cc runs
// it on the CPU under the sanitizers.
#pragma once

#include <string>

#include "host/batch_rows.h"
#include "idto/optimizer/solver_parameters.h"
#include "idto/optimizer/trajectory_optimizer_solution.h"

namespace idto {
namespace optimizer {
namespace internal {

constexpr int kLsRow = 12;   // IDTO_LS_ROW (static_assert where idto_hip.h is included as well)

// One enum for both loops' rows (SolveBatch takes an entry of either loop the same way).  Here:
//   kDone            `flag` is kSuccess or kLinesearchMaxIters
//   kNeedsHostLoop   flag 128: backtracking undecided within the device's candidates - the host loop runs the solve
//   kFailed          flag 32: the factorisation failed (`flag` is kFactorizationFailed, `error` says where)
//   kError           flag 4 (2): not a descent direction - `error` is the host loop's text
using LsRowsOutcome = RowsOutcome;

struct LsRowsResult {
  LsRowsOutcome outcome = LsRowsOutcome::kDone;
  int iterations = 0;   // rows taken into the statistics
  SolverFlag flag = SolverFlag::kSuccess;
  std::string error;
};

// rows: [iterations][kLsRow]; rows behind the last one that ran (clock and flags 0) do not count.  total_time: wall time of
// the whole call in seconds (the first iteration's time is what the device clock does not account for).  `stats` must be
// empty; solve_time is set to total_time.
void LsRowsToStats(const double* rows, int iterations, double total_time, LinesearchMethod method,
                   TrajectoryOptimizerStats<double>* stats, LsRowsResult* out);

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
