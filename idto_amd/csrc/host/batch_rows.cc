// batch_rows.cc — see batch_rows.h.  The order of the checks and the arithmetic of the iteration times are those of
// TrajectoryOptimizer::SolveOnDevice's resident-loop branch (host/trajectory_optimizer.cc).
#include "host/batch_rows.h"

#include <algorithm>
#include <cstddef>
#include <limits>

namespace idto {
namespace optimizer {
namespace internal {

void RowsToStats(const double* rows, int iterations, double Delta_end, double total_time, const SolverParameters& params,
                 TrajectoryOptimizerStats<double>* stats, BatchRowsResult* out) {
  *out = BatchRowsResult{};
  out->Delta = Delta_end;
  stats->solve_time = total_time;
  // (with the convergence criteria on, the rows behind the one that met them are zeros)
  int ran = std::max(iterations, 0);
  while (ran > 1 && rows[(std::size_t)(ran - 1) * kTrRow + 10] == 0.0) --ran;
  double timed = 0.0;
  for (int i = 1; i < ran; ++i) timed += (rows[(std::size_t)i * kTrRow + 10] - rows[(std::size_t)(i - 1) * kTrRow + 10]) * 1e-8;
  int k = 0;
  for (; k < ran; ++k) {
    const double* R = rows + (std::size_t)k * kTrRow;
    const int flags = (int)R[14];
    out->iterations = k;
    if (flags & 8) {
      out->outcome = RowsOutcome::kNeedsHostLoop;
      out->Delta = R[1];
      return;
    }
    if (flags & 32) {
      out->outcome = RowsOutcome::kFailed;
      out->flag = SolverFlag::kFactorizationFailed;
      out->error = "idto_hip: factorisation failed in iteration " + std::to_string(k);
      return;
    }
    if (flags & 3) {
      out->outcome = RowsOutcome::kFailed;
      out->flag = SolverFlag::kFactorizationFailed;
      out->error = "idto_hip: the dogleg step is not finite";
      return;
    }
    if (flags & 4) {
      out->outcome = RowsOutcome::kError;
      out->error = "step is not a descent direction (TO.cc:2531)";
      return;
    }
    const double iter_time = (k == 0) ? std::max(0.0, total_time - timed) : (R[10] - R[10 - kTrRow]) * 1e-8;
    stats->push_data(iter_time, R[0], 0, std::numeric_limits<double>::quiet_NaN(), R[1], R[3], R[4], R[5], R[2], R[6], R[7],
                     R[8], R[15]);   // TO.cc:2586-2598
    out->iterations = k + 1;
    out->last_accepted = R[9] != 0.0;
    if (params.check_convergence && out->last_accepted) {   // TO.cc:2600-2612
      const ConvergenceReason reason = static_cast<ConvergenceReason>((int)R[16]);
      stats->convergence_reason = reason;
      if (reason != kNoConvergenceCriteriaSatisfied) {   // (the reference leaves the loop before the radius update)
        out->converged = true;
        out->Delta = R[1];
        break;
      }
    }
  }
  // (a converged solve left the loop in front of its ++k: k counts the iterations completed in the reference's sense)
  out->flag = (k == params.max_iterations) ? SolverFlag::kMaxIterationsReached : SolverFlag::kSuccess;
}

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
