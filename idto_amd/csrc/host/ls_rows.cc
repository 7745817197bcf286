// ls_rows.cc — see ls_rows.h.
#include "host/ls_rows.h"

#include <algorithm>
#include <limits>

namespace idto {
namespace optimizer {
namespace internal {

void LsRowsToStats(const double* rows, int iterations, double total_time, LinesearchMethod method,
                   TrajectoryOptimizerStats<double>* stats, LsRowsResult* out) {
  *out = LsRowsResult{};
  int ran = iterations;
  while (ran > 0 && rows[(std::size_t)(ran - 1) * kLsRow + 10] == 0.0 && rows[(std::size_t)(ran - 1) * kLsRow + 11] == 0.0) --ran;
  double timed = 0.0;
  for (int i = 1; i < ran; ++i) timed += (rows[(std::size_t)i * kLsRow + 10] - rows[(std::size_t)(i - 1) * kLsRow + 10]) * 1e-8;
  bool limit = false;
  for (int k = 0; k < ran; ++k) {
    const double* R = rows + (std::size_t)k * kLsRow;
    const int flags = (int)R[11];
    if (flags & 128) { out->outcome = LsRowsOutcome::kNeedsHostLoop; break; }
    if (flags & 32) {
      out->outcome = LsRowsOutcome::kFailed;
      out->flag = SolverFlag::kFactorizationFailed;
      out->error = "idto_hip: factorisation failed in iteration " + std::to_string(k);
      break;
    }
    if (flags & (2 | 4)) {
      out->outcome = LsRowsOutcome::kError;
      out->error = method == LinesearchMethod::kArmijo ? "linesearch: not a descent direction (TO.cc:1951)"
                                                       : "linesearch: not a descent direction (TO.cc:1888)";
      break;
    }
    const double iter_time = (k == 0) ? std::max(0.0, total_time - timed) : (R[10] - R[10 - kLsRow]) * 1e-8;
    const double cost = R[0];
    stats->push_data(iter_time, cost, (int)R[2], R[1], std::numeric_limits<double>::quiet_NaN(), R[4], R[5], R[5], R[3], R[6],
                     R[7] / cost, R[8], cost);   // :2373-2385
    ++out->iterations;
    if (flags & 64) limit = true;
  }
  stats->solve_time = total_time;
  if (out->outcome == LsRowsOutcome::kDone) out->flag = limit ? SolverFlag::kLinesearchMaxIters : SolverFlag::kSuccess;
}

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
