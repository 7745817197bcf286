// batch_rows.cc — see batch_rows.h.
#include "host/batch_rows.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <stdexcept>

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
    out->iterate_cost = out->last_accepted ? R[13] : R[0];   // (NOT IDTO_ARR_COST, which a rejected trial point overwrites too)
    if (params.check_convergence && out->last_accepted) {   // TO.cc:2600-2612
      const ConvergenceReason reason = static_cast<ConvergenceReason>((int)R[16]);
      stats->convergence_reason = reason;
      out->reason_reported = true;
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

double SolveDoglegQuadratic(double a, double b, double c) {
  if (!(a > 0)) throw std::runtime_error("dogleg: a <= 0");
  double s;
  if (a < std::numeric_limits<double>::epsilon()) {
    s = -c / b;
  } else {
    const double bt = b / a, ct = c / a;
    const double det = bt * bt - 4 * ct;
    if (!(det > 0)) throw std::runtime_error("dogleg: determinant <= 0");
    s = (-bt + std::sqrt(det)) / 2;
  }
  if (!(0 < s && s < 1)) throw std::runtime_error("dogleg: s not in (0,1)");
  return s;
}

DoglegScalars CalcDoglegScalars(const double* S, double Delta) {
  const double gg = S[0], gHg = S[1], ww = S[2], gw = S[3];
  // CalcDoglegPoint, normalised by Delta: pU = cU g~ (:2157), pH = -w / Delta (:2139-2149)
  const double cU = -(gg / gHg) / Delta;
  const double pUn = std::fabs(cU) * std::sqrt(gg), pHn = std::sqrt(ww) / Delta;
  double a, b;
  bool active;
  if (1.0 <= pUn) {          // :2160-2168
    a = (Delta / pUn) * cU; b = 0.0; active = true;
  } else if (1.0 >= pHn) {   // :2171-2178
    a = 0.0; b = -1.0; active = false;
  } else {                   // :2180-2199
    const double pUpU = cU * cU * gg, pHpH = ww / (Delta * Delta), pUpH = -cU * gw / Delta;
    const double sq = SolveDoglegQuadratic(pHpH - 2 * pUpH + pUpU, 2 * (pUpH - pUpU), pUpU - 1.0);
    a = Delta * (1.0 - sq) * cU; b = -sq; active = true;
  }
  return {a, b, active, std::isfinite(a) && std::isfinite(b)};
}

TrustRatioScalars CalcTrustRatioScalars(const double* S, double a, double b, double gdqs, double cost, double cost_trial,
                                        double time_step) {
  const double gg = S[0], gHg = S[1], gw = S[3], gHw = S[4], wHw = S[5];
  const double dL_dq = gdqs / cost;   // :2517-2524
  // CalcTrustRatio (:2004-2034)
  const double gradient_term = a * gg + b * gw;
  const double hessian_term = 0.5 * (a * a * gHg + 2 * a * b * gHw + b * b * wHw);
  const double predicted = -gradient_term - hessian_term, actual = cost - cost_trial;
  const double eps = 10 * std::numeric_limits<double>::epsilon() / time_step / time_step;
  const double rho = (predicted < eps && actual < eps) ? 0.5 : actual / predicted;
  return {dL_dq, predicted, actual, rho, dL_dq < std::numeric_limits<double>::epsilon()};
}

}  // namespace internal
}  // namespace optimizer
}  // namespace idto
