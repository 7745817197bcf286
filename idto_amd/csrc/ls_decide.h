// ls_decide.h — the decisions of the two linesearches (reference optimizer/trajectory_optimizer.cc:1852-1929
// backtracking, :1931-1977 Armijo) as pure functions of numbers: the step lengths, the early-outs and the throw
// condition, and a scan over the candidates' costs in index order.  Plain C++, no HIP type: the host includes it as it
// is, hipcc compiles the same text for the device (`__host__ __device__`), so that a loop on either side takes the same
// decision from the same costs.  Every comparison is written as the host loop writes it (host/trajectory_optimizer.cc
// ArmijoLinesearch / BacktrackingLinesearch): a NaN cost makes `L_new > bound` false and is accepted at once, as the
// reference accepts it - do not negate or reorder them.
#pragma once

#if defined(__HIPCC__)
#define IDTO_LS_HD __host__ __device__
#else
#define IDTO_LS_HD
#endif

namespace idto_ls {

constexpr int kArmijo = 0, kBacktracking = 1;   // SolverParameters::linesearch_method
constexpr int kMaxCandidates = 64;             // = IDTO_LS_MAX_CANDIDATES (idto_hip.h)
constexpr double kC = 1e-4, kRho = 0.8;        // the sufficient-decrease constant and the contraction (:1863-1864, :1939-1940)
constexpr double kEps = 2.220446049250313e-16;       // std::numeric_limits<double>::epsilon()
constexpr double kSqrtEps = 1.4901161193847656e-08;  // its square root, 2^-26 exactly (the backtracking early-out)

// Candidate j's step length, formed as the host forms it: by repeated IEEE multiplication, never by pow.
//   Armijo:       alpha = 1.0 / rho; alpha *= rho per candidate      (1/0.8 * 0.8 == 1.0, then 0.8, 0.6400000000000001, ...)
//   backtracking: alpha = 1.0 is candidate 0; alpha *= rho per further candidate
IDTO_LS_HD inline void ls_alpha_chain(int method, int m, double* alphas) {
  double alpha = (method == kArmijo) ? 1.0 / kRho : 1.0;
  for (int j = 0; j < m; ++j) {
    if (method == kArmijo || j > 0) alpha *= kRho;
    alphas[j] = alpha;
  }
}

enum LsStatus {
  LS_UNDECIDED = 0,    // feed the next candidate's cost
  LS_DECIDED = 1,      // alpha / ls_iters hold the linesearch's answer
  LS_EXHAUSTED = 2,    // Armijo: max_linesearch_iterations candidates without sufficient decrease; alpha is the last
                       // candidate's and ls_iters the limit - the step is still taken, as the host takes it
  LS_NOT_DESCENT = 3,  // !(L' <= 0): where the host throws "linesearch: not a descent direction"
};

struct LsScan {
  int method, max_iters;
  double L, L_prime;
  int status;
  int next;         // index of the candidate whose cost comes next
  double cur;       // the step length of candidate next - 1 (Armijo: 1 / rho before the first)
  int armijo_met;   // backtracking: a candidate has met the sufficient-decrease condition
  double L_old;     // backtracking: the cost of candidate next - 1
  double alpha;     // the answer (LS_DECIDED, LS_EXHAUSTED)
  int ls_iters;
};

// The part in front of the first candidate: the throw condition (a status, so that a device loop can carry it as a
// sticky flag and the host raise the error afterwards) and the early-outs - Armijo |L'| / |L| <= 10 eps / dt^2,
// backtracking <= sqrt(eps) -, which answer {1.0, 0}: the full step is taken, and its cost is still wanted.
IDTO_LS_HD inline LsScan ls_begin(int method, double L, double L_prime, double dt, int max_iters) {
  LsScan s;
  s.method = method; s.max_iters = max_iters; s.L = L; s.L_prime = L_prime;
  s.status = LS_UNDECIDED; s.next = 0; s.cur = (method == kArmijo) ? 1.0 / kRho : 1.0;
  s.armijo_met = 0; s.L_old = 0.0; s.alpha = 1.0; s.ls_iters = 0;
  if (!(L_prime <= 0)) { s.status = LS_NOT_DESCENT; return s; }
  const double ratio = __builtin_fabs(L_prime) / __builtin_fabs(L);
  if (method == kArmijo) {
    const double thr = 10 * kEps / dt / dt;
    if (ratio <= thr) s.status = LS_DECIDED;
  } else if (ratio <= kSqrtEps) {
    s.status = LS_DECIDED;
  }
  return s;
}

// One more candidate's cost, in index order.  Returns the status; a scan that has an answer ignores further costs, so
// the outcome cannot depend on how many candidates were evaluated beyond the deciding one, nor on how they were grouped.
IDTO_LS_HD inline int ls_feed(LsScan* s, double L_new) {
  if (s->status != LS_UNDECIDED) return s->status;
  const int j = s->next++;
  if (s->method == kArmijo) {
    // do { alpha *= rho; L_new = cost; ++i; } while ((L_new > L + c * alpha * L_prime) && (i < max));
    s->cur *= kRho;
    const double alpha = s->cur;
    const int i = j + 1;
    if ((L_new > s->L + kC * alpha * s->L_prime) && (i < s->max_iters)) return LS_UNDECIDED;
    s->alpha = alpha; s->ls_iters = i;
    s->status = (L_new > s->L + kC * alpha * s->L_prime) ? LS_EXHAUSTED : LS_DECIDED;
    return s->status;
  }
  // L_old = L_new = cost(1.0); i = 0;
  // while (!(armijo_met && (L_new > L_old))) { L_old = L_new; alpha *= rho; L_new = cost(alpha);
  //                                            if (L_new <= L + c * alpha * L_prime) armijo_met = true; ++i; }
  // return {alpha / rho, i};            (not bounded by max_linesearch_iterations)
  if (j == 0) { s->L_old = L_new; return LS_UNDECIDED; }
  s->cur *= kRho;
  const double alpha = s->cur;
  if (L_new <= s->L + kC * alpha * s->L_prime) s->armijo_met = 1;
  if (s->armijo_met && (L_new > s->L_old)) {
    s->alpha = alpha / kRho; s->ls_iters = j;
    s->status = LS_DECIDED;
    return s->status;
  }
  s->L_old = L_new;
  return LS_UNDECIDED;
}

// The costs of candidates [s->next, s->next + m), in index order.
IDTO_LS_HD inline int ls_scan(LsScan* s, const double* costs, int m) {
  for (int j = 0; j < m && s->status == LS_UNDECIDED; ++j) ls_feed(s, costs[j]);
  return s->status;
}

// SolveWithLinesearch's `linesearch_failed` (:2316-2323): for either method, whatever the scan's status.
IDTO_LS_HD inline bool ls_limit_reached(int ls_iters, int max_iters) { return ls_iters >= max_iters; }

}  // namespace idto_ls
