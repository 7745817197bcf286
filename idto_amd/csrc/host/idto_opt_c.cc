// idto_opt_c.cc — extern "C" wrapper of idto::optimizer::TrajectoryOptimizer<double>
// (include/idto_opt.h).  Converts flat arrays <-> the C++ containers and exceptions -> codes.
#include "idto_opt.h"

#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>

#include "idto/examples/mpc_controller.h"
#include "idto/optimizer/trajectory_optimizer.h"
#include "mpc_spline.h"
#include "plant_step.h"

using namespace idto::optimizer;

struct idto_opt {
  std::unique_ptr<TrajectoryOptimizer<double>> to;
  int nq = 0, nv = 0, N = 0;
  TrajectoryOptimizer<double>::BatchSolveResult batch;   // of the last idto_opt_solve_batch (kept: its storage is reused)
};
struct idto_opt_warm_start {
  std::unique_ptr<WarmStart> ws;
};
struct idto_mpc {
  std::unique_ptr<idto::examples::mpc::ModelPredictiveController> mpc;
  idto_opt* opt = nullptr;
};
struct idto_mpc_batch {
  std::unique_ptr<idto::examples::mpc::BatchModelPredictiveController> mpc;
  idto_opt* opt = nullptr;
};

namespace {
thread_local std::string g_err;

std::vector<VectorXd> Rows(const double* flat, int count, int width) {
  std::vector<VectorXd> out((size_t)count, VectorXd((size_t)width));
  for (int t = 0; t < count; ++t) std::memcpy(out[t].data(), flat + (size_t)t * width, sizeof(double) * width);
  return out;
}
void Flat(const std::vector<VectorXd>& rows, double* out) {
  if (!out) return;
  size_t o = 0;
  for (const auto& r : rows) { std::memcpy(out + o, r.data(), sizeof(double) * r.size()); o += r.size(); }
}
void Flat(const VectorXd& v, double* out) {
  if (out) std::memcpy(out, v.data(), sizeof(double) * v.size());
}
MatrixXd Mat(const double* data, int n) {
  MatrixXd m(n, n);
  std::memcpy(m.data(), data, sizeof(double) * n * n);
  return m;
}
// B problems of the C-ABI as ProblemDefinitions (idto_opt_solve_batch, idto_mpc_batch_create)
std::vector<ProblemDefinition> BatchProblems(const idto_opt* o, int B, const idto_problem_t* problems, const char* who) {
  const int nq = o->nq, nv = o->nv;
  std::vector<ProblemDefinition> probs((size_t)B);
  for (int b = 0; b < B; ++b) {
    const idto_problem_t& p = problems[b];
    if (p.num_steps < 0) throw std::runtime_error(std::string(who) + ": problem " + std::to_string(b) + " has a negative num_steps");
    if (p.time_step != o->to->time_step())
      throw std::runtime_error(std::string(who) + ": problem " + std::to_string(b) + " has another time_step than the optimizer's");
    ProblemDefinition& prob = probs[b];
    prob.num_steps = p.num_steps;
    prob.q_init.assign(p.q_init, p.q_init + nq);
    prob.v_init.assign(p.v_init, p.v_init + nv);
    prob.Qq = Mat(p.Qq, nq); prob.Qv = Mat(p.Qv, nv); prob.Qf_q = Mat(p.Qf_q, nq); prob.Qf_v = Mat(p.Qf_v, nv);
    prob.R = Mat(p.R, nv);
    prob.q_nom = Rows(p.q_nom, p.num_steps + 1, nq);
    prob.v_nom = Rows(p.v_nom, p.num_steps + 1, nv);
  }
  return probs;
}
void FillStats(const TrajectoryOptimizerStats<double>& s, idto_stats_t* out) {
  if (!out) return;
  out->solve_time = s.solve_time;
  const int n = std::min<int>(out->capacity, (int)s.iteration_times.size());
  out->count = n;
  out->total = (int)s.iteration_times.size();
  for (int i = 0; i < n; ++i) {
    out->iteration_times[i] = s.iteration_times[i];
    out->iteration_costs[i] = s.iteration_costs[i];
    out->linesearch_iterations[i] = s.linesearch_iterations[i];
    out->linesearch_alphas[i] = s.linesearch_alphas[i];
    out->trust_region_radii[i] = s.trust_region_radii[i];
    out->q_norms[i] = s.q_norms[i];
    out->dq_norms[i] = s.dq_norms[i];
    out->dqH_norms[i] = s.dqH_norms[i];
    out->trust_ratios[i] = s.trust_ratios[i];
    out->gradient_norms[i] = s.gradient_norms[i];
    out->dL_dqs[i] = s.dL_dqs[i];
    out->h_norms[i] = s.h_norms[i];
    out->merits[i] = s.merits[i];
  }
}
template <class F>
int Guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  } catch (...) {
    g_err = "unknown exception";
    return -1;
  }
}
}  // namespace

extern "C" {

const char* idto_opt_last_error(void) { return g_err.c_str(); }

int idto_opt_dense_ldlt_solve(double* S, int n, double* b) {
  if (!S || !b || n < 1) { g_err = "dense_ldlt_solve: bad arguments"; return -1; }
  std::vector<double> M(S, S + (std::size_t)n * n);
  idto::optimizer::internal::DenseLdltSolve(&M, n, b);
  std::copy(M.begin(), M.end(), S);
  return 0;
}

int idto_opt_create(const idto_model_t* model, const idto_problem_t* p, const idto_contact_params_t* c,
                    const idto_solver_params_t* sp, int device, idto_opt** out) {
  return idto_opt_create_multi(model, p, c, sp, &device, 0, out);
}

int idto_opt_create_multi(const idto_model_t* model, const idto_problem_t* p, const idto_contact_params_t* c,
                          const idto_solver_params_t* sp, const int* devices, int ndev, idto_opt** out) {
  return Guard([&] {
    int nq = 0, nv = 0;
    for (int b = 0; b < model->nbodies; ++b) {
      const int jt = model->jtype[b];
      nq += (jt == IDTO_JOINT_FLOATING) ? 7 : (jt == IDTO_JOINT_PLANAR ? 3 : 1);
      nv += (jt == IDTO_JOINT_FLOATING) ? 6 : (jt == IDTO_JOINT_PLANAR ? 3 : 1);
    }
    ProblemDefinition prob;
    prob.num_steps = p->num_steps;
    prob.q_init.assign(p->q_init, p->q_init + nq);
    prob.v_init.assign(p->v_init, p->v_init + nv);
    prob.Qq = Mat(p->Qq, nq); prob.Qv = Mat(p->Qv, nv); prob.Qf_q = Mat(p->Qf_q, nq); prob.Qf_v = Mat(p->Qf_v, nv);
    prob.R = Mat(p->R, nv);
    prob.q_nom = Rows(p->q_nom, p->num_steps + 1, nq);
    prob.v_nom = Rows(p->v_nom, p->num_steps + 1, nv);
    SolverParameters params;
    params.check_convergence = sp->check_convergence != 0;
    params.convergence_tolerances = {sp->rel_cost_reduction, sp->abs_cost_reduction, sp->rel_gradient_along_dq,
                                     sp->abs_gradient_along_dq, sp->rel_state_change, sp->abs_state_change};
    params.method = static_cast<SolverMethod>(sp->method);
    params.linesearch_method = static_cast<LinesearchMethod>(sp->linesearch_method);
    params.max_iterations = sp->max_iterations;
    params.max_linesearch_iterations = sp->max_linesearch_iterations;
    params.gradients_method = static_cast<GradientsMethod>(sp->gradients_method);
    params.linear_solver = static_cast<SolverParameters::LinearSolverType>(sp->linear_solver);
    params.normalize_quaternions = sp->normalize_quaternions != 0;
    params.verbose = sp->verbose != 0;
    params.scaling = sp->scaling != 0;
    params.scaling_method = static_cast<ScalingMethod>(sp->scaling_method);
    params.equality_constraints = sp->equality_constraints != 0;
    params.Delta0 = sp->Delta0;
    params.Delta_max = sp->Delta_max;
    params.num_threads = sp->num_threads;
    params.print_debug_data = sp->print_debug_data != 0;
    params.debug_compare_against_dense = sp->debug_compare_against_dense != 0;
    params.exact_hessian = sp->exact_hessian != 0;
    params.save_contour_data = sp->plot_dumps != 0;
    params.contact_stiffness = c->contact_stiffness;
    params.dissipation_velocity = c->dissipation_velocity;
    params.stiction_velocity = c->stiction_velocity;
    params.friction_coefficient = c->friction_coefficient;
    params.smoothing_factor = c->smoothing_factor;
    auto h = std::make_unique<idto_opt>();
    if (ndev <= 0)   // (idto_opt_create: one device, no communicator)
      h->to = std::make_unique<TrajectoryOptimizer<double>>(*model, p->time_step, prob, params, devices[0]);
    else
      h->to = std::make_unique<TrajectoryOptimizer<double>>(*model, p->time_step, prob, params,
                                                            std::vector<int>(devices, devices + ndev));
    h->nq = nq; h->nv = nv; h->N = p->num_steps;
    *out = h.release();
  });
}
void idto_opt_destroy(idto_opt* o) { delete o; }

int idto_opt_num_steps(const idto_opt* o) { return o->to->num_steps(); }
double idto_opt_time_step(const idto_opt* o) { return o->to->time_step(); }
int idto_opt_num_equality_constraints(const idto_opt* o) { return o->to->num_equality_constraints(); }

int idto_opt_solve(idto_opt* o, const double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                   idto_stats_t* stats, int* flag, int* reason) {
  return Guard([&] {
    TrajectoryOptimizerSolution<double> sol;
    TrajectoryOptimizerStats<double> st;
    ConvergenceReason r = kNoConvergenceCriteriaSatisfied;
    const SolverFlag f = o->to->Solve(Rows(q_guess, o->N + 1, o->nq), &sol, &st, &r);
    Flat(sol.q, sol_q); Flat(sol.v, sol_v); Flat(sol.tau, sol_tau);
    FillStats(st, stats);
    if (flag) *flag = (int)f;
    if (reason) *reason = (int)r;
  });
}

int idto_opt_scene_sizes(idto_opt* o, int* nbodies, int* npairs, int* body_doubles, int* pair_doubles) {
  return Guard([&] {
    if (idto_hip_scene_sizes(o->to->device_context(), nbodies, npairs, body_doubles, pair_doubles))
      throw std::runtime_error(idto_hip_last_error());
  });
}
int idto_opt_scene_report(idto_opt* o, int nstates, const double* q, const double* v, double* bodies_out, double* pairs_out,
                          double* tau_contact_out, double* tau_pairs_out) {
  return Guard([&] {
    if (nstates < 1 || !q || !v) throw std::runtime_error("scene_report: nstates >= 1 states q[nstates][nq], v[nstates][nv] are required");
    if (!bodies_out && !pairs_out && !tau_contact_out && !tau_pairs_out) throw std::runtime_error("scene_report: every output is NULL: nothing to report");
    const SceneReport r = o->to->EvalScene(Rows(q, nstates, o->nq), Rows(v, nstates, o->nv), tau_pairs_out != nullptr);
    auto out = [](const std::vector<double>& from, double* to) { if (to) std::copy(from.begin(), from.end(), to); };
    out(r.bodies, bodies_out); out(r.pairs, pairs_out); out(r.tau_contact, tau_contact_out); out(r.tau_pairs, tau_pairs_out);
  });
}

int idto_opt_actuated_dofs(idto_opt* o, int* actuated_out) {
  const std::vector<int> dofs = o->to->actuated_dofs();
  if (actuated_out) std::copy(dofs.begin(), dofs.end(), actuated_out);
  return (int)dofs.size();
}

// a linearisation's arrays into the caller's (each may be NULL)
static void LinOut(const PlantLinearization& l, double* x_next_out, double* A_out, double* B_out, int* status_out) {
  const size_t w = (size_t)l.nq + l.nv, n = 2 * (size_t)l.nv;
  for (size_t k = 0; k < l.x_next.size(); ++k) {
    if (x_next_out) std::copy(l.x_next[k].begin(), l.x_next[k].end(), x_next_out + k * w);
    if (A_out) std::copy(l.A[k].data(), l.A[k].data() + n * n, A_out + k * n * n);
    if (B_out) std::copy(l.B[k].data(), l.B[k].data() + n * l.nv, B_out + k * n * l.nv);
  }
  if (status_out) std::copy(l.status.begin(), l.status.end(), status_out);
}

int idto_opt_plant_linearize(idto_opt* o, int nstates, const double* q, const double* v, const double* tau, double h, int substeps,
                             double* x_next_out, double* A_out, double* B_out, int* status_out) {
  return Guard([&] {
    if (nstates < 1 || !q || !v || !tau) throw std::runtime_error("plant_linearize: nstates >= 1 states q[nstates][nq], v[nstates][nv] and torques tau[nstates][nv] are required");
    LinOut(o->to->LinearizePlant(Rows(q, nstates, o->nq), Rows(v, nstates, o->nv), Rows(tau, nstates, o->nv), h, substeps), x_next_out,
           A_out, B_out, status_out);
  });
}

int idto_opt_tvlqr(idto_opt* o, const double* sol_q, const double* sol_v, const double* sol_tau, double h, const double* Qtheta,
                   const double* Qv, const double* R, const double* Qf_theta, const double* Qf_v, double* x_next_out, double* A_out,
                   double* B_out, int* status_out, double* K_out, double* P_out, int* lqr_status_out) {
  return Guard([&] {
    if (!sol_q || !sol_v || !sol_tau || !Qtheta || !Qv || !R || !Qf_theta || !Qf_v)
      throw std::runtime_error("tvlqr: the solution's q, v, tau and the weights Qtheta, Qv, R, Qf_theta, Qf_v are required");
    const int nv = o->nv, nu = (int)o->to->actuated_dofs().size(), n = 2 * nv;
    auto mat = [](const double* p, int m) { MatrixXd M(m, m); std::copy(p, p + (size_t)m * m, M.data()); return M; };
    TrajectoryOptimizerSolution<double> sol;
    sol.q = Rows(sol_q, o->N + 1, o->nq); sol.v = Rows(sol_v, o->N + 1, nv); sol.tau = Rows(sol_tau, o->N, nv);
    const TvlqrGains g = o->to->Tvlqr(sol, h, mat(Qtheta, nv), mat(Qv, nv), mat(R, nu), mat(Qf_theta, nv), mat(Qf_v, nv));
    LinOut(g.lin, x_next_out, A_out, B_out, status_out);
    for (size_t t = 0; K_out && t < g.K.size(); ++t) std::copy(g.K[t].data(), g.K[t].data() + (size_t)nu * n, K_out + t * nu * n);
    for (size_t t = 0; P_out && t < g.P.size(); ++t) std::copy(g.P[t].data(), g.P[t].data() + (size_t)n * n, P_out + t * n * n);
    if (lqr_status_out) *lqr_status_out = g.status[0];
  });
}

int idto_opt_track(idto_opt* o, const double* sol_q, const double* sol_v, const double* sol_tau, double h, const double* Qtheta,
                   const double* Qv, const double* R, const double* Qf_theta, const double* Qf_v, int nrollouts, const double* x0,
                   int zero_unactuated, double* x_next_out, double* A_out, double* B_out, int* status_out, double* K_out, double* P_out,
                   int* lqr_status_out, double* x_out, double* u_out, double* dx_out, int* track_status_out) {
  return Guard([&] {
    if (!sol_q || !sol_v || !sol_tau || !Qtheta || !Qv || !R || !Qf_theta || !Qf_v || !x0 || nrollouts < 1)
      throw std::runtime_error("track: the solution's q, v, tau, the weights Qtheta, Qv, R, Qf_theta, Qf_v and nrollouts >= 1 initial states x0 are required");
    const int nv = o->nv, nu = (int)o->to->actuated_dofs().size(), n = 2 * nv;
    auto mat = [](const double* p, int m) { MatrixXd M(m, m); std::copy(p, p + (size_t)m * m, M.data()); return M; };
    TrajectoryOptimizerSolution<double> sol;
    sol.q = Rows(sol_q, o->N + 1, o->nq); sol.v = Rows(sol_v, o->N + 1, nv); sol.tau = Rows(sol_tau, o->N, nv);
    const TrackedRollouts r = o->to->Track(sol, h, mat(Qtheta, nv), mat(Qv, nv), mat(R, nu), mat(Qf_theta, nv), mat(Qf_v, nv),
                                           Rows(x0, nrollouts, o->nq + nv), zero_unactuated != 0);
    const TvlqrGains& g = r.gains;
    LinOut(g.lin, x_next_out, A_out, B_out, status_out);
    for (size_t t = 0; K_out && t < g.K.size(); ++t) std::copy(g.K[t].data(), g.K[t].data() + (size_t)nu * n, K_out + t * nu * n);
    for (size_t t = 0; P_out && t < g.P.size(); ++t) std::copy(g.P[t].data(), g.P[t].data() + (size_t)n * n, P_out + t * n * n);
    if (lqr_status_out) *lqr_status_out = g.status[0];
    auto flat = [](const std::vector<VectorXd>& rows, double* out) {
      for (size_t k = 0; out && k < rows.size(); ++k) std::copy(rows[k].begin(), rows[k].end(), out + k * rows[k].size());
    };
    flat(r.x, x_out); flat(r.u, u_out); flat(r.dx, dx_out);
    if (track_status_out) std::copy(r.status.begin(), r.status.end(), track_status_out);
  });
}

int idto_opt_solve_batch(idto_opt* o, int B, const idto_problem_t* problems, const double* q_guesses, int only_best,
                         double* sol_q, double* sol_v, double* sol_tau, idto_stats_t* stats, int* flags, int* reasons,
                         double* final_costs, int* best) {
  return idto_opt_solve_batch_models(o, B, problems, nullptr, nullptr, q_guesses, only_best, sol_q, sol_v, sol_tau, stats, flags,
                                     reasons, final_costs, best);
}

int idto_opt_solve_batch_models(idto_opt* o, int B, const idto_problem_t* problems, const idto_model_t* const* models,
                                const idto_contact_params_t* const* contacts, const double* q_guesses, int only_best,
                                double* sol_q, double* sol_v, double* sol_tau, idto_stats_t* stats, int* flags, int* reasons,
                                double* final_costs, int* best) {
  return Guard([&] {
    if (B < 1 || !q_guesses) throw std::runtime_error("solve_batch: B >= 1 problems and their q_guesses are required");
    const int nq = o->nq, nv = o->nv;
    std::vector<ProblemDefinition> probs;
    if (problems) probs = BatchProblems(o, B, problems, "solve_batch");
    std::vector<std::vector<VectorXd>> guesses((size_t)B);
    const size_t nqa = (size_t)(o->N + 1) * nq, nva = (size_t)(o->N + 1) * nv, nta = (size_t)o->N * nv;
    for (int b = 0; b < B; ++b) guesses[b] = Rows(q_guesses + b * nqa, o->N + 1, nq);
    auto& R = o->batch;
    if (models || contacts) {
      std::vector<const idto_model_t*> ms;
      std::vector<const idto_contact_params_t*> cs;
      if (models) ms.assign(models, models + B);
      if (contacts) cs.assign(contacts, contacts + B);
      o->to->SolveBatch(guesses, problems ? &probs : nullptr, ms, cs, &R, only_best != 0);
    } else {
      o->to->SolveBatch(guesses, problems ? &probs : nullptr, &R, only_best != 0);
    }
    for (int b = 0; b < B; ++b) {
      if (!R.solutions[b].q.empty()) {   // (only_best: the best entry's alone; an entry that failed has none)
        Flat(R.solutions[b].q, sol_q ? sol_q + b * nqa : nullptr);
        Flat(R.solutions[b].v, sol_v ? sol_v + b * nva : nullptr);
        Flat(R.solutions[b].tau, sol_tau ? sol_tau + b * nta : nullptr);
      }
      if (stats) FillStats(R.stats[b], &stats[b]);
      if (flags) flags[b] = (int)R.flags[b];
      if (reasons) reasons[b] = (int)R.stats[b].convergence_reason;
      if (final_costs) final_costs[b] = R.final_costs[b];
    }
    if (best) *best = R.best;
  });
}
const char* idto_opt_batch_error(const idto_opt* o, int b) {
  return (b >= 0 && b < (int)o->batch.errors.size()) ? o->batch.errors[b].c_str() : "";
}
int idto_opt_last_batch_route(const idto_opt* o) { return o->to->last_batch_route(); }

int idto_opt_ws_create(idto_opt* o, const double* q_guess, idto_opt_warm_start** out) {
  return Guard([&] {
    auto w = std::make_unique<idto_opt_warm_start>();
    w->ws = o->to->CreateWarmStart(Rows(q_guess, o->N + 1, o->nq));
    *out = w.release();
  });
}
void idto_opt_ws_destroy(idto_opt_warm_start* w) { delete w; }
int idto_opt_ws_set_q(idto_opt* o, idto_opt_warm_start* w, const double* q) {
  return Guard([&] { w->ws->set_q(Rows(q, o->N + 1, o->nq)); });
}
int idto_opt_ws_get(idto_opt*, idto_opt_warm_start* w, double* q, double* Delta) {
  return Guard([&] {
    Flat(w->ws->get_q(), q);
    if (Delta) *Delta = w->ws->Delta;
  });
}
int idto_opt_ws_solve(idto_opt* o, idto_opt_warm_start* w, double* sol_q, double* sol_v, double* sol_tau,
                      idto_stats_t* stats, int* flag, int* reason) {
  return Guard([&] {
    TrajectoryOptimizerSolution<double> sol;
    TrajectoryOptimizerStats<double> st;
    ConvergenceReason r = kNoConvergenceCriteriaSatisfied;
    const SolverFlag f = o->to->SolveFromWarmStart(w->ws.get(), &sol, &st, &r);
    Flat(sol.q, sol_q); Flat(sol.v, sol_v); Flat(sol.tau, sol_tau);
    FillStats(st, stats);
    if (flag) *flag = (int)f;
    if (reason) *reason = (int)r;
  });
}

int idto_opt_reset_initial_conditions(idto_opt* o, const double* q_init, const double* v_init) {
  return Guard([&] { o->to->ResetInitialConditions(VectorXd(q_init, q_init + o->nq), VectorXd(v_init, v_init + o->nv)); });
}
int idto_opt_update_nominal_trajectory(idto_opt* o, const double* q_nom, const double* v_nom) {
  return Guard([&] { o->to->UpdateNominalTrajectory(Rows(q_nom, o->N + 1, o->nq), Rows(v_nom, o->N + 1, o->nv)); });
}

int idto_opt_eval(idto_opt* o, const double* q, double* cost, double* gradient, double* scaled_gradient,
                  double* scale_factors, double* lambda, double* merit, double* merit_gradient) {
  return Guard([&] {
    TrajectoryOptimizerState<double> s = o->to->CreateState();
    s.set_q(Rows(q, o->N + 1, o->nq));
    if (cost) *cost = o->to->EvalCost(s);
    if (gradient) Flat(o->to->EvalGradient(s), gradient);
    if (scaled_gradient) Flat(o->to->EvalScaledGradient(s), scaled_gradient);
    if (scale_factors) Flat(o->to->EvalScaleFactors(s), scale_factors);
    if (lambda) Flat(o->to->EvalLagrangeMultipliers(s), lambda);
    if (merit) *merit = o->to->EvalMeritFunction(s);
    if (merit_gradient) Flat(o->to->EvalMeritFunctionGradient(s), merit_gradient);
  });
}
int idto_opt_dogleg(idto_opt* o, const double* q, double Delta, double* dq, double* dqH, int* active) {
  return Guard([&] {
    TrajectoryOptimizerState<double> s = o->to->CreateState();
    s.set_q(Rows(q, o->N + 1, o->nq));
    VectorXd a, b;
    const bool act = o->to->CalcDoglegPoint(s, Delta, &a, &b);
    Flat(a, dq); Flat(b, dqH);
    if (active) *active = act ? 1 : 0;
  });
}
int idto_opt_trust_ratio(idto_opt* o, const double* q, const double* dq, double* rho) {
  return Guard([&] {
    TrajectoryOptimizerState<double> s = o->to->CreateState(), scratch = o->to->CreateState();
    s.set_q(Rows(q, o->N + 1, o->nq));
    *rho = o->to->CalcTrustRatio(s, VectorXd(dq, dq + (size_t)(o->N + 1) * o->nq), &scratch);
  });
}


// ---- model-predictive-control shell
int idto_mpc_create(idto_opt* opt, const double* warm_q, const double* warm_v, const double* warm_tau, const int* actuated,
                    const int* q_nom_relative_to_q_init, double replan_period, idto_mpc** out) {
  return Guard([&] {
    TrajectoryOptimizerSolution<double> warm;
    warm.q = Rows(warm_q, opt->N + 1, opt->nq);
    warm.v = Rows(warm_v, opt->N + 1, opt->nv);
    warm.tau = Rows(warm_tau, opt->N, opt->nv);
    std::vector<int> act;
    if (actuated) act.assign(actuated, actuated + opt->nv);
    std::vector<bool> sel((size_t)opt->nq, false);
    if (q_nom_relative_to_q_init)
      for (int i = 0; i < opt->nq; ++i) sel[i] = q_nom_relative_to_q_init[i] != 0;
    auto m = std::make_unique<idto_mpc>();
    m->opt = opt;
    m->mpc = std::make_unique<idto::examples::mpc::ModelPredictiveController>(opt->to.get(), warm, act, replan_period, sel);
    *out = m.release();
  });
}
void idto_mpc_destroy(idto_mpc* mpc) { delete mpc; }
int idto_mpc_num_actuators(const idto_mpc* mpc) { return mpc->mpc->num_actuators(); }
int idto_mpc_update(idto_mpc* mpc, double time, const double* x0, double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                    double* first_cost, int* flag) {
  return Guard([&] {
    const idto_opt* o = mpc->opt;
    mpc->mpc->UpdateAbstractState(time, VectorXd(x0, x0 + o->nq + o->nv));
    if (q_guess) Flat(mpc->mpc->last_guess(), q_guess);   // (what it used: the stored trajectory shifted to `time`, row 0 = q0)
    const auto& sol = mpc->mpc->last_solution();
    Flat(sol.q, sol_q); Flat(sol.v, sol_v); Flat(sol.tau, sol_tau);
    const auto& st = mpc->mpc->last_stats();
    if (first_cost) *first_cost = st.iteration_costs.empty() ? 0.0 : st.iteration_costs[0];
    if (flag) *flag = (int)mpc->mpc->last_flag();   // (kFactorizationFailed = 2: the outputs are the previous re-plan's)
  });
}
int idto_mpc_state(const idto_mpc* mpc, double time, double* x) {
  return Guard([&] { Flat(idto::examples::mpc::Interpolator::State(mpc->mpc->stored_trajectory(), time), x); });
}
int idto_mpc_control(const idto_mpc* mpc, double time, double* u) {
  return Guard([&] { Flat(idto::examples::mpc::Interpolator::Control(mpc->mpc->stored_trajectory(), time), u); });
}
double idto_mpc_start_time(const idto_mpc* mpc) { return mpc->mpc->stored_trajectory().start_time; }
int idto_mpc_spline_eval(const double* breaks, const double* knots, int n, int dim, const double* times, int nt, double* out) {
  return Guard([&] {
    const idto::examples::mpc::PiecewiseCubic sp(std::vector<double>(breaks, breaks + n), Rows(knots, n, dim));
    for (int i = 0; i < nt; ++i) Flat(sp.value(times[i]), out + (size_t)i * dim);
  });
}
int idto_mpc_stats(const idto_mpc* mpc, idto_stats_t* stats, double* radius) {
  return Guard([&] {
    FillStats(mpc->mpc->last_stats(), stats);
    if (radius) *radius = mpc->mpc->trust_region_radius();
  });
}

// ---- B controllers in one device pass per tick
int idto_mpc_batch_create(idto_opt* opt, int B, const idto_problem_t* problems, const double* warm_q, const double* warm_v,
                          const double* warm_tau, const int* actuated, const int* q_nom_relative_to_q_init, idto_mpc_batch** out) {
  return Guard([&] {
    if (B < 0 || !warm_q || !warm_v || !warm_tau) throw std::runtime_error("mpc_batch_create: B warm-start solutions are required");
    const size_t nqa = (size_t)(opt->N + 1) * opt->nq, nva = (size_t)(opt->N + 1) * opt->nv, nta = (size_t)opt->N * opt->nv;
    std::vector<TrajectoryOptimizerSolution<double>> warm((size_t)B);
    for (int b = 0; b < B; ++b) {
      warm[b].q = Rows(warm_q + b * nqa, opt->N + 1, opt->nq);
      warm[b].v = Rows(warm_v + b * nva, opt->N + 1, opt->nv);
      warm[b].tau = Rows(warm_tau + b * nta, opt->N, opt->nv);
    }
    std::vector<ProblemDefinition> probs;
    if (problems) probs = BatchProblems(opt, B, problems, "mpc_batch_create");
    std::vector<int> act;
    if (actuated) act.assign(actuated, actuated + opt->nv);
    std::vector<bool> sel((size_t)opt->nq, false);
    if (q_nom_relative_to_q_init)
      for (int i = 0; i < opt->nq; ++i) sel[i] = q_nom_relative_to_q_init[i] != 0;
    auto m = std::make_unique<idto_mpc_batch>();
    m->opt = opt;
    m->mpc = std::make_unique<idto::examples::mpc::BatchModelPredictiveController>(opt->to.get(), warm, act, sel, problems ? &probs : nullptr);
    *out = m.release();
  });
}
void idto_mpc_batch_destroy(idto_mpc_batch* mpc) { delete mpc; }
int idto_mpc_batch_num_actuators(const idto_mpc_batch* mpc) { return mpc->mpc->num_actuators(); }
int idto_mpc_batch_update(idto_mpc_batch* mpc, const double* times, const double* x0, double* q_guess, double* sol_q, double* sol_v,
                          double* sol_tau, idto_stats_t* stats, int* flags, double* radii, int* tick_ok) {
  return Guard([&] {
    if (!times || !x0) throw std::runtime_error("mpc_batch_update: times[B] and x0[B][nq + nv] are required");
    const idto_opt* o = mpc->opt;
    const int B = mpc->mpc->num_controllers();
    const size_t nqa = (size_t)(o->N + 1) * o->nq, nva = (size_t)(o->N + 1) * o->nv, nta = (size_t)o->N * o->nv;
    const bool ok = mpc->mpc->UpdateAll(times, x0);
    if (tick_ok) *tick_ok = ok ? 1 : 0;
    for (int b = 0; b < B; ++b) {
      if (q_guess) Flat(mpc->mpc->last_guess(b), q_guess + b * nqa);
      const auto& sol = mpc->mpc->last_solution(b);   // (a controller that failed: its previous re-plan's)
      Flat(sol.q, sol_q ? sol_q + b * nqa : nullptr);
      Flat(sol.v, sol_v ? sol_v + b * nva : nullptr);
      Flat(sol.tau, sol_tau ? sol_tau + b * nta : nullptr);
      if (stats) FillStats(mpc->mpc->last_stats(b), &stats[b]);
      if (flags) flags[b] = (int)mpc->mpc->last_flag(b);
      if (radii) radii[b] = mpc->mpc->trust_region_radius(b);
    }
  });
}
static void CheckController(const idto_mpc_batch* mpc, int b) {
  if (b < 0 || b >= mpc->mpc->num_controllers()) throw std::runtime_error("mpc_batch: controller index outside the batch");
}
// the outputs of a tick, as idto_mpc_batch_update hands them out
static void BatchTickOutputs(idto_mpc_batch* mpc, double* q_guess, double* sol_q, double* sol_v, double* sol_tau, idto_stats_t* stats,
                             int* flags, double* radii) {
  const idto_opt* o = mpc->opt;
  const int B = mpc->mpc->num_controllers();
  const size_t nqa = (size_t)(o->N + 1) * o->nq, nva = (size_t)(o->N + 1) * o->nv, nta = (size_t)o->N * o->nv;
  for (int b = 0; b < B; ++b) {
    if (q_guess) Flat(mpc->mpc->last_guess(b), q_guess + b * nqa);
    const auto& sol = mpc->mpc->last_solution(b);
    Flat(sol.q, sol_q ? sol_q + b * nqa : nullptr);
    Flat(sol.v, sol_v ? sol_v + b * nva : nullptr);
    Flat(sol.tau, sol_tau ? sol_tau + b * nta : nullptr);
    if (stats) FillStats(mpc->mpc->last_stats(b), &stats[b]);
    if (flags) flags[b] = (int)mpc->mpc->last_flag(b);
    if (radii) radii[b] = mpc->mpc->trust_region_radius(b);
  }
}
int idto_mpc_batch_plants_begin(idto_mpc_batch* mpc, double sim_time_step, const double* Kp, int kp_size, const double* Kd, int kd_size,
                                int feed_forward, int record_capacity) {
  return Guard([&] {
    idto::examples::mpc::BatchModelPredictiveController::PlantParams p;
    p.sim_time_step = sim_time_step; p.feed_forward = feed_forward != 0; p.record_capacity = record_capacity;
    if (Kp && kp_size > 0) p.Kp.assign(Kp, Kp + kp_size);
    if (Kd && kd_size > 0) p.Kd.assign(Kd, Kd + kd_size);
    mpc->mpc->BeginPlants(p);
  });
}
int idto_mpc_batch_plants_set_model(idto_mpc_batch* mpc, int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  return Guard([&] { mpc->mpc->SetPlantModel(b, model, contact); });
}
int idto_mpc_batch_plants_set_states(idto_mpc_batch* mpc, const double* times, const double* x) {
  return Guard([&] {
    if (!times || !x) throw std::runtime_error("mpc_batch_plants_set_states: times[B] and x[B][nq + nv] are required");
    mpc->mpc->SetPlantStates(times, x);
  });
}
int idto_mpc_batch_plants_step(idto_mpc_batch* mpc, int substeps) { return Guard([&] { mpc->mpc->StepPlants(substeps); }); }
int idto_mpc_batch_plants_state(idto_mpc_batch* mpc, int b, double* time, double* x, int* status) {
  return Guard([&] {
    CheckController(mpc, b);
    if (x) Flat(mpc->mpc->plant_state(b), x);
    if (time) *time = mpc->mpc->plant_time(b);
    if (status) *status = mpc->mpc->plant_status(b);
  });
}
int idto_mpc_batch_plants_tick(idto_mpc_batch* mpc, int substeps, double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                               idto_stats_t* stats, int* flags, double* radii, int* tick_ok) {
  return Guard([&] {
    const bool ok = mpc->mpc->TickWithPlants(substeps);
    if (tick_ok) *tick_ok = ok ? 1 : 0;
    BatchTickOutputs(mpc, q_guess, sol_q, sol_v, sol_tau, stats, flags, radii);
  });
}
// the Plants view on an optimizer's own context (one plant)
int idto_plant_forward_dynamics(idto_opt* opt, const double* x, const double* tau, double* a, double* M, double* bias) {
  return Guard([&] { idto::examples::mpc::Plants(opt->to->device_context()).ForwardDynamics(x, tau, a, M, bias); });
}
int idto_plant_begin(idto_opt* opt, double sim_time_step, int record_capacity) {
  return Guard([&] { idto::examples::mpc::Plants(opt->to->device_context()).Begin(sim_time_step, record_capacity); });
}
int idto_plant_set_state(idto_opt* opt, double time, const double* x) {
  return Guard([&] { idto::examples::mpc::Plants(opt->to->device_context()).SetStates(&time, x); });
}
int idto_plant_get_state(idto_opt* opt, double* time, double* x) {
  return Guard([&] { idto::examples::mpc::Plants(opt->to->device_context()).GetStates(time, x); });
}
int idto_plant_step(idto_opt* opt, int substeps, const double* tau_hold, int record_every, double* x_record, int* status) {
  return Guard([&] { idto::examples::mpc::Plants(opt->to->device_context()).Step(substeps, tau_hold, record_every, x_record, status); });
}

int idto_mpc_batch_state(const idto_mpc_batch* mpc, int b, double time, double* x) {
  return Guard([&] { CheckController(mpc, b); Flat(idto::examples::mpc::Interpolator::State(mpc->mpc->stored_trajectory(b), time), x); });
}
int idto_mpc_batch_control(const idto_mpc_batch* mpc, int b, double time, double* u) {
  return Guard([&] { CheckController(mpc, b); Flat(idto::examples::mpc::Interpolator::Control(mpc->mpc->stored_trajectory(b), time), u); });
}
double idto_mpc_batch_start_time(const idto_mpc_batch* mpc, int b) {
  return (b >= 0 && b < mpc->mpc->num_controllers()) ? mpc->mpc->stored_trajectory(b).start_time : std::numeric_limits<double>::quiet_NaN();
}
int idto_mpc_batch_flag(const idto_mpc_batch* mpc, int b) {
  return (b >= 0 && b < mpc->mpc->num_controllers()) ? (int)mpc->mpc->last_flag(b) : -1;
}
const char* idto_mpc_batch_error(const idto_mpc_batch* mpc, int b) {
  if (b < 0) return mpc->mpc->last_tick_error().c_str();
  return b < mpc->mpc->num_controllers() ? mpc->mpc->last_error(b).c_str() : "";
}

// ---- csrc/mpc_spline.h on the host, for the tests that hold the device's kernels to it
int idto_mpc_spline_fit(const double* breaks, const double* knots, int n, int dim, double* m_out) {
  return Guard([&] {
    if (n < 2 || dim < 0) throw std::runtime_error("mpc_spline_fit: at least two knots");
    std::vector<double> w((size_t)n * dim, 0.0);
    for (int c = 0; c < dim; ++c)
      if (idto_spline::spline_fit(breaks, n, knots + c, m_out + c, w.data() + c, dim)) throw std::runtime_error("mpc_spline_fit: singular system");
  });
}
int idto_mpc_shift_reference(const double* breaks, const double* y_q, const double* m_q, int n, int nq, double start_time, double time,
                             double time_step, const double* q0, const int* selector, double* q_nom, double* guess_out) {
  return Guard([&] {
    const double start = time - start_time;
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < nq; ++c)
        guess_out[(size_t)i * nq + c] = i == 0 ? q0[c] : idto_spline::spline_value(breaks, n, y_q + c, m_q + c, nq, idto_spline::guess_time(start, i, time_step));
    const std::vector<double> old0(q_nom, q_nom + nq);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < nq; ++c)
        q_nom[(size_t)i * nq + c] = idto_spline::nominal_shift(q_nom[(size_t)i * nq + c], selector[c] != 0, q0[c], old0[(size_t)c]);
  });
}

// ---- csrc/plant_step.h on the host, for the tests that hold plant_kernel to it
int idto_plant_solve_host(const double* M, const double* tau_applied, const double* bias, int n, double* a_out) {
  if (n < 1) return 0;
  std::vector<double> A(M, M + (size_t)n * n), work((size_t)n, 0.0);
  for (int i = 0; i < n; ++i) a_out[i] = tau_applied[i] - bias[i];
  return idto_plant::plant_ldlt_solve(A.data(), n, a_out, work.data());
}
void idto_plant_pd_plus_host(const double* Kp, const double* Kd, int nu, int nq, int nv, const int* actuated_dofs, const double* q,
                             const double* v, const double* q_nom, const double* v_nom, int feed_forward, const double* u_nom,
                             double* tau_out) {
  idto_plant::plant_pd_plus(Kp, Kd, nu, nq, nv, actuated_dofs, q, v, q_nom, v_nom, feed_forward != 0, u_nom, tau_out);
}
void idto_plant_advance_host(int nbodies, const int* jtype, const int* qstart, const int* vstart, int nq, double h, double* q,
                             double* v, const double* a) {
  std::vector<double> qdot((size_t)(nq > 0 ? nq : 1), 0.0);
  idto_plant::plant_advance(nbodies, jtype, qstart, vstart, h, q, v, a, qdot.data());
}
}  // extern "C"
