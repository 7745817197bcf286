// mpc_controller.cc — include/idto/examples/mpc_controller.h (reference examples/mpc_controller.cc:13-178).
#include "idto/examples/mpc_controller.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <stdexcept>
#include <string>

#include "host/batch_rows.h"

#include "mpc_spline.h"

namespace idto {
namespace examples {
namespace mpc {

// ---- PiecewiseCubic: first derivatives m_i at the knots from the linear system of C2 continuity
//   h_i m_{i-1} + 2 (h_{i-1} + h_i) m_i + h_{i-1} m_{i+1} = 3 (h_i d_{i-1} + h_{i-1} d_i),  d_i = (y_{i+1} - y_i) / h_i
// closed by the not-a-knot conditions at both ends; one dense LU with partial pivoting (n <= a few hundred knots)
// serves every component.
PiecewiseCubic::PiecewiseCubic(const std::vector<double>& breaks, const std::vector<VectorXd>& knots) {
  Assign(breaks, knots, (int)knots.size());
}
// (an object that is assigned again keeps its storage: three splines per MPC re-plan, no allocation in the steady state)
void PiecewiseCubic::Assign(const std::vector<double>& breaks, const std::vector<VectorXd>& knots, int count) {
  const int n = (int)breaks.size();
  if (n < 2 || count != n || (int)knots.size() < n) throw std::invalid_argument("PiecewiseCubic: at least two knots, one value per break");
  dim_ = (int)knots[0].size();
  y_.resize((size_t)n * dim_);
  for (int i = 0; i < n; ++i) {
    if ((int)knots[i].size() != dim_) throw std::invalid_argument("PiecewiseCubic: knots of different sizes");
    for (int c = 0; c < dim_; ++c) y_[(size_t)i * dim_ + c] = knots[i][c];
  }
  Fit(breaks);
}
void PiecewiseCubic::AssignFlat(const std::vector<double>& breaks, const double* knots, int dim) {
  const int n = (int)breaks.size();
  if (n < 2 || dim < 0) throw std::invalid_argument("PiecewiseCubic: at least two knots, one value per break");
  dim_ = dim;
  y_.assign(knots, knots + (size_t)n * dim_);
  Fit(breaks);
}
void PiecewiseCubic::Fit(const std::vector<double>& breaks) {
  const int n = (int)breaks.size();
  for (int i = 0; i + 1 < n; ++i)
    if (!(breaks[i + 1] > breaks[i])) throw std::invalid_argument("PiecewiseCubic: breaks must increase");
  t_ = breaks;
  m_.assign((size_t)n * dim_, 0.0);
  // the fit itself, per component: csrc/mpc_spline.h (the device fits the same text, mpc_batch.h); B_ is its work space
  B_.assign((size_t)n * dim_, 0.0);
  for (int c = 0; c < dim_; ++c)
    if (idto_spline::spline_fit(t_.data(), n, y_.data() + c, m_.data() + c, B_.data() + c, dim_))
      throw std::runtime_error("PiecewiseCubic: singular system");
}

void PiecewiseCubic::AssignFitted(const std::vector<double>& breaks, const double* y, const double* m, int dim) {
  const int n = (int)breaks.size();
  if (n < 2 || dim < 0) throw std::invalid_argument("PiecewiseCubic: at least two knots, one value per break");
  dim_ = dim;
  t_ = breaks;
  y_.assign(y, y + (size_t)n * dim_);
  m_.assign(m, m + (size_t)n * dim_);
}

VectorXd PiecewiseCubic::value(double t) const {
  VectorXd out((size_t)dim_);
  value(t, &out);
  return out;
}
void PiecewiseCubic::value(double t, VectorXd* out_ptr) const {
  if (t_.empty()) throw std::runtime_error("PiecewiseCubic: empty trajectory");
  const int n = (int)t_.size();
  const int i = idto_spline::spline_interval(t_.data(), n, &t);   // (t clamped to the breaks' range)
  VectorXd& out = *out_ptr;
  out.resize((size_t)dim_);
  for (int c = 0; c < dim_; ++c)
    out[c] = idto_spline::spline_piece(t_[i], t_[i + 1], y_[(size_t)i * dim_ + c], y_[(size_t)(i + 1) * dim_ + c],
                                    m_[(size_t)i * dim_ + c], m_[(size_t)(i + 1) * dim_ + c], t);
}

// ---- ModelPredictiveController (mpc_controller.cc:13-41)
ModelPredictiveController::ModelPredictiveController(TrajectoryOptimizer<double>* optimizer,
                                                     const TrajectoryOptimizerSolution<double>& warm_start_solution,
                                                     const std::vector<int>& actuated, double replan_period,
                                                     const std::vector<bool>& q_nom_relative_to_q_init)
    : time_step_(optimizer->time_step()),
      num_steps_(optimizer->num_steps() + 1),
      nq_(optimizer->num_positions()),
      nv_(optimizer->num_velocities()),
      optimizer_(optimizer),
      warm_start_(optimizer->CreateWarmStart(warm_start_solution.q)),
      replan_period_(replan_period),
      selector_override_(q_nom_relative_to_q_init) {
  for (int j = 0; j < (int)actuated.size() && j < nv_; ++j)
    if (actuated[j]) actuated_dofs_.push_back(j);
  if (actuated_dofs_.empty())
    for (int j = 0; j < nv_; ++j) actuated_dofs_.push_back(j);
  nu_ = (int)actuated_dofs_.size();
  StoreOptimizerSolution(warm_start_solution, 0.0, &stored_);
  solution_ = warm_start_solution;
}

// UpdateAbstractState (:43-85)
const StoredTrajectory& ModelPredictiveController::UpdateAbstractState(double time, const VectorXd& x0) {
  const SolverParameters& params = optimizer_->params();
  const std::vector<bool>& selector = selector_override_.empty() ? params.q_nom_relative_to_q_init : selector_override_;
  if ((int)selector.size() != nq_)
    throw std::invalid_argument("q_nom_relative_to_q_init must have one entry per position (mpc_controller.cc:45)");
  if ((int)x0.size() != nq_ + nv_) throw std::invalid_argument("state estimate must be [q0; v0]");
  idto_hip_trace_mark("mpc: UpdateAbstractState begins");
  const VectorXd q0(x0.begin(), x0.begin() + nq_), v0(x0.begin() + nq_, x0.end());
  // the initial guess from the stored solution, consistent with the initial condition (:55-58)
  // (the three trajectories below live in the controller: 120 small vectors allocated and freed per re-plan were ~10 us
  // of a 0.2 ms call)
  std::vector<VectorXd>& q_guess = guess_scratch_;
  if ((int)q_guess.size() != num_steps_) q_guess.assign((size_t)num_steps_, VectorXd((size_t)nq_));
  UpdateInitialGuess(stored_, time, &q_guess);
  q_guess[0] = q0;
  warm_start_->set_q(q_guess);
  last_guess_ = q_guess;
  idto_hip_trace_mark("mpc: initial guess from the stored splines");
  // shift the nominal trajectory for some DoFs, if requested (:60-69)
  const ProblemDefinition& prob = optimizer_->prob();
  const VectorXd q0_nom_old = prob.q_nom[0];
  std::vector<VectorXd>& q_nom_new = q_nom_scratch_;
  q_nom_new = prob.q_nom;
  for (VectorXd& qt_nom : q_nom_new)
    for (int i = 0; i < nq_; ++i) qt_nom[i] = idto_spline::nominal_shift(qt_nom[i], selector[i], q0[i], q0_nom_old[i]);
  std::vector<VectorXd>& v_nom = v_nom_scratch_;
  v_nom = prob.v_nom;
  optimizer_->UpdateNominalTrajectory(q_nom_new, v_nom);
  idto_hip_trace_mark("mpc: nominal trajectory shifted");
  // solve from the new initial condition (:71-75)
  optimizer_->ResetInitialConditions(q0, v0);
  idto_hip_trace_mark("mpc: initial conditions reset");
  stats_ = TrajectoryOptimizerStats<double>();
  TrajectoryOptimizerSolution<double>& solution = scratch_solution_;   // (keeps the rows' storage of the re-plan before last)
  last_flag_ = optimizer_->SolveFromWarmStart(warm_start_.get(), &solution, &stats_);
  idto_hip_trace_mark("mpc: SolveFromWarmStart returned");
  // (a failed factorisation returns an empty solution - the previous plan stays in force and the caller is
  // told through last_flag(); the reference, a Drake LeafSystem, has nowhere to report it and would throw from
  // StoreOptimizerSolution with the controller's state half updated)
  if (last_flag_ == optimizer::SolverFlag::kFactorizationFailed || (int)solution.q.size() < num_steps_) return stored_;
  std::swap(solution_.q, solution.q); std::swap(solution_.v, solution.v); std::swap(solution_.tau, solution.tau);
  StoreOptimizerSolution(solution_, time, &stored_);
  idto_hip_trace_mark("mpc: solution stored as splines");
  return stored_;
}

// UpdateInitialGuess (:87-97)
void ModelPredictiveController::UpdateInitialGuess(const StoredTrajectory& stored_trajectory, double current_time,
                                                   std::vector<VectorXd>* q_guess) const {
  if ((int)q_guess->size() != num_steps_) throw std::invalid_argument("UpdateInitialGuess: q_guess must have num_steps + 1 entries");
  const double start_time = current_time - stored_trajectory.start_time;
  for (int i = 0; i < num_steps_; ++i) stored_trajectory.q.value(idto_spline::guess_time(start_time, i, time_step_), &(*q_guess)[i]);   // (in place: no temporary per step)
}

// StoreOptimizerSolution (:99-138)
void ModelPredictiveController::StoreOptimizerSolution(const TrajectoryOptimizerSolution<double>& solution, double start_time,
                                                       StoredTrajectory* stored_trajectory) const {
  if ((int)solution.q.size() < num_steps_ || (int)solution.v.size() < num_steps_ || (int)solution.tau.size() < num_steps_ - 1)
    throw std::invalid_argument("StoreOptimizerSolution: solution shorter than the horizon");
  std::vector<double>& time_steps = times_;
  time_steps.resize((size_t)num_steps_);
  for (int i = 0; i < num_steps_; ++i) time_steps[i] = i * time_step_;
  // control inputs, which are undefined at the last time step (:122-126): u = B^T tau
  u_flat_.resize((size_t)num_steps_ * nu_);
  for (int i = 0; i < num_steps_; ++i) {
    const VectorXd& tau = solution.tau[idto_spline::control_row(i, num_steps_)];
    for (int j = 0; j < nu_; ++j) u_flat_[(size_t)i * nu_ + j] = tau[actuated_dofs_[j]];
  }
  stored_trajectory->start_time = start_time;
  stored_trajectory->q.Assign(time_steps, solution.q, num_steps_);
  stored_trajectory->v.Assign(time_steps, solution.v, num_steps_);
  stored_trajectory->u.AssignFlat(time_steps, u_flat_.data(), nu_);
}

// ---- BatchModelPredictiveController: B controllers, one device pass per tick (include/idto_hip.h idto_hip_mpc_batch_*)
namespace {
void HipCheck(int rc, const char* what) {
  if (rc != 0) throw std::runtime_error(std::string(what) + ": " + idto_hip_last_error());
}
void RowsFromFlat(const double* flat, int count, int width, std::vector<VectorXd>* out) {
  out->resize((size_t)count);
  for (int t = 0; t < count; ++t) (*out)[(size_t)t].assign(flat + (size_t)t * width, flat + (size_t)(t + 1) * width);
}
}  // namespace

BatchModelPredictiveController::BatchModelPredictiveController(TrajectoryOptimizer<double>* optimizer,
                                                               const std::vector<TrajectoryOptimizerSolution<double>>& warm,
                                                               const std::vector<int>& actuated,
                                                               const std::vector<bool>& q_nom_relative_to_q_init,
                                                               const std::vector<ProblemDefinition>* problems)
    : optimizer_(optimizer),
      B_((int)warm.size()),
      N_(optimizer->num_steps()),
      nq_(optimizer->num_positions()),
      nv_(optimizer->num_velocities()) {
  if (problems && (int)problems->size() != B_)
    throw std::invalid_argument("BatchModelPredictiveController: one problem per warm-start solution (or none)");
  std::vector<const ProblemDefinition*> probs((size_t)B_, &optimizer->prob());
  for (int b = 0; problems && b < B_; ++b) probs[(size_t)b] = &(*problems)[(size_t)b];
  const std::string why = optimizer->BatchLoopRefusal(B_, probs);
  if (!why.empty())
    throw std::invalid_argument("BatchModelPredictiveController: the device's batch loop does not serve " + why +
                                " - use B ModelPredictiveControllers, each on an optimizer of its own");
  const std::vector<bool>& selector = q_nom_relative_to_q_init.empty() ? optimizer->params().q_nom_relative_to_q_init : q_nom_relative_to_q_init;
  if ((int)selector.size() != nq_)
    throw std::invalid_argument("q_nom_relative_to_q_init must have one entry per position (mpc_controller.cc:45)");
  std::vector<int> sel((size_t)nq_), dofs;
  for (int i = 0; i < nq_; ++i) sel[(size_t)i] = selector[(size_t)i] ? 1 : 0;
  for (int j = 0; j < (int)actuated.size() && j < nv_; ++j)
    if (actuated[(size_t)j]) dofs.push_back(j);
  if (dofs.empty())
    for (int j = 0; j < nv_; ++j) dofs.push_back(j);
  nu_ = (int)dofs.size();
  const int n = N_ + 1;
  const size_t nqa = (size_t)n * nq_, nva = (size_t)n * nv_, nta = (size_t)N_ * nv_, len = IDTO_MPC_PLAN_LEN(n, nq_, nv_, nu_);
  q_.resize(B_ * nqa); v_.resize(B_ * nva); tau_.resize(B_ * nta); guess_.resize(B_ * nqa); plans_.resize(B_ * len);
  for (int b = 0; b < B_; ++b) {
    const TrajectoryOptimizerSolution<double>& w = warm[(size_t)b];
    bool ok = (int)w.q.size() >= n && (int)w.v.size() >= n && (int)w.tau.size() >= N_;
    for (int t = 0; ok && t < n; ++t) ok = (int)w.q[(size_t)t].size() == nq_ && (int)w.v[(size_t)t].size() == nv_;
    for (int t = 0; ok && t < N_; ++t) ok = (int)w.tau[(size_t)t].size() == nv_;
    if (!ok) throw std::invalid_argument("BatchModelPredictiveController: warm-start solution " + std::to_string(b) + " is shorter than the horizon");
    for (int t = 0; t < n; ++t) {
      std::copy(w.q[(size_t)t].begin(), w.q[(size_t)t].end(), q_.begin() + b * nqa + (size_t)t * nq_);
      std::copy(w.v[(size_t)t].begin(), w.v[(size_t)t].end(), v_.begin() + b * nva + (size_t)t * nv_);
    }
    for (int t = 0; t < N_; ++t) std::copy(w.tau[(size_t)t].begin(), w.tau[(size_t)t].end(), tau_.begin() + b * nta + (size_t)t * nv_);
  }
  breaks_.resize((size_t)n);
  for (int i = 0; i < n; ++i) breaks_[(size_t)i] = i * optimizer->time_step();
  stored_.resize((size_t)B_); flags_.assign((size_t)B_, optimizer::SolverFlag::kSuccess); errors_.resize((size_t)B_);
  stats_.resize((size_t)B_); solutions_ = warm; guesses_.resize((size_t)B_);
  Delta_.assign((size_t)B_, optimizer->params().Delta0); Delta_out_.resize((size_t)B_);
  final_cost_.resize((size_t)B_); status_.resize((size_t)B_); x0_.resize((size_t)B_ * (nq_ + nv_));
  rows_.resize((size_t)B_ * std::max(1, optimizer->params().max_iterations) * IDTO_TR_ROW);
  // ---- the first device work
  ctx_ = optimizer->CreateBatchContext(probs);
  try {
    HipCheck(idto_hip_mpc_batch_begin(ctx_, sel.data(), dofs.data(), nu_), "idto_hip_mpc_batch_begin");
    const std::vector<double> t0((size_t)B_, 0.0);   // (the constructor's StoreOptimizerSolution(warm_start_solution, 0.0))
    HipCheck(idto_hip_mpc_batch_store(ctx_, q_.data(), v_.data(), tau_.data(), t0.data(), plans_.data()), "idto_hip_mpc_batch_store");
    loop_ = optimizer->PrepareBatchLoop(ctx_);
    if (loop_.nu > 0) {   // (the context's own word on the constraint route, whatever set its option)
      int con_kkt = 1;
      HipCheck(idto_hip_get_option(ctx_, "con_kkt", &con_kkt), "idto_hip_get_option");
      if (!con_kkt)
        throw std::invalid_argument("BatchModelPredictiveController: the device's batch loop does not serve the child-context constraint "
                                    "route (option con_kkt = 0) - use B ModelPredictiveControllers, each on an optimizer of its own");
    }
  } catch (...) {
    idto_hip_destroy(ctx_);
    ctx_ = nullptr;
    throw;
  }
  for (int b = 0; b < B_; ++b) AdoptPlan(b, plans_.data() + b * len);
}

BatchModelPredictiveController::~BatchModelPredictiveController() {
  if (ctx_) idto_hip_destroy(ctx_);
}

void BatchModelPredictiveController::AdoptPlan(int b, const double* plan) {
  const size_t n = (size_t)N_ + 1;
  StoredTrajectory& s = stored_[(size_t)b];
  s.start_time = plan[0];
  const double* p = plan + 1;
  s.q.AssignFitted(breaks_, p, p + n * nq_, nq_); p += 2 * n * nq_;
  s.v.AssignFitted(breaks_, p, p + n * nv_, nv_); p += 2 * n * nv_;
  s.u.AssignFitted(breaks_, p, p + n * nu_, nu_);
}

bool BatchModelPredictiveController::UpdateAll(const std::vector<double>& times, const std::vector<VectorXd>& x0s) {
  if ((int)times.size() != B_ || (int)x0s.size() != B_) throw std::invalid_argument("UpdateAll: one time and one state estimate per controller");
  for (int b = 0; b < B_; ++b) {
    if ((int)x0s[(size_t)b].size() != nq_ + nv_) throw std::invalid_argument("state estimate must be [q0; v0]");
    std::copy(x0s[(size_t)b].begin(), x0s[(size_t)b].end(), x0_.begin() + (size_t)b * (nq_ + nv_));
  }
  return UpdateAll(times.data(), x0_.data());
}

bool BatchModelPredictiveController::UpdateAll(const double* times, const double* x0s) { return Tick(times, x0s, -1); }

// ---- the plants
static void PlantOk(int rc, const char* who) {
  if (rc != 0) throw std::runtime_error(std::string(who) + ": " + idto_hip_last_error());
}
void BatchModelPredictiveController::BeginPlants(const PlantParams& params) {
  idto_plant_params_t p{};
  p.h = params.sim_time_step; p.mode = IDTO_PLANT_PD_PLUS;
  p.Kp = params.Kp.data(); p.kp_size = (int)params.Kp.size(); p.Kd = params.Kd.data(); p.kd_size = (int)params.Kd.size();
  p.feed_forward = params.feed_forward ? 1 : 0; p.record_capacity = params.record_capacity;
  PlantOk(idto_hip_plant_begin(ctx_, &p), "BeginPlants");
  plants_ = true; plants_stale_ = true;
  plant_times_.assign((size_t)B_, 0.0); plant_x_.assign((size_t)B_ * (nq_ + nv_), 0.0); plant_status_.assign((size_t)B_ * 2, 0);
  plant_states_.assign((size_t)B_, VectorXd((size_t)(nq_ + nv_)));
}
void BatchModelPredictiveController::SetPlantModel(int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  PlantOk(idto_hip_plant_set_model(ctx_, b, model, contact), "SetPlantModel");
}
void BatchModelPredictiveController::SetPlantStates(const double* times, const double* x) {
  PlantOk(idto_hip_plant_set_state(ctx_, times, x), "SetPlantStates");
  plants_stale_ = true;
}
void BatchModelPredictiveController::SetPlantStates(const std::vector<double>& times, const std::vector<VectorXd>& x) {
  if ((int)times.size() != B_ || (int)x.size() != B_) throw std::invalid_argument("SetPlantStates: one time and one state per plant");
  std::vector<double> flat((size_t)B_ * (nq_ + nv_));
  for (int b = 0; b < B_; ++b) {
    if ((int)x[(size_t)b].size() != nq_ + nv_) throw std::invalid_argument("a plant's state must be [q; v]");
    std::copy(x[(size_t)b].begin(), x[(size_t)b].end(), flat.begin() + (size_t)b * (nq_ + nv_));
  }
  SetPlantStates(times.data(), flat.data());
}
void BatchModelPredictiveController::StepPlants(int substeps) {
  if (!plants_) throw std::runtime_error("StepPlants: call BeginPlants first");
  PlantOk(idto_hip_plant_step(ctx_, substeps, nullptr, 0, nullptr, plant_status_.data()), "StepPlants");
  plants_stale_ = true;
}
void BatchModelPredictiveController::FetchPlants() {
  if (!plants_) throw std::runtime_error("the plants: call BeginPlants first");
  if (!plants_stale_) return;
  PlantOk(idto_hip_plant_get_state(ctx_, plant_times_.data(), plant_x_.data()), "plant_state");
  for (int b = 0; b < B_; ++b)
    std::copy(plant_x_.begin() + (size_t)b * (nq_ + nv_), plant_x_.begin() + (size_t)(b + 1) * (nq_ + nv_), plant_states_[(size_t)b].begin());
  plants_stale_ = false;
}
const VectorXd& BatchModelPredictiveController::plant_state(int b) { FetchPlants(); return plant_states_.at((size_t)b); }
double BatchModelPredictiveController::plant_time(int b) { FetchPlants(); return plant_times_.at((size_t)b); }
int BatchModelPredictiveController::plant_status(int b) { FetchPlants(); return plant_status_.at((size_t)b * 2); }
bool BatchModelPredictiveController::TickWithPlants(int substeps) {
  if (!plants_) throw std::runtime_error("TickWithPlants: call BeginPlants first");
  if (substeps < 0) throw std::runtime_error("TickWithPlants: substeps must not be negative");
  return Tick(nullptr, nullptr, substeps);
}

Plants::Plants(idto_hip_ctx* context) : ctx_(context), B_(context ? idto_hip_batch_size(context) : 0) {
  if (!context) throw std::invalid_argument("Plants: a device context is required");
}
void Plants::ForwardDynamics(const double* x, const double* tau, double* a, double* M, double* bias) {
  PlantOk(idto_hip_forward_dynamics(ctx_, x, tau, a, M, bias), "Plants::ForwardDynamics");
}
void Plants::Begin(double sim_time_step, int record_capacity) {
  idto_plant_params_t p{};
  p.h = sim_time_step; p.mode = IDTO_PLANT_HOLD; p.record_capacity = record_capacity;
  PlantOk(idto_hip_plant_begin(ctx_, &p), "Plants::Begin");
}
void Plants::SetModel(int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  PlantOk(idto_hip_plant_set_model(ctx_, b, model, contact), "Plants::SetModel");
}
void Plants::SetStates(const double* times, const double* x) { PlantOk(idto_hip_plant_set_state(ctx_, times, x), "Plants::SetStates"); }
void Plants::GetStates(double* times, double* x) { PlantOk(idto_hip_plant_get_state(ctx_, times, x), "Plants::GetStates"); }
void Plants::Step(int substeps, const double* tau_hold, int record_every, double* x_record, int* status) {
  PlantOk(idto_hip_plant_step(ctx_, substeps, tau_hold, record_every, x_record, status), "Plants::Step");
}

// One tick of the B controllers: from times / x0s (substeps < 0: UpdateAll), or from the plants after `substeps` substeps of
// theirs (TickWithPlants) - the same adoption of the device's results either way
bool BatchModelPredictiveController::Tick(const double* times, const double* x0s, int substeps) {
  using clock = std::chrono::high_resolution_clock;
  idto_hip_trace_mark("mpc batch: UpdateAll begins");
  const auto start = clock::now();
  const int n = N_ + 1, iters = loop_.iterations;
  const size_t nqa = (size_t)n * nq_, nva = (size_t)n * nv_, nta = (size_t)N_ * nv_, len = IDTO_MPC_PLAN_LEN(n, nq_, nv_, nu_);
  int best = -1;
  int rc;
  if (substeps < 0) {
    rc = idto_hip_mpc_batch_replan(ctx_, times, x0s, iters, loop_.scaling_method, loop_.scaling, loop_.normalize_quaternions,
                                   Delta_.data(), loop_.Delta_max, loop_.eta, loop_.constrained_dofs, loop_.nu, rows_.data(),
                                   Delta_out_.data(), q_.data(), v_.data(), tau_.data(), final_cost_.data(), status_.data(),
                                   &best, guess_.data(), plans_.data());
  } else {
    rc = idto_hip_mpc_batch_tick_plants(ctx_, substeps, iters, loop_.scaling_method, loop_.scaling, loop_.normalize_quaternions,
                                        Delta_.data(), loop_.Delta_max, loop_.eta, loop_.constrained_dofs, loop_.nu, rows_.data(),
                                        Delta_out_.data(), q_.data(), v_.data(), tau_.data(), final_cost_.data(), status_.data(),
                                        &best, guess_.data(), plans_.data(), plant_x_.data(), plant_status_.data());
    plants_stale_ = true;   // (the states came back with the tick; the times have not: plant_time fetches them)
  }
  idto_hip_trace_mark("mpc batch: idto_hip_mpc_batch_replan returned");
  tick_error_.clear();
  if (rc == IDTO_HIP_SOLVER_TIMEOUT) {
    // nothing of this tick counts: every plan, solution and radius stays (the device's plans too: include/idto_hip.h)
    tick_error_ = std::string("the batch loop timed out on the device: ") + idto_hip_last_error();
    for (int b = 0; b < B_; ++b) {
      flags_[(size_t)b] = optimizer::SolverFlag::kFactorizationFailed;
      errors_[(size_t)b] = tick_error_;
      stats_[(size_t)b] = TrajectoryOptimizerStats<double>();
    }
    return false;
  }
  if (rc != 0 && rc != IDTO_HIP_FACTORIZATION_FAILED) throw std::runtime_error(std::string("idto_hip_mpc_batch_replan: ") + idto_hip_last_error());
  const double total = std::chrono::duration<double>(clock::now() - start).count();
  for (int b = 0; b < B_; ++b) {
    RowsFromFlat(guess_.data() + b * nqa, n, nq_, &guesses_[(size_t)b]);
    stats_[(size_t)b] = TrajectoryOptimizerStats<double>();
    errors_[(size_t)b].clear();
    optimizer::internal::BatchRowsResult r;
    optimizer::internal::RowsToStats(rows_.data() + (size_t)b * iters * IDTO_TR_ROW, iters, Delta_out_[(size_t)b], total, optimizer_->params(),
                                     &stats_[(size_t)b], &r);
    // (the device kept this controller's plan exactly when its status carries one of these bits: mpc_store_kernel)
    if ((status_[(size_t)b] & (1 | 2 | 4 | 8 | 32)) != 0) {
      flags_[(size_t)b] = optimizer::SolverFlag::kFactorizationFailed;
      errors_[(size_t)b] = !r.error.empty() ? r.error
                           : (status_[(size_t)b] & 8) ? std::string("singular constraint Schur complement: the batch loop has no host loop to finish in")
                                                      : std::string("idto_hip: the re-plan failed (status ") + std::to_string(status_[(size_t)b]) + ")";
      continue;
    }
    flags_[(size_t)b] = r.flag;
    Delta_[(size_t)b] = r.Delta;
    TrajectoryOptimizerSolution<double>& sol = solutions_[(size_t)b];
    RowsFromFlat(q_.data() + b * nqa, n, nq_, &sol.q);
    RowsFromFlat(v_.data() + b * nva, n, nv_, &sol.v);
    RowsFromFlat(tau_.data() + b * nta, N_, nv_, &sol.tau);
    AdoptPlan(b, plans_.data() + b * len);
  }
  idto_hip_trace_mark("mpc batch: plans adopted");
  return true;
}

// Interpolator::SendState / SendControl (:163-178)
VectorXd Interpolator::State(const StoredTrajectory& traj, double time) {
  VectorXd x = traj.q.value(time - traj.start_time);
  const VectorXd v = traj.v.value(time - traj.start_time);
  x.insert(x.end(), v.begin(), v.end());
  return x;
}
VectorXd Interpolator::Control(const StoredTrajectory& traj, double time) { return traj.u.value(time - traj.start_time); }

}  // namespace mpc
}  // namespace examples
}  // namespace idto
