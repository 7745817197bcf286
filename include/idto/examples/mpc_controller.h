// mpc_controller.h — the model-predictive-control shell around TrajectoryOptimizer<double>: the caller of the hot
// path in the reference's closed-loop examples (reference examples/mpc_controller.h:43-214, mpc_controller.cc:13-178).
//
// Same classes, names and behaviour: StoredTrajectory (q, v, u as cubic splines with continuous second
// derivatives), ModelPredictiveController::UpdateAbstractState (time-shifted initial guess from the stored solution,
// q_nom shifted for the DoFs of q_nom_relative_to_q_init, ResetInitialConditions, SolveFromWarmStart, store),
// Interpolator (x(t), u(t)).  What Drake provides is replaced: the LeafSystem ports / abstract state by plain method
// calls (the caller owns the clock), PiecewisePolynomial<double>::CubicWithContinuousSecondDerivatives by
// PiecewiseCubic below (not-a-knot end conditions - Drake's default `periodic_end_condition = false` - and, like
// PiecewisePolynomial::value, evaluation clamped to the knots' time range), plant->MakeActuationMatrix() by the
// model's actuated mask (B^T tau = the actuated components of tau).
// Every solve runs on the device through the optimizer; this shell is O(num_steps) host bookkeeping.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "idto/optimizer/trajectory_optimizer.h"

namespace idto {
namespace examples {
namespace mpc {

using optimizer::ProblemDefinition;
using optimizer::SolverParameters;
using optimizer::TrajectoryOptimizer;
using optimizer::TrajectoryOptimizerSolution;
using optimizer::TrajectoryOptimizerStats;
using optimizer::VectorXd;
using optimizer::WarmStart;

// A vector-valued cubic spline through (t_i, y_i) with continuous first and second derivatives and not-a-knot end
// conditions (the third derivative is continuous at the second and the second-to-last knot).  Three knots: the
// parabola through them; two: the line.
class PiecewiseCubic {
 public:
  PiecewiseCubic() = default;
  PiecewiseCubic(const std::vector<double>& breaks, const std::vector<VectorXd>& knots);
  // the same through the first `count` rows of `knots` / through row-major values [break][dim], into an existing object
  // (its storage is kept: no allocation when the sizes repeat)
  void Assign(const std::vector<double>& breaks, const std::vector<VectorXd>& knots, int count);
  void AssignFlat(const std::vector<double>& breaks, const double* knots, int dim);
  // values and knot derivatives [break][dim] that were fitted elsewhere (csrc/mpc_spline.h on the device: the batch controller)
  void AssignFitted(const std::vector<double>& breaks, const double* y, const double* m, int dim);
  bool empty() const { return t_.empty(); }
  double start_time() const { return t_.front(); }
  double end_time() const { return t_.back(); }
  int rows() const { return dim_; }
  // the value at t clamped to [start_time, end_time] (drake::trajectories::PiecewisePolynomial::value)
  VectorXd value(double t) const;
  void value(double t, VectorXd* out) const;   // (the same into existing storage)

 private:
  int dim_ = 0;
  std::vector<double> t_;
  std::vector<double> y_, m_;   // [knot][dim]: values and first derivatives at the knots
  std::vector<double> B_;       // work space of Fit
  void Fit(const std::vector<double>& breaks);
};

// reference examples/mpc_controller.h:43-55
struct StoredTrajectory {
  double start_time{-1.0};   // time (in seconds) at which this trajectory was generated
  PiecewiseCubic q;          // generalized positions
  PiecewiseCubic v;          // generalized velocities
  PiecewiseCubic u;          // control torques
};

// reference examples/mpc_controller.h:59-150
class ModelPredictiveController {
 public:
  // `optimizer` (not owned) solves the problem `prob` with `params` (params.max_iterations = the example's mpc_iters);
  // `actuated[j] != 0` marks the actuated velocities (all of them if empty or all zero: B = I).
  // `q_nom_relative_to_q_init`: if not empty, used instead of the optimizer's params().q_nom_relative_to_q_init (bindings
  // whose parameter struct has no room for a vector: include/idto_opt.h).
  ModelPredictiveController(TrajectoryOptimizer<double>* optimizer, const TrajectoryOptimizerSolution<double>& warm_start_solution,
                            const std::vector<int>& actuated, double replan_period,
                            const std::vector<bool>& q_nom_relative_to_q_init = {});

  double replan_period() const { return replan_period_; }
  int num_actuators() const { return nu_; }
  const StoredTrajectory& stored_trajectory() const { return stored_; }
  double trust_region_radius() const { return warm_start_->Delta; }   // what the next re-plan's loop starts from
  const TrajectoryOptimizerStats<double>& last_stats() const { return stats_; }
  const TrajectoryOptimizerSolution<double>& last_solution() const { return solution_; }
  // what the last UpdateAbstractState's SolveFromWarmStart returned; kFactorizationFailed: the stored trajectory and
  // last_solution() are still the previous re-plan's
  optimizer::SolverFlag last_flag() const { return last_flag_; }
  // the initial guess the last UpdateAbstractState used (the stored trajectory shifted to its time, row 0 = q0)
  const std::vector<VectorXd>& last_guess() const { return last_guess_; }

  // UpdateAbstractState (mpc_controller.cc:43-85) at time `time` with the state estimate x0 = [q0; v0]
  const StoredTrajectory& UpdateAbstractState(double time, const VectorXd& x0);
  // StoreOptimizerSolution (:99-138)
  void StoreOptimizerSolution(const TrajectoryOptimizerSolution<double>& solution, double start_time,
                              StoredTrajectory* stored_trajectory) const;
  // UpdateInitialGuess (:87-97)
  void UpdateInitialGuess(const StoredTrajectory& stored_trajectory, double current_time, std::vector<VectorXd>* q_guess) const;

 private:
  const double time_step_;
  const int num_steps_;   // knots: prob.num_steps + 1 (:16)
  const int nq_, nv_;
  int nu_;
  std::vector<int> actuated_dofs_;
  TrajectoryOptimizer<double>* optimizer_;
  std::unique_ptr<WarmStart> warm_start_;
  StoredTrajectory stored_;
  TrajectoryOptimizerStats<double> stats_;
  TrajectoryOptimizerSolution<double> solution_, scratch_solution_;
  mutable std::vector<double> times_, u_flat_;   // work space of StoreOptimizerSolution
  optimizer::SolverFlag last_flag_{optimizer::SolverFlag::kSuccess};
  std::vector<VectorXd> last_guess_;
  std::vector<VectorXd> guess_scratch_, q_nom_scratch_, v_nom_scratch_;   // (UpdateAbstractState's work trajectories: no allocation per re-plan)
  double replan_period_;
  std::vector<bool> selector_override_;
};

// B ModelPredictiveControllers of one model, horizon and parameter set (a parallel simulation, a multi-start MPC) whose
// whole tick - the time-shifted guesses, the shifted nominal trajectories, the new initial conditions, the warm-started
// trust-region loops and the new plans as splines - is enqueued on the device at once and waited for once
// (include/idto_hip.h idto_hip_mpc_batch_replan; csrc/mpc_batch.h).  No counterpart in the reference, whose caller would
// loop over B controllers.  Controller b's guess, solution, plan, flag, statistics and radius are those of a
// ModelPredictiveController on an optimizer of its own with problem b (bit for bit where a batch entry equals its single
// Solve: TrajectoryOptimizer::SolveBatch), because both run the arithmetic of csrc/mpc_spline.h.
//
// EVERY controller re-plans in EVERY tick.  A mask of idle controllers would need an "idle from the start" state in the
// trust-region kernels; that is out of scope here - a caller with idle controllers passes them their current time and state.
//
// What the device's batch loop does not serve makes the constructor throw std::invalid_argument with the configuration's
// name, before any device work: method = kLinesearch, the adaptive scalings, dense weights, several devices, verbose, the
// debug switches, linear_solver = kDenseLdlt, the child-context constraint route (enforced constraints with nq + nu > 30),
// B < 2.  There is no entry-by-entry fallback - one optimizer cannot hold B cumulative nominal trajectories: use B
// ModelPredictiveControllers, each on an optimizer of its own.
//
// At run time:
//   * controller b's factorisation fails (status bit 32; also a dogleg step that is not finite, bits 1 | 2, and a step that
//     is not a descent direction, bit 4): last_flag(b) == kFactorizationFailed, last_error(b) says which, and its plan,
//     last_solution(b) and radius stay the previous re-plan's - as the single controller keeps its own;
//   * controller b meets a singular constraint Schur complement (bit 8), where the single controller would finish the solve
//     in the host loop: reported as a failure of that controller in the same way; its plan stays;
//   * the loop's workgroups time out on a shared device: UpdateAll returns false, last_tick_error() says so, every
//     controller's plan, solution and radius stay, flags are kFactorizationFailed; the next tick proceeds (the context
//     has stepped down to a solver variant with fewer co-resident workgroups; if the iteration kernel itself timed out,
//     the next UpdateAll throws what idto_hip_tr_solve reports).
//
// The B controllers share ONE model and ONE set of contact parameters: a model per controller (idto_hip_set_model_batch,
// SolveBatch with models) is out of scope here.
class BatchModelPredictiveController {
 public:
  // `optimizer` (not owned; its model, horizon and parameters serve every controller), one warm-start solution per
  // controller; `problems`: one per controller (SolveBatch's rule: the optimizer's num_steps and sizes), null: the
  // optimizer's own for every controller.  `actuated`, `q_nom_relative_to_q_init`: as ModelPredictiveController's.
  BatchModelPredictiveController(TrajectoryOptimizer<double>* optimizer,
                                 const std::vector<TrajectoryOptimizerSolution<double>>& warm_start_solutions,
                                 const std::vector<int>& actuated, const std::vector<bool>& q_nom_relative_to_q_init = {},
                                 const std::vector<ProblemDefinition>* problems = nullptr);
  ~BatchModelPredictiveController();
  BatchModelPredictiveController(const BatchModelPredictiveController&) = delete;
  BatchModelPredictiveController& operator=(const BatchModelPredictiveController&) = delete;

  int num_controllers() const { return B_; }
  int num_actuators() const { return nu_; }
  // UpdateAbstractState of every controller: controller b at times[b] from the state estimate x0s[b] = [q0; v0].
  // false: the tick did not count (last_tick_error()).
  bool UpdateAll(const std::vector<double>& times, const std::vector<VectorXd>& x0s);
  bool UpdateAll(const double* times, const double* x0s);   // [B], [B][nq + nv]
  const std::string& last_tick_error() const { return tick_error_; }

  const StoredTrajectory& stored_trajectory(int b) const { return stored_[b]; }   // (Interpolator works on it as before)
  optimizer::SolverFlag last_flag(int b) const { return flags_[b]; }
  const std::string& last_error(int b) const { return errors_[b]; }
  const TrajectoryOptimizerStats<double>& last_stats(int b) const { return stats_[b]; }
  const TrajectoryOptimizerSolution<double>& last_solution(int b) const { return solutions_[b]; }
  const std::vector<VectorXd>& last_guess(int b) const { return guesses_[b]; }
  double trust_region_radius(int b) const { return Delta_[b]; }   // what the next tick starts controller b's loop from

  // ---- B plants beside the B controllers (include/idto_hip.h idto_hip_plant_*, csrc/plant.h): plant b is simulated on the
  // device with the optimizer's own contact model at `sim_time_step`, under the PD+ law of reference
  // examples/pd_plus_controller.cc on controller b's stored plan; TickWithPlants is one closed-loop tick - the substeps,
  // then every controller's re-plan from its plant's state - enqueued at once and waited for once, no state crossing the
  // bus on the way in.  Kp [nu][nq] and Kd [nu][nv] row-major (nu = num_actuators()).
  struct PlantParams {
    double sim_time_step = 1e-3;
    std::vector<double> Kp, Kd;
    bool feed_forward = false;
    int record_capacity = 0;   // states per plant that one step may record (0: the library's default)
  };
  void BeginPlants(const PlantParams& params);   // throws std::runtime_error with the library's refusal
  // plant b gets physics of its own (null: the controllers'): the rules of idto_hip_set_model_batch; the controllers keep theirs
  void SetPlantModel(int b, const idto_model_t* model, const idto_contact_params_t* contact);
  void SetPlantStates(const double* times, const double* x);   // [B], [B][nq + nv]
  void SetPlantStates(const std::vector<double>& times, const std::vector<VectorXd>& x);
  void StepPlants(int substeps);                 // one launch, one wait (the status words come back); plant_state / plant_time fetch
  // StepPlants(substeps) + UpdateAll(plant times, plant states) as one device pass; its outputs are UpdateAll's
  bool TickWithPlants(int substeps);
  const VectorXd& plant_state(int b);            // [q; v]
  double plant_time(int b);
  int plant_status(int b);                       // of the last StepPlants / TickWithPlants: 0 ok, 1 a failed pivot, 2 a non-finite state or input

 private:
  bool Tick(const double* times, const double* x0s, int substeps);
  void FetchPlants();
  bool plants_ = false, plants_stale_ = true;
  std::vector<double> plant_times_, plant_x_;
  std::vector<int> plant_status_;
  std::vector<VectorXd> plant_states_;
  void AdoptPlan(int b, const double* plan);
  TrajectoryOptimizer<double>* optimizer_;
  idto_hip_ctx* ctx_ = nullptr;             // the controllers' batch context (owned)
  TrajectoryOptimizer<double>::BatchLoopArgs loop_{};
  int B_ = 0, N_ = 0, nq_ = 0, nv_ = 0, nu_ = 0;
  std::vector<double> breaks_;
  std::vector<StoredTrajectory> stored_;
  std::vector<optimizer::SolverFlag> flags_;
  std::vector<std::string> errors_;
  std::vector<TrajectoryOptimizerStats<double>> stats_;
  std::vector<TrajectoryOptimizerSolution<double>> solutions_;
  std::vector<std::vector<VectorXd>> guesses_;
  std::vector<double> Delta_, Delta_out_, rows_, q_, v_, tau_, guess_, plans_, final_cost_, x0_;
  std::vector<int> status_;
  std::string tick_error_;
};

// Plants on any optimizer's context, without controllers: forward dynamics a = M^-1 (tau - ID(q, v, 0)) and rollouts under
// a held torque (include/idto_hip.h idto_hip_forward_dynamics, idto_hip_plant_* in hold mode), one plant per problem of the
// context - the optimizer's own context has one.  A view: it owns nothing but the plants' storage inside the context.
class Plants {
 public:
  explicit Plants(idto_hip_ctx* context);   // e.g. optimizer.device_context()
  int num_plants() const { return B_; }
  // x [B][nq + nv], tau [B][nv] -> a [B][nv]; M [B][nv * nv] column-major and bias [B][nv] may be null
  void ForwardDynamics(const double* x, const double* tau, double* a, double* M = nullptr, double* bias = nullptr);
  void Begin(double sim_time_step, int record_capacity = 0);
  void SetModel(int b, const idto_model_t* model, const idto_contact_params_t* contact);
  void SetStates(const double* times, const double* x);
  void GetStates(double* times, double* x);
  // `substeps` under tau_hold [B][nv]; x_record [B][substeps / record_every][nq + nv] and status [B][2] may be null
  void Step(int substeps, const double* tau_hold, int record_every = 0, double* x_record = nullptr, int* status = nullptr);
 private:
  idto_hip_ctx* ctx_;
  int B_;
};

// reference examples/mpc_controller.h:155-214: x(t) = [q(t); v(t)] and u(t) of a stored trajectory
struct Interpolator {
  static VectorXd State(const StoredTrajectory& traj, double time);
  static VectorXd Control(const StoredTrajectory& traj, double time);
};

}  // namespace mpc
}  // namespace examples
}  // namespace idto
