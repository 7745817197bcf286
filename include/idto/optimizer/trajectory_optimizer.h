// trajectory_optimizer.h — idto::optimizer::TrajectoryOptimizer<double> on MI355X.
//
// Mirrors the public API of reference optimizer/trajectory_optimizer.h:41-483 (same method
// names, argument meaning, return values and error behaviour) with the Drake handles
// replaced: the constructor takes the model tables (include/idto_model.h) and the time step
// instead of (Diagram*, MultibodyPlant*).  Every Calc* on the hot path runs in
// libidto_hip.so through the C-ABI of include/idto_hip.h:
//
//   CalcCacheTrajectoryData (TO.cc:1463-1480)            -> idto_hip_eval_tau
//   CalcInverseDynamicsPartials (:400-563)               -> idto_hip_eval_partials
//   CalcGradient / CalcHessian (:1021-1165)              -> idto_hip_grad_hess
//   SolveLinearSystemInPlace (:2077-2096), H^-1 J^T of
//   CalcLagrangeMultipliers (:1371-1396)                 -> idto_hip_solve_host
//
// and only the O(num_vars) outer-loop numerics (scaling :1181-1255, equality constraints
// :1267-1456, dogleg :2108-2202, trust ratio :1979-2035, convergence :2653-2689, the
// trust-region loop :2449-2651) run on the host.  There is no CPU implementation of the hot
// path: construction throws std::runtime_error if no HIP device is available.
//
// Differences from the reference, reported through exceptions in the constructor: gradients_method must
// be one of the finite-difference methods (forward, central, central4; kAutoDiff needs Drake's AutoDiffXd
// plant, reference TO.cc:410-423 has the same kind of runtime check), exact_hessian is not supported
// (it needs autodiff as well).  Every other field of SolverParameters is honoured: linear_solver =
// kDenseLdlt routes SolveLinearSystemInPlace (:2088-2093) to a dense LDL^T of MakeDense() on the device
// (idto_hip_solve_dense_ldlt), debug_compare_against_dense prints the reference's "Sparse vs. Dense error"
// per dogleg point (:2142-2150), print_debug_data its condition numbers (:2349-2365, :2499-2507); these
// three take the stepwise loop (one synchronisation per quantity), not the device-resident one.
// The plotting dumps (save_contour_data, save_lineplot_data, linesearch_plot_every_iteration: CSV files for
// the 2-DoF toy examples' figures, TO.cc:1650-1830) are not produced: the constructor throws if one is set.
#pragma once

#include <chrono>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "idto/optimizer/penta_diagonal_matrix.h"
#include "idto/optimizer/problem_definition.h"
#include "idto/optimizer/scene_report.h"
#include "idto/optimizer/solver_parameters.h"
#include "idto/optimizer/trajectory_optimizer_solution.h"
#include "idto/optimizer/trajectory_optimizer_state.h"
#include "idto/optimizer/tracking.h"
#include "idto/optimizer/tvlqr.h"
#include "idto/optimizer/warm_start.h"
#include "idto_hip.h"

namespace idto {
namespace optimizer {

namespace internal {
// S x = b for the symmetric positive (semi-)definite Schur complement of the multipliers
// (column-major, lower triangle read, overwritten): LDL^T with diagonal pivoting (TO.cc:1395).
void DenseLdltSolve(std::vector<double>* S, int n, double* b);
enum class RowsOutcome;   // how a device loop's statistics rows ended (csrc/host/batch_rows.h)
}  // namespace internal

template <typename T>
class TrajectoryOptimizer;

template <>
class TrajectoryOptimizer<double> {
 public:
  using T = double;
  // `model` is copied into the device context; it need not outlive the optimizer.
  TrajectoryOptimizer(const idto_model_t& model, double time_step, const ProblemDefinition& prob,
                      const SolverParameters& params = SolverParameters{}, int device = 0);
  // Several devices of one node (the counterpart of the reference's `num_threads`, which
  // parallelises CalcInverseDynamicsPartialsFiniteDiff over timesteps with OpenMP,
  // optimizer/trajectory_optimizer.cc:455-457, :476): devices[0] hosts the optimizer as above, the
  // others hold a copy of the problem and evaluate their k-range of the finite-difference grid;
  // one RCCL all-gather per evaluation of the partials completes dtau/dq on every device
  // (idto_hip_comm_init_all / idto_hip_eval_partials_multi of include/idto_hip.h; no torch, no MPI).
  TrajectoryOptimizer(const idto_model_t& model, double time_step, const ProblemDefinition& prob,
                      const SolverParameters& params, const std::vector<int>& devices);
  ~TrajectoryOptimizer();
  TrajectoryOptimizer(const TrajectoryOptimizer&) = delete;
  TrajectoryOptimizer& operator=(const TrajectoryOptimizer&) = delete;

  double time_step() const { return time_step_; }
  int num_steps() const { return prob_.num_steps; }
  int num_positions() const { return nq_; }
  int num_velocities() const { return nv_; }
  const std::vector<int>& unactuated_dofs() const { return unactuated_dofs_; }
  int num_equality_constraints() const { return (int)unactuated_dofs_.size() * num_steps(); }
  const SolverParameters& params() const { return params_; }
  const ProblemDefinition& prob() const { return prob_; }

  TrajectoryOptimizerState<T> CreateState() const { return TrajectoryOptimizerState<T>(num_steps(), nq_); }
  std::unique_ptr<WarmStart> CreateWarmStart(const std::vector<VectorXd>& q_guess) const {
    return std::make_unique<WarmStart>(num_steps(), nq_, q_guess, params_.Delta0);
  }

  void CalcGradient(const TrajectoryOptimizerState<T>& state, VectorXd* g) const { *g = EvalGradient(state); }
  void CalcHessian(const TrajectoryOptimizerState<T>& state, PentaDiagonalMatrix<T>* H) const { *H = EvalHessian(state); }

  SolverFlag Solve(const std::vector<VectorXd>& q_guess, TrajectoryOptimizerSolution<T>* solution,
                   TrajectoryOptimizerStats<T>* stats, ConvergenceReason* reason = nullptr) const;
  SolverFlag SolveFromWarmStart(WarmStart* warm_start, TrajectoryOptimizerSolution<T>* solution,
                                TrajectoryOptimizerStats<T>* stats, ConvergenceReason* reason = nullptr) const;

  // Several problems of this optimizer's model, horizon, SolverParameters and contact parameters at once (no counterpart in
  // the reference, whose caller loops over Solve): what a sampling-based planner, a multi-start on a non-convex contact
  // problem or an MPC server with several warm-started problems per tick asks for.
  struct BatchSolveResult {
    std::vector<TrajectoryOptimizerSolution<T>> solutions;   // [B]; only_best: only solutions[best] is filled
    std::vector<TrajectoryOptimizerStats<T>> stats;          // [B]
    std::vector<SolverFlag> flags;                           // [B]; meaningful where errors[b] is empty or names a failed factorisation
    std::vector<std::string> errors;                         // [B]; non-empty: entry b has no solution, and this says why
    std::vector<double> final_costs;                         // [B]; the cost of entry b's final iterate (NaN: none)
    int best = -1;   // the entry of the lowest final cost among those that ended kSuccess / kMaxIterationsReached with a
                     // finite cost, the lowest index among equals; -1: none
  };
  // Entry b is Solve(q_guesses[b]) on an optimizer constructed with (*problems)[b] (null: this optimizer's own problem for
  // every entry) from a fresh state: Delta = Delta0, the adaptive scalings' memory ones.  One entry's failure is its own
  // flags[b] / errors[b].  Configurations the device's batch loop serves (trust region, one device, the device-resident
  // loop, diagonal cost weights, no adaptive scaling, verbose off, enforced constraints through the banded KKT step) run as
  // ONE loop for all entries with one wait for everything that comes back (idto_hip_tr_solve_batch_fetch) on a batch context
  // created on first use and kept per B.  method = kLinesearch takes the device's batch linesearch loop the same way
  // (idto_hip_ls_solve_batch_fetch, one wait) where the single problem takes the device's linesearch loop - scaling off, no
  // enforced constraints, the banded solver, no debug switches, max_linesearch_iterations <= 64 - with B >= 2, one device,
  // verbose off and diagonal weights in every entry; an entry whose backtracking stays undecided within the device's
  // candidates is solved again alone, a loop time-out sends every entry there.  Every other configuration runs the entries one after another on this
  // optimizer's own context, with the same result layout.  A batch of more than two small models (blocks up to 4) takes
  // the block solver kernels where one problem alone takes the scalar band kernels: the entries then agree with Solve to
  // the solver's round-off, otherwise bit for bit.
  // Throws, before any device work, when q_guesses and problems disagree in length or a problem's num_steps / vector
  // sizes differ from this optimizer's.
  void SolveBatch(const std::vector<std::vector<VectorXd>>& q_guesses, const std::vector<ProblemDefinition>* problems,
                  BatchSolveResult* out, bool only_best = false) const;
  // The same with a model and contact parameters per entry (each vector empty or of B entries, an entry nullptr: the
  // optimizer's own): entry b is Solve(q_guesses[b]) on an optimizer constructed with entry b's model, contact
  // parameters and problem.  The models share the optimizer's topology - sizes, tree, joint and geometry types, pairs
  // and paths, actuated mask, gravity switches - and may differ in the double tables, gravity and the five contact
  // parameters (include/idto_hip.h idto_hip_set_model_batch).  Such a batch has NO entry-by-entry route - this
  // optimizer's own context holds its own model -: std::invalid_argument, before any device work, names what the two
  // batch loops do not serve (BatchLoopRefusal's list for the trust region, the linesearch loop's conditions above), B < 2
  // or the table in which a model differs from the optimizer's; an entry the loop leaves to the host loop is reported in
  // its own flags[b] / errors[b], and a loop time-out on a shared device is a std::runtime_error.  last_batch_route() is 1.
  void SolveBatch(const std::vector<std::vector<VectorXd>>& q_guesses, const std::vector<ProblemDefinition>* problems,
                  const std::vector<const idto_model_t*>& models, const std::vector<const idto_contact_params_t*>& contacts,
                  BatchSolveResult* out, bool only_best = false) const;
  // how the last SolveBatch ran: 1 a batch loop of the device (trust region or linesearch), 0 entry by entry (tests and tools/solve_batch_bench.py ask)
  int last_batch_route() const { return last_batch_route_; }

  // ---- what examples::mpc::BatchModelPredictiveController (mpc_controller.h) builds on: the device's batch loop for B
  // problems of this optimizer on a batch context of the caller's own.
  // Why B controllers with these problems cannot take the batch loop - the name of the configuration it does not serve
  // (SolveBatch's rule, without its entry-by-entry fallback) - or "" when they can.  No device work.
  std::string BatchLoopRefusal(int B, const std::vector<const ProblemDefinition*>& probs) const;
  // A batch context for `probs` (one entry per problem; SolveBatch's stays its own).  The caller destroys it: idto_hip_destroy.
  idto_hip_ctx* CreateBatchContext(const std::vector<const ProblemDefinition*>& probs) const;
  // What SolveBatch sets on a batch context in front of the loop (the |h| column's degrees of freedom, the convergence
  // criteria), done for `ctx`, and the arguments it hands idto_hip_tr_solve_batch_fetch.
  struct BatchLoopArgs {
    int iterations, scaling_method, scaling, normalize_quaternions;
    double Delta_max, eta;
    const int* constrained_dofs;   // (this optimizer's storage)
    int nu;
  };
  BatchLoopArgs PrepareBatchLoop(idto_hip_ctx* ctx) const;

  const std::vector<VectorXd>& EvalV(const TrajectoryOptimizerState<T>& state) const;
  const std::vector<VectorXd>& EvalA(const TrajectoryOptimizerState<T>& state) const;
  const std::vector<VectorXd>& EvalTau(const TrajectoryOptimizerState<T>& state) const;
  const std::vector<MatrixXd>& EvalNplus(const TrajectoryOptimizerState<T>& state) const;
  const VelocityPartials<T>& EvalVelocityPartials(const TrajectoryOptimizerState<T>& state) const;
  const InverseDynamicsPartials<T>& EvalInverseDynamicsPartials(const TrajectoryOptimizerState<T>& state) const;
  T EvalCost(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalGradient(const TrajectoryOptimizerState<T>& state) const;
  const PentaDiagonalMatrix<T>& EvalHessian(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalScaleFactors(const TrajectoryOptimizerState<T>& state) const;
  const PentaDiagonalMatrix<T>& EvalScaledHessian(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalScaledGradient(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalEqualityConstraintViolations(const TrajectoryOptimizerState<T>& state) const;
  const MatrixXd& EvalEqualityConstraintJacobian(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalLagrangeMultipliers(const TrajectoryOptimizerState<T>& state) const;
  T EvalMeritFunction(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalMeritFunctionGradient(const TrajectoryOptimizerState<T>& state) const;

  void ResetInitialConditions(const VectorXd& q_init, const VectorXd& v_init);
  void UpdateNominalTrajectory(const std::vector<VectorXd>& q_nom, const std::vector<VectorXd>& v_nom);

  // pieces of the iteration the reference's tests reach through TrajectoryOptimizerTester
  // (optimizer/test/trajectory_optimizer_test.cc:31-89)
  bool CalcDoglegPoint(const TrajectoryOptimizerState<T>& state, double Delta, VectorXd* dq, VectorXd* dqH) const;
  T CalcTrustRatio(const TrajectoryOptimizerState<T>& state, const VectorXd& dq,
                   TrajectoryOptimizerState<T>* scratch_state) const;

  idto_hip_ctx* device_context() const { return dev(); }

  // The local model of the plant about given states (idto/optimizer/tvlqr.h, include/idto_hip.h idto_hip_plant_linearize):
  // x+ ~ f(x_s, tau_s) + A_s dx + B_s du for the map f of `substeps` substeps of h under the held torque tau[s] (all nv
  // components), with this optimizer's model and contact parameters, in tangent coordinates.  One pass of the device, one wait.
  PlantLinearization LinearizePlant(const std::vector<VectorXd>& q, const std::vector<VectorXd>& v, const std::vector<VectorXd>& tau,
                                    double h, int substeps) const;
  // The time-varying LQR gains about a solution: the states (q_t, v_t), t = 0 ... N - 1, the held torque solution.tau[t], the map
  // of one time step in substeps of h (time_step / h must be a whole number to 1e-9: std::invalid_argument otherwise), the
  // weights Q = blkdiag(Qtheta, Qv), R [nu x nu] and Qf = blkdiag(Qf_theta, Qf_v) in tangent coordinates, time-invariant; the
  // controls are the model's actuated dofs (actuated_dofs(): every dof of a model without an actuator).  K[t] (nu x n) gives
  // u = solution.tau[t][actuated] - K[t] [q (-) q_t; v - v_t]; P[t], t = 0 ... N, is the cost-to-go.
  TvlqrGains Tvlqr(const TrajectoryOptimizerSolution<T>& solution, double h, const MatrixXd& Qtheta, const MatrixXd& Qv, const MatrixXd& R,
                   const MatrixXd& Qf_theta, const MatrixXd& Qf_v) const;
  std::vector<int> actuated_dofs() const;
  // Tvlqr's gains about a solution, and on the device behind them one rollout per entry of x0s ([q; v] each) under
  // u_t = tau*_t[actuated] - K_t [q (-) q_t; v - v_t] held over a time step, tau* = solution.tau[t] (with zero_unactuated: zero on the
  // unactuated dofs, where a solution carries the constraint's residual), against the states (q_t, v_t), t = 0 ... N: one pass of
  // the device, one wait (idto/optimizer/tracking.h, include/idto_hip.h idto_hip_plant_tvlqr_track).  time_step / h as in Tvlqr.
  TrackedRollouts Track(const TrajectoryOptimizerSolution<T>& solution, double h, const MatrixXd& Qtheta, const MatrixXd& Qv, const MatrixXd& R,
                        const MatrixXd& Qf_theta, const MatrixXd& Qf_v, const std::vector<VectorXd>& x0s, bool zero_unactuated = false) const;

  // What replaces the reference's EvalPlantContext(state, t) (optimizer/trajectory_optimizer.h:452): body poses and spatial
  // velocities, per-pair signed distances, witness points and contact forces, and the generalised force of contact at the
  // states (q[t], v[t]) - every t in ONE launch of the device and one wait (idto/optimizer/scene_report.h, include/idto_hip.h
  // idto_hip_scene_report).  The contact inside solution.tau[t] is -tau_contact of state t + 1.
  SceneReport EvalScene(const std::vector<VectorXd>& q, const std::vector<VectorXd>& v, bool pair_rows = false) const;
  SceneReport EvalScene(const TrajectoryOptimizerSolution<T>& solution, bool pair_rows = false) const {
    return EvalScene(solution.q, solution.v, pair_rows);
  }

 private:
  int num_vars() const { return (num_steps() + 1) * nq_; }
  void UploadProblem() const;
  void UploadProblemDefinition(const ProblemDefinition& prob) const;   // `prob` onto this optimizer's context(s)
  // SolveBatch: the batch context of a given B with the host buffers of its calls (allocated once per B)
  struct BatchContext {
    idto_hip_ctx* ctx = nullptr;
    std::vector<double> q, rows, Delta0, Delta_out, sol_q, sol_v, sol_tau, final_cost, q_nom, v_nom;
    std::vector<int> status;
  };
  // SolveBatch's per-entry models and contact parameters ([B] each, nullptr: the optimizer's own)
  struct BatchPhysics { std::vector<const idto_model_t*> models; std::vector<const idto_contact_params_t*> contacts; };
  // (physics != nullptr: a context of its own per B, its parameter records uploaded per call as its problems are)
  BatchContext* GetBatchContext(int B, const std::vector<const ProblemDefinition*>& probs, const BatchPhysics* physics = nullptr) const;
  void SolveBatchImpl(const std::vector<std::vector<VectorXd>>& q_guesses, const std::vector<ProblemDefinition>* problems,
                      const BatchPhysics* physics, BatchSolveResult* out, bool only_best) const;
  // the two batch loops' shared steps: the guesses into bc->q, and entry b of a loop that ran into `out` (its outcome as the
  // rows unit reports it; slot: where its solution lies in bc's arrays, -1: not fetched; an entry left to the host loop is
  // marked in `alone`, or fails by name when per-entry models leave no context to run it on)
  void PackGuesses(BatchContext* bc, const std::vector<std::vector<VectorXd>>& q_guesses) const;
  void TakeEntry(int b, int slot, internal::RowsOutcome outcome, SolverFlag flag, const std::string& error, const BatchContext& bc,
                 const BatchPhysics* physics, BatchSolveResult* out, std::vector<char>* alone) const;
  std::string LinesearchBatchRefusal(int B, const std::vector<const ProblemDefinition*>& probs) const;
  void CheckBatchProblem(const ProblemDefinition& p, int b) const;
  // entry b of a batch solved alone on this optimizer's own context (the fallback of SolveBatch)
  void SolveBatchEntryAlone(const ProblemDefinition* prob, const std::vector<VectorXd>& q_guess, int b, BatchSolveResult* out) const;
  // the context, with the problem data on the device up to date (ResetInitialConditions / UpdateNominalTrajectory only
  // mark them: an MPC re-plan calls both, examples/mpc_controller.cc:60-75, and pays for one upload)
  idto_hip_ctx* dev() const { if (problem_dirty_) UploadProblem(); return hip_; }
  // makes the device hold `state`: level 0 q, 1 + tau/cost, 2 + dtau/dq, 3 + gradient/Hessian
  void EnsureDevice(const TrajectoryOptimizerState<T>& state, int level) const;
  std::vector<double> Fetch(int what) const;
  void CalcTrajectoryData(const TrajectoryOptimizerState<T>& state) const;   // tau, cost
  void CalcKinematics(const TrajectoryOptimizerState<T>& state) const;       // v, a, N+
  void CalcVelocityPartials(const TrajectoryOptimizerState<T>& state) const;
  void CalcDerivatives(const TrajectoryOptimizerState<T>& state) const;
  void CalcGradHess(const TrajectoryOptimizerState<T>& state) const;
  const VectorXd& EvalHinvMeritGradient(const TrajectoryOptimizerState<T>& state) const;
  // SolveLinearSystemInPlace (TO.cc:2077-2096) for the Hessian of `state`: params().linear_solver (solver < 0), the
  // dense LDL^T (0) or the block Thomas algorithm (1)
  bool DenseLinearSolver() const;
  void SolveLinearSystem(const TrajectoryOptimizerState<T>& state, const VectorXd& b, VectorXd* x, int solver = -1) const;
  double DebugConditionNumber(const TrajectoryOptimizerState<T>& state, bool scaled) const;
  void NormalizeQuaternions(TrajectoryOptimizerState<T>* state) const;
  std::pair<double, int> ArmijoLinesearch(const TrajectoryOptimizerState<T>& state, const VectorXd& dq,
                                          TrajectoryOptimizerState<T>* scratch) const;
  std::pair<double, int> BacktrackingLinesearch(const TrajectoryOptimizerState<T>& state, const VectorXd& dq,
                                                TrajectoryOptimizerState<T>* scratch) const;
  SolverFlag SolveWithLinesearch(const std::vector<VectorXd>& q_guess, TrajectoryOptimizerSolution<T>* solution,
                                 TrajectoryOptimizerStats<T>* stats) const;
  SolverFlag SolveFromWarmStartImpl(WarmStart* warm_start, TrajectoryOptimizerSolution<T>* solution,
                                    TrajectoryOptimizerStats<T>* stats, ConvergenceReason* reason) const;
  bool LinesearchLoopEligible() const;
  SolverFlag SolveLinesearchOnDevice(const std::vector<VectorXd>& q_guess, TrajectoryOptimizerSolution<T>* solution,
                                     TrajectoryOptimizerStats<T>* stats) const;
  bool DeviceLoopEligible() const;
  bool ResidentLoopEligible() const;
  // SolveOnDevice: prologue (q, first evaluation), ResidentPhase (every iteration enqueued at once), StepwisePhase (two
  // returns to the host per iteration: IDTO_OPT_STEPWISE, or what a truncated resident run left over), epilogue (the
  // solution's arrays).  What crosses between them:
  struct DeviceLoop {
    std::chrono::high_resolution_clock::time_point start;
    int k = 0;                    // iterations completed
    double cost = 0.0;            // L(q_k) (the stepwise phase's; the resident loop keeps it on the device)
    bool last_accepted = true, converged = false;
    bool fetched = false;         // q, v, tau, dq, w are the final iterate's, brought along by idto_hip_tr_solve_fetch
    std::vector<double> q, v, tau, dq, w;
    SolverFlag handed_over = SolverFlag::kSuccess;   // ResidentPhase returned true: what the host loop made of the rest
  };
  bool ResidentPhase(WarmStart* warm_start, const BatchLoopArgs& args, TrajectoryOptimizerSolution<T>* solution,
                     TrajectoryOptimizerStats<T>* stats, ConvergenceReason* reason, DeviceLoop* loop) const;
  void StepwisePhase(const BatchLoopArgs& args, double* Delta, TrajectoryOptimizerStats<T>* stats, DeviceLoop* loop) const;
  SolverFlag SolveOnDevice(WarmStart* warm_start, TrajectoryOptimizerSolution<T>* solution,
                           TrajectoryOptimizerStats<T>* stats, ConvergenceReason* reason) const;
  // what the device's trust-region loops are told, in one place
  bool AdaptiveScaling() const {
    return params_.scaling && (params_.scaling_method == kAdaptiveSqrt || params_.scaling_method == kAdaptiveDoubleSqrt);
  }
  bool Constrained() const { return params_.equality_constraints && num_equality_constraints() > 0; }
  BatchLoopArgs LoopArgs() const;
  void SetConvergence(idto_hip_ctx* ctx) const;   // VerifyConvergenceCriteria's tolerances, or none (check_convergence off)
  void InvalidateDevice() const { resident_ = nullptr; device_level_ = 0; }   // no state's results are on the device any more
  void AdoptTrialPoint(const TrajectoryOptimizerState<T>& scratch, TrajectoryOptimizerState<T>* state) const;
  ConvergenceReason VerifyConvergenceCriteria(const TrajectoryOptimizerState<T>& state, T previous_cost,
                                              const VectorXd& dq) const;
  void Check(int rc) const;

  double time_step_;
  int nq_ = 0, nv_ = 0;
  ProblemDefinition prob_;
  const SolverParameters params_;
  std::vector<int> unactuated_dofs_;
  std::vector<int> quaternion_starts_;
  idto_hip_ctx* hip_ = nullptr;
  std::vector<idto_hip_ctx*> shard_ctx_;    // [hip_, contexts on the other devices] when sharded over devices
  mutable bool problem_dirty_ = false;      // prob_ changed since the last upload
  mutable const void* resident_ = nullptr;  // state whose q is on the device
  mutable int device_level_ = 0;            // what has been evaluated for it there
  // the device-resident loop met a singular constraint Schur complement at iteration resume_k_: the
  // host loop (pivoted LDL^T) finishes the solve from that iterate
  mutable bool force_host_loop_ = false;
  mutable int resume_k_ = 0;
  mutable std::map<int, BatchContext> batch_ctx_;   // SolveBatch: per batch size (key -B: the context of a batch with per-entry models)
  mutable int last_batch_route_ = -1;
  mutable double last_sparse_vs_dense_ = -1.0;   // debug_compare_against_dense: the figure CalcDoglegPoint printed last
};

}  // namespace optimizer
}  // namespace idto
