/* idto_opt.h — C-ABI of libidto_opt.so: the host-side TrajectoryOptimizer
 * (include/idto/optimizer/trajectory_optimizer.h, C++) for bindings that cannot consume
 * C++ (ctypes, cgo, JNI ...).  One entry point per public method of the reference class
 * (optimizer/trajectory_optimizer.h:41-483) that the reference's own pybind11 module exports
 * (python_bindings/trajectory_optimizer_py.cc:34-59: constructor, time_step, num_steps, Solve,
 * SolveFromWarmStart, CreateWarmStart, ResetInitialConditions, UpdateNominalTrajectory, params,
 * prob) plus the Eval* accessors the reference's tests use.  All heavy work happens in
 * libidto_hip.so (include/idto_hip.h); return value 0 = ok, negative = failure described by
 * idto_opt_last_error(); C++ exceptions never cross this boundary. */
#ifndef IDTO_OPT_H_
#define IDTO_OPT_H_

#include "idto_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct idto_opt idto_opt;
typedef struct idto_opt_warm_start idto_opt_warm_start;

const char* idto_opt_last_error(void);

/* The small dense solve of CalcLagrangeMultipliers (optimizer/trajectory_optimizer.cc:1395,
 * Eigen ldlt()): S x = b, S symmetric positive (semi-)definite n x n column-major (lower triangle
 * read; overwritten by the factors), b overwritten by x.  Host only; exported for tests. */
int idto_opt_dense_ldlt_solve(double* S, int n, double* b);

/* TrajectoryOptimizer(diagram, plant, prob, params) (trajectory_optimizer.h:56-72) with the
 * plant replaced by model tables + time step. */
int idto_opt_create(const idto_model_t* model, const idto_problem_t* problem, const idto_contact_params_t* contact,
                    const idto_solver_params_t* params, int device, idto_opt** out);
/* The same optimizer sharded over `ndev` >= 1 devices of one node (devices[0] hosts it): the
 * finite-difference grid is split into k-ranges, one RCCL all-gather per evaluation of the
 * partials (idto_hip_comm_init_all / idto_hip_eval_partials_multi). */
int idto_opt_create_multi(const idto_model_t* model, const idto_problem_t* problem, const idto_contact_params_t* contact,
                          const idto_solver_params_t* params, const int* devices, int ndev, idto_opt** out);
void idto_opt_destroy(idto_opt* opt);

int idto_opt_num_steps(const idto_opt* opt);
double idto_opt_time_step(const idto_opt* opt);
int idto_opt_num_equality_constraints(const idto_opt* opt);

/* Solve (trajectory_optimizer.h:176-194).  q_guess: (N+1)*nq; outputs sized (N+1)*nq, (N+1)*nv,
 * N*nv.  *flag receives the SolverFlag, *reason the ConvergenceReason bitmask. */
int idto_opt_solve(idto_opt* opt, const double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                   idto_stats_t* stats, int* flag, int* reason);

/* TrajectoryOptimizer::EvalScene (what replaces the reference's EvalPlantContext; include/idto_hip.h idto_hip_scene_report,
 * whose layouts these are): the sizes - nbodies, npairs, doubles per body (18) and per pair (20), each may be NULL - and the
 * report at nstates states q[nstates][nq], v[nstates][nv], e.g. a solution's sol_q, sol_v with nstates = N + 1.  Outputs, each
 * may be NULL (not all): bodies_out[nstates][nbodies][18], pairs_out[nstates][npairs][20], tau_contact_out[nstates][nv],
 * tau_pairs_out[nstates][npairs][nv].  One launch, one wait. */
int idto_opt_scene_sizes(idto_opt* opt, int* nbodies, int* npairs, int* body_doubles, int* pair_doubles);
int idto_opt_scene_report(idto_opt* opt, int nstates, const double* q, const double* v, double* bodies_out, double* pairs_out,
                          double* tau_contact_out, double* tau_pairs_out);

/* TrajectoryOptimizer::LinearizePlant and ::Tvlqr (include/idto/optimizer/tvlqr.h; include/idto_hip.h idto_hip_plant_linearize,
 * idto_hip_plant_tvlqr, whose layouts these are: matrices column-major, deviations in tangent coordinates, n = 2 nv).
 * idto_opt_actuated_dofs: the velocity indices of the controls, actuated_out[nv] filled from the front (may be NULL); returns nu.
 * idto_opt_plant_linearize: about nstates states q[nstates][nq], v[nstates][nv] under the held torques tau[nstates][nv], the map
 * of `substeps` substeps of h; outputs, each may be NULL: x_next_out[nstates][nq + nv], A_out[nstates][n * n],
 * B_out[nstates][n * nv], status_out[nstates][2].
 * idto_opt_tvlqr: about a solution's (sol_q[t], sol_v[t]), t = 0 ... N - 1, under sol_tau[t], the map of one time step in
 * substeps of h (time_step / h a whole number to 1e-9, or the call fails); Qtheta, Qv, Qf_theta, Qf_v [nv * nv] and R [nu * nu]
 * symmetric; outputs, each may be NULL: idto_opt_plant_linearize's with nstates = N, K_out[N][nu * n], P_out[N + 1][n * n],
 * *lqr_status_out (0, or 1 + t: K and P from t downward are NaN). */
int idto_opt_actuated_dofs(idto_opt* opt, int* actuated_out);
int idto_opt_plant_linearize(idto_opt* opt, int nstates, const double* q, const double* v, const double* tau, double h, int substeps,
                             double* x_next_out, double* A_out, double* B_out, int* status_out);
int idto_opt_tvlqr(idto_opt* opt, const double* sol_q, const double* sol_v, const double* sol_tau, double h, const double* Qtheta,
                   const double* Qv, const double* R, const double* Qf_theta, const double* Qf_v, double* x_next_out, double* A_out,
                   double* B_out, int* status_out, double* K_out, double* P_out, int* lqr_status_out);

/* TrajectoryOptimizer::Track (include/idto/optimizer/tracking.h; include/idto_hip.h idto_hip_plant_tvlqr_track, whose layouts these
 * are): idto_opt_tvlqr's gains about the solution, and behind them on the device nrollouts rollouts from x0[nrollouts][nq + nv] under
 * u_t = sol_tau[t][actuated] - K_t [q (-) sol_q[t]; v - sol_v[t]], held over a time step; zero_unactuated != 0 zeroes sol_tau on the
 * unactuated dofs first.  Outputs, each may be NULL: idto_opt_tvlqr's, then x_out[nrollouts][N][nq + nv], u_out[nrollouts][N][nu],
 * dx_out[nrollouts][N + 1][n], track_status_out[nrollouts][2] ({code, substeps completed}). */
int idto_opt_track(idto_opt* opt, const double* sol_q, const double* sol_v, const double* sol_tau, double h, const double* Qtheta,
                   const double* Qv, const double* R, const double* Qf_theta, const double* Qf_v, int nrollouts, const double* x0,
                   int zero_unactuated, double* x_next_out, double* A_out, double* B_out, int* status_out, double* K_out, double* P_out,
                   int* lqr_status_out, double* x_out, double* u_out, double* dx_out, int* track_status_out);

/* TrajectoryOptimizer::SolveBatch (include/idto/optimizer/trajectory_optimizer.h): B problems of the optimizer's model,
 * horizon, solver and contact parameters; entry b is idto_opt_solve of q_guesses[b] on an optimizer created with problems[b]
 * (NULL: the optimizer's own problem for every entry).  q_guesses: [B][(N+1)*nq]; sol_q / sol_v / sol_tau: [B][...] (any may
 * be NULL) - the block of an entry without a solution (it failed, or only_best != 0 and it is not the best) is left
 * untouched; stats: B blocks; flags, reasons (ConvergenceReason bitmasks), final_costs: [B] (any may be NULL); *best: the
 * entry of the lowest final cost among those that ended kSuccess / kMaxIterationsReached, -1: none.  One entry's failure is
 * its own flag (kFactorizationFailed) and text (idto_opt_batch_error, valid until the next idto_opt_solve_batch of the
 * optimizer; "" for an entry that has its solution); the call itself fails only for what concerns the whole batch: a
 * problem of another num_steps / time_step, a device error.
 * Routes: method = trust region runs the device's batch loop (idto_hip_tr_solve_batch_fetch) for what it serves; method =
 * linesearch runs the batch linesearch loop (idto_hip_ls_solve_batch_fetch: every iteration of every entry enqueued at
 * once, one wait) with scaling off, no enforced constraints, the banded solver, no debug switches,
 * max_linesearch_iterations <= 64, B >= 2, one device, verbose off and diagonal weights in every entry; everything else
 * runs entry by entry.  (The batch of MPC controllers below still does not serve method = linesearch.) */
int idto_opt_solve_batch(idto_opt* opt, int B, const idto_problem_t* problems, const double* q_guesses, int only_best,
                         double* sol_q, double* sol_v, double* sol_tau, idto_stats_t* stats, int* flags, int* reasons,
                         double* final_costs, int* best);
/* idto_opt_solve_batch with a model and contact parameters per entry: models / contacts are NULL or [B] pointers, an entry
 * NULL = the optimizer's own (both NULL: idto_opt_solve_batch).  Entry b is idto_opt_solve on an optimizer created with
 * models[b], contacts[b] and problems[b].  The models share the optimizer's topology and differ in the double tables,
 * gravity and the contact parameters (include/idto_hip.h idto_hip_set_model_batch).  Such a batch runs the device's batch
 * loops only: the call fails, before any device work and with the name in idto_opt_last_error, for B < 2, for a
 * configuration the loops do not serve, and for a model that differs in a shared table. */
int idto_opt_solve_batch_models(idto_opt* opt, int B, const idto_problem_t* problems, const idto_model_t* const* models,
                                const idto_contact_params_t* const* contacts, const double* q_guesses, int only_best,
                                double* sol_q, double* sol_v, double* sol_tau, idto_stats_t* stats, int* flags, int* reasons,
                                double* final_costs, int* best);
const char* idto_opt_batch_error(const idto_opt* opt, int b);
/* 1: the last idto_opt_solve_batch ran one of the device's batch loops (trust region or linesearch), 0: entry by entry on the optimizer's own context, -1: none yet */
int idto_opt_last_batch_route(const idto_opt* opt);

/* CreateWarmStart / SolveFromWarmStart (trajectory_optimizer.h:156-211, warm_start.h:23-76) */
int idto_opt_ws_create(idto_opt* opt, const double* q_guess, idto_opt_warm_start** out);
void idto_opt_ws_destroy(idto_opt_warm_start* ws);
int idto_opt_ws_set_q(idto_opt* opt, idto_opt_warm_start* ws, const double* q);
int idto_opt_ws_get(idto_opt* opt, idto_opt_warm_start* ws, double* q, double* Delta);
int idto_opt_ws_solve(idto_opt* opt, idto_opt_warm_start* ws, double* sol_q, double* sol_v, double* sol_tau,
                      idto_stats_t* stats, int* flag, int* reason);

/* ResetInitialConditions / UpdateNominalTrajectory (trajectory_optimizer.h:429-470) */
int idto_opt_reset_initial_conditions(idto_opt* opt, const double* q_init, const double* v_init);
int idto_opt_update_nominal_trajectory(idto_opt* opt, const double* q_nom, const double* v_nom);

/* Eval* at a given q (a fresh state is created per call): cost, gradient ((N+1)*nq),
 * lagrange multipliers (num_equality_constraints), merit; NULL outputs are skipped. */
int idto_opt_eval(idto_opt* opt, const double* q, double* cost, double* gradient, double* scaled_gradient,
                  double* scale_factors, double* lambda, double* merit, double* merit_gradient);
/* CalcDoglegPoint / CalcTrustRatio (TO.cc:2108-2202, 1979-2035) for the property tests */
int idto_opt_dogleg(idto_opt* opt, const double* q, double Delta, double* dq, double* dqH, int* active);
int idto_opt_trust_ratio(idto_opt* opt, const double* q, const double* dq, double* rho);

/* ---- the model-predictive-control shell (include/idto/examples/mpc_controller.h; reference examples/mpc_controller.h:59-214,
 * mpc_controller.cc:13-178).  The optimizer handed in is the controller's (params.max_iterations = the example's mpc_iters) and
 * must outlive it. */
typedef struct idto_mpc idto_mpc;
/* ModelPredictiveController(diagram, plant, prob, warm_start_solution, params, replan_period) (mpc_controller.cc:13-41).
 * warm_q / warm_v: (N+1)*nq, (N+1)*nv; warm_tau: N*nv; actuated: nv flags (NULL: every DoF); q_nom_relative_to_q_init: nq flags
 * (SolverParameters::q_nom_relative_to_q_init, solver_parameters.h:166; NULL: none). */
int idto_mpc_create(idto_opt* opt, const double* warm_q, const double* warm_v, const double* warm_tau, const int* actuated,
                    const int* q_nom_relative_to_q_init, double replan_period, idto_mpc** out);
void idto_mpc_destroy(idto_mpc* mpc);
int idto_mpc_num_actuators(const idto_mpc* mpc);
/* UpdateAbstractState (mpc_controller.cc:43-85): replan at `time` from the state estimate x0 = [q0; v0]; outputs (any may be
 * NULL): the initial guess that was used ((N+1)*nq), the solution, the cost of the first iteration, the solver flag. */
int idto_mpc_update(idto_mpc* mpc, double time, const double* x0, double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                    double* first_cost, int* flag);
/* Interpolator::SendState / SendControl (mpc_controller.cc:163-178) on the stored trajectory: x = [q(t); v(t)], u(t) */
int idto_mpc_state(const idto_mpc* mpc, double time, double* x);
int idto_mpc_control(const idto_mpc* mpc, double time, double* u);
double idto_mpc_start_time(const idto_mpc* mpc);
/* PiecewisePolynomial::CubicWithContinuousSecondDerivatives(breaks, knots).value(t) (host only; exported for tests): n knots of
 * `dim` components at `breaks`, evaluated at nt times (clamped to the breaks' range); out: nt*dim. */
int idto_mpc_spline_eval(const double* breaks, const double* knots, int n, int dim, const double* times, int nt, double* out);

/* the statistics of the last idto_mpc_update's solve, and the trust-region radius the next one starts from */
int idto_mpc_stats(const idto_mpc* mpc, idto_stats_t* stats, double* radius);

/* ---- B controllers of one model, horizon and parameter set whose tick is one device pass, waited for once
 * (idto::examples::mpc::BatchModelPredictiveController, include/idto/examples/mpc_controller.h; the device side:
 * include/idto_hip.h idto_hip_mpc_batch_*).  Controller b equals an idto_mpc on an optimizer of its own created with
 * problems[b].  Every controller re-plans in every tick.  idto_mpc_batch_create fails, naming the configuration, for what
 * the device's batch loop does not serve (method = linesearch, adaptive scalings, dense weights, several devices, verbose,
 * the debug switches, linear_solver = dense LDL^T, the child-context constraint route, B < 2): use B idto_mpc. */
typedef struct idto_mpc_batch idto_mpc_batch;
/* problems: [B] (NULL: the optimizer's own for every controller); warm_q / warm_v / warm_tau: [B][...] as idto_mpc_create's;
 * actuated, q_nom_relative_to_q_init: as idto_mpc_create's, shared by the controllers.  `opt` must outlive the controllers. */
int idto_mpc_batch_create(idto_opt* opt, int B, const idto_problem_t* problems, const double* warm_q, const double* warm_v,
                          const double* warm_tau, const int* actuated, const int* q_nom_relative_to_q_init, idto_mpc_batch** out);
void idto_mpc_batch_destroy(idto_mpc_batch* mpc);
int idto_mpc_batch_num_actuators(const idto_mpc_batch* mpc);
/* One tick: controller b re-plans at times[b] from x0[b] = [q0; v0] (x0: [B][nq + nv]).  Outputs (any may be NULL), [B][...]:
 * the guesses used, the solutions (a controller that failed: its previous one), stats (B blocks), flags (SolverFlag;
 * kFactorizationFailed = 2: controller b keeps its previous plan, idto_mpc_batch_error(mpc, b) says why), radii (what the
 * next tick starts from), *tick_ok (0: the loop timed out on the device, nothing of this tick counts, every plan stays;
 * idto_mpc_batch_error(mpc, -1)). */
int idto_mpc_batch_update(idto_mpc_batch* mpc, const double* times, const double* x0, double* q_guess, double* sol_q, double* sol_v,
                          double* sol_tau, idto_stats_t* stats, int* flags, double* radii, int* tick_ok);
/* Interpolator on controller b's stored trajectory (host only: the plans come back with the tick) */
int idto_mpc_batch_state(const idto_mpc_batch* mpc, int b, double time, double* x);
int idto_mpc_batch_control(const idto_mpc_batch* mpc, int b, double time, double* u);
double idto_mpc_batch_start_time(const idto_mpc_batch* mpc, int b);
int idto_mpc_batch_flag(const idto_mpc_batch* mpc, int b);
const char* idto_mpc_batch_error(const idto_mpc_batch* mpc, int b);   /* b = -1: the last tick's own */

/* csrc/mpc_spline.h on the host (exported for the tests that hold the device's kernels to it): the knot derivatives
 * m_out[n][dim] of the not-a-knot cubic through knots[n][dim] at `breaks`; and the front half of a controller's tick - the
 * guess [n][nq] from the stored q-spline (y_q, m_q) made at start_time, evaluated for the tick at `time` with row 0 = q0,
 * and q_nom[n][nq] shifted in place for the selected positions. */
int idto_mpc_spline_fit(const double* breaks, const double* knots, int n, int dim, double* m_out);
int idto_mpc_shift_reference(const double* breaks, const double* y_q, const double* m_q, int n, int nq, double start_time, double time,
                             double time_step, const double* q0, const int* selector, double* q_nom, double* guess_out);

/* ---- B plants beside the B controllers of a batch controller: BatchModelPredictiveController::BeginPlants ... TickWithPlants,
 * include/idto/examples/mpc_controller.h; the device side: include/idto_hip.h idto_hip_plant_*, idto_hip_mpc_batch_tick_plants.
 * Plant b is simulated on the device with the optimizer's own contact model at sim_time_step under the PD+ law on controller
 * b's stored plan: Kp[nu][nq], Kd[nu][nv] row-major with their sizes in doubles, feed_forward != 0 adds the plan's control. */
int idto_mpc_batch_plants_begin(idto_mpc_batch* mpc, double sim_time_step, const double* Kp, int kp_size, const double* Kd, int kd_size,
                                int feed_forward, int record_capacity);
/* plant b gets physics of its own (NULL: the controllers'); the controllers keep theirs */
int idto_mpc_batch_plants_set_model(idto_mpc_batch* mpc, int b, const idto_model_t* model, const idto_contact_params_t* contact);
int idto_mpc_batch_plants_set_states(idto_mpc_batch* mpc, const double* times, const double* x);   /* [B], [B][nq + nv] */
int idto_mpc_batch_plants_step(idto_mpc_batch* mpc, int substeps);   /* one launch, one wait */
/* plant b's time, state [q; v] and the status of its last step (0 ok, 1 failed pivot, 2 non-finite); any may be NULL */
int idto_mpc_batch_plants_state(idto_mpc_batch* mpc, int b, double* time, double* x, int* status);
/* One closed-loop tick: idto_mpc_batch_plants_step(substeps), then idto_mpc_batch_update from the plants' times and states, as
 * ONE device pass waited for once, no state crossing the bus on the way in.  Outputs: idto_mpc_batch_update's. */
int idto_mpc_batch_plants_tick(idto_mpc_batch* mpc, int substeps, double* q_guess, double* sol_q, double* sol_v, double* sol_tau,
                               idto_stats_t* stats, int* flags, double* radii, int* tick_ok);

/* ---- One plant on an optimizer's own context (idto::examples::mpc::Plants): forward dynamics a[nv] = M^-1 (tau - ID(q, v, 0)) at
 * x = [q; v] (M[nv * nv] column-major and bias[nv] may be NULL), and rollouts under a held torque: begin, set / get the state,
 * `substeps` substeps in one launch (x_record[substeps / record_every][nq + nv] and status[2] may be NULL). */
int idto_plant_forward_dynamics(idto_opt* opt, const double* x, const double* tau, double* a, double* M, double* bias);
int idto_plant_begin(idto_opt* opt, double sim_time_step, int record_capacity);
int idto_plant_set_state(idto_opt* opt, double time, const double* x);
int idto_plant_get_state(idto_opt* opt, double* time, double* x);
int idto_plant_step(idto_opt* opt, int substeps, const double* tau_hold, int record_every, double* x_record, int* status);

/* csrc/plant_step.h on the host (exported for the tests that hold the device's plant_kernel to it; include/idto_hip.h
 * idto_hip_plant_*).  idto_plant_solve_host: a = M^-1 (tau_applied - bias) by the un-pivoted LDL^T, M[n][n] column-major (its
 * lower triangle is read); returns -1, or the index of the first pivot that is not > 0 and finite.  idto_plant_pd_plus_host:
 * tau_out[nv] = the PD+ law's u (Kp[nu][nq], Kd[nu][nv] row-major; u_nom[nu] is read only with feed_forward) on the actuated
 * dofs, 0 elsewhere.  idto_plant_advance_host: one semi-implicit Euler substep in place, v += h a, q += h N(q) v, the
 * quaternions of floating joints normalised (jtype, qstart, vstart: the model's tables). */
int idto_plant_solve_host(const double* M, const double* tau_applied, const double* bias, int n, double* a_out);
void idto_plant_pd_plus_host(const double* Kp, const double* Kd, int nu, int nq, int nv, const int* actuated_dofs, const double* q,
                             const double* v, const double* q_nom, const double* v_nom, int feed_forward, const double* u_nom,
                             double* tau_out);
void idto_plant_advance_host(int nbodies, const int* jtype, const int* qstart, const int* vstart, int nq, double h, double* q,
                             double* v, const double* a);

#ifdef __cplusplus
}
#endif
#endif /* IDTO_OPT_H_ */
