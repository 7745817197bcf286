/* idto_hip.h — C-ABI of libidto_hip.so, the MI355X (gfx950) implementation of
 * IDTO's per-iteration gradient/Hessian path.
 *
 * The reference (ToyotaResearchInstitute/idto) has no FFI layer: this path lives
 * in private C++ methods of `TrajectoryOptimizer<double>` that call Drake.  The
 * entry points below are what a binding for that path replaces, one per
 * reference routine (file:line under /root/reference):
 *
 *   idto_hip_eval_tau        CalcNplus                optimizer/trajectory_optimizer.cc:1633-1647
 *                            CalcVelocities           :178-191
 *                            CalcAccelerations        :193-202
 *                            CalcInverseDynamics      :204-226  (+ :228-245, contact :247-386)
 *                            CalcCost                 :147-176
 *   idto_hip_eval_partials   CalcInverseDynamicsPartialsFiniteDiff :426-563
 *                            CalcVelocityPartials     :962-973
 *   idto_hip_grad_hess       CalcGradient             :1021-1081
 *                            CalcHessian              :1093-1165
 *   idto_hip_factor_solve    PentaDiagonalFactorization::Factorize   optimizer/penta_diagonal_solver.h:124-197
 *                            PentaDiagonalFactorization::SolveInPlace :199-248
 *                            SolveLinearSystemInPlace optimizer/trajectory_optimizer.cc:2077-2096
 *   idto_hip_gn_step         the chain above, i.e. what the first CalcDoglegPoint after an
 *                            accepted step computes (:2108-2140) with scaling and equality
 *                            constraints off — the unit of BASELINE.json's metric.
 *
 * Data contract: fp64 everywhere; trajectories are t-major flat arrays
 * (q: (N+1)*nq, v: (N+1)*nv, a/tau: N*nv); per-timestep blocks are column-major
 * (Eigen's default), stored t-major and contiguous.  Everything stays resident
 * in HBM inside the context between calls; `idto_hip_get` copies out.
 * All functions return 0 on success and a negative code on failure
 * (`idto_hip_last_error()` describes it); nothing throws across the boundary.
 * Calls on one context must come from one thread at a time (the reference's
 * optimizer is likewise single-caller: SURVEY.md §8b "Threading").
 */
#ifndef IDTO_HIP_H_
#define IDTO_HIP_H_

#include "idto_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct idto_hip_ctx idto_hip_ctx;

enum idto_hip_array {
  IDTO_ARR_Q = 0,        /* (N+1)*nq */
  IDTO_ARR_V = 1,        /* (N+1)*nv */
  IDTO_ARR_A = 2,        /* N*nv */
  IDTO_ARR_TAU = 3,      /* N*nv */
  IDTO_ARR_NPLUS = 4,    /* (N+1) blocks nv x nq */
  IDTO_ARR_DTAU_DQM = 5, /* N blocks nv x nq ; block 0 is NaN, block 1 is 0 (inverse_dynamics_partials.h:35-42) */
  IDTO_ARR_DTAU_DQT = 6, /* N blocks ; block 0 is 0 */
  IDTO_ARR_DTAU_DQP = 7, /* N blocks */
  IDTO_ARR_GRADIENT = 8, /* (N+1)*nq */
  IDTO_ARR_H_A = 9,      /* (N+1) blocks nq x nq: two below the diagonal */
  IDTO_ARR_H_B = 10,     /* one below the diagonal */
  IDTO_ARR_H_C = 11,     /* diagonal (symmetric, both triangles filled) */
  IDTO_ARR_STEP = 12,    /* (N+1)*nq : solution of the last factor_solve / gn_step */
  IDTO_ARR_COST = 13,    /* 1 */
  IDTO_ARR_SLAB = 14,    /* N * slab_stride: per tau-index k [dtau_dqm | dtau_dqt | dtau_dqp | tau_k] — the
                            buffer a multi-GPU run all-gathers (contiguous in k) */
  IDTO_ARR_DEBUG = 15,   /* solver cycle stamps (option "solver_debug") */
  IDTO_ARR_HBANDS = 16,  /* the three Hessian bands in one copy: [A | B | C], each (N+6) blocks nq x nq
                            (N+1 used, 5 trailing zero blocks: the solver's prefetch margin) */
  IDTO_ARR_TR_DQ = 17,   /* (N+1)*nq : the step dq of the last idto_hip_tr_trial */
  IDTO_ARR_TR_W = 18,    /* (N+1)*nq : w = D^-1 H^-1 (g + J^T lambda) of the last idto_hip_tr_prepare */
  IDTO_ARR_TR_SCALE = 19, /* (N+1)*nq : scale factors D (CalcScaleFactors) */
  IDTO_ARR_CON_S = 21,      /* n_eq*n_eq + n_eq : S = J H^-1 J^T (column-major) then J H^-1 g, of the last constraint step
                               (overwritten by its factors when idto_hip_constraint_solve factorised it in place) */
  IDTO_ARR_CON_LAMBDA = 22, /* n_eq : the multipliers of the last constraint step */
  IDTO_ARR_ASM_TERMS = 20 /* N*(6 nq^2 + 3 nq (+1)) : per-record assembly products (kernels.h asm_terms_stride) */
};

const char* idto_hip_last_error(void);

/* Positive status of the entry points that synchronise after a factorisation of H
 * (idto_hip_get(IDTO_ARR_STEP), idto_hip_solve_host, idto_hip_constraint_schur / _solve / _step):
 * a pivot of the block factorisation was non-positive, non-finite or cancelled completely, i.e. H
 * is not numerically positive definite.  The reference reports this as
 * PentaDiagonalFactorizationStatus::kFailure (optimizer/penta_diagonal_solver.h:181-185) and the
 * optimizer demands success (optimizer/trajectory_optimizer.cc:2084, :2091); the host-side
 * TrajectoryOptimizer maps it to SolverFlag::kFactorizationFailed. */
#define IDTO_HIP_FACTORIZATION_FAILED 2
/* The solver variants that spread one factorisation over several workgroups (two-sided, nested dissection,
 * pipelined chains, the fused Gauss-Newton launch) need those workgroups resident at the same time.  On a
 * device shared with other kernels that is not guaranteed: every wait between workgroups is bounded (50 ms),
 * a launch whose wait ran out ends normally with this status at the next synchronisation, and the context
 * steps down to a variant with fewer co-resident workgroups (ultimately one, which cannot wait for anybody).
 * idto_hip_get(IDTO_ARR_STEP) repeats the solve itself; from the other entry points the caller repeats the
 * call.  idto_hip_get_option("solver_timeouts") counts the occurrences. */
#define IDTO_HIP_SOLVER_TIMEOUT 3

/* Creates a context on HIP device `device` for the given model, problem and
 * contact parameters (copied). */
int idto_hip_create(const idto_model_t* model, const idto_problem_t* problem,
                    const idto_contact_params_t* contact, int device, idto_hip_ctx** out);
void idto_hip_destroy(idto_hip_ctx* ctx);

/* Batch of `batch` problems of the same model, horizon and time step (different initial
 * conditions, weights, nominal and decision trajectories) resident on one device and advanced by
 * ONE launch per kernel: what a controller does that runs one Gauss-Newton iteration per control
 * tick on several warm-started problems (examples/mpc_controller.cc:43-85, BASELINE config 5), or a
 * sampling-based planner.  Every per-problem array gets a leading batch dimension; idto_hip_set_q
 * / idto_hip_get / idto_hip_set_problem address problem 0, the *_batch forms any problem;
 * idto_hip_eval_tau / eval_partials / grad_hess / factor_solve(NULL) / gn_step work on all problems
 * at once (grid.y = problem).  Entry points with explicit right-hand sides, the trial-point call
 * and the equality-constraint step serve single-problem contexts only (the host-side
 * TrajectoryOptimizer uses those).  idto_hip_create == idto_hip_create_batch(..., 1, ...).
 * The problems share ONE model and ONE set of contact parameters unless idto_hip_set_model_batch (below) gives a problem
 * its own.  What may then differ per problem: the model's double tables (X_PF, axis, mass, com, inertia, damping, geom_X,
 * geom_size), gravity[3] and all five contact parameters.  What may not: the sizes, the tree, the joint and geometry
 * types, the pairs and their paths, the actuated mask and the gravity switches - the batch's topology, by which its
 * launches are sized. */
int idto_hip_create_batch(const idto_model_t* model, const idto_problem_t* problems /* [batch] */,
                          const idto_contact_params_t* contact, int device, int batch, idto_hip_ctx** out);
int idto_hip_batch_size(idto_hip_ctx* ctx);
/* A batch context for the model, the contact parameters, the device and the "gradients_method" option of an existing
 * context (which keeps host copies of the first two): how the host-side TrajectoryOptimizer, which holds a context and
 * not the model it was made from, gets the batch behind SolveBatch. */
int idto_hip_create_batch_like(idto_hip_ctx* like, const idto_problem_t* problems /* [batch] */, int batch, idto_hip_ctx** out);
int idto_hip_set_problem_batch(idto_hip_ctx* ctx, int problem, const idto_problem_t* p);
/* Gives problem `problem` of a batch context (batch >= 2) a model and contact parameters of its own (copied; NULL: the
 * ones the context was created with).  The model is checked like any model, then against the batch's: a difference
 * outside the free tables is refused with "model of problem 2 differs from the batch's model in pair_path" (the first
 * size, table or derived scalar that differs) in the last error, before anything is enqueued.  The first successful call
 * switches the context to kernels that read every problem's model from a parameter record per problem - problems that
 * were never named hold the context's model - and option "model_batch" (read-only) reads 1 from then on; a context
 * that never gets the call runs the launches it always ran.  Such a context takes no single-workgroup step (gn_small)
 * and its constrained loop only the banded KKT route: the child-context route is refused by name.  The call waits for
 * the upload (with option "async_uploads" it goes from pinned staging, ordered on the context's stream, without a
 * wait); what the device holds of the resident q (v, a, tau, partials, cost) is stale afterwards. */
int idto_hip_set_model_batch(idto_hip_ctx* ctx, int problem, const idto_model_t* model, const idto_contact_params_t* contact);
/* The check of idto_hip_set_model_batch alone, against the model of any context (a single-problem one included), with
 * `problem` only the number the refusal names: no device work.  How a caller that builds its batch context later - the
 * host-side TrajectoryOptimizer's SolveBatch - refuses a batch before it creates or uploads anything. */
int idto_hip_check_model_batch(idto_hip_ctx* ctx, int problem, const idto_model_t* model, const idto_contact_params_t* contact);
int idto_hip_set_q_batch(idto_hip_ctx* ctx, const double* q_host /* [batch][(N+1)*nq] */);
int idto_hip_gn_step_batch(idto_hip_ctx* ctx); /* = idto_hip_gn_step: every problem of the batch */
int idto_hip_get_batch(idto_hip_ctx* ctx, int what, int problem, double* host_out);
/* Several arrays with ONE synchronisation: the copies are enqueued side by side into pinned staging memory (what a
 * caller that wants the solution of a solve - q, v, tau, the step - pays for is one wait, not one per array; reference:
 * the fields TrajectoryOptimizer<T>::SolveFromWarmStart hands back, trajectory_optimizer.cc:2627-2650).  Not for
 * IDTO_ARR_STEP (whose idto_hip_get also reports the factorisation's status). */
int idto_hip_get_many(idto_hip_ctx* ctx, int n, const int* what, double* const* host_out);
int idto_hip_solver_status_batch(idto_hip_ctx* ctx, int* failed /* [batch] */);

/* Replaces q_init/v_init/weights/q_nom/v_nom (ResetInitialConditions /
 * UpdateNominalTrajectory, reference trajectory_optimizer.h:429-470). num_steps and
 * time_step must not change. */
int idto_hip_set_problem(idto_hip_ctx* ctx, const idto_problem_t* problem);

/* All work of the context is enqueued on this hipStream_t (default: a private stream). */
int idto_hip_set_stream(idto_hip_ctx* ctx, void* hip_stream);
void* idto_hip_get_stream(idto_hip_ctx* ctx);

/* Restricts eval_partials to tau-indices k in [k_begin, k_end) (multi-GPU t-range
 * sharding); the caller all-gathers IDTO_ARR_SLAB before grad_hess. */
int idto_hip_set_shard(idto_hip_ctx* ctx, int k_begin, int k_end);

/* Multi-GPU iteration (the reference parallelises the same loop over timesteps with
 * OpenMP, optimizer/trajectory_optimizer.cc:455-457, :476): every GPU holds the whole problem, its
 * finite-difference kernel covers a contiguous k-range of the (k, column) perturbation grid, ONE
 * RCCL all-gather (in place: a rank's records already sit at their final offset of the slab)
 * completes dtau/dq on every GPU, and every GPU assembles and solves redundantly - identical
 * bits on all ranks, no second collective.  Two ways to form the communicator:
 *   one process per GPU:  rank 0 calls idto_hip_comm_unique_id and ships the 128 bytes to the
 *     other ranks by any means (MPI, a file, torch.distributed's store); every rank then calls
 *     idto_hip_comm_init(ctx, id, rank, world) - collective, like ncclCommInitRank;
 *   one process, several devices:  idto_hip_comm_init_all(ctxs, n) with one context per device,
 *     then idto_hip_gn_step_multi(ctxs, n).
 * Both set the context's shard to its rank's k-range.  idto_hip_gn_step_sharded =
 * eval_partials (own range) + idto_hip_allgather_slab + grad_hess + factor_solve, all enqueued on
 * the context's stream. */
int idto_hip_comm_unique_id(char* id_out, int bytes /* >= 128 */);
/* The RCCL the process resolved (a host that loaded torch first carries torch's bundled librccl under the
 * same soname): file path and ncclGetVersion() code.  Forming a communicator fails with an error naming both
 * versions when the loaded library's major version is not the one this library was compiled against. */
int idto_hip_rccl_info(char* path_out, int path_cap, int* version_out);
int idto_hip_comm_init(idto_hip_ctx* ctx, const char* unique_id, int rank, int world);
int idto_hip_comm_init_all(idto_hip_ctx** ctxs, int n);
int idto_hip_comm_destroy(idto_hip_ctx* ctx);
int idto_hip_allgather_slab(idto_hip_ctx* ctx);
int idto_hip_gn_step_sharded(idto_hip_ctx* ctx);
int idto_hip_eval_partials_multi(idto_hip_ctx** ctxs, int n); /* fd shards + grouped all-gather */
int idto_hip_gn_step_multi(idto_hip_ctx** ctxs, int n);

int idto_hip_set_q(idto_hip_ctx* ctx, const double* q_host);         /* H2D copy */
int idto_hip_set_q_device(idto_hip_ctx* ctx, const double* q_device); /* D2D copy */

int idto_hip_eval_tau(idto_hip_ctx* ctx);
/* The same for a q whose partials come next (idto_hip_tr_solve, idto_hip_gn_step): v, a, N+, tau, the cost AND the
 * partials from one finite-difference launch (CalcInverseDynamicsPartialsFiniteDiff, optimizer/trajectory_optimizer.cc:426-563,
 * evaluates the nominal point as well); the next idto_hip_eval_partials of this q returns at once. */
int idto_hip_eval_tau_partials(idto_hip_ctx* ctx);

/* One trial point of the trust-region loop in one call and one synchronisation (what
 * CalcTrustRatio, optimizer/trajectory_optimizer.cc:1979-2035, needs at q + dq): uploads q
 * ((N+1)*nq, host), evaluates v, a, tau and the cost L(q) (:147-176), returns tau (N*nv, may be
 * NULL) and the cost to host memory.  Equivalent to set_q + eval_tau + get(TAU) + get(COST). */
int idto_hip_trial_cost(idto_hip_ctx* ctx, const double* q_host, double* tau_host, double* cost_host);

/* The cost along the search direction at many step lengths, one launch set and one wait: what the linesearches
 * (ArmijoLinesearch / BacktrackingLinesearch, optimizer/trajectory_optimizer.cc:1931-1977 / :1852-1929) ask for one step
 * length at a time - each an upload of q, an evaluation and a synchronising fetch through idto_hip_trial_cost - although
 * the candidates alpha_j = rho^j are known in advance and independent of each other.
 * Input: the resident q and IDTO_ARR_STEP, the dq of the last solve (idto_hip_gn_step / idto_hip_factor_solve(NULL), whose
 * status the caller has looked at).  costs_host[j] = L(q + alphas_host[j] dq) for m <= IDTO_LS_MAX_CANDIDATES step lengths:
 * bit for bit what idto_hip_trial_cost returns for the trial point formed as the host loop forms it - step = fl(alpha dq_i),
 * then fl(q_i + step), then (normalize_quaternions) per quaternion n = sqrt(((w w + x x) + y y) + z z) and four divisions.
 * Every candidate is evaluated in an arena of its own (csrc/linesearch.h): the resident iterate is not disturbed - q, its v,
 * a, tau, cost, partials, g, H and the step are afterwards what they were.  Single-problem contexts. */
#define IDTO_LS_MAX_CANDIDATES 64
int idto_hip_costs_along(idto_hip_ctx* ctx, const double* alphas_host, int m, int normalize_quaternions, double* costs_host);
/* The same for a batch context: the same m step lengths along every problem's own step (IDTO_ARR_STEP of problem b, e.g.
 * behind idto_hip_gn_step_batch), one launch set with the problem in the grid (fd_along_batch_kernel: candidate in
 * blockIdx.y, problem in blockIdx.z), one wait.  costs_host[batch][m]; costs_host[b][j] is bit for bit what
 * idto_hip_costs_along returns on a single-problem context holding problem b.  Nothing resident of any problem is written.
 * The candidates' arenas are batch x m x ls_arena(N, nq, nv).stride doubles (csrc/linesearch.h; mini_cheetah, N = 40:
 * 144 KB a candidate), allocated on first use and grown to the largest m asked for. */
int idto_hip_costs_along_batch(idto_hip_ctx* ctx, const double* alphas_host, int m, int normalize_quaternions, double* costs_host);
/* The step lengths the two linesearches try, in the order they try them, formed as the host loops form them (repeated
 * IEEE multiplication by rho = 0.8, never pow; csrc/ls_decide.h): linesearch_method 0 kArmijo (1/rho * rho = 1.0, 0.8,
 * 0.6400000000000001, ...), 1 kBacktracking (1.0, then the same products).  No device involved. */
int idto_hip_ls_alphas(int linesearch_method, int m, double* alphas_host);

/* The whole linesearch method without the host (reference SolveWithLinesearch, optimizer/trajectory_optimizer.cc:2244-2407,
 * for scaling off and no enforced constraints): `iterations` iterations are enqueued back to back and the host waits once.
 * Per iteration: the launches of idto_hip_eval_partials, idto_hip_grad_hess and idto_hip_factor_solve(NULL) at q_k (g, H
 * unscaled, dq = -H^-1 g by the solver the planner picks); ls_prepare_kernel (L' = g.dq, |g|, |dq|, |h| on the dofs of
 * idto_hip_set_unactuated_dofs - the host's Dot and Norm: one thread, index order -, the throw condition, the early-outs);
 * the candidate step lengths in waves (csrc/linesearch.h: trial points, the tau-only evaluation (fd_along_kernel) with the candidate in
 * blockIdx.y, cost_body per candidate, then the scan of csrc/ls_decide.h over the wave's costs in index order; a wave whose
 * iteration is decided returns at its first instruction; how many candidates a wave takes: host/solver_plan.h PlanLsWaves,
 * option "ls_waves" = k > 0: k per wave); then the accepted step - its trial point once more at the decided alpha, the
 * trust ratio of CalcTrustRatio (:1979-2035), the statistics row, q <- q + alpha dq on the device.
 * linesearch_method 0 kArmijo / 1 kBacktracking; max_linesearch_iterations <= IDTO_LS_MAX_CANDIDATES.  The iterate q must
 * be resident (idto_hip_set_q).  rows_host[iterations][IDTO_LS_ROW], a row per iteration that ran (the others are zeros):
 *   [0] L(q_k) [1] alpha [2] ls_iters [3] the trust ratio [4] |q_{k+1}| [5] |dq| [6] |g| [7] L' = g.dq [8] |h|
 *   [9] L(q_{k+1}) [10] device clock at the decision (100 MHz ticks) [11] flags: 2 the step is not finite, 4 it is not a
 *   descent direction (where the reference throws), 32 the factorisation behind the step met a bad pivot, 64 ls_iters
 *   reached max_linesearch_iterations (the step is taken, as the host takes it; the reference's linesearch_failed),
 *   128 backtracking was undecided within IDTO_LS_MAX_CANDIDATES candidates (q stays q_k: continue on the host).  A row
 *   with a flag is the last one: the remaining iterations are idle.
 * On return q, v, a, tau and the cost in device memory are the final iterate's.  _fetch also brings q ((N+1) nq), v
 * ((N+1) nv) and tau (N nv) back under the same wait (any pointer may be NULL).
 * The Newton-step launches of the iterations behind a flagged row still run (the host enqueued them before it could know),
 * at the final iterate, so g, H and IDTO_ARR_STEP are then those of the final iterate; their status is not reported.
 * Returns IDTO_HIP_FACTORIZATION_FAILED when a row carries flag 32 (which names the iteration),
 * IDTO_HIP_SOLVER_TIMEOUT as the other loops.  Option "ls_solves" (read-only) counts the calls on the context. */
#define IDTO_LS_ROW 12
int idto_hip_ls_solve(idto_hip_ctx* ctx, int iterations, int linesearch_method, int max_linesearch_iterations,
                      int normalize_quaternions, double* rows_host);
int idto_hip_ls_solve_fetch(idto_hip_ctx* ctx, int iterations, int linesearch_method, int max_linesearch_iterations,
                            int normalize_quaternions, double* rows_host, double* q_out, double* v_out, double* tau_out);
/* The same loop for every problem of a batch context side by side: every iteration of every problem is enqueued at once -
 * the Newton-step launches with their batch dimension, the ls_* kernels and the tau-only evaluation with the problem in the
 * grid - and the call waits once.  Every problem has its own loop state, scan, rows and gate and stop words: a problem that
 * has decided its iteration, or that carries a flag, idles on its own while the others go on; no kernel waits for another
 * workgroup.  A wave takes the same candidates of every problem; its width is PlanLsWaves' for a horizon of N * batch (the
 * first wave gives every compute unit one workgroup across the whole batch), option "ls_waves" = k: k candidates per problem.
 * The iterates must be resident (idto_hip_set_q_batch).  rows_host[batch][iterations][IDTO_LS_ROW] in the row format above;
 * q_out [batch][(N+1) nq], v_out [batch][(N+1) nv], tau_out [batch][N nv] (any may be NULL) come back packed by one launch
 * under one copy (csrc/ls_fetch.h); final_cost[b] is the cost at problem b's final iterate, status[b] the OR of its rows'
 * flags.  With equal inputs problem b's rows and iterate are bit for bit those of idto_hip_ls_solve_fetch on a
 * single-problem context wherever both run the same solver kernel.
 * Device memory: the candidates' arenas are batch x IDTO_LS_MAX_CANDIDATES x ls_arena(N, nq, nv).stride doubles
 * (csrc/linesearch.h: (N+1)(nq + nv + nv nq) + 2 N nv + 3 nv nq + 1 doubles rounded up to 8 - hopper, N = 50: 19 KB a
 * candidate, 1.2 MB a problem; mini_cheetah, N = 40: 144 KB a candidate, 9.2 MB a problem, 590 MB at batch = 64); an
 * allocation that fails is reported by name, with the bytes asked for.
 * Returns IDTO_HIP_FACTORIZATION_FAILED when some row carries flag 32 (that row names the problem and the iteration; every
 * other problem's outputs are valid), IDTO_HIP_SOLVER_TIMEOUT as the other loops.  Option "ls_batch_solves" (read-only)
 * counts the calls on the context. */
int idto_hip_ls_solve_batch_fetch(idto_hip_ctx* ctx, int iterations, int linesearch_method, int max_linesearch_iterations,
                                  int normalize_quaternions, double* rows_host, double* q_out, double* v_out, double* tau_out,
                                  double* final_cost, int* status);
int idto_hip_eval_partials(idto_hip_ctx* ctx);
int idto_hip_grad_hess(idto_hip_ctx* ctx);
/* Factorises the resident Hessian and solves H x = rhs for `nrhs` right-hand
 * sides given as DEVICE pointers (column-major (N+1)*nq each); rhs == NULL means
 * rhs = -gradient, result in IDTO_ARR_STEP. */
int idto_hip_factor_solve(idto_hip_ctx* ctx, const double* rhs_device, int nrhs, double* x_device);
int idto_hip_gn_step(idto_hip_ctx* ctx);
/* Same solve with HOST right-hand sides / solutions ((N+1)*nq doubles each, nrhs of them,
 * contiguous), staged through buffers the context owns; synchronises.  This is how the
 * host-side trust-region loop obtains H^-1 [J^T | g] for CalcLagrangeMultipliers
 * (optimizer/trajectory_optimizer.cc:1371-1396) and CalcDoglegPoint (:2108-2202). */
int idto_hip_solve_host(idto_hip_ctx* ctx, const double* rhs_host, int nrhs, double* x_host);
/* SolveLinearSystemInPlace with SolverParameters::linear_solver = kDenseLdlt (reference
 * optimizer/trajectory_optimizer.cc:2088-2093: H.MakeDense().ldlt().solve(b)): the resident Hessian
 * as a dense (N+1)*nq square matrix, a blocked LDL^T of it on the device (csrc/dense_ldl.h) and the
 * solution of H x = rhs for ONE host right-hand side; synchronises.  The reference's cross-check of
 * the block Thomas solver (debug_compare_against_dense, :2142-2150) is this call next to
 * idto_hip_solve_host.  IDTO_HIP_FACTORIZATION_FAILED when a pivot is not positive and finite. */
int idto_hip_solve_dense_ldlt(idto_hip_ctx* ctx, const double* rhs_host, double* x_host);
long idto_hip_dense_solve_count(void);   /* calls of the above in this process (the tests' proof of which branch ran) */

/* Equality-constraint step of the trust-region iteration, kept on the device (reference
 * CalcEqualityConstraintJacobian / CalcLagrangeMultipliers, optimizer/trajectory_optimizer.cc:
 * 1292-1396, and the H^-1 (g + J^T lambda) of CalcDoglegPoint :2139-2149).  The constraint is
 * h(q) = [tau_t[dof] : t < N, dof in `dofs`] (the unactuated dofs, :1267-1290); its Jacobian J
 * consists of rows of the dtau/dq blocks already in device memory.
 *   idto_hip_constraint_schur: after idto_hip_grad_hess, solves H Y = [g | J^T] (n_eq + 1
 *     columns, n_eq = nu * N) and returns S = J H^-1 J^T (n_eq x n_eq, column-major) and
 *     J H^-1 g (n_eq) to host memory; Y stays on the device.
 *   idto_hip_constraint_step: given the multipliers lambda (n_eq, host) returns
 *     H^-1 (g + J^T lambda) and J^T lambda (both (N+1)*nq) to host memory. */
int idto_hip_constraint_schur(idto_hip_ctx* ctx, const int* dofs, int nu, double* S_host, double* Jy_host);
/* Only enqueues the work of idto_hip_constraint_schur (no synchronisation; a no-op if it is
 * already enqueued for the current Hessian); a following idto_hip_constraint_schur with the same
 * dofs waits for it and returns the results. */
int idto_hip_constraint_schur_begin(idto_hip_ctx* ctx, const int* dofs, int nu);
int idto_hip_constraint_step(idto_hip_ctx* ctx, const double* lambda_host, double* step_host, double* jtl_host);
/* The whole multiplier computation on the device, after idto_hip_constraint_schur_begin: uploads
 * the constraint violations h (n_eq), factorises S = J H^-1 J^T there (blocked LDL^T without
 * pivoting, csrc/dense_ldl.h), solves S lambda = h - J H^-1 g and returns lambda (n_eq),
 * H^-1 (g + J^T lambda) and J^T lambda (both (N+1)*nq) - one synchronisation, S never leaves
 * the device.  Returns 1 (outputs untouched) when S is numerically singular (smallest pivot
 * <= 1e-13 x largest): the caller then uses idto_hip_constraint_schur + a pivoted factorisation
 * on the host + idto_hip_constraint_step, as Eigen's ldlt() tolerates semi-definite S. */
int idto_hip_constraint_solve(idto_hip_ctx* ctx, const double* h_host, double* lambda_host, double* step_host,
                              double* jtl_host);

/* Trust-region bookkeeping on the resident arrays: what CalcScaleFactors, the
 * scaled gradient / Hessian products, CalcDoglegPoint and CalcTrustRatio
 * (optimizer/trajectory_optimizer.cc:1181-1255, 2108-2202, 1979-2035) compute from g and H, without g
 * or H leaving the device.
 *   idto_hip_tr_prepare: after idto_hip_gn_step (or, with_lambda = 1, after the constraint step).
 *     scaling_method -1 = no scaling, else SolverParameters::scaling_method.  With D the scale
 *     factors, g~ = D (g + J^T lambda), H~ = D H D and w = D^-1 H^-1 (g + J^T lambda) it returns
 *     out[9] = { g~.g~, g~.H~g~, w.w, g~.w, g~.H~w, w.H~w, q.q, h.h, h.lambda } (synchronises).
 *     The Newton point of the dogleg is pH = -w / Delta, the Cauchy point pU = -(g~.g~ / g~.H~g~) g~ / Delta.
 *   idto_hip_tr_trial: every dogleg step is dq = D (a g~ + b w); forms q + dq (quaternions
 *     normalised on request), evaluates tau and the cost there and returns
 *     out[4] = { dq.dq, g~.(a g~ + b w), L(q + dq), h(q + dq).lambda } (synchronises).
 *     speculate_scaling_method >= -1 (else -2): right behind the trial point's evaluation the NEXT
 *     iteration on q + dq is enqueued too - idto_hip_gn_step and idto_hip_tr_prepare with that scaling
 *     method - while the host is still waiting for the trial point's cost: when the step is accepted
 *     (idto_hip_tr_accept) the following idto_hip_gn_step / idto_hip_tr_prepare return what is already
 *     there; when it is rejected (idto_hip_tr_reject) g, H and the Newton step of q have been
 *     overwritten and must be recomputed.  (Not for the adaptive scaling methods, which update D in
 *     place; then the call behaves as without speculation.)
 *   idto_hip_tr_accept: q + dq becomes the resident q (its v, a, tau, cost are already resident).
 *   idto_hip_tr_reject: q stays; v, a, tau in device memory belong to the dropped trial point. */
/* The unactuated dofs (rows of the actuation matrix that are zero, TO.cc:63-72): h.h of
 * idto_hip_tr_prepare is reported for them even when the constraints are not enforced (the
 * reference logs |h| in every iteration, TO.cc:2509, :2586-2598). */
int idto_hip_set_unactuated_dofs(idto_hip_ctx* ctx, const int* dofs, int nu);
int idto_hip_tr_prepare(idto_hip_ctx* ctx, int scaling_method, int with_lambda, double* out_host /* [9] */);
int idto_hip_tr_trial(idto_hip_ctx* ctx, double a, double b, int scaling, int normalize_quaternions, int with_lambda,
                      int speculate_scaling_method, double* out_host /* [4] */);
int idto_hip_tr_accept(idto_hip_ctx* ctx);
int idto_hip_tr_reject(idto_hip_ctx* ctx);
/* The adaptive scalings (kAdaptiveSqrt / kAdaptiveDoubleSqrt, reference optimizer/trajectory_optimizer.cc:1241-1255)
 * take the minimum of the new scale factors and the previous ones, which the reference keeps in the state's
 * cache: ones in a fresh state (`Solve`), the last solve's in a WarmStart (`SolveFromWarmStart`).  This sets
 * that memory: D_prev_host[(N+1)*nq], or NULL for ones.  After a solve IDTO_ARR_TR_SCALE holds the last D. */
int idto_hip_tr_set_scale_memory(idto_hip_ctx* ctx, const double* D_prev_host);

/* The whole trust-region loop without the host (reference optimizer/trajectory_optimizer.cc:2495-2625
 * for the case the stepwise calls above serve: no enforced constraints, no convergence checks).
 * `iterations` iterations are enqueued back to back - per iteration idto_hip_gn_step, one launch
 * for scale factors / inner products / dogleg point (CalcDoglegPoint :2108-2202) / trial point, the
 * inverse dynamics and the cost there, whose kernel also forms the trust ratio (:1979-2035), accepts
 * (q <- q + dq on the device) or rejects, and updates the radius (:2614-2622) - and the host waits
 * once.  The iterate q must be resident with its cost evaluated (idto_hip_set_q + idto_hip_eval_tau).
 * rows_host[iterations][IDTO_TR_ROW]: per iteration
 *   [0] L(q_k) [1] Delta_k [2] rho [3] |q| [4] |dq| [5] |dqH| [6] |g~| [7] dL/dq [8] |h| [9] accepted
 *   [10] device clock at the decision (100 MHz ticks) [11] a [12] b (dq = D (a g~ + b w)) [13] L(q_k + dq)
 *   [14] flags: 1 dogleg quadratic has no root in (0,1), 2 step not finite, 4 step is not a descent
 *   direction (where the reference throws), 16 a convergence criterion held (idto_hip_tr_set_convergence), 32 the
 *   factorisation behind this iteration's step met a bad pivot; once a flag is set the remaining iterations are idle.
 *   [15] the merit function L(q_k) + h(q_k).lambda_k.  [16] see idto_hip_tr_set_convergence.  Flag 8: the constraints' Schur complement is
 *   numerically singular (redundant constraints; the host's pivoted LDL^T copes, the single-workgroup
 *   solve does not): continue from the iterate with the stepwise calls.
 * constrained_dofs / nu: the unactuated degrees of freedom whose tau is constrained to zero
 * (CalcEqualityConstraintViolations, TO.cc:1257-1290), nu = 0: none enforced.  With nu > 0 every iteration
 * also runs H^-1 [g | J^T], S = J H^-1 J^T, lambda = S^-1 (h - J H^-1 g) (TO.cc:1371-1396; one workgroup for
 * nu * num_steps <= 128, the blocked factorisation above) and the step H^-1 (g + J^T lambda) on the device, and
 * the ratio uses the merit function.
 * scaling_method: -1 none, else ScalingMethod (solver_parameters.h:52-62): 0 kSqrt, 1 kAdaptiveSqrt, 2 kDoubleSqrt,
 * 3 kAdaptiveDoubleSqrt; the adaptive methods' memory of D is idto_hip_tr_set_scale_memory's (a rejected step does
 * not advance it: g and H stay, min(D, f(diag H)) = D).
 * On return q, v, a, tau, N+ in device memory are those of the final iterate when the last step was
 * accepted; after a rejected last step v, a, tau belong to the dropped trial point.
 * Returns IDTO_HIP_FACTORIZATION_FAILED when any iteration's factorisation failed. */
#define IDTO_TR_ROW 17
/* VerifyConvergenceCriteria (reference trajectory_optimizer.cc:2654-2689) inside idto_hip_tr_solve.
 * tolerances: {rel_cost_reduction, abs_cost_reduction, rel_gradient_along_dq, abs_gradient_along_dq, rel_state_change,
 * abs_state_change} (solver_parameters.h:17-31), or NULL: no checks (the default).  With tolerances set, row k of
 * idto_hip_tr_solve carries in [16] the ConvergenceReason bitmask of the step accepted in iteration k (1 cost reduction,
 * 2 gradient along dq, 4 state change; 0: none, or the step was rejected); the first row with a non-zero mask is the
 * last iteration that ran - the ones behind it are idle, flag 16 - and q on the device is its iterate. */
int idto_hip_tr_set_convergence(idto_hip_ctx* ctx, const double* tolerances);
int idto_hip_tr_solve(idto_hip_ctx* ctx, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                      double Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                      double* rows_host, double* Delta_out);

/* idto_hip_tr_solve that also returns what the caller fetches next anyway - the iterate q ((N+1) nq), its v ((N+1) nv) and
 * tau (N nv), the last step dq and w = H^-1 (g + J^T lambda) ((N+1) nq each; any pointer may be NULL) - gathered on the
 * device into one buffer and copied under the solve's own wait (the solution fetch of
 * TrajectoryOptimizer::SolveFromWarmStart, optimizer/trajectory_optimizer.cc:2627-2640, without a second round trip).
 * v and tau are the iterate's when the cost weights are diagonal (two output sets) or the last trial point was
 * accepted (rows[last][9] != 0); with dense weights after a rejected last step they are the trial point's: evaluate
 * tau again then, as after idto_hip_tr_solve. */
int idto_hip_tr_solve_fetch(idto_hip_ctx* ctx, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                            double Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                            double* rows_host, double* Delta_out, double* q_out, double* v_out, double* tau_out,
                            double* dq_out, double* w_out);


/* The same loop for every problem of a batch context at once (idto_hip_create_batch): one launch set per iteration
 * with grid.y = problem, one host thread, one wait - the call pattern of an MPC server that advances several
 * warm-started problems per tick (reference examples/mpc_controller.cc:43-85, BASELINE config 5).  Every problem keeps
 * its own radius, accepts or rejects on its own, and idles on its own flags; no equality constraints (nu = 0; with constraints:
 * idto_hip_tr_solve_batch_constrained).
 * Delta0[batch], Delta_out[batch] (may be NULL); rows_host[batch][iterations][IDTO_TR_ROW]: problem b's rows are
 * what idto_hip_tr_solve returns for the same problem in a context of its own - bit for bit when both contexts run the
 * same linear solver, to the solver's round-off otherwise: from 16 block rows on (option "nd_min_rows") a
 * single-problem context takes the scalar band factorisation for blocks up to 5, while a batch of more than two
 * problems keeps the block kernels; option "solver_band" = 0 on both contexts puts them on the same kernel
 * (tests/test_gpu_batch.py does that for the spinner).  Every problem's q must be resident with its cost evaluated
 * (idto_hip_set_q_batch + idto_hip_eval_tau). */
int idto_hip_tr_solve_batch(idto_hip_ctx* ctx, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                            const double* Delta0, double Delta_max, double eta, double* rows_host, double* Delta_out);
/* ... with ENFORCED equality constraints on the `nu` degrees of freedom `constrained_dofs` (the unactuated ones:
 * h = tau[unactuated] = 0, reference TO.cc:1267-1396; BASELINE config 5's own YAML enforces them,
 * examples/allegro_hand/allegro_hand.yaml:95).  With the banded KKT step (nq + nu <= 30: every example) the constrained
 * iteration is one launch set for the whole batch, grid.y = problem, like idto_hip_tr_solve_batch; otherwise (option
 * con_kkt = 0) the multiplier chain is single-problem launches and every problem is advanced in a single-problem context
 * of its own (created on first use inside this context) on its own stream and host thread.  Either way rows and iterates
 * are those of idto_hip_tr_solve on the same problem alone (bit for bit under the same linear solver: see
 * idto_hip_tr_solve_batch).  nu = 0 forwards to idto_hip_tr_solve_batch.
 * Same residency requirement: every problem's q set (idto_hip_set_q_batch). */
int idto_hip_tr_solve_batch_constrained(idto_hip_ctx* ctx, int iterations, int scaling_method, int scaling,
                                        int normalize_quaternions, const double* Delta0, double Delta_max, double eta,
                                        const int* constrained_dofs, int nu, double* rows_host, double* Delta_out);

/* The batch loop of idto_hip_tr_solve_batch(_constrained) that also brings back what the caller reads next, and chooses
 * the best problem: behind the last iteration ONE launch packs every problem's state words, rows, iterate q, its v and tau
 * (from the set of outputs the problem's own iterate ended up in), the last step dq and w into one buffer, one copy takes
 * it to pinned memory of the context (grown on demand, kept), and the call waits for the device exactly once - where
 * idto_hip_tr_solve_batch + idto_hip_get_batch wait about three times per problem.  The context is left as
 * idto_hip_tr_solve_batch leaves it.
 *   final_cost[b]: the cost of problem b's iterate as the loop's state holds it;
 *   status[b]: the OR of column [14] over problem b's rows;
 *   best: among the problems with status & (1|2|4|8|32) == 0 and a finite cost the one of the lowest final_cost, the
 *     lowest index among equals (a fixed scan from 0 to batch - 1 on the device: the same answer at every launch
 *     geometry), -1 when there is none;
 *   only_best != 0: q_out ... w_out receive the best problem's arrays alone ([1][...]; untouched when best is -1), and
 *     only those are packed and copied; rows, radii, costs and statuses come back for every problem.
 * Every problem's outputs are filled even when a factorisation failed (status bit 32 names the problem); the return value
 * is then IDTO_HIP_FACTORIZATION_FAILED, or IDTO_HIP_SOLVER_TIMEOUT as for the other loops.  On a context of one problem
 * the call is idto_hip_tr_solve_fetch.  Enforced constraints that idto_hip_tr_solve_batch_constrained would advance in
 * child contexts (option con_kkt = 0, nq + nu > 30, dense cost weights) are refused with -1 before any device work.
 * Residency as for idto_hip_tr_solve_batch: idto_hip_set_q_batch + idto_hip_eval_tau. */
int idto_hip_tr_solve_batch_fetch(idto_hip_ctx* ctx, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                                  const double* Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                                  double* rows_host, double* Delta_out, int only_best, double* q_out, double* v_out,
                                  double* tau_out, double* dq_out, double* w_out, double* final_cost, int* status, int* best);

/* ---- B model-predictive controllers on a batch context (csrc/mpc_batch.h; the shell of
 * include/idto/examples/mpc_controller.h for every problem of the batch at once).  The context keeps every problem's plan
 * - the splines of q, v and u = the actuated components of tau over the n = num_steps + 1 knots i * time_step, and the
 * time the plan was made at - on the device, in an allocation of its own made by idto_hip_mpc_batch_begin.  A plan as the
 * host sees it is IDTO_MPC_PLAN_LEN(n, nq, nv, nu) doubles:
 *   [start_time | y_q[n][nq] | m_q[n][nq] | y_v[n][nv] | m_v[n][nv] | y_u[n][nu] | m_u[n][nu]]
 * values y and knot derivatives m of the not-a-knot cubic (csrc/mpc_spline.h: the arithmetic PiecewiseCubic runs on the
 * host, so the numbers are those of B single controllers), enough to interpolate x(t), u(t) without a device call.
 * These calls refuse, by name, a context with child contexts (idto_hip_tr_solve_batch_constrained's Schur-complement
 * route made them): the shift changes q_nom, v_init and q on the device only, and keeps the context's host copies of the
 * problems - which only that route reads - in step, but not the children. */
#define IDTO_MPC_PLAN_LEN(n, nq, nv, nu) (1 + 2 * (size_t)(n) * ((nq) + (nv) + (nu)))
/* selector[nq]: q_nom_relative_to_q_init (non-zero: q_nom of that position moves with the initial condition);
 * actuated_dofs[nu]: the velocity index of every control component, 1 <= nu <= nv.  May be called again (new storage). */
int idto_hip_mpc_batch_begin(idto_hip_ctx* ctx, const int* selector, const int* actuated_dofs, int nu);
/* StoreOptimizerSolution for every problem: q[B][(N+1)*nq], v[B][(N+1)*nv], tau[B][N*nv], start_times[B] from the host
 * become the stored plans; plans_out[B][IDTO_MPC_PLAN_LEN] (may be NULL) receives them.  Waits. */
int idto_hip_mpc_batch_store(idto_hip_ctx* ctx, const double* q, const double* v, const double* tau, const double* start_times,
                             double* plans_out);
/* The front half of a tick alone: times[B], x0[B][nq + nv] = [q0; v0] go to the device in one copy, mpc_shift_kernel
 * writes every problem's guess (row i = the stored q-spline at times[b] - start_time[b] + i * time_step, row 0 = q0) as
 * the resident q, v_init = v0 and q_nom shifted for the selected positions; then guess_out[B][(N+1)*nq] and
 * q_nom_out[B][(N+1)*nq] (either may be NULL) are fetched.  Waits.  The context is left as idto_hip_set_q_batch +
 * idto_hip_set_problem_batch leave it. */
int idto_hip_mpc_batch_shift(idto_hip_ctx* ctx, const double* times, const double* x0, double* guess_out, double* q_nom_out);
/* One tick, enqueued at once and waited for once: the copy of times and x0, the shift, idto_hip_eval_tau, the loop of
 * idto_hip_tr_solve_batch_fetch (its arguments, only_best = 0), mpc_store_kernel, one copy back.  Delta0[b]: the radius
 * the previous tick returned in Delta_out[b] (the first tick: the solver parameters' Delta0).  A problem whose status
 * carries one of the bits 1 | 2 | 4 | 8 | 32 keeps its plan; the others' plans are the splines through the loop's final
 * q, v and tau, with start_time = times[b].  guess_out[B][(N+1)*nq] (may be NULL): the guesses the loop started from;
 * plans_out[B][IDTO_MPC_PLAN_LEN] (may be NULL): every problem's plan after the tick (a failed problem's: its old one).
 * Return value as idto_hip_tr_solve_batch_fetch; after IDTO_HIP_SOLVER_TIMEOUT or a negative value every stored plan is
 * the one from before the tick. */
int idto_hip_mpc_batch_replan(idto_hip_ctx* ctx, const double* times, const double* x0, int iterations, int scaling_method,
                              int scaling, int normalize_quaternions, const double* Delta0, double Delta_max, double eta,
                              const int* constrained_dofs, int nu, double* rows_host, double* Delta_out, double* q_out,
                              double* v_out, double* tau_out, double* final_cost, int* status, int* best, double* guess_out,
                              double* plans_out);

/* ---- Plants on the device (csrc/plant.h, csrc/plant_step.h): forward dynamics a = M(q)^-1 (tau_applied - ID(q, v, 0)) from
 * the optimizer's own inverse dynamics and compliant contact model, and semi-implicit Euler substeps of it, one workgroup
 * per plant.  A context of batch B has B plants.  Plant b's physics is the context's model - the context's record b where
 * idto_hip_set_model_batch gave it one - until idto_hip_plant_set_model gives it its own.  The plants' storage (parameter
 * records, states, torques, the state record, status words) is one allocation of the context's, made by
 * idto_hip_plant_begin (by the first idto_hip_forward_dynamics on a context that never began a plant, with default
 * parameters); a context that calls neither runs exactly the launches it ran before.
 * The plants' records are a SNAPSHOT taken when the storage is made: a later idto_hip_set_model_batch on the context does
 * not reach the plants (call idto_hip_plant_begin again, or idto_hip_plant_set_model).
 * Every entry returns 0, or a negative value with idto_hip_last_error. */

/* a[B][nv] = the forward dynamics at x[B][nq + nv] = [q; v] under tau_applied[B][nv]; M_out[B][nv * nv] (column-major) and
 * bias_out[B][nv] (either may be NULL): the mass matrix' columns ID(q, 0, e_j) and the bias ID(q, v, 0) as evaluated.  One
 * launch, one wait.  A plant whose M has a pivot of its LDL^T that is not > 0 and finite, or whose input is not finite, makes
 * the call fail, naming the plant (the other plants' outputs are valid). */
int idto_hip_forward_dynamics(idto_hip_ctx* ctx, const double* x, const double* tau_applied, double* a_out, double* M_out,
                              double* bias_out);

#define IDTO_PLANT_HOLD 0     /* tau_applied = idto_hip_plant_step's tau_hold, held over the launch */
#define IDTO_PLANT_PD_PLUS 1  /* tau_applied = Kp (q_nom - q) + Kd (v_nom - v) [+ u_nom] on the actuated dofs, the nominal values
                                 from the plant's stored plan (idto_hip_mpc_batch_*) at the substep's time */
typedef struct {
  double h;                  /* the substep, > 0 */
  int mode;                  /* IDTO_PLANT_HOLD / IDTO_PLANT_PD_PLUS */
  /* PD+ only: Kp[nu][nq] and Kd[nu][nv] row-major with their sizes in doubles (checked against the context's nu, nq, nv),
   * feed_forward != 0 adds the plan's control; the actuated dofs are idto_hip_mpc_batch_begin's */
  const double* Kp; int kp_size;
  const double* Kd; int kd_size;
  int feed_forward;
  int record_capacity;       /* states per plant that one idto_hip_plant_step may record (0: 64) */
  int block_threads;         /* 0: from the model's size; 64, 128, 192 or 256: the workgroup (a test aid: a small one makes
                                the nv + 1 evaluations of a substep go in rounds) */
} idto_plant_params_t;
#define IDTO_PLANT_MAX_SUBSTEPS 4096   /* of one launch: a single launch stays short on a shared device */
/* Refused by name before any device work: a context with child contexts, h <= 0, an unknown mode, PD+ before
 * idto_hip_mpc_batch_begin, gains of the wrong size or not finite, nv > 64 (the solve runs a lane per row on one
 * wavefront; idto_hip_forward_dynamics refuses it as well).  May be called again: new storage, every plant the context's model again, states zero. */
int idto_hip_plant_begin(idto_hip_ctx* ctx, const idto_plant_params_t* params);
/* Plant b gets `model` (the context's topology; NULL: the context's model) and `contact` (NULL: the context's): the
 * checks, the record and the refusal texts are idto_hip_set_model_batch's.  The context's own model is untouched. */
int idto_hip_plant_set_model(idto_hip_ctx* ctx, int b, const idto_model_t* model, const idto_contact_params_t* contact);
/* times[B], x[B][nq + nv] = [q; v] */
int idto_hip_plant_set_state(idto_hip_ctx* ctx, const double* times, const double* x);
int idto_hip_plant_get_state(idto_hip_ctx* ctx, double* times_out, double* x_out);
/* `substeps` substeps of every plant in ONE launch (1 <= substeps <= IDTO_PLANT_MAX_SUBSTEPS).  tau_hold[B][nv]: hold mode
 * only (PD+: NULL).  x_record_out[B][substeps / record_every][nq + nv] (may be NULL; then record_every is ignored): the
 * state behind every record_every-th substep.  status_out[B][2] (may be NULL): {0 ok | 1 failed pivot | 2 non-finite state
 * or input, substeps completed}: a plant that fails stops and keeps the state from before the failing substep, the
 * others are unaffected.  One wait if an output pointer is given; none otherwise - the launch is enqueued only. */
int idto_hip_plant_step(idto_hip_ctx* ctx, int substeps, const double* tau_hold, int record_every, double* x_record_out,
                        int* status_out);
/* One closed-loop tick of B plants and B controllers, enqueued at once and waited for ONCE, no state crossing the bus on the
 * way in: `substeps` substeps of every plant under PD+ on the current plans (idto_hip_plant_begin with IDTO_PLANT_PD_PLUS);
 * the kernel's last act writes every plant's [t, q, v] into the tick buffer that mpc_shift_kernel reads; then the body of
 * idto_hip_mpc_batch_replan (shared code: its arguments without times and x0, its outputs, its return value), the tick
 * re-planning at the plants' times from the plants' states; one more copy back, x_after_out[B][nq + nv] (may be NULL): the
 * plants' states behind the substeps, i.e. the x0 of this tick; plant_status_out[B][2] (may be NULL): idto_hip_plant_step's
 * status words of the tick's substeps - a plant that stopped re-plans from the state it stopped in.  Refused by name before any device work: everything
 * idto_hip_mpc_batch_replan and idto_hip_plant_step refuse, and plants that are not in PD+ mode. */
int idto_hip_mpc_batch_tick_plants(idto_hip_ctx* ctx, int substeps, int iterations, int scaling_method, int scaling,
                                   int normalize_quaternions, const double* Delta0, double Delta_max, double eta,
                                   const int* constrained_dofs, int nu, double* rows_host, double* Delta_out, double* q_out,
                                   double* v_out, double* tau_out, double* final_cost, int* status, int* best, double* guess_out,
                                   double* plans_out, double* x_after_out, int* plant_status_out);

/* ---- Scene report (csrc/scene_report.h): where every body is and what every candidate contact pair does at the states
 * [q; v] of a trajectory - an optimizer's solution (q_t, v_t) or the rows that idto_hip_plant_step recorded.  It stands
 * where the reference's EvalPlantContext stands: body poses, spatial velocities, signed-distance pairs and contact results,
 * without a plant's context.  One workgroup per state and problem, one launch.  The table the kernel needs beside the
 * model (the body of every geometry) is storage the context allocates at the first report; a context that never asks for
 * a report runs exactly the launches it ran before, and a report changes none of the context's state: the iterate, the
 * prefetches and the trust-region sets are as they were.
 *
 * The contact inside tau_t (IDTO_ARR_TAU, row t) is the report's tau_contact row for (q_{t+1}, v_{t+1}) with a minus sign:
 * tau_contact is the generalised force that contact applies to the system, and inverse dynamics at (q_{t+1}, v_{t+1}, a_t)
 * subtracts it. */
#define IDTO_SCENE_MODELS_PROBLEMS 0   /* problem b's physics: the context's model, or its record b after idto_hip_set_model_batch */
#define IDTO_SCENE_MODELS_PLANTS 1     /* plant b's physics (idto_hip_plant_begin, idto_hip_plant_set_model) */
#define IDTO_SCENE_BODY_DOUBLES 18     /* a body: R_WB row-major [0, 9), p [9, 12), w [12, 15), v of the body origin [15, 18); world frame */
#define IDTO_SCENE_PAIR_DOUBLES 20     /* a candidate pair, the entries at these offsets: */
#define IDTO_SCENE_PAIR_ACTIVE 0       /* 1.0 or 0.0: phi <= the contact threshold */
#define IDTO_SCENE_PAIR_PHI 1          /* signed distance */
#define IDTO_SCENE_PAIR_N 2            /* [3] unit normal from A towards B */
#define IDTO_SCENE_PAIR_CA 5           /* [3] witness point on A, world */
#define IDTO_SCENE_PAIR_CB 8           /* [3] witness point on B, world */
#define IDTO_SCENE_PAIR_VN 11          /* normal velocity of B relative to A at pC = (Ca + Cb) / 2 */
#define IDTO_SCENE_PAIR_VT 12          /* [3] tangential part of that velocity */
#define IDTO_SCENE_PAIR_FN 15          /* normal force */
#define IDTO_SCENE_PAIR_F 16           /* [3] the force on body B at pC, world frame; body A gets -f */
#define IDTO_SCENE_PAIR_PAD 19         /* 0.0 */
/* An inactive pair keeps its geometry and velocities and has fn and f exactly zero; an active pair that separates at twice
 * the dissipation velocity or faster is active with an exactly zero force. */

/* nbodies, npairs, IDTO_SCENE_BODY_DOUBLES, IDTO_SCENE_PAIR_DOUBLES (each pointer may be NULL) */
int idto_hip_scene_sizes(idto_hip_ctx* ctx, int* nbodies, int* npairs, int* body_doubles, int* pair_doubles);
/* x[batch][nstates][nq + nv]: the layout of a plant's record rows and of a solution's (q_t, v_t).  models:
 * IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS.  Outputs, each may be NULL (not all):
 *   bodies_out[batch][nstates][nbodies][18], pairs_out[batch][nstates][npairs][20],
 *   tau_contact_out[batch][nstates][nv], tau_pairs_out[batch][nstates][npairs][nv] (a pair's row of tau_contact; the rows
 *   sum to it in ascending pair index from +0).
 * One upload, one launch, one copy back through pinned staging, one wait.  Refused by name before any device work: x NULL,
 * nstates < 1, all outputs NULL, an entry of x that is not finite (named by problem, state and index), an unknown `models`,
 * the plants' models on a context without a begun plant. */
int idto_hip_scene_report(idto_hip_ctx* ctx, int nstates, const double* x, int models, double* bodies_out, double* pairs_out,
                          double* tau_contact_out, double* tau_pairs_out);

/* ---- Plant linearisation and time-varying LQR gains (csrc/plant_lin.h, csrc/plant_tangent.h, csrc/tvlqr_step.h): the local
 * model x+ ~ f(x*, u*) + A dx + B du of the plants' own map f of `substeps` substeps of h under a held torque, about the
 * states of a trajectory, and the gains K_t of the finite-horizon LQR problem along them.  Deviations are in TANGENT
 * coordinates: dx = [dtheta (nv); dv (nv)], n = 2 nv - a floating joint's quaternion deviates by three angular components in
 * the world frame (the convention of the velocities), every other joint's positions by themselves.  A and B are central
 * differences of step eps over plant_kernel's rollouts, P = 1 + 6 nv columns per state (column 0 the nominal, then +eps, -eps
 * along each component of dtheta, dv and tau); the storage is an allocation of the feature's own, made at the first call
 * and grown on demand: a context that never calls these runs exactly the launches it ran before, and a call changes none
 * of the context's state nor the plants'.  Matrices are column-major.  `models` is the scene report's selector. */
#define IDTO_LIN_EPS_DEFAULT 6.0554544523933395e-06   /* cbrt(2^-52): the step of a central difference */
/* n = 2 nv, the columns per state P, and the number of doubles of every output for `nstates` states and `nu` controls
 * (each pointer may be NULL) */
int idto_hip_lin_sizes(idto_hip_ctx* ctx, int nstates, int nu, int* n, int* columns, long* x_next_count, long* A_count,
                       long* B_count, long* K_count, long* P_count);
/* x[batch][nstates][nq + nv] = [q; v], tau[batch][nstates][nv] the held torque (all nv components).  Outputs, each may be
 * NULL and is then not fetched:
 *   x_next_out[batch][nstates][nq + nv]: f(x, tau), the nominal column's final state
 *   A_out[batch][nstates][n * n], B_out[batch][nstates][n * nv]
 *   status_out[batch][nstates][2]: {0, 0}, or {plant_kernel's code, the column} of the first column whose rollout did not end
 *   well - A, B and x_next of that state are then NaN, the other states are unaffected.
 * Everything is enqueued at once (the perturbation, one plant_kernel launch per problem, the difference) and waited for
 * once.  Refused by name before any device work: x or tau NULL or not finite, nstates < 1, substeps outside
 * [1, IDTO_PLANT_MAX_SUBSTEPS], h or eps not > 0 and finite, nstates * P > 65536, an unknown `models`, the plants' models on
 * a context without a begun plant, nv > 64, a context with child contexts. */
int idto_hip_plant_linearize(idto_hip_ctx* ctx, int nstates, const double* x, const double* tau, double h, int substeps,
                             double eps, int models, double* x_next_out, double* A_out, double* B_out, int* status_out);
/* The same, and behind it on the device the Riccati recursion over the problem's nstates linearisations, one workgroup per
 * problem, A and B read where the difference left them: actuated[nu] the velocity indices whose columns of B are Bu;
 * Q[n * n], R[nu * nu], Qf[n * n] symmetric, time-invariant, in tangent coordinates.  With S = nstates, P_S = Qf and for
 * t = S - 1 ... 0: G = R + Bu^T P Bu, K_t = G^-1 Bu^T P A (un-pivoted LDL^T), P_t = Q + K_t^T R K_t + (A - Bu K_t)^T P (A - Bu K_t).
 *   K_out[batch][nstates][nu * n], P_out[batch][nstates + 1][n * n]
 *   lqr_status_out[batch]: 0, or 1 + t for the first step t whose G has a pivot that is not > 0 and finite: K and P from t
 *   downward are NaN.  A state whose linearisation failed ends the recursion there in the same way.
 * Refused by name as well: nu outside [1, nv], an index of actuated outside [0, nv), Q, R or Qf NULL or not finite, matrices
 * that do not fit the 160 KiB of LDS (5 n^2 + 4 n nu + 2 nu^2 + nu doubles). */
int idto_hip_plant_tvlqr(idto_hip_ctx* ctx, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                         int models, int nu, const int* actuated, const double* Q, const double* R, const double* Qf,
                         double* x_next_out, double* A_out, double* B_out, int* status_out, double* K_out, double* P_out,
                         int* lqr_status_out);

/* ---- Plants under the time-varying LQR law (csrc/plant.h plant_body with LAW, track_kernel): `nrollouts` rollouts per
 * problem of nsteps control steps, each `substeps` substeps of h under the torque
 *   tau_t = tau*_t, with u_t = tau*_t[actuated] - K_t [q (-) q*_t ; v - v*_t] on the actuated dofs (tvlqr_step.h tvlqr_control),
 * formed at the start of the step and HELD over it: the map that idto_hip_plant_linearize's A_t, B_t linearise.  With
 * S = nsteps, R = nrollouts, n = 2 nv:
 *   x_nom[batch][S + 1][nq + nv], tau_nom[batch][S][nv] (all nv components), K[batch][S][nu * n] column-major,
 *   x0[batch][R][nq + nv] the rollouts' initial states.
 * Outputs, each may be NULL and is then not fetched:
 *   x_out[batch][R][S][nq + nv]: the state behind every step
 *   u_out[batch][R][S][nu], dx_out[batch][R][S + 1][n]: the law's control and deviation in front of step t; row S of dx the
 *   deviation of the final state from x*_S
 *   status_out[batch][R][2]: idto_hip_plant_step's {code, substeps completed}; a non-finite u_t (a NaN in K_t, say) ends the
 *   rollout with code 2 at that substep.  The rows of a rollout behind its last completed step are NaN (x and u from row
 *   completed / substeps on, dx behind that row); the other rollouts are unaffected.
 * The steps are cut into launches of whole steps of at most max_launch_substeps substeps (0: IDTO_PLANT_MAX_SUBSTEPS; a
 * smaller figure is a test aid), all enqueued at once and waited for once; a rollout that ended in one launch is skipped by
 * the later ones.  The storage is an allocation of the feature's own, made at the first call and grown on demand; a call
 * changes none of the context's state nor the plants'.  `models` is the scene report's selector.  Refused by name before any
 * device work: what idto_hip_plant_linearize refuses of its kind (an unknown `models`, the plants' models without a begun
 * plant, nv > 64, child contexts, h not > 0 and finite, substeps outside [1, IDTO_PLANT_MAX_SUBSTEPS]), nsteps < 1,
 * nrollouts < 1, batch * nrollouts > 65536, max_launch_substeps neither 0 nor in [substeps, IDTO_PLANT_MAX_SUBSTEPS], nu outside [1, nv], an index of
 * actuated outside [0, nv), an input NULL, an entry of x_nom, tau_nom or x0 that is not finite (named by array and index; K may
 * hold NaN: that is a status), a block whose LDS would exceed 160 KiB. */
int idto_hip_plant_track(idto_hip_ctx* ctx, int nsteps, int substeps, double h, int models, int nu, const int* actuated,
                         const double* x_nom, const double* tau_nom, const double* K, int nrollouts, const double* x0,
                         int max_launch_substeps, double* x_out, double* u_out, double* dx_out, int* status_out);
/* idto_hip_plant_tvlqr about x[batch][nsteps + 1][nq + nv] (the linearisations of its first nsteps rows) and
 * tau[batch][nsteps][nv], and behind it on the same stream the rollouts of idto_hip_plant_track about the same x and tau, K read
 * where the recursion left it on the device: one wait for everything.  Refuses what either refuses. */
int idto_hip_plant_tvlqr_track(idto_hip_ctx* ctx, int nsteps, const double* x, const double* tau, double h, int substeps, double eps,
                               int models, int nu, const int* actuated, const double* Q, const double* R, const double* Qf,
                               int nrollouts, const double* x0, int max_launch_substeps, double* x_next_out, double* A_out,
                               double* B_out, int* status_out, double* K_out, double* P_out, int* lqr_status_out, double* x_out,
                               double* u_out, double* dx_out, int* track_status_out);

/* Options: "gradients_method" = 0 forward differences (default), 1 / 2 central differences of
 * 2nd / 4th order (SolverParameters::gradients_method, reference solver_parameters.h:26-50,
 * trajectory_optimizer.cc:565-885); 3 (autodiff) is refused.  "reference_solver" = 1 selects the bit-exact restatement of the reference's
 * pivoted-LU block Thomas (slow) instead of the banded block LDL^T solver (default 0; the
 * environment variable IDTO_SOLVER_REFERENCE=1 sets it at creation); "two_sided" = 0 keeps the
 * LDL^T solver on one workgroup (default 1: two workgroups eliminate from both ends of the
 * horizon); "fused" = 0 makes idto_hip_gn_step three launches
 * (fd, assemble, solve) instead of one persistent launch whose workgroups take the three roles and
 * synchronise through device-memory counters (default 1; single-problem contexts with diagonal
 * weights and the reference's example models; csrc/fused.h); "solver_nd" = 0 keeps the single-right-hand-side solve on the
 * two-workgroup kernel instead of the nested-dissection form (csrc/penta_nd.h: four chain workgroups,
 * two spike workgroups and a separator; default 1, used for block sizes 2 / 3 / 5 / 19 and at least 24
 * block rows; explicit multi-right-hand-side solves always use the two-workgroup factors);
 * "solver_pipe" = 0 keeps the nested dissection on the seven-workgroup kernel instead of the pipelined chains
 * (csrc/penta_pipe.h: five workgroups, block sizes up to 20; default 1); "solver_band": the small models' scalar band
 * factorisation in one workgroup, which takes the pipelined chains' place (csrc/penta_band.h; 0 off, 1 = blocks up to 4 - in a
 * batch context up to 2 -, the default, 2 = up to 5, batches included; IDTO_SOLVER_BAND overrides it at creation); "asm_in_solver" = 0 gives the assembly of
 * idto_hip_gn_step / of the trust-region loop a launch of its own instead of workgroups of the pipelined solver's
 * launch (default 1); a launch whose workgroups were not co-resident steps these down by itself (IDTO_HIP_SOLVER_TIMEOUT);
 * "gn_small" = 0 keeps the small all-revolute models (acrobot, spinner) on fd_kernel + the band solver's launch instead of the
 * one-workgroup step (csrc/gn_small.h; default 1); inside idto_hip_tr_solve: "tr_small" = 0 keeps fd_kernel, cost_kernel and
 * the solver's launch per iteration for them, "tr_fold" = 0 keeps tr_iter_kernel a launch of its own in front of the
 * one-workgroup launch (defaults 1: a whole trust-region iteration of a small model, its enforced constraint included, is
 * ONE launch), "kkt_fold" = 0 takes the banded KKT step's solution apart in a launch of its own (kkt_extract_kernel) instead of
 * inside tr_iter_kernel, "kkt_in_asm" = 0 builds the KKT system in a launch of its own (kkt_build_kernel) instead of
 * having the gated assembly write it along, "decide_in_solver" = 0 keeps cost_kernel a launch of its own in front of the
 * pipelined solver's instead of one more workgroup of that launch; all of these leave every result bit for bit as it is (tests/test_gpu_small.py,
 * tests/test_gpu_trust_region.py);
 * "fd_dedup" = 0 runs the forward differences of a model that has the lane map without the redundant path lanes (mini_cheetah:
 * a column of a leg's joint evaluated on that leg's lane only, the freed lanes evaluating contact pairs) with every
 * evaluation on all its paths again (default 1; IDTO_FD_DEDUP overrides it at creation; any other model ignores it; the results
 * are equal value for value, tests/test_gpu_fd_dedup.py); "last_fd_dedup" reads back whether the last launch ran on that map;
 * "solver_debug" = 1 records per-phase cycle stamps (IDTO_ARR 15, tools/solver_phases.py);
 * "asm_stop" truncates the assembly kernel after a phase (tools/asm_phases.py). */
int idto_hip_set_option(idto_hip_ctx* ctx, const char* name, int value);
/* Reads an option back; additionally "last_solver": which factorisation the last solve used
 * (1 two-workgroup block LDL^T, 2 nested dissection over seven workgroups, 3 reference-order LU, 4 nested dissection
 * with pipelined chains, 5 inside the fused launch, 6 the scalar band factorisation). */
int idto_hip_get_option(idto_hip_ctx* ctx, const char* name, int* value);

/* Device-side timing of the last `idto_hip_gn_step`-shaped launches: average
 * milliseconds per launch of kernel `which` (0 fd, 1 assemble, 2 factor_solve, 3 the fused
 * single-launch iteration of idto_hip_gn_step)
 * over the launches recorded since idto_hip_timing_reset, measured with HIP
 * events on the context's stream.  enable = 1 times every launch, enable = s > 1 every
 * s-th launch (an event pair costs ~4 us of stream time: sampling keeps the timed
 * region representative), 0 switches timing off. */
int idto_hip_timing_enable(idto_hip_ctx* ctx, int enable);
int idto_hip_timing_reset(idto_hip_ctx* ctx);
int idto_hip_timing_get(idto_hip_ctx* ctx, int which, double* avg_ms, int* launches);

int idto_hip_sync(idto_hip_ctx* ctx);
/* Synchronises and reports the status of the most recent factorisation launched on this context
 * (idto_hip_factor_solve / idto_hip_gn_step / the constraint step): *failed = 1 if it met a bad
 * pivot (see IDTO_HIP_FACTORIZATION_FAILED), else 0; *failed_rows_total (may be NULL) counts the
 * failing block rows since the context was created. */
int idto_hip_solver_status(idto_hip_ctx* ctx, int* failed, int* failed_rows_total);
/* Enqueues, behind the work submitted so far, an asynchronous copy of array `what` (a
 * contiguous one: not TAU / DTAU_*) to pinned staging memory on a side stream.  The next
 * idto_hip_get of the same array waits for that copy only - not for kernels launched after
 * the prefetch (how the host loop reads g and the Hessian bands while the solver runs).  A
 * pending prefetch is dropped if the array is recomputed before it is read. */
int idto_hip_prefetch(idto_hip_ctx* ctx, int what);
/* Synchronises and copies array `what` to host memory (sizes above). */
int idto_hip_get(idto_hip_ctx* ctx, int what, double* host_out);
/* Raw device pointer / element count of a resident array (for zero-copy interop).  Handing out a
 * Hessian band or the slab tells the context that the caller may write it (the solver then takes H
 * as a general matrix, the assembly reads the slab instead of fd_kernel's products).  The pointers of
 * IDTO_ARR_V / A / NPLUS / SLAB / ASM_TERMS are stable between calls EXCEPT across idto_hip_tr_solve,
 * which keeps two sets of them and may leave the iterate's in the other one: ask again afterwards. */
void* idto_hip_device_ptr(idto_hip_ctx* ctx, int what);
long idto_hip_array_size(idto_hip_ctx* ctx, int what);
int idto_hip_slab_stride(idto_hip_ctx* ctx);

/* Self-test of device arithmetic the bit-exactness argument relies on: evaluates
 * sqrt, division and idto::detmath on `n` inputs on the device (outputs to host arrays). */
int idto_hip_math_probe(int device, const double* x, int n, double* sqrt_out, double* recip_out,
                        double* sin_out, double* cos_out, double* exp_out, double* log_out);

/* Host-side timeline: wall-clock marks of what the calling thread does inside and between the entry points above
 * (tools/host_profile.py --mpc: one MPC re-plan, reference examples/mpc_controller.cc:43-85, accounted for step by step).
 * enable(1) clears the marks and starts the clock; mark(label) appends "<us since enable> label"; dump writes the lines
 * into out (NUL-terminated, truncated to cap) and returns the bytes the whole text needs.  Not thread-safe: a
 * measurement aid for one host thread. */
void idto_hip_trace_enable(int on);
void idto_hip_trace_mark(const char* label);
int idto_hip_trace_dump(char* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* IDTO_HIP_H_ */
