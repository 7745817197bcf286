// plant_calls.h — what the entries of the plant family (include/idto_hip.h idto_hip_plant_*, idto_hip_forward_dynamics,
// idto_hip_scene_report, idto_hip_mpc_batch_tick_plants' step) decide on the host before any device work: what they refuse,
// the block and the dynamic LDS of their launches, and where every array of a call lies in the feature's device buffer and in
// its pinned mirror.  Host-only C++ (no HIP include): csrc/*_abi.inc fill a PlantShape from the context and act on the
// answers; tests/cpp/plant_calls_check.cc holds the unit to tests/golden/plant_call_layouts.txt and to every message on the CPU.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "fd_sizes.h"
#include "idto_hip.h"

namespace idto_host {

// What the refusals and the layouts read of a context (idto_hip.hip PlantShapeOf fills it)
struct PlantShape {
  int batch, nq, nv, nb, npairs, ngeoms, blob_n, nxb, nstem, npaths, maxc;
  bool children;        // child contexts exist
  bool model_records;   // the context has a parameter record per problem
  bool host_model;      // ... and keeps the host copy of its model and tables
  // the plants: begun by idto_hip_plant_begin, and what it fixed
  bool plants_begun; int plant_mode, plant_nu, plant_block, plant_lds, plant_record_capacity;
  bool plant_mpc_current;   // the stored plans are those of the idto_hip_mpc_batch_begin that the plants were begun behind
  // the stored MPC plans (idto_hip_mpc_batch_begin)
  bool mpc; int mpc_nu, mpc_n; size_t mpc_len;
};

// rc 0: the call is accepted (msg is empty and nothing was allocated); else the entry's return code and its message
struct Refusal {
  int rc = 0;
  std::string msg;
};

// ---- the block and the dynamic LDS of plant_kernel / track_kernel; beside: the doubles that lie in LDS beside the block's
// own (PlantPdDoubles, plant_sizes.h plant_law_doubles, or 0)
constexpr int kPlantMaxLds = idto_dev::kMaxDynamicLds;
size_t PlantPdDoubles(const PlantShape& s);
// bytes; 1 << 27 where the count of doubles is beyond 2^24 (no int overflow, and past every bound)
int PlantLdsBytes(const PlantShape& s, int threads, size_t beside);
// Threads of the block, beside host/fd_plan.cc's: a wavefront per 64 lanes of the (nv + 1) * npaths that a substep's evaluations want,
// up to 256 (or `forced`); the block shrinks by a wavefront at a time where the exchange areas of its concurrent evaluations do
// not fit the 160 KiB of LDS beside the rest (the evaluations then go in rounds)
int PlantBlock(const PlantShape& s, int forced, size_t beside);

// ---- layouts: a call's arrays in one device buffer, carved in the table's order, every entry on a 64-byte boundary (counts
// in doubles, rounded up to 8; an entry of 0 doubles takes none).  [inputs | work | outputs]: the inputs are staged in the
// pinned mirror at their device offsets and go up in one copy of in_n doubles; an output at device offset o comes back to
// mirror offset o - out0 (Mirror), the inputs' staging being free again behind the upload.
struct CallEntry { const char* name; size_t offset, count; };
struct CallPlan {
  std::vector<CallEntry> entries;   // in the table's order; a mirror-only entry (behind `total`) names a place in the mirror alone
  size_t in_n = 0, out0 = 0, total = 0, pinned = 0;   // the inputs end, the outputs start, the device buffer ends; doubles of the mirror
  size_t at(int e) const { return entries[e].offset; }
  size_t count(int e) const { return entries[e].count; }
  size_t Mirror(int e) const { return entries[e].offset - out0; }
};

// X(name, doubles); IN: the inputs end here, OUT: the outputs start here.  B = batch, w = nq + nv, n = 2 nv.
// The plants' storage (idto_hip_plant_begin): a record of rec_n doubles a plant, cap recorded states a launch.  in_n and
// pinned are idto_hip_forward_dynamics' staging: x and tau_applied one behind the other, then [a | M | bias] from out0 and the
// status words (two ints a plant) behind them.
#define IDTO_PLANT_STORAGE_PLAN(X, IN, OUT)                                                                         \
  X(records, B * rec_n) X(state, B * (1 + w)) X(tau, B * nv) X(record, B * cap * w) X(fd_x, B * w) OUT              \
  X(fd_a, B * nv) X(fd_M, B * nv * nv) X(fd_bias, B * nv) X(Kp, nu * nq) X(Kd, nu * nv) X(status, B)
// The scene report's outputs (the states lie in a buffer of their own: in_n doubles of them): an output that was not asked
// for takes nothing
#define IDTO_SCENE_PLAN(X, IN, OUT)                                                                                  \
  X(bodies, mask & 1 ? B * S * nb * IDTO_SCENE_BODY_DOUBLES : 0) X(pairs, mask & 2 ? B * S * np * IDTO_SCENE_PAIR_DOUBLES : 0) \
  X(tau_contact, mask & 4 ? B * S * nv : 0) X(tau_pairs, mask & 8 ? B * S * np * nv : 0)
// The linearisation's: SP = S * lin_columns(nv) plants a problem; tv: the Riccati recursion runs behind it (nu = 0 without)
#define IDTO_LIN_PLAN(X, IN, OUT)                                                                                    \
  X(x, B * S * w) X(tau, B * S * nv) X(Q, tv ? n * n : 0) X(R, nu * nu) X(Qf, tv ? n * n : 0) X(actuated, (nu + 1) / 2) IN \
  X(pstate, B * SP * (1 + w)) X(ptau, B * SP * nv) X(pstatus, B * SP) OUT                                            \
  X(x_next, B * S * w) X(A, B * S * n * n) X(Bm, B * S * n * nv) X(status, B * S) X(K, tv ? B * S * nu * n : 0)      \
  X(P, tv ? B * (S + 1) * n * n : 0) X(lqr_status, tv ? (B + 1) / 2 : 0)
// The tracked rollouts': R rollouts a problem; own_K: the call brings its gains.  The status words (two ints a rollout) are
// zeroed by the inputs' upload and come back behind the outputs: status_back, in the mirror alone.
#define IDTO_TRACK_PLAN(X, IN, OUT)                                                                                  \
  X(x_nom, B * (S + 1) * w) X(tau_nom, B * S * nv) X(K, own_K ? B * S * nu * n : 0) X(actuated, (nu + 1) / 2)        \
  X(state, B * R * (1 + w)) X(status, B * R) IN OUT X(x_out, B * R * S * w) X(u_out, B * R * S * nu) X(dx_out, B * R * (S + 1) * n)

#define IDTO_PLAN_ID(name, count) name,
#define IDTO_PLAN_NONE
namespace plant_storage { enum { IDTO_PLANT_STORAGE_PLAN(IDTO_PLAN_ID, IDTO_PLAN_NONE, IDTO_PLAN_NONE) status_back }; }
namespace scene { enum { IDTO_SCENE_PLAN(IDTO_PLAN_ID, IDTO_PLAN_NONE, IDTO_PLAN_NONE) count }; }
namespace lin { enum { IDTO_LIN_PLAN(IDTO_PLAN_ID, IDTO_PLAN_NONE, IDTO_PLAN_NONE) count }; }
namespace track { enum { IDTO_TRACK_PLAN(IDTO_PLAN_ID, IDTO_PLAN_NONE, IDTO_PLAN_NONE) status_back }; }

inline int PlantRecordCapacity(int asked) { return asked > 0 ? asked : 64; }
CallPlan PlanPlantStorage(const PlantShape& s, size_t rec_n, int record_capacity, int nu);
CallPlan PlanScene(const PlantShape& s, int nstates, unsigned mask);   // mask: bit i set = output i of the table was asked for
CallPlan PlanLin(const PlantShape& s, int nstates, bool tv, int nu);
CallPlan PlanTrack(const PlantShape& s, int nsteps, int nrollouts, int nu, bool own_K);

// ---- refusals, every one before any device work; who: the entry's name as its messages begin
#define IDTO_LIN_MAX_COLUMNS 65536     /* S * P of one problem: a plant_kernel launch of at most that many workgroups */
#define IDTO_TRACK_MAX_ROLLOUTS 65536  /* batch * nrollouts: the workgroups of one launch */

// what idto_hip_plant_tvlqr has beside idto_hip_plant_linearize's arguments
struct LinTv {
  int nu; const int* actuated; const double* Q; const double* R; const double* Qf;
  double* K_out; double* P_out; int* lqr_status_out;
};
// a tracked call's arguments beside the gains
struct TrackCall {
  int S, substeps; double h; int models, nu; const int* actuated;
  const double* x_nom; const double* tau_nom; int R; const double* x0; int max_launch_substeps;
  double* x_out; double* u_out; double* dx_out; int* status_out;
};

Refusal RefusePlantBegin(const PlantShape& s, const idto_plant_params_t* prm);
// the storage that idto_hip_plant_begin and a first idto_hip_forward_dynamics make (both speak as plant_begin)
Refusal RefusePlantStorage(const PlantShape& s, int block_threads, bool pd);
Refusal RefusePlantsBegun(const PlantShape& s, const char* who);
Refusal RefusePlantSetModel(const PlantShape& s, int b);
Refusal RefusePlantSetState(const PlantShape& s, const double* times, const double* x);
// a step of the plants; *nrec: the states it records.  tick: as idto_hip_mpc_batch_tick_plants' step part (no torque, no record)
Refusal RefusePlantStep(const PlantShape& s, const char* who, int substeps, const double* tau_hold, int record_every, bool record, int* nrec);
Refusal RefuseTickPlantsStep(const PlantShape& s, int substeps);
Refusal RefuseForwardDynamics(const PlantShape& s, const double* x, const double* tau_applied, const double* a_out);
Refusal RefuseSceneReport(const PlantShape& s, int nstates, const double* x, int models, unsigned mask);
// idto_hip_plant_linearize (tv null), idto_hip_plant_tvlqr, and idto_hip_plant_tvlqr_track's second half
Refusal RefuseLin(const PlantShape& s, const char* who, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                  int models, const LinTv* tv);
// idto_hip_plant_track (own_K: the call brings its gains, K), and idto_hip_plant_tvlqr_track's first half
Refusal RefuseTrack(const PlantShape& s, const char* who, const TrackCall& a, bool own_K, const double* K);

}  // namespace idto_host
