// idto_hip.hip — C-ABI (include/idto_hip.h) over the gfx950 kernels in kernels.h.
// Owns the HBM-resident state of one trajectory-optimisation problem:
//   q, N+, v, a | slab (dtau/dq + tau, t-major) | g, H bands | factors | step
// Nothing in here falls back to the CPU: if no HIP device is present every
// entry point fails with a negative status.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <limits>
#include <memory>
#include <mutex>
#include <type_traits>
#include <utility>
#include <thread>
#include <string>
#include <vector>

#include "idto_hip.h"
#include "kernels.h"
#include "fd_launch.h"
#include "penta_ldl.h"
#include "fused.h"
#include "penta_nd.h"
#include "penta_pipe.h"
#include "penta_band.h"
#include "gn_small.h"
#include "penta_apply.h"
#include "constraints.h"
#include "dense_ldl.h"
#include "trust_region.h"
#include "kkt.h"
#include "linesearch.h"
#include "mpc_batch.h"
#include "plant_launch.h"
#include "scene_launch.h"
#include "lin_launch.h"
#include "track_launch.h"
#include "host/context_layout.h"
#include "host/ctx_buffers.h"
#include "host/fd_plan.h"
#include "host/model_batch.h"
#include "host/model_tables.h"
#include "host/plant_calls.h"
#include "host/solver_plan.h"

using namespace idto_dev;

namespace {
thread_local std::string g_err;

// ---- host-side timeline (idto_hip_trace_*): wall-clock marks of what the host thread does between the C-ABI's entry
// points, for tools/host_profile.py --mpc (one MPC re-plan accounted for in steps of 10 us).  Off: one
// predictable branch per mark.
struct HostTrace {
  bool on = false;
  std::chrono::steady_clock::time_point t0;
  std::vector<std::pair<std::string, double>> ev;
};
static HostTrace g_trace;
static std::mutex g_trace_mu;   // (idto_hip_tr_solve_batch_constrained marks from several host threads)
extern "C" void idto_hip_trace_enable(int on) {
  std::lock_guard<std::mutex> lk(g_trace_mu);
  g_trace.on = on != 0;
  g_trace.ev.clear();
  g_trace.ev.reserve(256);
  g_trace.t0 = std::chrono::steady_clock::now();
}
extern "C" void idto_hip_trace_mark(const char* label) {
  if (!g_trace.on) return;
  std::lock_guard<std::mutex> lk(g_trace_mu);
  g_trace.ev.emplace_back(label, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g_trace.t0).count());
}
// "<microseconds since enable> <label>\n" per mark; returns the number of bytes the whole text needs
extern "C" int idto_hip_trace_dump(char* out, int cap) {
  std::string t;
  char buf[64];
  std::lock_guard<std::mutex> lk(g_trace_mu);
  for (const auto& e : g_trace.ev) { std::snprintf(buf, sizeof buf, "%.1f ", e.second); t += buf; t += e.first; t += "\n"; }
  if (out && cap > 0) std::snprintf(out, (size_t)cap, "%s", t.c_str());
  return (int)t.size() + 1;
}
#define TRACE(label) idto_hip_trace_mark(label)

#define HIP_OK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) {                                                                       \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                  \
      return -2;                                                                                  \
    }                                                                                             \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// The memory calls of host/ctx_buffers.h's owners (and DevAlloc of Alloc's): -2 with g_err written when HIP refuses
struct HipMem {
  static int PinAlloc(void** p, size_t bytes) { HIP_OK(hipHostMalloc(p, bytes, hipHostMallocDefault)); return 0; }
  static void PinFree(void* p) { (void)hipHostFree(p); }
  static int DevAlloc(void** out, size_t bytes) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, bytes));
    // hipMemset on device memory runs on the NULL stream and does not block the host; the context's
    // stream is non-blocking, i.e. NOT ordered after the NULL stream: without the synchronisation the
    // zero fill can land after work the caller enqueues next on the context's stream (seen as a
    // one-in-fifty wrong first solve on the smallest model)
    hipError_t e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) (void)hipFree(p);
    HIP_OK(e);
    *out = p;
    return 0;
  }
  static void DevFree(void* p) { (void)hipFree(p); }
};
template <class T> using Pinned = idto_host::Pinned<T, HipMem>;
template <class T> using Grown = idto_host::Grown<T, HipMem>;
}  // namespace

// Host copies of what a context was created from: a batch context builds single-problem child contexts from them for
// the trust-region loop with ENFORCED CONSTRAINTS (idto_hip_tr_solve_batch_constrained)
struct HostModelCopy {
  idto_model_t m;
  std::vector<int> parent, jtype, qstart, vstart, actuated, geom_body, geom_type, pair_a, pair_b, body_path, pair_path;
  std::vector<int> gravity_enabled;
  std::vector<double> X_PF, axis, mass, com, inertia, damping, geom_X, geom_size;
  void Set(const idto_model_t& s) {
    m = s;
    const int nb = s.nbodies, ng = s.ngeoms, np = s.npairs;
    auto ci = [](const int* p, size_t n) { return p ? std::vector<int>(p, p + n) : std::vector<int>(); };
    auto cd = [](const double* p, size_t n) { return p ? std::vector<double>(p, p + n) : std::vector<double>(); };
    parent = ci(s.parent, nb); jtype = ci(s.jtype, nb); qstart = ci(s.qstart, nb); vstart = ci(s.vstart, nb);
    actuated = ci(s.actuated, s.nv); geom_body = ci(s.geom_body, ng); geom_type = ci(s.geom_type, ng);
    pair_a = ci(s.pair_a, np); pair_b = ci(s.pair_b, np); body_path = ci(s.body_path, nb); pair_path = ci(s.pair_path, np);
    gravity_enabled = ci(s.gravity_enabled, nb);
    X_PF = cd(s.X_PF, (size_t)12 * nb); axis = cd(s.axis, (size_t)3 * nb); mass = cd(s.mass, nb); com = cd(s.com, (size_t)3 * nb);
    inertia = cd(s.inertia, (size_t)6 * nb); damping = cd(s.damping, s.nv); geom_X = cd(s.geom_X, (size_t)12 * ng);
    geom_size = cd(s.geom_size, (size_t)3 * ng);
    m.parent = parent.data(); m.jtype = jtype.data(); m.qstart = qstart.data(); m.vstart = vstart.data();
    m.actuated = actuated.empty() ? nullptr : actuated.data(); m.geom_body = geom_body.data(); m.geom_type = geom_type.data();
    m.pair_a = pair_a.data(); m.pair_b = pair_b.data(); m.body_path = body_path.data(); m.pair_path = pair_path.data();
    m.X_PF = X_PF.data(); m.axis = axis.data(); m.mass = mass.data(); m.com = com.data(); m.inertia = inertia.data();
    m.damping = damping.data(); m.geom_X = geom_X.data(); m.geom_size = geom_size.data();
    m.gravity_enabled = gravity_enabled.empty() ? nullptr : gravity_enabled.data();
  }
};
struct HostProblemCopy {
  idto_problem_t p;
  std::vector<double> q_init, v_init, Qq, Qv, Qf_q, Qf_v, R, q_nom, v_nom;
  void Set(const idto_problem_t& s, int nq, int nv) {
    p = s;
    const size_t N1 = (size_t)s.num_steps + 1;
    auto cd = [](const double* x, size_t n) { return x ? std::vector<double>(x, x + n) : std::vector<double>(n, 0.0); };
    q_init = cd(s.q_init, nq); v_init = cd(s.v_init, nv); Qq = cd(s.Qq, (size_t)nq * nq); Qv = cd(s.Qv, (size_t)nv * nv);
    Qf_q = cd(s.Qf_q, (size_t)nq * nq); Qf_v = cd(s.Qf_v, (size_t)nv * nv); R = cd(s.R, (size_t)nv * nv);
    q_nom = cd(s.q_nom, N1 * nq); v_nom = cd(s.v_nom, N1 * nv);
    p.q_init = q_init.data(); p.v_init = v_init.data(); p.Qq = Qq.data(); p.Qv = Qv.data(); p.Qf_q = Qf_q.data();
    p.Qf_v = Qf_v.data(); p.R = R.data(); p.q_nom = q_nom.data(); p.v_nom = v_nom.data();
  }
};

// RCCL is resolved at run time, when the first communicator call needs it: libidto_hip.so has no NEEDED entry for it
// (VERDICT r4 "weak" #8: the link-time dependency carried a RUNPATH of the build image's /opt/rocm-7.2.0/lib, and on a
// box with another ROCm the library loaded only where torch had mapped its own librccl first - a plain C++ consumer has
// no such luck, and one that never shards needs no RCCL at all).  Order: a librccl the process has mapped already (a
// host that imported torch: both must talk to the SAME library), $IDTO_RCCL_LIB, the loader's search path, /opt/rocm/lib.
struct RcclApi {
  void* handle = nullptr;
  std::string path, tried;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
};
static RcclApi& RcclState() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    std::vector<std::pair<std::string, int>> cand = {{"librccl.so.1", RTLD_NOW | RTLD_NOLOAD}, {"librccl.so", RTLD_NOW | RTLD_NOLOAD}};
    if (const char* e = std::getenv("IDTO_RCCL_LIB")) cand.push_back({e, RTLD_NOW});
    for (const char* n : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) cand.push_back({n, RTLD_NOW});
    for (const auto& c : cand) {
      void* h = dlopen(c.first.c_str(), c.second | RTLD_GLOBAL);
      if (!h) { if (!(c.second & RTLD_NOLOAD)) api.tried += " " + c.first; continue; }
      api.handle = h;
      break;
    }
    if (!api.handle) return;
    bool all = true;
    auto sym = [&](const char* name, auto& fn) {
      fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(api.handle, name));
      if (!fn) { all = false; api.tried += std::string(" (no ") + name + ")"; }
    };
    sym("ncclGetVersion", api.GetVersion); sym("ncclGetErrorString", api.GetErrorString); sym("ncclGetUniqueId", api.GetUniqueId);
    sym("ncclCommInitRank", api.CommInitRank); sym("ncclCommInitAll", api.CommInitAll); sym("ncclCommDestroy", api.CommDestroy);
    sym("ncclAllGather", api.AllGather); sym("ncclGroupStart", api.GroupStart); sym("ncclGroupEnd", api.GroupEnd);
    if (!all) { api.handle = nullptr; return; }
    Dl_info info;
    api.path = (dladdr(reinterpret_cast<void*>(api.AllGather), &info) && info.dli_fname) ? info.dli_fname : "?";
  });
  return api;
}
#define RCCL_OR_FAIL(R)                                                                                        \
  RcclApi* R = RcclState().handle ? &RcclState() : nullptr;                                                    \
  if (!R) { g_err = "librccl could not be loaded (set IDTO_RCCL_LIB; tried:" + RcclState().tried + ")"; return -4; }


// idto_hip_mpc_batch_*: the stored plans of a batch of controllers (mpc_batch.h), an allocation of its own
struct MpcBatchState {
  explicit MpcBatchState(idto_hip_ctx* ctx) : c(ctx) {}
  ~MpcBatchState();                          // returns the device buffers below to the device (they are in c->allocs)
  idto_hip_ctx* c;
  MpcPlanLayout L{};
  std::vector<int> selector;                 // host copy (the host copies of the problems are shifted with it)
  double* breaks = nullptr; int* selector_dev = nullptr; int* actuated_dev = nullptr;
  double* plan[2] = {nullptr, nullptr};      // two planes of [batch][L.len()]; `cur` is the one in force
  int cur = 0;
  double* work = nullptr;                    // spline_fit's work space, [batch][n * dims]
  double* tick_dev = nullptr; Pinned<double> tick_pin;      // [batch][1 + nq + nv]: time, q0, v0
  double* io_dev = nullptr; Pinned<double> io_pin; size_t io_count = 0;   // idto_hip_mpc_batch_store / _shift: plans in, plans / guesses out
};
// what idto_hip_mpc_batch_replan hangs behind the batch fetch's own doubles: [guess [B][(N+1) nq] | plans [B][L.len()]]
struct MpcTickHook {
  MpcBatchState* m;
  const double* times; const double* x0;     // host: [B], [B][nq + nv]
  double* guess_out; double* plans_out;      // host, may be null
  size_t nguess, nplans;                     // doubles of the two parts
  // idto_hip_mpc_batch_tick_plants: times and x0 are null - the plants' kernel wrote the tick buffer on the device -, and the
  // plants' [t, q, v] come back under the tick's one wait: x_after_out [B][nq + nv], host, may be null
  // plant_status_out [B][2], host, may be null: {code, substeps completed} of the tick's substeps; followed: the host copies of
  // the problems have been moved with the plants' states (behind the wait; MpcReplanRun does it where the loop returned early)
  struct PlantState* plant = nullptr; double* x_after_out = nullptr; int* plant_status_out = nullptr; mutable bool followed = false;
};

// idto_hip_plant_*: the plants' storage (plant.h), ONE allocation made by idto_hip_plant_begin and cut up here - the plants'
// parameter records, their states [B][1 + nq + nv] (the layout of the controllers' tick buffer), the held torques, the state
// record of a launch, forward dynamics' inputs and outputs, the PD+ gains, the status words
struct PlantState {
  explicit PlantState(idto_hip_ctx* ctx) : c(ctx) {}
  ~PlantState();                             // returns `base` to the device (it is in c->allocs)
  idto_hip_ctx* c;
  double* base = nullptr;
  double *records = nullptr, *state = nullptr, *tau = nullptr, *record = nullptr;
  double *fd_x = nullptr, *fd_a = nullptr, *fd_M = nullptr, *fd_bias = nullptr, *Kp = nullptr, *Kd = nullptr;
  int* status = nullptr;
  size_t mstride = 0;
  int record_capacity = 64, nu = 0;
  unsigned mpc_generation = 0;               // (PD+) the idto_hip_mpc_batch_begin whose plans the LDS was sized for
  double h = 0; int mode = 0, feed_forward = 0, block = 64, lds = 0;
  bool begun = false;                         // idto_hip_plant_begin made it (idto_hip_forward_dynamics alone: not)
  Pinned<double> pin;                          // pinned staging of what comes back
  size_t fd_pinned = 0;                        // ... its doubles for idto_hip_forward_dynamics (the storage plan's)
  Pinned<double> tick_pin;                     // ... of the plants' states behind a tick (idto_hip_mpc_batch_tick_plants)
};

// A device buffer with its pinned mirror, both grown on demand (GrownEnsure): where a call of the scene report, the
// linearisation or the tracked rollouts keeps its arrays, laid out by host/plant_calls.h's CallPlan
using GrownBuffer = idto_host::GrownPair<HipMem>;
// idto_hip_scene_report, made at the first report: the body of every geometry, the states (in, whose mirror stages both ways) and the outputs
struct SceneState { int* geom_body = nullptr; GrownBuffer in, out; };
// idto_hip_plant_linearize, idto_hip_plant_tvlqr, made at the first call: the context's own parameter record, a call's arrays
struct LinState { double* record = nullptr; GrownBuffer buf; };

// What a context owns besides its arena and its pool (idto_hip_ctx::allocs): every buffer that is made on first use or grown
// on demand, and the storage of the MPC, plant, scene, linearisation and tracking entries.  idto_hip_destroy empties it in
// one assignment (ReleaseBuffers), the stream drained and still alive; an entry that needs another buffer adds a member here.
struct CtxBuffers {
  std::unique_ptr<MpcBatchState> mpc; std::unique_ptr<PlantState> plant;   // (their destructors return their share of the pool)
  std::unique_ptr<SceneState> scene; std::unique_ptr<LinState> lin;
  std::unique_ptr<GrownBuffer> track;   // idto_hip_plant_track, idto_hip_plant_tvlqr_track: a call's arrays, made at the first call
  Grown<double> stage_rhs, stage_x;     // idto_hip_solve_host (the same capacity, EnsureStage)
  Pinned<double> pin;                   // pinned host staging of idto_hip_trial_cost: q in, [tau | cost] out
  Grown<double> ls_arenas, ls_costs;    // idto_hip_costs_along: candidate arenas (linesearch.h LsArena, LsCap of them), their costs
  Pinned<double> ls_pin;                // ... and the costs' pinned staging ([IDTO_LS_MAX_CANDIDATES])
  // idto_hip_ls_solve: the statistics rows, the pinned staging of [rows | q | v | tau] and (idto_hip_ls_solve_batch_fetch) its device
  // side, packed by ls_gather_batch_kernel (a batch context: arenas [batch][LsCap], costs [batch][64], rows [batch][iterations])
  Grown<double> ls_rows, ls_fetch_dev; Pinned<double> ls_fetch_pin;
  Pinned<char> prob_pin;                // ... of the problem arrays (UploadProblemArrays)
  Pinned<double> many_pin;              // ... of idto_hip_get_many
  Pinned<double> rows_pin;              // ... of idto_hip_tr_solve's statistics rows
  Pinned<char> up_pin[2];               // option "async_uploads": the two staging buffers taken in turn (UploadStage)
  Pinned<double> pre_pin;               // idto_hip_prefetch: the staged copies
  // equality-constraint step (constraints.h): the constrained dofs; [S | J y_g]; dense LDL^T: pivots, [min, max | h], the
  // factor L (dense_ldl_step_kernel only reads S's panels), L^-1 (h - J y_g), carried along by the factorisation; pinned staging
  Grown<int> con_dofs;
  Grown<double> con_S, con_d, con_h, con_L, con_rv;
  Pinned<double> con_pin;
  GrownBuffer fetch;                    // idto_hip_tr_solve_fetch's staging (and the batch form's), EnsureFetch
  Pinned<double> bstate_pin;            // idto_hip_tr_solve_batch_fetch: the initial state words of every problem ([batch][TRS_COUNT])
  Grown<double> tr_rows;                // idto_hip_tr_solve: the per-iteration statistics rows
  Pinned<double> tr_pin;                // the trust-region scalars, [16]
};

struct idto_hip_ctx : CtxBuffers {
  int device = 0;
  unsigned mpc_generation = 0;   // calls of idto_hip_mpc_batch_begin so far
  // (batch contexts) what the context was created from, and one single-problem context per problem, made on first use
  std::unique_ptr<HostModelCopy> host_model;
  std::vector<std::unique_ptr<HostProblemCopy>> host_problems;
  idto_contact_params_t host_contact{};
  // per-problem models (idto_hip_set_model_batch): the base model's tables (every batch context keeps them, for the
  // check of a variant) and, from the first successful call on, one parameter record per problem (model_layout.h
  // model_record_*: blob | contact | gravity), mstride bytes apart - LaunchFd then starts fd_models_kernel /
  // fd_along_models_kernel, which read problem b's model, contact parameters and gravity from record b
  std::unique_ptr<idto_host::ModelTables> host_tables;
  double* model_records = nullptr; size_t mstride = 0;
  std::vector<idto_hip_ctx*> children;
  // batch: `batch` problems of the same model / horizon, one arena each (identical layout,
  // `pstride` bytes apart); the pointers below address problem 0
  int batch = 1;
  size_t pstride = 0;
  char* arena = nullptr;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int nb = 0, nq = 0, nv = 0, N = 0, npaths = 1, maxc = 1;
  bool capsules = false;   // the model has a capsule (include/idto_model.h): no fast shape, no fused launch
  bool cylinders = false;  // the model has a cylinder: the same
  double dt = 0;
  std::vector<void*> allocs;
  DevModel M;
  DevContact cp;
  DevProblem P;
  // problem arrays (device)
  double *d_vinit = nullptr, *d_qnom = nullptr, *d_vnom = nullptr;
  double* d_w[10] = {nullptr};
  // state
  double *q = nullptr, *v = nullptr, *a = nullptr, *nplus = nullptr, *slab = nullptr;
  double *g = nullptr, *HA = nullptr, *HB = nullptr, *HC = nullptr, *step = nullptr, *cost = nullptr;
  double *g2 = nullptr, *HA2 = nullptr, *HB2 = nullptr, *HC2 = nullptr;   // the trial point's g and H while a deciding launch runs (penta_pipe.h PipeAsm::g2)
  double *Kst = nullptr, *LUst = nullptr, *Yst = nullptr, *Zst = nullptr;
  int* pivst = nullptr;
  double *Ust = nullptr, *Hst = nullptr, *Est = nullptr, *Dst = nullptr;  // LDL^T factors (padded K x K blocks)
  double* dbg = nullptr;  // cycle stamps of the solver (8 per block row)
  bool solver_debug = false;
  int slab_stride = 0;
  int k_begin = 0, k_end = 0;
  bool weights_diagonal = false;
  std::vector<char> prob_diag;            // per problem of the batch
  bool reference_solver = false;  // bit-exact pivoted-LU block Thomas (kernels.h penta_kernel)
  int asm_diag_lds = 0;
  int asm_terms_lds = 0;
  int asm_terms_threads = 256;              // a thread per item of the largest part (allegro: 299 items - a second pass of 43 cost 2 us)
  double* terms = nullptr;                // per-record assembly products written by fd_kernel (asm_terms_stride)
  bool asm_fold = true;                   // option "asm_fold": fd_kernel forms them, assemble_terms_kernel combines
  bool terms_valid = false;               // ... and they belong to the resident slab, for every k
  int last_assembly = 0;                  // 1 assemble_terms_kernel, 2 assemble_diag_kernel (also inside the fused launch), 3 assemble_kernel,
                                          // 4 inside the solver's launch, 5 inside gn_small_kernel
  // launch geometry
  int asm_lds = 0, penta_lds = 0, solve_lds = 0, cost_lds = 0;
  // timing
  bool timing = false;
  int timing_stride = 1;     // record events on every timing_stride-th launch of each kernel
  unsigned timing_tick[4] = {0, 0, 0, 0};
  bool timing_open = false;  // TimeBegin recorded an event that TimeEnd must close
  struct Timed { hipEvent_t a, b; int which; };
  std::vector<Timed> pending;
  bool fd_full = false;                   // v / N+ in HBM belong to the resident q for every t
  bool partials_ahead = false;            // idto_hip_eval_tau_partials has left the partials of the resident q: the next idto_hip_eval_partials is done
  int gradients_method = 0;               // 0 forward, 1 central, 2 central 4th order (solver_parameters.h:26-50)
  int fd_stop = 0;                        // same for the finite-difference kernel
  int nd_min_rows = 16;                   // option "nd_min_rows": systems of at least this many block rows take the five-workgroup / band kernels
  bool fd_fast = true;                    // option "fd_fast": id_fast.h's evaluation when the model has an instantiated shape
  // option "fd_dedup": forward differences on the lane map without the redundant path lanes, where the model has it
  // (model_has_fd_dedup: host/model_tables.cc BuildFdDedup; any other model ignores the option).  0: every evaluation on all its paths.
  bool fd_dedup = true;
  bool model_has_fd_dedup = false;
  bool last_fd_dedup = false;             // the most recent finite-difference launch ran on that lane map (fd_dedup_kernel)
  int asm_stop = 0;                       // profiling aid: truncate the assembly kernel after a phase
  bool two_sided = true;                  // solver: two workgroups eliminating from both ends
  bool fused = true;                      // gn_step: one persistent launch (fused.h) when eligible
  bool solver_nd = true;                  // solver: nested dissection over 7 workgroups (penta_nd.h) when eligible
  bool solver_pipe = true;                // ... with pipelined chains (penta_pipe.h: 5 workgroups) when the block size allows
  BandStageItem* small_stage = nullptr; int small_stage_n = 0, small_stage_N = -1;   // gn_small.h: the solver's staging table for horizon small_stage_N
  int gn_small = 1;                       // option "gn_small": the whole step of a small model in one workgroup (gn_small.h; see SmallEligible)
  int solver_band = 1;                    // small blocks: the scalar band factorisation in one workgroup (penta_band.h; host/solver_plan.cc BandEligible)
  unsigned long long* nd_rowcnt = nullptr; // its per-row release counters, buffers and launch count
  unsigned* asm_ready = nullptr;               // penta_pipe.h PipeAsm: [N + 1][4] epoch words of the assembly inside the solver's launch
  bool tr_conv_on = false;                 // idto_hip_tr_set_convergence
  double tr_conv_tol[6] = {0, 0, 0, 0, 0, 0};
  bool asm_in_solver = true;                  // option "asm_in_solver": idto_hip_gn_step assembles g and H inside the pipelined solver's launch
  unsigned long long* pipe_rowcnt = nullptr;   // the same for the pipelined variant (its own launch count: the two
  unsigned long long pipe_launches = 0;        // variants release a row with different increments)
  int solver_timeouts = 0;                // launches whose waits between workgroups ran out (FactorStatus)
  unsigned timeouts_handled = 0;          // ... the device's count of them (status word) that FactorStatus has acted on
  int last_step_kind = 0;                 // what produced IDTO_ARR_STEP last: 1 factor_solve of -g, 2 the fused launch, 0 other
  int debug_skip_role = -1;               // test aid: a role of the nested-dissection kernels that returns at once
  int debug_pipe_tail = 0;                // measurement aid: pipelined solver with 1 the row-by-row back substitution, 2 the recursion form without the producers' closed form
  double* nd_buf = nullptr;
  double* nd_wst = nullptr;   // the seven-workgroup kernel's W rows (penta_pipe.h chain_recursion_tail), blocks of 21 .. 32 only
  int nd_recursion = 1;       // option "nd_recursion": its back substitution in recursion form where the matrices fit the LDS
  unsigned long long nd_launches = 0;
  int last_solver = 0;                     // 0 none yet, 1 two-workgroup LDL^T, 2 nested dissection, 3 reference LU
  bool kkt_debug = false;                 // option "solver_debug" 2
  bool fused_debug = false;               // ... with per-workgroup time stamps in IDTO_ARR_DEBUG
  double* xch = nullptr;                  // their exchange buffer / flags
  unsigned* flags = nullptr;
  size_t xch_count = 0, flag_count = 0;
  unsigned epoch = 0;
  unsigned long long* sync_cnt = nullptr;            // fused launch: [fd blocks done, assembly blocks done] (monotonic)
  unsigned long long sync_steps = 0;                 // fused launches so far
  double* Tst = nullptr;                             // column-major copies of the factor blocks (penta_apply.h)
  double* pack = nullptr;                            // [tau | cost] of idto_hip_trial_cost (device)
  // idto_hip_ls_solve: the loop's state words, the scan, the trust ratio's [step | H step] (a batch context: per problem);
  // option "ls_waves"; calls so far (the tests' proof of which loop ran), of idto_hip_ls_solve_batch_fetch too
  double *ls_state = nullptr, *ls_work = nullptr; idto_ls::LsScan* ls_scan = nullptr;
  int ls_waves = 0, ls_solves = 0, compute_units = 0;
  int ls_batch_solves = 0;
  // equality-constraint step (constraints.h)
  int con_nu = 0, con_neq = 0;
  std::vector<int> con_dofs_host;
  bool con_schur_valid = false;            // con_S, con_d, ... are allocated for con_dofs_host
  double *con_lambda = nullptr, *con_out = nullptr;                    // device: lambda, [step | J^T lambda]
  bool con_S_factored = false;                                         // con_S holds the LDL^T factors, not S
  // SolverParameters::linear_solver = kDenseLdlt (idto_hip_solve_dense_ldlt): [H dense | L], pivots, [min, max], [r | y]
  double *dn_S = nullptr, *dn_d = nullptr, *dn_stat = nullptr, *dn_rv = nullptr; int dn_n = 0;
  // option "async_uploads": idto_hip_set_q / idto_hip_set_problem copy from pinned staging of the context - two buffers
  // taken in turn, an event each - and return without waiting (everything else the context does is ordered behind them on
  // its stream); a caller that reads device memory on ANOTHER stream keeps the default, the blocking copies
  bool async_uploads = false;
  hipEvent_t up_ev[2] = {nullptr, nullptr}; int up_next = 0;
  bool h_assembled = false;                                            // H comes from idto_hip_grad_hess: block row 0 is the identity
  bool con_begun = false;                                              // constraint_schur_begin enqueued for the current H
  // idto_hip_prefetch: copies enqueued on a side stream behind an event of the main stream
  struct Prefetch { int what = -1; size_t off = 0, count = 0; bool pending = false; hipEvent_t ev = nullptr; };
  Prefetch pre[4];
  hipStream_t side = nullptr;
  bool con_ready = false;                                              // stage_x holds H^-1 [g | J^T] of the current H
  std::vector<hipEvent_t> event_pool;  // recycled: creating events in the timed loop costs host time
  double tsum[4] = {0, 0, 0, 0};
  int tcnt[4] = {0, 0, 0, 0};
  // factorisation status, written by the solver kernels into pinned host memory only when a pivot
  // fails: [0] = id of the last failing factorisation, [1] = failing block rows since creation
  unsigned* status_pin = nullptr;
  unsigned* status_dev = nullptr;   // the same memory as the device addresses it
  unsigned fact_id = 0;             // id of the most recent factorisation launched
  // multi-GPU: this context is rank `comm_rank` of `comm_world` in an RCCL communicator;
  // its finite-difference kernel covers the k-range [k_begin, k_end) and one in-place all-gather
  // completes the slab (records are contiguous in k, every rank's range has `comm_per` records,
  // the last ones padded: the slab is allocated with IDTO_SLAB_PAD spare records)
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1, comm_per = 0;
  // device-side trust-region bookkeeping (trust_region.h): scale factors, scaled merit gradient,
  // w = D^-1 H^-1 g_merit, the last step, the trial trajectory; [16] scalars on the device + pinned
  double *tr_Dprev = nullptr, *tr_part = nullptr;   // the adaptive scalings' previous D; per-block-row partial sums
  // idto_hip_tr_solve: the iteration state and the arrival counter of tr_iter_kernel (device)
  double* tr_state = nullptr;
  // second set of fd_kernel's outputs (v, a, N+, slab, products), alt_off bytes behind the first, and
  // the selectors the launches pass (batch.h AltSel): inactive (state == nullptr) outside idto_hip_tr_solve
  long long alt_off = 0;
  AltSel alt_r{nullptr, 0, 0}, alt_w{nullptr, 0, 1};
  unsigned long long* tr_cnt = nullptr;
  unsigned long long tr_target = 0;
  double *tr_part_ll = nullptr, *tr_part2 = nullptr;   // tr_iter_kernel: the block rows' sums with the launch's epoch in every word; dq.dq, g~.dqs per row
  unsigned tr_epoch = 0;
  double *tr_D = nullptr, *tr_gt = nullptr, *tr_w = nullptr, *tr_dq = nullptr, *q_trial = nullptr, *tr_out = nullptr;
  int* tr_quat = nullptr; int tr_nquat = 0;
  bool trial_resident = false;         // v / a / tau / cost in device memory belong to q_trial
  // speculation: idto_hip_tr_trial enqueued the next iteration's gn_step + tr_prepare on the trial
  // point before the host knew whether it accepts it (spec_scaling: the arguments it used)
  bool spec_pending = false, spec_ready = false;
  int spec_scaling = -2;
  hipEvent_t spec_ev = nullptr;
  const double* con_lambda_at = nullptr;  // where the current multipliers live (con_lambda or con_lambda + 2)
  int* una_dofs = nullptr; int una_nu = 0; // unactuated dofs for |h| of the statistics (idto_hip_set_unactuated_dofs)
  std::vector<int> una_dofs_host;
  // the equality-constraint step of the resident loop as one banded solve (kkt.h): a solver-only context of block size
  // nq + nu on this context's stream, made on first use
  idto_hip_ctx* kkt = nullptr; int kkt_nu = 0;
  bool con_kkt = true;                     // option "con_kkt" (0: the Schur-complement chain of constraints.h)
  bool kkt_fold = true;                    // option "kkt_fold" (0: kkt_extract_kernel in a launch of its own in front of tr_iter_kernel)
  bool tr_small = true;                    // option "tr_small" (0: fd_kernel, cost_kernel and the solver's launch per iteration also for the small models)
  bool tr_fold = true;                     // option "tr_fold" (0: tr_iter_kernel stays a launch of its own in front of the small models' launch)
  bool kkt_in_asm = true;                  // option "kkt_in_asm" (0: kkt_build_kernel stays a launch of its own behind the assembly)
  bool decide_in_solver = true;            // option "decide_in_solver" (0: cost_kernel stays a launch of its own in front of the pipelined solver's)
  double* decide_word = nullptr; unsigned decide_epoch = 0;   // ... and the word it publishes it in (per problem, epoch in every word)
  bool tr_resident_ok = true;              // false once tr_iter_kernel's wait between its workgroups ran out (FactorStatus): idto_hip_tr_solve then refuses
  int ldl_npos = 0;                        // (a KKT context) the solver expects the pivots [ldl_npos, nq) of a block negative
};

// The options: X(name = the field of idto_hip_ctx, kind, access, environment variable that seeds the default at create or
// nullptr, follows the parent into its KKT context, is given to a batch context's children).  idto_hip_get_option,
// idto_hip_set_option, OptionsFromEnvironment, MakeKkt and CopyOptionsToChild are generated from it; what an option does
// beyond storing a value stands in front of the lookup in those functions.
enum { OPT_BOOL, OPT_FLAG, OPT_INT };   // environment "1" / value != 0; atoi != 0 / value != 0; atoi / value
enum { OPT_GET = 1, OPT_SET = 2, OPT_RW = 3 };
#define IDTO_OPTIONS(X)                                                          \
  X(reference_solver, OPT_BOOL, OPT_RW, "IDTO_SOLVER_REFERENCE", 0, 1)           \
  X(two_sided, OPT_BOOL, OPT_RW, "IDTO_TWO_SIDED", 0, 1)                         \
  X(fused, OPT_BOOL, OPT_RW, "IDTO_FUSED", 0, 1)                                 \
  X(async_uploads, OPT_BOOL, OPT_RW, nullptr, 0, 0)                              \
  X(nd_min_rows, OPT_INT, OPT_RW, "IDTO_ND_MIN_ROWS", 1, 0)                      \
  X(nd_recursion, OPT_FLAG, OPT_RW, "IDTO_ND_RECURSION", 1, 0)                   \
  X(solver_nd, OPT_BOOL, OPT_RW, "IDTO_SOLVER_ND", 0, 1)                         \
  X(solver_pipe, OPT_BOOL, OPT_RW, "IDTO_SOLVER_PIPE", 0, 1)                     \
  X(solver_band, OPT_INT, OPT_RW, "IDTO_SOLVER_BAND", 1, 1) /* measurement aid: penta_band.h off / on / on for blocks of 5 too */ \
  X(gn_small, OPT_FLAG, OPT_RW, nullptr, 0, 0)                                   \
  X(asm_in_solver, OPT_BOOL, OPT_RW, nullptr, 0, 1)                              \
  X(debug_skip_role, OPT_INT, OPT_SET, "IDTO_DEBUG_SKIP_ROLE", 1, 0) /* test aid (tests/test_gpu_timeout.py) */ \
  X(debug_pipe_tail, OPT_INT, OPT_SET, nullptr, 0, 0)                /* measurement aid */ \
  X(asm_fold, OPT_BOOL, OPT_RW, "IDTO_ASM_FOLD", 0, 1)                           \
  X(con_kkt, OPT_BOOL, OPT_RW, "IDTO_CON_KKT", 0, 1)                             \
  X(kkt_fold, OPT_BOOL, OPT_RW, "IDTO_KKT_FOLD", 0, 0)                           \
  X(ls_waves, OPT_INT, OPT_RW, nullptr, 0, 0)                                    \
  X(tr_small, OPT_BOOL, OPT_RW, "IDTO_TR_SMALL", 0, 0)                           \
  X(tr_fold, OPT_BOOL, OPT_RW, "IDTO_TR_FOLD", 0, 0)                             \
  X(kkt_in_asm, OPT_BOOL, OPT_RW, "IDTO_KKT_IN_ASM", 0, 0)                       \
  X(decide_in_solver, OPT_BOOL, OPT_RW, "IDTO_DECIDE_IN_SOLVER", 0, 0)           \
  X(fused_debug, OPT_BOOL, OPT_SET, nullptr, 0, 0)                               \
  X(asm_stop, OPT_INT, OPT_SET, nullptr, 0, 0) /* profiling aid */               \
  X(fd_stop, OPT_INT, OPT_SET, nullptr, 0, 0)  /* profiling aid */               \
  X(fd_fast, OPT_BOOL, OPT_RW, nullptr, 0, 1)                                    \
  X(fd_dedup, OPT_BOOL, OPT_RW, "IDTO_FD_DEDUP", 0, 1)                           \
  X(gradients_method, OPT_INT, OPT_RW, nullptr, 0, 1)                            \
  X(last_solver, OPT_INT, OPT_GET, nullptr, 0, 0)                                \
  X(last_assembly, OPT_INT, OPT_GET, nullptr, 0, 0)                              \
  X(last_fd_dedup, OPT_BOOL, OPT_GET, nullptr, 0, 0)                             \
  X(weights_diagonal, OPT_BOOL, OPT_GET, nullptr, 0, 0)                          \
  X(solver_timeouts, OPT_INT, OPT_GET, nullptr, 0, 0)                            \
  X(ls_solves, OPT_INT, OPT_GET, nullptr, 0, 0)                                  \
  X(ls_batch_solves, OPT_INT, OPT_GET, nullptr, 0, 0)                            \
  X(tr_resident_ok, OPT_BOOL, OPT_GET, nullptr, 0, 0)

namespace {

template <class T>
void OptAssign(T& field, int kind, int value) { field = kind == OPT_INT ? (T)value : (T)(value != 0); }

// the defaults that the environment seeds (debugging and measurement aids)
void OptionsFromEnvironment(idto_hip_ctx* c) {
#define X(name, kind, access, env, to_kkt, to_child)                                                    \
  if (const char* v = env)                                                                              \
    if (const char* e = getenv(v)) OptAssign(c->name, kind, kind == OPT_BOOL ? (e[0] == '1') : std::atoi(e));
  IDTO_OPTIONS(X)
#undef X
  c->nd_min_rows = std::max(16, c->nd_min_rows);   // (idto_hip_set_option's bound)
}

// One arena per problem: the plan of host/context_layout.cc, one allocation of batch * pstride bytes, zero-filled, and the
// context's fields - problem 0's - pointed into it in the table's order.
int PointIntoArena(idto_hip_ctx* c, idto_host::ArenaKind kind, const char* what) {
  const idto_host::ArenaPlan plan = idto_host::PlanArena(kind, c->nq, c->nv, c->N);
  c->pstride = plan.pstride; c->alt_off = plan.alt_off; c->slab_stride = plan.slab_stride;
  c->xch_count = plan.xch_count; c->flag_count = plan.flag_count;
  void* p = nullptr;
  const size_t bytes = c->pstride * (size_t)c->batch;
  if (hipMalloc(&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {   // (see Alloc: the fill must not trail the uploads on the context's stream)
    g_err = what;
    return -2;
  }
  c->allocs.push_back(p);
  c->arena = static_cast<char*>(p);
  if (getenv("IDTO_DEBUG_PTRS")) {   // (investigation aid: where a faulting address lies)
    fprintf(stderr, "%s arena %p .. %p (pstride %zu x %d):", kind == idto_host::ARENA_KKT ? "kkt" : "model", p, (void*)(c->arena + bytes), c->pstride, c->batch);
    for (const idto_host::ArenaEntry& e : plan.entries) fprintf(stderr, " %s %zu", e.name, e.offset);
    fprintf(stderr, "\n");
  }
  size_t i = 0;
#define X(field, type, count) c->field = reinterpret_cast<type*>(c->arena + plan.entries[i++].offset);
#define U(name, type, count) ++i;
#define B(field, entry, index) c->field = c->entry + (size_t)index * plan.band;
  if (kind == idto_host::ARENA_MODEL) { IDTO_MODEL_ARENA(X, U) IDTO_MODEL_BANDS(B) }
  else { IDTO_KKT_ARENA(X, U) IDTO_KKT_BANDS(B) }
#undef X
#undef U
#undef B
  if (!plan.has_wst) c->nd_wst = nullptr;
  return 0;
}

// The solver's status words in pinned host memory, zeroed: per problem [id of the last failed factorisation, count];
// behind them [id of the last launch in which a wait between workgroups ran out, count] (penta_ldl.h spin_wait)
int AllocStatusWords(idto_hip_ctx* c, const char* what) {
  const size_t words = 2 * (size_t)c->batch + 2;
  if (hipHostMalloc((void**)&c->status_pin, words * sizeof(unsigned), hipHostMallocDefault) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->status_dev, c->status_pin, 0) != hipSuccess) {
    g_err = what;
    return -2;
  }
  for (size_t i = 0; i < words; ++i) c->status_pin[i] = 0;
  return 0;
}

template <class T>
int Upload(idto_hip_ctx* c, const T* host, size_t count, T** dev) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
  c->allocs.push_back(p);
  if (count) HIP_OK(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
  *dev = static_cast<T*>(p);
  return 0;
}
template <class T>
int Alloc(idto_hip_ctx* c, size_t count, T** dev) {
  void* p = nullptr;
  if (int rc = HipMem::DevAlloc(&p, std::max<size_t>(count, 1) * sizeof(T))) return rc;   // (zero-filled, behind a device-wide wait)
  c->allocs.push_back(p);
  *dev = static_cast<T*>(p);
  return 0;
}
// a buffer of Alloc's that has been superseded: returned to the device now, not at idto_hip_destroy
template <class T>
void Release(idto_hip_ctx* c, T** dev) {
  if (!*dev) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), static_cast<void*>(*dev));
  if (it != c->allocs.end()) { (void)hipFree(*it); c->allocs.erase(it); }
  *dev = nullptr;
}
}  // namespace
// (the one place each of them is released: "begin again" resets the context's pointer, idto_hip_destroy resets them all)
MpcBatchState::~MpcBatchState() {
  for (double** p : {&breaks, &plan[0], &plan[1], &work, &tick_dev, &io_dev}) Release(c, p);
  Release(c, &selector_dev); Release(c, &actuated_dev);
}
PlantState::~PlantState() { Release(c, &base); }
namespace {

// pinned staging for an upload that must not wait (option "async_uploads"): the buffer that was used the time before
// last - its copy has long run, the event only makes that certain
static int UploadStage(idto_hip_ctx* c, size_t bytes, char** buf, int* slot) {
  const int s = c->up_next;
  c->up_next ^= 1;
  if (c->up_ev[s]) HIP_OK(hipEventSynchronize(c->up_ev[s]));
  else HIP_OK(hipEventCreateWithFlags(&c->up_ev[s], hipEventDisableTiming));
  if (int rc = c->up_pin[s].Ensure(bytes, 4096)) return rc;
  *buf = c->up_pin[s]; *slot = s;
  return 0;
}

// (problem `pb` of the batch: destination = problem 0's arrays shifted by pb * pstride)
int UploadProblemArrays(idto_hip_ctx* c, const idto_problem_t* p, int pb = 0) {
  TRACE("hip: problem upload begins");
  const int nq = c->nq, nv = c->nv, N = c->N;
  const size_t po = (size_t)pb * c->pstride;
  const double dt = c->dt;
  auto scaled = [](const double* W, size_t n, double s1, double s2) {
    std::vector<double> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = (s1 * W[i]) * s2;  // reference TO.cc:1103-1107
    return out;
  };
  const std::vector<double> w[10] = {
      scaled(p->Qq, (size_t)nq * nq, 2, dt), scaled(p->Qv, (size_t)nv * nv, 2, dt), scaled(p->R, (size_t)nv * nv, 2, dt),
      scaled(p->Qf_q, (size_t)nq * nq, 2, 1), scaled(p->Qf_v, (size_t)nv * nv, 2, 1),
      std::vector<double>(p->Qq, p->Qq + (size_t)nq * nq), std::vector<double>(p->Qv, p->Qv + (size_t)nv * nv),
      std::vector<double>(p->R, p->R + (size_t)nv * nv), std::vector<double>(p->Qf_q, p->Qf_q + (size_t)nq * nq),
      std::vector<double>(p->Qf_v, p->Qf_v + (size_t)nv * nv)};
  {
    // ONE copy: v_init, q_nom, v_nom and the ten weight matrices sit next to each other in the problem's arena (64-byte
    // aligned), a pinned host buffer mirrors that stretch (13 copies from pageable memory were 0.12 ms of an MPC re-plan)
    char* lo = reinterpret_cast<char*>(c->d_vinit);
    char* hi = reinterpret_cast<char*>(c->d_w[9]) + w[9].size() * sizeof(double);
    const size_t bytes = (size_t)(hi - lo);
    char* stage = nullptr; int slot = -1;
    if (c->async_uploads) { if (int rc = UploadStage(c, bytes, &stage, &slot)) return rc; }
    if (!stage && c->prob_pin.cap() < bytes) {
      if (int rc = c->prob_pin.Ensure(bytes)) return rc;
      std::memset(c->prob_pin, 0, bytes);
    }
    if (!stage) stage = c->prob_pin;
    else std::memset(stage, 0, bytes);   // (the alignment gaps between the arrays)
    auto put = [&](const double* dev, const double* src, size_t count) {
      std::memcpy(stage + (reinterpret_cast<const char*>(dev) - lo), src, count * sizeof(double));
    };
    put(c->d_vinit, p->v_init, nv);
    put(c->d_qnom, p->q_nom, (size_t)(N + 1) * nq);
    put(c->d_vnom, p->v_nom, (size_t)(N + 1) * nv);
    for (int i = 0; i < 10; ++i) put(c->d_w[i], w[i].data(), w[i].size());
    HIP_OK(hipMemcpyAsync(lo + po, stage, bytes, hipMemcpyHostToDevice, c->stream));
    if (slot >= 0) {
      HIP_OK(hipEventRecord(c->up_ev[slot], c->stream));
      TRACE("hip: problem upload done (one copy enqueued)");
    } else {
      HIP_OK(hipStreamSynchronize(c->stream));  // (the pinned buffer is reused by the next upload)
      TRACE("hip: problem upload done (one copy + wait)");
    }
  }
  auto is_diag = [](const double* W, int n) {
    for (int c2 = 0; c2 < n; ++c2)
      for (int r = 0; r < n; ++r)
        if (r != c2 && W[(size_t)c2 * n + r] != 0.0) return false;
    return true;
  };
  const bool diag = is_diag(p->Qq, nq) && is_diag(p->Qv, nv) && is_diag(p->R, nv) && is_diag(p->Qf_q, nq) &&
                    is_diag(p->Qf_v, nv);
  // (one assembly kernel serves the whole batch: the diagonal fast path needs every problem's
  // weights diagonal; a batch re-evaluates the flag when problem 0 is replaced)
  if ((int)c->prob_diag.size() != c->batch) c->prob_diag.assign((size_t)c->batch, 0);
  c->prob_diag[(size_t)pb] = diag ? 1 : 0;
  c->weights_diagonal = true;
  for (char d : c->prob_diag) c->weights_diagonal = c->weights_diagonal && d;
  DevProblem& P = c->P;
  P.N = N; P.dt = dt; P.v_init = c->d_vinit; P.q_nom = c->d_qnom; P.v_nom = c->d_vnom;
  P.Qq = c->d_w[0]; P.Qv = c->d_w[1]; P.R = c->d_w[2]; P.Qfq = c->d_w[3]; P.Qfv = c->d_w[4];
  P.Qq0 = c->d_w[5]; P.Qv0 = c->d_w[6]; P.R0 = c->d_w[7]; P.Qfq0 = c->d_w[8]; P.Qfv0 = c->d_w[9];
  return 0;
}

// The model tables as the device sees them: the blob that host/model_tables.cc built, uploaded, and DevModel's pointers
// into it.  (Every check of the model has been made by then, on the host's tables.)
int UploadModel(idto_hip_ctx* c, const idto_model_t* m, const idto_host::ModelTables& t) {
  double* bd = nullptr;
  if (Upload(c, t.blob.data(), t.blob.size(), &bd)) return -2;
  const int* bi = reinterpret_cast<const int*>(bd);
  DevModel& M = c->M;
  M.blob = bd; M.blob_n = (int)t.blob.size();
#define X(name) M.name = bd + t.at.name;
  IDTO_MODEL_DOUBLE_TABLES(X)
#undef X
#define X(name) M.name = bi + t.at.name;
  IDTO_MODEL_INT_TABLES(X)
#undef X
  M.nb = m->nbodies; M.nq = m->nq; M.nv = m->nv; M.npaths = m->npaths; M.common_body = m->common_body;
  M.ngeoms = m->ngeoms; M.npairs = m->npairs; M.maxpp = t.maxpp;
  for (int i = 0; i < 3; ++i) M.gravity[i] = m->gravity[i];
  M.nfloat = t.nfloat;
  for (int i = 0; i < 4; ++i) { M.float_qs[i] = t.float_qs[i]; M.float_vs[i] = t.float_vs[i]; }
  M.fast_shape = t.fast_shape; M.fast_lo = t.fast_lo; M.fast_n = t.fast_n; M.f_maxpp = t.f_maxpp;
  M.gslots = t.gslots; M.gcommon = t.gcommon; M.gstem = t.gstem; M.nxb = t.nxb; M.nstem = t.nstem;
  c->maxc = t.maxc; c->capsules = t.capsules; c->cylinders = t.cylinders; c->model_has_fd_dedup = t.fd_dedup;
  return 0;
}


// what host/fd_plan.cc reads of a context
static idto_host::FdShape FdShapeOf(const idto_hip_ctx* c) {
  idto_host::FdShape s;
  s.nq = c->nq; s.nv = c->nv; s.npaths = c->npaths; s.batch = c->batch;
  s.blob_n = c->M.blob_n; s.fast_n = c->M.fast_n; s.fast_shape = c->M.fast_shape; s.maxc = c->maxc; s.nxb = c->M.nxb; s.nstem = c->M.nstem;
  s.lane_map = c->model_has_fd_dedup; s.model_records = c->model_records != nullptr;
  s.fd_fast = c->fd_fast; s.fd_dedup = c->fd_dedup; s.asm_fold = c->asm_fold; s.weights_diagonal = c->weights_diagonal;
  s.gradients_method = c->gradients_method;
  return s;
}

// along (idto_hip_costs_along, mode 0): the launch evaluates `m` candidate points of the context's one problem instead
// of the resident q - grid.y = candidate, q and the outputs in arenas of their own (linesearch.h LsArena), nothing of the
// resident iterate is written
// (a batch context: grid.z = problem - the problems' arenas bstride bytes apart, their gate words gstride bytes)
struct FdAlong { const double* q; double *slab, *v, *a, *nplus; int slab_stride; size_t cstride; int m; const double* gate; size_t bstride = 0, gstride = 0; };
int LaunchFd(idto_hip_ctx* c, int mode, int kb, int ke, AltSel alt = AltSel{nullptr, 0, 0}, const FdAlong* along = nullptr) {
  if (!along) c->partials_ahead = false;   // (whatever idto_hip_eval_tau_partials left is about to be overwritten; it sets the flag after its own launch)
  if (ke <= kb) return 0;
  // the block, the evaluations per pass, the fold, the LDS, the grid, the shape and the kernel: host/fd_plan.cc
  idto_host::FdRequest rq;
  rq.kind = along ? idto_host::FdRequest::CANDIDATES : idto_host::FdRequest::RESIDENT;
  rq.mode = mode; rq.kb = kb; rq.ke = ke; rq.m = along ? along->m : 0;
  FdLaunch fl;
  if (idto_host::PlanFd(FdShapeOf(c), rq, &fl.plan, &g_err)) return -1;
  const idto_host::FdPlan& p = fl.plan;
  if (p.mode >= 1) c->terms_valid = p.fold && kb == 0 && ke == c->N;
  fl.stream = c->stream; fl.M = c->M; fl.cp = c->cp; fl.P = c->P;
  fl.q = c->q; fl.slab = c->slab; fl.slab_stride = c->slab_stride; fl.v = c->v; fl.a = c->a; fl.nplus = c->nplus;
  fl.k_begin = kb; fl.stop_after = c->fd_stop; fl.pstride = c->pstride; fl.terms = p.fold ? c->terms : nullptr;
  fl.alt = alt;
  if (c->model_records) {   // (a batch: idto_hip_set_model_batch)
    fl.records = c->model_records; fl.mstride = c->mstride;
    fl.rec_contact = model_record_contact_at((size_t)c->M.blob_n) * sizeof(double);
    fl.rec_model = model_record_devmodel_at((size_t)c->M.blob_n) * sizeof(double);
  }
  if (along) {
    fl.q = along->q; fl.slab = along->slab; fl.slab_stride = along->slab_stride; fl.v = along->v; fl.a = along->a;
    fl.nplus = along->nplus; fl.cstride = along->cstride; fl.gate = along->gate;
    if (c->batch > 1) { fl.bstride = along->bstride; fl.gstride = along->gstride; }
  }
  if (!along) c->last_fd_dedup = p.dedup;
  fd_launch(fl);
  HIP_OK(hipGetLastError());
  return 0;
}

int TimeBegin(idto_hip_ctx* c, int which) {
  c->timing_open = false;
  if (!c->timing) return 0;
  if ((c->timing_tick[which]++ % (unsigned)c->timing_stride) != 0) return 0;
  c->timing_open = true;
  idto_hip_ctx::Timed t;
  t.which = which;
  hipEvent_t* ev[2] = {&t.a, &t.b};
  for (hipEvent_t* e : ev) {
    if (c->event_pool.empty()) {
      HIP_OK(hipEventCreate(e));
    } else {
      *e = c->event_pool.back();
      c->event_pool.pop_back();
    }
  }
  HIP_OK(hipEventRecord(t.a, c->stream));
  c->pending.push_back(t);
  return 0;
}
int TimeEnd(idto_hip_ctx* c) {
  if (!c->timing || !c->timing_open) return 0;
  c->timing_open = false;
  HIP_OK(hipEventRecord(c->pending.back().b, c->stream));
  return 0;
}
int TimeDrain(idto_hip_ctx* c) {
  for (auto& t : c->pending) {
    HIP_OK(hipEventSynchronize(t.b));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, t.a, t.b));
    c->tsum[t.which] += ms;
    c->tcnt[t.which] += 1;
    c->event_pool.push_back(t.a);
    c->event_pool.push_back(t.b);
  }
  c->pending.clear();
  return 0;
}

// (the stream is drained before a device buffer that a launch may still read is released)
int GrownEnsure(idto_hip_ctx* c, GrownBuffer* b, size_t dev_count, size_t pin_count) {
  if (b->dev.cap() < dev_count) HIP_OK(hipStreamSynchronize(c->stream));
  return b->Ensure(dev_count, pin_count);
}
// staging buffers grow on demand and are reused; the superseded ones, which enqueued work may still read, are freed behind
// the new ones' device-wide wait
int EnsureStage(idto_hip_ctx* c, size_t count) {
  if (c->stage_rhs.Ensure(count, 0, true) || c->stage_x.Ensure(count, 0, true)) {
    c->con_ready = false; c->con_begun = false;   // (what stage_x held is gone)
    return -2;
  }
  return 0;
}
void ReleaseBuffers(idto_hip_ctx* c) { static_cast<CtxBuffers&>(*c) = CtxBuffers(); }
// a pending idto_hip_prefetch of an array is dropped when that array is about to be recomputed
// (idto_hip_get then reads the new contents instead of the stale staged copy)
// after a stream synchronisation: did the most recent factorisation report a failed pivot?
// (problem `pb` of the batch, or any of them for pb < 0)
int FactorStatus(idto_hip_ctx* c, int pb = -1) {
  const volatile unsigned* st = c->status_pin;
  // (the COUNT of launches whose waits ran out, not the id of the last one: idto_hip_tr_solve enqueues a factorisation
  // per iteration and waits once - a timeout in any of them shows here; and a second status query about a launch
  // that has been handled does not step the context down once more)
  const unsigned timeouts_now = st[2 * c->batch + 1];
  if (timeouts_now != c->timeouts_handled) {
    const bool iteration_kernel = ((timeouts_now ^ c->timeouts_handled) >> 16) != 0u;   // (trust_region.h tr_iter_kernel's own wait)
    c->timeouts_handled = timeouts_now;
    if (iteration_kernel) {
      // the workgroups of tr_iter_kernel did not find each other resident within their bound: the resident loop is off for
      // the rest of the context's life (option "tr_resident_ok" reads 0), the caller's loop returns to the host twice an
      // iteration - kernels without a wait between workgroups
      c->tr_resident_ok = false;
      ++c->solver_timeouts;
      g_err = "the trust-region iteration's workgroups timed out waiting for each other (device shared with other kernels); "
              "the resident loop is off for this context: repeat the call";
      return IDTO_HIP_SOLVER_TIMEOUT;
    }
    // A wait between the workgroups of a multi-workgroup solver ran out: its partners were not resident at the
    // same time (other contexts' kernels on the device).  The result of that launch is garbage.  Step down to a
    // variant with fewer co-resident workgroups for the rest of the context's life; the caller repeats the solve
    // (idto_hip_get(STEP) and idto_hip_tr_prepare do it themselves).
    if (c->solver_band > 0 && c->last_solver == 6) c->solver_band = 0;   // (its wait for the launch's own assembly)
    else if (c->solver_pipe && c->last_solver == 4) c->solver_pipe = false;
    else if (c->solver_nd && (c->last_solver == 2 || c->last_solver == 4)) c->solver_nd = false;
    else if (c->fused && c->last_solver == 5) c->fused = false;
    else if (c->two_sided) { c->solver_nd = false; c->fused = false; c->two_sided = false; }
    ++c->solver_timeouts;
    g_err = "a solver launch timed out waiting for a partner workgroup (device shared with other kernels); the "
            "context has stepped down to a variant with fewer co-resident workgroups: repeat the call";
    return IDTO_HIP_SOLVER_TIMEOUT;
  }
  bool any = false;
  for (int b = (pb < 0 ? 0 : pb); b < (pb < 0 ? c->batch : pb + 1); ++b) any = any || st[2 * b] == c->fact_id;
  if (c->fact_id != 0 && any) {
    g_err = "factorisation failed: the Hessian is not numerically positive definite (a pivot was non-positive, "
            "non-finite or fully cancelled)";
    return IDTO_HIP_FACTORIZATION_FAILED;
  }
  return 0;
}
void* DevPtr(idto_hip_ctx* c, int what);
void DropPrefetch(idto_hip_ctx* c, std::initializer_list<int> arrays) {
  for (auto& pf : c->pre)
    for (int a : arrays)
      if (pf.what == a) pf.pending = false;
}
}  // namespace

extern "C" {

const char* idto_hip_last_error(void) { return g_err.c_str(); }

int idto_hip_create(const idto_model_t* model, const idto_problem_t* problem, const idto_contact_params_t* contact,
                    int device, idto_hip_ctx** out) {
  return idto_hip_create_batch(model, problem, contact, device, 1, out);
}

int idto_hip_create_batch(const idto_model_t* model, const idto_problem_t* problems, const idto_contact_params_t* contact,
                          int device, int batch, idto_hip_ctx** out) {
  *out = nullptr;
  idto_host::ModelTables tables;   // (every refusal of a model is made here: the same with or without a GPU)
  if (int rc = idto_host::BuildModelTables(model, &tables, &g_err)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device available (the product path has no CPU fallback)";
    return -3;
  }
  if (batch < 1 || batch > 65535) { g_err = "batch must be in [1, 65535]"; return -1; }
  for (int b = 1; b < batch; ++b)
    if (problems[b].num_steps != problems[0].num_steps || problems[b].time_step != problems[0].time_step) {
      g_err = "all problems of a batch share num_steps and time_step";
      return -1;
    }
  const idto_problem_t* problem = problems;
  HIP_OK(hipSetDevice(device));
  idto_hip_ctx* c = new idto_hip_ctx();
  c->device = device;
  c->batch = batch;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { g_err = "hipStreamCreate failed"; delete c; return -2; }
  c->own_stream = true;
  c->nb = model->nbodies; c->nq = model->nq; c->nv = model->nv; c->N = problem->num_steps;
  c->dt = problem->time_step; c->npaths = model->npaths;
  const int nq = c->nq, nv = c->nv, N = c->N;
  int rc = UploadModel(c, model, tables);
  if (rc) { idto_hip_destroy(c); return rc; }
  // (host copies: of the model and the contact parameters always - idto_hip_create_batch_like builds a batch context from
  // them -, of the problems for a batch, whose constrained loop may build child contexts)
  c->host_model = std::make_unique<HostModelCopy>();
  c->host_model->Set(*model);
  c->host_contact = *contact;
  c->host_tables = std::make_unique<idto_host::ModelTables>(tables);
  if (batch > 1) {
    for (int b = 0; b < batch; ++b) {
      c->host_problems.push_back(std::make_unique<HostProblemCopy>());
      c->host_problems.back()->Set(problems[b], model->nq, model->nv);
    }
  }
  {
    double cv[6];
    idto_host::ContactValues(*contact, cv);   // (host/model_batch.h: the threshold's one expression)
    c->cp.k = cv[0]; c->cp.vd = cv[1]; c->cp.vs = cv[2]; c->cp.mu = cv[3]; c->cp.sigma = cv[4]; c->cp.threshold = cv[5];
  }
  // ---- one arena per problem (identical layout, host/context_layout.h): batch * pstride bytes at once (zero-filled), the
  // problem-0 pointers into the first arena
  if (PointIntoArena(c, idto_host::ARENA_MODEL, "hipMalloc of the problem arenas failed")) { idto_hip_destroy(c); return -2; }
  const size_t nvars = (size_t)(N + 1) * nq;
  {  // adaptive scaling methods start from D = 1 (TO.cc:1233-1236: scale_factors initialised to ones)
    std::vector<double> ones(nvars, 1.0);
    for (int b = 0; b < batch; ++b)
      if (hipMemcpy(at_problem(c->tr_D, (size_t)b * c->pstride), ones.data(), nvars * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(at_problem(c->tr_Dprev, (size_t)b * c->pstride), ones.data(), nvars * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        g_err = "hipMemcpy (scale factors) failed"; idto_hip_destroy(c); return -2;
      }
    std::vector<int> qs;
    for (int i = 0; i < model->nbodies; ++i)
      if (model->jtype[i] == IDTO_JOINT_FLOATING) qs.push_back(model->qstart[i]);
    c->tr_nquat = (int)qs.size();
    if (!qs.empty() && Upload(c, qs.data(), qs.size(), &c->tr_quat)) { idto_hip_destroy(c); return -2; }
    if (c->tr_pin.Ensure(16)) {
      g_err = "hipHostMalloc (trust-region scalars) failed";
      idto_hip_destroy(c);
      return -2;
    }
  }
  for (int b = 0; b < batch; ++b) {
    rc = UploadProblemArrays(c, problems + b, b);
    if (rc) { idto_hip_destroy(c); return rc; }
  }
  if (AllocStatusWords(c, "hipHostMalloc (solver status) failed")) { idto_hip_destroy(c); return -2; }
  c->k_begin = 0; c->k_end = N;

  // launch geometry: the widest block of the finite-difference kernel and its smallest LDS carve-up (host/fd_plan.cc;
  // LaunchFd uses more when it fits)
  const int fd_lds = idto_host::FdCreateGeometry(FdShapeOf(c)).fd_lds;
  // (the launches whose sizes are a pure function of nq, nv, N: host/context_layout.cc)
  const idto_host::LaunchSizes ls = idto_host::PlanLaunchSizes(nq, nv, N);
  c->asm_lds = ls.asm_lds; c->asm_diag_lds = ls.asm_diag_lds; c->asm_terms_lds = ls.asm_terms_lds; c->asm_terms_threads = ls.asm_terms_threads;
  c->penta_lds = ls.penta_lds; c->solve_lds = ls.solve_lds; c->cost_lds = ls.cost_lds;
  const int max_lds = kMaxDynamicLds;
  if (fd_lds > max_lds || c->asm_lds > max_lds || c->penta_lds > max_lds || c->cost_lds > max_lds ||
      ls.apply_lds > max_lds) {
    g_err = "problem too large for the 160 KiB LDS carve-up of the v1 kernels (fd / assemble / solver / cost / "
            "multi-rhs substitution)";
    idto_hip_destroy(c);
    return -1;
  }
  // kernels that need more than the default 64 KiB of dynamic LDS must opt in
  fd_set_max_lds(max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&assemble_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
#define MAX_LDS(KERNEL) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  // (every instantiation of the solver families: solver_layout.h)
#define BAND_ATTR(WM) MAX_LDS(penta_band_kernel<WM>)
  IDTO_BAND_KERNELS(BAND_ATTR)
#undef BAND_ATTR
#define SMALL_ATTR(SH, WM, WSM, TR) MAX_LDS((gn_small_kernel<SH, WM, 256, WSM, TR>))
  IDTO_SMALL_KERNELS(SMALL_ATTR)
#undef SMALL_ATTR
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&penta_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&assemble_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cost_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ls_cost_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&assemble_terms_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&constraint_lambda_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
#define APPLY_ATTR(KM) MAX_LDS((penta_apply_kernel<KM, (KM <= 8)>))
  IDTO_APPLY_KERNELS(APPLY_ATTR)
#undef APPLY_ATTR
#define LDL_ATTR(KM, PD, GW) MAX_LDS((penta_ldl_kernel<KM, 256, PD, GW>))
  IDTO_LDL_KERNELS(LDL_ATTR)
#undef LDL_ATTR
#define ND_ATTR(KM) MAX_LDS((penta_nd_kernel<KM, false>))
  IDTO_ND_KERNELS(ND_ATTR)
#undef ND_ATTR
#define PIPE_ATTR(KM) MAX_LDS(penta_pipe_kernel<KM>)
#define PIPE_DEC_ATTR(KM) MAX_LDS((penta_pipe_kernel<KM, true>))
  IDTO_PIPE_DEC_KERNELS(PIPE_DEC_ATTR)
  IDTO_PIPE_KERNELS(PIPE_ATTR)
#undef PIPE_ATTR
#undef PIPE_DEC_ATTR
#define FUSED_ATTR(MC, KM, PD, GW) MAX_LDS((gn_fused_kernel<MC, KM, PD, GW>))
  IDTO_FUSED_KERNELS(FUSED_ATTR)
#undef FUSED_ATTR
#undef MAX_LDS
  OptionsFromEnvironment(c);
  (void)hipGetLastError();
  *out = c;
  return 0;
}

void idto_hip_destroy(idto_hip_ctx* c) {
  if (!c) return;
  for (idto_hip_ctx* ch : c->children) idto_hip_destroy(ch);
  c->children.clear();
  if (c->kkt) { idto_hip_destroy(c->kkt); c->kkt = nullptr; }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) { if (RcclState().handle) (void)RcclState().CommDestroy(c->comm); c->comm = nullptr; }
  (void)TimeDrain(c);
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  if (c->spec_ev) (void)hipEventDestroy(c->spec_ev);
  for (hipEvent_t e : c->up_ev) if (e) (void)hipEventDestroy(e);
  if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
  for (auto& pf : c->pre) if (pf.ev) (void)hipEventDestroy(pf.ev);
  // the memory, both streams drained and the context's own still alive: the owned buffers and the entries' storage (which
  // returns its share of the pool), then the pool, the arena in it
  ReleaseBuffers(c);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->status_pin) (void)hipHostFree(c->status_pin);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int idto_hip_set_problem(idto_hip_ctx* c, const idto_problem_t* p) { return idto_hip_set_problem_batch(c, 0, p); }

int idto_hip_set_problem_batch(idto_hip_ctx* c, int b, const idto_problem_t* p) {
  if (b < 0 || b >= c->batch) { g_err = "problem index outside the batch"; return -1; }
  if (p->num_steps != c->N || p->time_step != c->dt) { g_err = "num_steps / time_step cannot change"; return -1; }
  HIP_OK(hipSetDevice(c->device));
  c->fd_full = false; c->partials_ahead = false;  // v_0 = v_init
  c->con_ready = false; c->con_begun = false;
  if (b < (int)c->host_problems.size()) {
    c->host_problems[b]->Set(*p, c->nq, c->nv);
    if (b < (int)c->children.size() && c->children[b]) {
      const int rc = idto_hip_set_problem_batch(c->children[b], 0, &c->host_problems[b]->p);
      if (rc) return rc;
    }
  }
  return UploadProblemArrays(c, p, b);
}

int idto_hip_batch_size(idto_hip_ctx* c) { return c->batch; }

int idto_hip_check_model_batch(idto_hip_ctx* c, int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  if (!c->host_tables || !c->host_model) { g_err = "check_model_batch: the context keeps no host copy of its model"; return -1; }
  const idto_model_t* base = &c->host_model->m;
  std::vector<double> record;
  return idto_host::BuildModelVariant(base, *c->host_tables, b, model ? model : base, contact ? *contact : c->host_contact, &record, &g_err);
}

int idto_hip_set_model_batch(idto_hip_ctx* c, int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  if (!c->host_tables || !c->host_model || c->batch < 2) {
    g_err = "set_model_batch: a context of one problem (a model of its own is what idto_hip_create gives it)";
    return -1;
  }
  if (b < 0 || b >= c->batch) { g_err = "problem index outside the batch"; return -1; }
  const idto_model_t* base = &c->host_model->m;
  // every refusal is made here, on the host's tables: nothing has been enqueued or allocated by then
  std::vector<double> record;
  if (int rc = idto_host::BuildModelVariant(base, *c->host_tables, b, model ? model : base, contact ? *contact : c->host_contact,
                                            &record, &g_err))
    return rc;
  HIP_OK(hipSetDevice(c->device));
  const size_t bytes = record.size() * sizeof(double), mat = model_record_devmodel_at((size_t)c->M.blob_n);
  // the record's DevModel: the context's, its tables the blob at the head of the record at device address `dev`
  auto put_model = [&](std::vector<double>& rec, size_t at, const double* dev, const double* gravity) {
    DevModel Mb = c->M;
    shift_model(Mb, dev);
    for (int i = 0; i < 3; ++i) Mb.gravity[i] = gravity[i];
    std::memcpy(rec.data() + at + mat, &Mb, sizeof(DevModel));
  };
  if (!c->model_records) {   // the first call: every problem gets a record, the base model's
    const std::vector<double> base_record = idto_host::ModelRecord(base, *c->host_tables, c->host_contact);
    std::vector<double> all((size_t)c->batch * base_record.size());
    double* dev = nullptr;
    if (Alloc(c, all.size(), &dev)) return -2;
    for (int p = 0; p < c->batch; ++p) {
      std::copy(base_record.begin(), base_record.end(), all.begin() + (size_t)p * base_record.size());
      put_model(all, (size_t)p * base_record.size(), dev + (size_t)p * base_record.size(), base->gravity);
    }
    if (hipMemcpy(dev, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = "hipMemcpy (parameter records) failed"; Release(c, &dev); return -2;
    }
    c->model_records = dev; c->mstride = bytes;
  }
  put_model(record, 0, at_problem(c->model_records, (size_t)b * c->mstride), (model ? model : base)->gravity);
  // (behind whatever the context has enqueued: a launch in flight keeps the record it started with)
  if (c->async_uploads) {   // (from the context's pinned staging, no wait: as idto_hip_set_problem_batch uploads)
    char* buf = nullptr; int slot = 0;
    if (int rc = UploadStage(c, bytes, &buf, &slot)) return rc;
    std::memcpy(buf, record.data(), bytes);
    HIP_OK(hipMemcpyAsync(at_problem(c->model_records, (size_t)b * c->mstride), buf, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->up_ev[slot], c->stream));
  } else {
    HIP_OK(hipMemcpyAsync(at_problem(c->model_records, (size_t)b * c->mstride), record.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
  }
  // what the device holds of the resident q belongs to the old record
  c->fd_full = false; c->partials_ahead = false; c->terms_valid = false;
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  c->con_ready = false; c->con_begun = false;
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_COST});
  return 0;
}

int idto_hip_create_batch_like(idto_hip_ctx* like, const idto_problem_t* problems, int batch, idto_hip_ctx** out) {
  *out = nullptr;
  if (!like || !like->host_model) { g_err = "create_batch_like: the context keeps no host copy of its model"; return -1; }
  const int rc = idto_hip_create_batch(&like->host_model->m, problems, &like->host_contact, like->device, batch, out);
  if (rc) return rc;
  (*out)->gradients_method = like->gradients_method;
  return 0;
}

int idto_hip_set_stream(idto_hip_ctx* c, void* s) {
  if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  c->stream = static_cast<hipStream_t>(s);
  c->own_stream = false;
  return 0;
}
void* idto_hip_get_stream(idto_hip_ctx* c) { return c->stream; }

int idto_hip_set_shard(idto_hip_ctx* c, int kb, int ke) {
  if (kb < 0 || ke > c->N || kb > ke) { g_err = "bad shard range"; return -1; }
  c->k_begin = kb; c->k_end = ke;
  return 0;
}

int idto_hip_set_q(idto_hip_ctx* c, const double* q_host) {
  TRACE("hip: set_q begins");
  HIP_OK(hipSetDevice(c->device));
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_Q});
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  const size_t qbytes = (size_t)(c->N + 1) * c->nq * sizeof(double);
  if (c->async_uploads) {
    char* buf = nullptr; int slot = 0;
    if (int rc = UploadStage(c, qbytes, &buf, &slot)) return rc;
    std::memcpy(buf, q_host, qbytes);
    HIP_OK(hipMemcpyAsync(c->q, buf, qbytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->up_ev[slot], c->stream));
    TRACE("hip: set_q done (copy enqueued)");
    return 0;
  }
  HIP_OK(hipMemcpyAsync(c->q, q_host, qbytes, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));  // the host buffer may be reused by the caller
  TRACE("hip: set_q done (copy + wait)");
  return 0;
}
int idto_hip_set_q_batch(idto_hip_ctx* c, const double* q_host) {
  HIP_OK(hipSetDevice(c->device));
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_Q});
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  const size_t row = (size_t)(c->N + 1) * c->nq * sizeof(double);  // one trajectory per arena
  HIP_OK(hipMemcpy2DAsync(c->q, c->pstride, q_host, row, row, (size_t)c->batch, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}
int idto_hip_set_q_device(idto_hip_ctx* c, const double* q_dev) {
  HIP_OK(hipSetDevice(c->device));
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_Q});
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  HIP_OK(hipMemcpyAsync(c->q, q_dev, (size_t)(c->N + 1) * c->nq * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int idto_hip_eval_tau(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  c->partials_ahead = false;
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_COST});
  int rc = LaunchFd(c, 0, 0, c->N);
  if (rc) return rc;
  hipLaunchKernelGGL(cost_kernel, dim3(1, c->batch), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->q, c->v, c->slab,
                     c->slab_stride, c->cost, c->weights_diagonal ? 1 : 0, (double*)nullptr, c->pstride, (double*)nullptr,
                     TrDecideArgs{}, AltSel{nullptr, 0, 0});
  HIP_OK(hipGetLastError());
  return 0;
}

// idto_hip_eval_tau for a q whose partials are wanted next (the start of idto_hip_tr_solve / idto_hip_gn_step): ONE
// finite-difference launch leaves v, a, N+, tau AND the partials (fd_kernel's derivative modes evaluate the nominal
// point too: same tau, bit for bit), the cost follows; the idto_hip_eval_partials that comes next returns at once.
int idto_hip_eval_tau_partials(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  if (!(c->k_begin == 0 && c->k_end == c->N)) return idto_hip_eval_tau(c);   // (a shard of the horizon: tau of every step is needed)
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_COST});
  c->con_ready = false; c->con_begun = false;
  int rc = LaunchFd(c, 1, 0, c->N);
  if (rc) return rc;
  c->fd_full = true;
  c->partials_ahead = true;
  TRACE("hip: eval_tau_partials: fd_kernel enqueued");
  hipLaunchKernelGGL(cost_kernel, dim3(1, c->batch), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->q, c->v, c->slab,
                     c->slab_stride, c->cost, c->weights_diagonal ? 1 : 0, (double*)nullptr, c->pstride, (double*)nullptr,
                     TrDecideArgs{}, AltSel{nullptr, 0, 0});
  HIP_OK(hipGetLastError());
  return 0;
}

int idto_hip_trial_cost(idto_hip_ctx* c, const double* q_host, double* tau_host, double* cost_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch != 1) { g_err = "trial_cost serves single-problem contexts"; return -1; }
  if (!q_host || !cost_host) { g_err = "trial_cost: bad arguments"; return -1; }
  DropPrefetch(c, {IDTO_ARR_Q, IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_COST});
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  const size_t nq_all = (size_t)(c->N + 1) * c->nq, ntau = (size_t)c->N * c->nv;
  if (!c->pack && Alloc(c, ntau + 1, &c->pack)) return -2;
  if (int rc = c->pin.Ensure(nq_all + ntau + 1)) return rc;
  // one stream synchronisation for the whole trial point: q through pinned memory, N
  // inverse-dynamics evaluations, the cost, and [tau | cost] back in one copy
  std::memcpy(c->pin, q_host, nq_all * sizeof(double));
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  HIP_OK(hipMemcpyAsync(c->q, c->pin, nq_all * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int rc = LaunchFd(c, 0, 0, c->N);
  if (rc) return rc;
  hipLaunchKernelGGL(cost_kernel, dim3(1), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->q, c->v, c->slab,
                     c->slab_stride, c->cost, c->weights_diagonal ? 1 : 0, c->pack, (size_t)0, (double*)nullptr, TrDecideArgs{}, AltSel{nullptr, 0, 0});
  HIP_OK(hipGetLastError());
  double* out = c->pin + nq_all;
  HIP_OK(hipMemcpyAsync(out, c->pack, (ntau + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (tau_host) std::memcpy(tau_host, out, ntau * sizeof(double));
  *cost_host = out[ntau];
  return 0;
}

int idto_hip_ls_alphas(int linesearch_method, int m, double* alphas_host) {
  if ((linesearch_method != idto_ls::kArmijo && linesearch_method != idto_ls::kBacktracking) || m < 0 || (m > 0 && !alphas_host)) {
    g_err = "ls_alphas: bad arguments";
    return -1;
  }
  idto_ls::ls_alpha_chain(linesearch_method, m, alphas_host);
  return 0;
}

// the candidates' arenas for m step lengths (grown to the largest m asked for; they hold nothing between calls), their
// costs and the costs' pinned staging
// (a batch context: m arenas, IDTO_LS_MAX_CANDIDATES costs for every problem - [problem][candidate])
static int LsEnsureArenas(idto_hip_ctx* c, int m) {
  const LsArena A = ls_arena(c->N, c->nq, c->nv);
  const size_t B = (size_t)c->batch;
  if (c->ls_arenas.Ensure(A.stride * (size_t)m * B)) {
    g_err = "linesearch: the candidates' arenas could not be allocated (" + std::to_string(A.stride * (size_t)m * B * sizeof(double)) +
            " bytes for " + std::to_string(B) + " problems x " + std::to_string(m) + " candidates): " + g_err;
    return -2;
  }
  if (int rc = c->ls_costs.Ensure(B * IDTO_LS_MAX_CANDIDATES)) return rc;
  return c->ls_pin.Ensure(B * IDTO_LS_MAX_CANDIDATES);
}
// the candidates every problem's stretch of ls_arenas has room for
static size_t LsCap(const idto_hip_ctx* c, const LsArena& A) { return c->ls_arenas.cap() / (A.stride * (size_t)c->batch); }

// trial points [first, first + m) -> their tau -> their costs (alpha_dev: ONE point at a step length the device holds)
static int LsEvaluate(idto_hip_ctx* c, const LsAlphas& al, int first, int m, int normalize_quaternions, const double* gate,
                      const double* alpha_dev) {
  const int N = c->N, nq = c->nq, nv = c->nv, n = (N + 1) * nq;
  const LsArena A = ls_arena(N, nq, nv);
  // (a batch context: the same candidates of every problem - the problems' arenas pcstride doubles apart, their costs
  // IDTO_LS_MAX_CANDIDATES, their gate / alpha words LSS_COUNT)
  const size_t pcstride = LsCap(c, A) * A.stride, gstride = LSS_COUNT, cstride = IDTO_LS_MAX_CANDIDATES;
  hipLaunchKernelGGL(ls_trial_kernel, dim3(m, c->batch), dim3(256), 0, c->stream, n, nq, c->q, c->step, al, c->tr_quat,
                     normalize_quaternions ? c->tr_nquat : 0, c->ls_arenas, A.stride, first, gate, alpha_dev, c->pstride,
                     pcstride, gstride);
  HIP_OK(hipGetLastError());
  double* base = c->ls_arenas + (size_t)first * A.stride;
  FdAlong along;
  along.q = base + A.q; along.slab = base + A.slab; along.slab_stride = nv; along.v = base + A.v; along.a = base + A.a;
  along.nplus = base + A.nplus; along.cstride = A.stride * sizeof(double); along.m = m; along.gate = gate;
  along.bstride = pcstride * sizeof(double); along.gstride = gstride * sizeof(double);
  if (int rc = LaunchFd(c, 0, 0, N, AltSel{nullptr, 0, 0}, &along)) return rc;
  hipLaunchKernelGGL(ls_cost_kernel, dim3(m, c->batch), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->ls_arenas, A,
                     c->weights_diagonal ? 1 : 0, c->ls_costs, first, gate, c->pstride, pcstride, cstride, gstride);
  HIP_OK(hipGetLastError());
  return 0;
}

int idto_hip_costs_along(idto_hip_ctx* c, const double* alphas_host, int m, int normalize_quaternions, double* costs_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch != 1) { g_err = "costs_along serves single-problem contexts"; return -1; }
  if (!alphas_host || !costs_host || m < 1 || m > IDTO_LS_MAX_CANDIDATES) {
    g_err = "costs_along: 1 .. IDTO_LS_MAX_CANDIDATES step lengths and room for their costs";
    return -1;
  }
  TRACE("hip: costs_along begins");
  if (int rc = LsEnsureArenas(c, m)) return rc;
  LsAlphas al;
  for (int j = 0; j < IDTO_LS_MAX_CANDIDATES; ++j) al.a[j] = j < m ? alphas_host[j] : 0.0;
  if (int rc = LsEvaluate(c, al, 0, m, normalize_quaternions, nullptr, nullptr)) return rc;
  HIP_OK(hipMemcpyAsync(c->ls_pin, c->ls_costs, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: costs_along: waited for the device (the candidates' costs back)");
  std::memcpy(costs_host, c->ls_pin, (size_t)m * sizeof(double));
  return 0;
}

// the same m step lengths along every problem's own step: one launch set, one wait; costs_host[batch][m]
int idto_hip_costs_along_batch(idto_hip_ctx* c, const double* alphas_host, int m, int normalize_quaternions, double* costs_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch < 2) { g_err = "costs_along_batch serves batch contexts (idto_hip_costs_along: a single problem)"; return -1; }
  if (!alphas_host || !costs_host || m < 1 || m > IDTO_LS_MAX_CANDIDATES) {
    g_err = "costs_along_batch: 1 .. IDTO_LS_MAX_CANDIDATES step lengths and room for their costs";
    return -1;
  }
  TRACE("hip: costs_along_batch begins");
  if (int rc = LsEnsureArenas(c, m)) return rc;
  LsAlphas al;
  for (int j = 0; j < IDTO_LS_MAX_CANDIDATES; ++j) al.a[j] = j < m ? alphas_host[j] : 0.0;
  if (int rc = LsEvaluate(c, al, 0, m, normalize_quaternions, nullptr, nullptr)) return rc;
  HIP_OK(hipMemcpyAsync(c->ls_pin, c->ls_costs, (size_t)c->batch * IDTO_LS_MAX_CANDIDATES * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: costs_along_batch: waited for the device (the candidates' costs of every problem back)");
  for (int b = 0; b < c->batch; ++b)
    std::memcpy(costs_host + (size_t)b * m, c->ls_pin + (size_t)b * IDTO_LS_MAX_CANDIDATES, (size_t)m * sizeof(double));
  return 0;
}

// bo: (idto_hip_ls_solve_batch_fetch) the loop of every problem of a batch context side by side - the same launches with the
// problem in the grid, every problem behind gate and stop words of its own; rows_host [batch][iterations][IDTO_LS_ROW], the
// outputs [batch][...], one gather launch and one copy (ls_fetch.h) instead of the single problem's four copies
struct LsBatchOut { double* final_cost; int* status; };
// every problem's final cost and [rows | q | v | tau] packed by one launch, one copy, the call's one wait
static int LsFinishBatch(idto_hip_ctx* c, const idto_fetch::LsFetchLayout& FL, int iterations, double* rows_host, double* q_out,
                         double* v_out, double* tau_out, const LsBatchOut& bo) {
  using idto_fetch::LsFetchLayout;
  const int B = c->batch;
  LsGatherArgs G;
  G.state = c->ls_state; G.rows = c->ls_rows; G.q = c->q; G.v = c->v; G.slab = c->slab; G.N = c->N; G.nv = c->nv;
  G.slab_stride = c->slab_stride; G.tau_off = 3 * c->nv * c->nq; G.pstride = c->pstride; G.rows_stride = FL.nrows; G.L = FL;
  G.out = c->ls_fetch_dev;
  hipLaunchKernelGGL(ls_gather_batch_kernel, dim3(4, B), dim3(256), 0, c->stream, G);
  HIP_OK(hipGetLastError());
  const double* pin = c->ls_fetch_pin;
  HIP_OK(hipMemcpyAsync(c->ls_fetch_pin, c->ls_fetch_dev, FL.total() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  TRACE("hip: ls_solve_batch: every iteration of every problem and the copy enqueued");
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: ls_solve_batch: waited for the device (every problem's rows and solution back)");
  bool named = false;
  for (int b = 0; b < B; ++b) {
    double* rows = rows_host + (size_t)b * FL.nrows;
    std::memcpy(rows, pin + FL.rows(b), FL.nrows * sizeof(double));
    if (q_out) std::memcpy(q_out + (size_t)b * FL.cnt[LsFetchLayout::Q], pin + FL.part(b, LsFetchLayout::Q), FL.cnt[LsFetchLayout::Q] * sizeof(double));
    if (v_out) std::memcpy(v_out + (size_t)b * FL.cnt[LsFetchLayout::V], pin + FL.part(b, LsFetchLayout::V), FL.cnt[LsFetchLayout::V] * sizeof(double));
    if (tau_out) std::memcpy(tau_out + (size_t)b * FL.cnt[LsFetchLayout::TAU], pin + FL.part(b, LsFetchLayout::TAU), FL.cnt[LsFetchLayout::TAU] * sizeof(double));
    bo.final_cost[b] = pin[FL.final_cost() + b];
    int st = 0;
    for (int k = 0; k < iterations; ++k) st |= (int)rows[(size_t)k * LSR_COUNT + LSR_FLAGS];
    bo.status[b] = st;
    named = named || (st & LSF_BAD_PIVOT) != 0;
  }
  // (as in the single problem's loop: a failed factorisation that no row names belongs to an idle iteration behind a
  // problem's stop flag and is nobody's failure; a time-out of a solver's waits is the whole call's)
  const int fs = FactorStatus(c);
  if (fs != 0 && fs != IDTO_HIP_FACTORIZATION_FAILED) return fs;
  if (named && fs == 0) g_err = "factorisation failed: the Hessian is not numerically positive definite (the row with flag 32 names the problem and the iteration)";
  return named ? IDTO_HIP_FACTORIZATION_FAILED : 0;
}
static int LsSolve(idto_hip_ctx* c, int iterations, int method, int max_ls, int normalize_quaternions, double* rows_host,
                   double* q_out, double* v_out, double* tau_out, const LsBatchOut* bo = nullptr) {
  HIP_OK(hipSetDevice(c->device));
  if (!bo && c->batch != 1) { g_err = "ls_solve serves single-problem contexts"; return -1; }
  if (bo && c->batch < 2) { g_err = "ls_solve_batch serves batch contexts (idto_hip_ls_solve: a single problem)"; return -1; }
  if (bo && (!bo->final_cost || !bo->status)) { g_err = "ls_solve_batch: bad arguments (final_cost and status are required)"; return -1; }
  if (iterations < 1 || !rows_host) { g_err = bo ? "ls_solve_batch: bad arguments" : "ls_solve: bad arguments"; return -1; }
  if (method != idto_ls::kArmijo && method != idto_ls::kBacktracking) {
    g_err = bo ? "ls_solve_batch: bad arguments (linesearch_method is 0, Armijo, or 1, backtracking)" : "ls_solve: bad arguments";
    return -1;
  }
  static_assert(LSR_COUNT == IDTO_LS_ROW, "a statistics row as idto_hip.h documents it");
  static_assert(idto_ls::kMaxCandidates == IDTO_LS_MAX_CANDIDATES && idto_host::kLsMaxCandidates == IDTO_LS_MAX_CANDIDATES, "one cap");
  if (max_ls > IDTO_LS_MAX_CANDIDATES) { g_err = "ls_solve: max_linesearch_iterations above IDTO_LS_MAX_CANDIDATES"; return -1; }
  if (!(c->k_begin == 0 && c->k_end == c->N)) { g_err = "ls_solve: the context evaluates a shard of the horizon"; return -1; }
  const int N = c->N, nq = c->nq, nv = c->nv, n = (N + 1) * nq;
  const LsArena A = ls_arena(N, nq, nv);
  if (int rc = LsEnsureArenas(c, IDTO_LS_MAX_CANDIDATES)) return rc;
  const size_t B = (size_t)c->batch;
  static_assert(sizeof(idto_ls::LsScan) % 8 == 0, "the problems' scans lie one LsScan apart in an array of doubles");
  if (!c->ls_state) {
    double* scan = nullptr;
    if (Alloc(c, B * LSS_COUNT, &c->ls_state) || Alloc(c, B * 2 * n, &c->ls_work) ||
        Alloc(c, B * ((sizeof(idto_ls::LsScan) + 7) / 8), &scan))
      return -2;
    c->ls_scan = reinterpret_cast<idto_ls::LsScan*>(scan);
  }
  if (int rc = c->ls_rows.Ensure(B * iterations * LSR_COUNT)) return rc;
  const size_t nrow = (size_t)iterations * LSR_COUNT, nqa = (size_t)n, nva = (size_t)(N + 1) * nv, nta = (size_t)N * nv;
  const idto_fetch::LsFetchLayout FL = idto_fetch::LsFetchLayout::Make(c->batch, iterations, LSR_COUNT, N, nq, nv, bo != nullptr);
  if (int rc = c->ls_fetch_pin.Ensure(FL.total())) return rc;
  if (bo) if (int rc = c->ls_fetch_dev.Ensure(FL.total())) return rc;
  if (!c->compute_units) {
    HIP_OK(hipDeviceGetAttribute(&c->compute_units, hipDeviceAttributeMultiprocessorCount, c->device));
  }
  // (a batch: a wave of k candidates is k N workgroups of every problem - the first wave gives every compute unit one
  // workgroup across the whole batch, which is the plan of a horizon of N B)
  int widths[idto_host::kLsMaxCandidates];
  const int nwaves = idto_host::PlanLsWaves(N * c->batch, c->compute_units, method, max_ls, c->ls_waves, widths);
  LsAlphas al;
  idto_ls::ls_alpha_chain(method, IDTO_LS_MAX_CANDIDATES, al.a);
  if (bo) { ++c->ls_batch_solves; TRACE("hip: ls_solve_batch begins"); }
  else { ++c->ls_solves; TRACE("hip: ls_solve begins"); }
  // L(q_0) and the loop's state
  if (int rc = idto_hip_eval_tau(c)) return rc;
  HIP_OK(hipMemsetAsync(c->ls_state, 0, B * LSS_COUNT * sizeof(double), c->stream));
  HIP_OK(hipMemsetAsync(c->ls_rows, 0, B * nrow * sizeof(double), c->stream));
  if (!bo) {
    HIP_OK(hipMemcpyAsync(c->ls_state + LSS_COST, c->cost, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  } else {
    HIP_OK(hipMemcpy2DAsync(c->ls_state + LSS_COST, LSS_COUNT * sizeof(double), c->cost, c->pstride, sizeof(double), B,
                            hipMemcpyDeviceToDevice, c->stream));
  }
  LsLoopArgs L;
  L.pstride = c->pstride; L.rows_stride = nrow; L.costs_stride = IDTO_LS_MAX_CANDIDATES; L.pcstride = LsCap(c, A) * A.stride;
  L.n = n; L.nq = nq; L.nv = nv; L.N = N; L.g = c->g; L.dq = c->step; L.HA = c->HA; L.HB = c->HB; L.HC = c->HC;
  L.slab = c->slab; L.slab_stride = c->slab_stride; L.tau_off = 3 * nv * nq; L.dofs = c->una_dofs; L.nu = c->una_nu;
  L.q = c->q; L.cost = c->cost; L.state = c->ls_state; L.scan = c->ls_scan; L.rows = c->ls_rows; L.work = c->ls_work;
  L.arena = c->ls_arenas; L.arena_cost = A.cost; L.status = c->status_dev; L.fact_id = 0; L.method = method;
  L.max_iters = max_ls; L.dt = c->dt;
  const double* gate = c->ls_state + LSS_GATE;
  const double* stop = c->ls_state + LSS_STOP;
  for (int it = 0; it < iterations; ++it) {
    // the Newton step at q_k: the partials, g and H, dq = -H^-1 g - the launches of the stepwise calls, the planner's solver
    if (int rc = idto_hip_eval_partials(c)) return rc;
    if (int rc = idto_hip_grad_hess(c)) return rc;
    if (int rc = idto_hip_factor_solve(c, nullptr, 1, nullptr)) return rc;
    L.fact_id = c->fact_id;
    hipLaunchKernelGGL(ls_prepare_kernel, dim3(1, c->batch), dim3(256), 0, c->stream, L);
    HIP_OK(hipGetLastError());
    for (int w = 0, first = 0; w < nwaves; first += widths[w], ++w) {
      if (int rc = LsEvaluate(c, al, first, widths[w], normalize_quaternions, gate, nullptr)) return rc;
      hipLaunchKernelGGL(ls_scan_kernel, dim3(1, c->batch), dim3(64), 0, c->stream, L, c->ls_costs, first, widths[w], w + 1 == nwaves ? 1 : 0);
      HIP_OK(hipGetLastError());
    }
    // the accepted step: its trial point once more at the decided alpha (arena 0), the ratio, the row, q <- q + alpha dq
    if (int rc = LsEvaluate(c, al, 0, 1, normalize_quaternions, stop, c->ls_state + LSS_ALPHA)) return rc;
    hipLaunchKernelGGL(ls_finish_kernel, dim3(1, c->batch), dim3(256), 0, c->stream, L);
    HIP_OK(hipGetLastError());
    // (what the context remembers about the resident q: it has moved on)
    c->fd_full = false; c->partials_ahead = false; c->terms_valid = false; c->con_ready = false; c->con_begun = false;
    c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  }
  DropPrefetch(c, {IDTO_ARR_Q, IDTO_ARR_COST});
  // v, a, tau of the final iterate, then [rows | q | v | tau] under one wait
  if (int rc = idto_hip_eval_tau(c)) return rc;
  double* pin = c->ls_fetch_pin;
  if (bo) return LsFinishBatch(c, FL, iterations, rows_host, q_out, v_out, tau_out, *bo);
  HIP_OK(hipMemcpyAsync(pin, c->ls_rows, nrow * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(pin + nrow, c->q, nqa * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(pin + nrow + nqa, c->v, nva * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpy2DAsync(pin + nrow + nqa + nva, (size_t)nv * sizeof(double), c->slab + 3 * nv * nq,
                          (size_t)c->slab_stride * sizeof(double), (size_t)nv * sizeof(double), (size_t)N,
                          hipMemcpyDeviceToHost, c->stream));
  TRACE("hip: ls_solve: every iteration and the copies enqueued");
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: ls_solve: waited for the device (rows and the solution back)");
  std::memcpy(rows_host, pin, nrow * sizeof(double));
  if (q_out) std::memcpy(q_out, pin + nrow, nqa * sizeof(double));
  if (v_out) std::memcpy(v_out, pin + nrow + nqa, nva * sizeof(double));
  if (tau_out) std::memcpy(tau_out, pin + nrow + nqa + nva, nta * sizeof(double));
  // The Newton-step launches of the iterations behind a stop flag cannot be held back - the host does not know of the
  // stop - and run at the final iterate; the ls_* kernels behind them are idle.  FactorStatus reports the LAST
  // factorisation: when that one failed and no row carries flag 32, it belongs to such an idle iteration, which the host
  // loop never ran, and is nobody's failure.
  const int fs = FactorStatus(c);
  if (fs != 0 && fs != IDTO_HIP_FACTORIZATION_FAILED) return fs;
  bool named = false;
  for (int k = 0; k < iterations; ++k) named = named || (((int)rows_host[(size_t)k * LSR_COUNT + LSR_FLAGS]) & LSF_BAD_PIVOT) != 0;
  if (named && fs == 0) g_err = "factorisation failed: the Hessian is not numerically positive definite (the row with flag 32 names the iteration)";
  return named ? IDTO_HIP_FACTORIZATION_FAILED : 0;
}

int idto_hip_ls_solve(idto_hip_ctx* c, int iterations, int linesearch_method, int max_linesearch_iterations,
                      int normalize_quaternions, double* rows_host) {
  return LsSolve(c, iterations, linesearch_method, max_linesearch_iterations, normalize_quaternions, rows_host, nullptr, nullptr,
                 nullptr);
}
int idto_hip_ls_solve_fetch(idto_hip_ctx* c, int iterations, int linesearch_method, int max_linesearch_iterations,
                            int normalize_quaternions, double* rows_host, double* q_out, double* v_out, double* tau_out) {
  return LsSolve(c, iterations, linesearch_method, max_linesearch_iterations, normalize_quaternions, rows_host, q_out, v_out,
                 tau_out);
}

int idto_hip_ls_solve_batch_fetch(idto_hip_ctx* c, int iterations, int linesearch_method, int max_linesearch_iterations,
                                  int normalize_quaternions, double* rows_host, double* q_out, double* v_out, double* tau_out,
                                  double* final_cost, int* status) {
  const LsBatchOut bo{final_cost, status};
  return LsSolve(c, iterations, linesearch_method, max_linesearch_iterations, normalize_quaternions, rows_host, q_out, v_out,
                 tau_out, &bo);
}

int idto_hip_eval_partials(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  if (c->partials_ahead && c->k_begin == 0 && c->k_end == c->N) {   // (idto_hip_eval_tau_partials: they are there)
    c->partials_ahead = false;
    return 0;
  }
  c->partials_ahead = false;
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB});
  c->con_ready = false; c->con_begun = false;
  if (TimeBegin(c, 0)) return -2;
  int rc = LaunchFd(c, 1, c->k_begin, c->k_end);
  if (rc) return rc;
  c->fd_full = (c->k_begin == 0 && c->k_end == c->N);
  return TimeEnd(c);
}

// g and the bands of H from the resident slab / products (gate: see assemble_terms_kernel)
// sink: (the constrained loop) the banded KKT system's bands and right-hand side are written along (kernels.h KktSink) -
// by the kernel that combines the records' products only; *sink_used says whether that was the one
static int LaunchAssemble(idto_hip_ctx* c, const double* gate, const KktSink* sink = nullptr, size_t kstride = 0, bool* sink_used = nullptr) {
  if (!c->h_assembled) {  // x_0 = -g_0 = 0 is no longer written by the solver (SolverFirstRow)
    HIP_OK(hipMemset2DAsync(c->step, c->pstride, 0, (size_t)c->nq * sizeof(double), (size_t)c->batch, c->stream));
    c->h_assembled = true;
  }
  c->con_ready = false; c->con_begun = false;
  const bool combine = c->weights_diagonal && c->terms_valid && c->fd_full && c->asm_stop == 0;
  c->last_assembly = combine ? 1 : (c->weights_diagonal ? 2 : 3);
  if (sink_used) *sink_used = combine && sink;
  if (combine) {
    hipLaunchKernelGGL(assemble_terms_kernel, dim3(c->N + 1, 4, c->batch), dim3(c->asm_terms_threads), c->asm_terms_lds, c->stream, c->M, c->P,
                       c->q, c->terms, c->v, c->nplus, c->g, c->HA, c->HB, c->HC, c->pstride, gate, c->alt_r,
                       sink ? *sink : KktSink{}, kstride);
  } else if (c->weights_diagonal) {
    hipLaunchKernelGGL(assemble_diag_kernel, dim3(c->N + 1, 4, c->batch), dim3(256), c->asm_diag_lds, c->stream, c->M,
                       c->P, c->q, c->slab, c->slab_stride, c->g, c->HA, c->HB, c->HC, c->asm_stop,
                       c->fd_full ? c->v : nullptr, c->fd_full ? c->nplus : nullptr, c->pstride, gate, c->alt_r);
  } else {
    if (gate) { g_err = "gated assembly needs diagonal cost weights"; return -1; }
    hipLaunchKernelGGL(assemble_kernel, dim3(c->N + 1, c->batch), dim3(256), c->asm_lds, c->stream, c->M, c->P, c->q,
                       c->slab, c->slab_stride, c->g, c->HA, c->HB, c->HC, c->pstride);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int idto_hip_grad_hess(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  DropPrefetch(c, {IDTO_ARR_GRADIENT, IDTO_ARR_H_A, IDTO_ARR_H_B, IDTO_ARR_H_C, IDTO_ARR_HBANDS});
  if (TimeBegin(c, 1)) return -2;
  if (int rc = LaunchAssemble(c, nullptr)) return rc;
  return TimeEnd(c);
}

// ---- the banded solvers.  Which kernel serves a system, with which block size, split, grid and LDS, is decided in
// host/solver_plan.cc (PlanSolve, host-only); the launch functions below fill arguments and launch what the plan names.
using idto_host::SolverPlan;
using idto_host::SolveRequest;
static idto_host::SolverShape ShapeOf(const idto_hip_ctx* c, bool assembled) {
  idto_host::SolverShape s;
  s.k = c->nq; s.N = c->N; s.batch = c->batch; s.npos = c->ldl_npos; s.h_assembled = assembled;
  s.two_sided = c->two_sided; s.solver_nd = c->solver_nd; s.solver_pipe = c->solver_pipe;
  s.solver_band = c->solver_band; s.nd_min_rows = c->nd_min_rows; s.nd_recursion = c->nd_recursion;
  s.has_wst = c->nd_wst != nullptr;
  s.asm_terms_lds = c->asm_terms_lds; s.cost_lds = c->cost_lds;
  return s;
}
// assembled: plan for the system as it is once the bands count as assembled (block row 0 the identity), whatever
// c->h_assembled says now - the launches that assemble H themselves
static int Plan(const idto_hip_ctx* c, bool assembled, const SolveRequest& rq, SolverPlan* p) {
  std::string err;
  if (idto_host::PlanSolve(ShapeOf(c, assembled), rq, p, &err)) { g_err = err; return -1; }
  return 0;
}
static SolveRequest WholeStep(const idto_hip_ctx* c) {   // (c: the context of the model, also where a KKT context's system is solved)
  SolveRequest rq;
  rq.kind = SolveRequest::WHOLE_STEP; rq.step_nq = c->nq; rq.step_fast_n = c->M.fast_n;
  return rq;
}
static int NoKernel(const char* family, int size) {   // (PlanSolve names instantiated sizes only: tests/cpp/solver_plan_check.cc)
  g_err = std::string("no ") + family + " instantiation of size " + std::to_string(size);
  return -1;
}

// What a solver's launch is to do besides solving (SolverPlan::can_assemble / can_decide; penta_pipe.h PipeAsm):
// assemble g and the bands itself - 4 (N + 1) workgroups behind the solver's own run assemble_terms_kernel's rows,
// gated: problems whose word is 0 keep their g and H (idto_hip_tr_solve) - and decide on the trial point first
struct SolverExtras {
  bool assemble = false;
  const double* gate = nullptr;
  const TrDecideArgs* decide = nullptr;
};
static PipeAsm MakeAsm(idto_hip_ctx* c, const SolverPlan& p, const SolverExtras& ex) {
  PipeAsm F{};
  F.on = ex.assemble ? 1 : 0;
  if (F.on) {
    F.nq = c->nq; F.nv = c->nv; F.rows = c->N + 1; F.first = p.r0;
    F.P = c->P; F.q = c->q; F.terms = c->terms; F.v_res = c->v; F.nplus = c->nplus;
    F.g = c->g; F.HA = c->HA; F.HB = c->HB; F.HC = c->HC; F.alt = c->alt_r; F.ready = c->asm_ready; F.gate = ex.gate;
    c->last_assembly = 4;
  }
  if (!(F.on && ex.decide)) return F;
  F.decide = 1;
  F.dq = c->q_trial; F.dv = c->v; F.dslab = c->slab; F.dslab_stride = (int)c->slab_stride; F.dcost = c->cost;
  F.ddiag = c->weights_diagonal ? 1 : 0;
  F.dT = *ex.decide; F.dalt = c->alt_w;
  F.dword = c->decide_word;
  F.g2 = c->g2; F.HA2 = c->HA2; F.HB2 = c->HB2; F.HC2 = c->HC2;
  F.curpre = c->decide_word + 2;
  if (++c->decide_epoch == 0u) c->decide_epoch = 1u;
  F.depoch = c->decide_epoch;
  return F;
}

// The scalar band factorisation (penta_band.h)
static int LaunchBand(idto_hip_ctx* c, const SolverPlan& p, const double* b, double sign, double* xo, const SolverExtras& ex) {
  BandArgs A;
  A.n = p.n; A.k = p.k;
  A.HA = c->HA + p.qq0; A.HB = c->HB + p.qq0; A.HC = c->HC + p.qq0;
  A.b = b + (size_t)p.r0 * p.k; A.rhs_sign = sign; A.x = xo + (size_t)p.r0 * p.k; A.Dst = c->Dst;
  ++c->epoch;
  if (++c->fact_id == 0) c->fact_id = 1;
  A.status = c->status_dev; A.fact_id = c->fact_id; A.epoch = c->epoch; A.pstride = c->pstride;
  A.npos = c->ldl_npos;
  A.ts = c->solver_debug ? c->dbg : nullptr;
  c->last_solver = 6;
  const PipeAsm F = MakeAsm(c, p, ex);
  const int lds = F.on ? p.lds_assemble : p.lds;
  const dim3 grid(p.grid + (F.on ? 4 * (c->N + 1) : 0), c->batch);
  switch (3 * p.k) {
#define BAND_CASE(WM) case WM: hipLaunchKernelGGL((penta_band_kernel<WM>), grid, dim3(p.threads), lds, c->stream, A, F); break;
    IDTO_BAND_KERNELS(BAND_CASE)
#undef BAND_CASE
    default: return NoKernel("penta_band_kernel", 3 * p.k);
  }
  HIP_OK(hipGetLastError());
  return 0;
}
// Nested dissection: the pipelined chains (penta_pipe.h, five workgroups) or the seven-workgroup kernel (penta_nd.h)
static int LaunchNd(idto_hip_ctx* c, const SolverPlan& p, const double* b, double sign, double* xo, const SolverExtras& ex) {
  NdArgs A;
  A.debug_skip_role = c->debug_skip_role;
  A.debug_pipe_tail = c->debug_pipe_tail;
  A.asm_ready = nullptr; A.asm_first = 0; A.wt_rows = 0;
  A.rec_tail = 0; A.lds_doubles = 0; A.wst = nullptr;
  A.spin = SpinCtl{nullptr, 0};   // (set by the kernel: behind the per-problem status words)
  A.n = p.n; A.k = p.k;
  A.HA = c->HA + p.qq0; A.HB = c->HB + p.qq0; A.HC = c->HC + p.qq0;
  A.b = b + (size_t)p.r0 * p.k; A.rhs_sign = sign; A.x = xo + (size_t)p.r0 * p.k;
  A.Ust = c->Ust; A.Hst = c->Hst; A.Est = c->Est; A.Dst = c->Dst;
  A.s = p.s; A.j1 = p.j1; A.j2 = p.j2;
  A.npos = c->ldl_npos; A.lds_rows = p.lds_rows;
  A.xch = c->xch; A.xch_pair = (int)c->xch_count; A.flags = c->flags;
  if (p.kind == idto_host::SOLVER_PIPE) {
    A.rowcnt = c->pipe_rowcnt; A.ndbuf = c->nd_buf;
    ++c->pipe_launches;
    c->last_solver = 4;
    A.rowunit = 1ull; A.rowtarget = c->pipe_launches;
    ++c->epoch;
    if (++c->fact_id == 0) c->fact_id = 1;
    A.epoch = c->epoch; A.status = c->status_dev; A.fact_id = c->fact_id; A.pstride = c->pstride;
    A.ts = c->solver_debug ? c->dbg : nullptr;
    // (idto_hip_gn_step: g and the bands are assembled by 4 (N + 1) more workgroups of this launch, penta_pipe.h PipeAsm)
    const PipeAsm F = MakeAsm(c, p, ex);
    const int plds = F.decide ? p.lds_decide : (F.on ? p.lds_assemble : p.lds);
    const dim3 pgrid(p.grid + (F.on ? 4 * (c->N + 1) : 0) + (F.decide ? 1 : 0), c->batch);
#define PIPE_CASE(KM) case KM: hipLaunchKernelGGL((penta_pipe_kernel<KM>), pgrid, dim3(p.threads), plds, c->stream, A, F); break;
#define PIPE_DEC_CASE(KM) case KM: hipLaunchKernelGGL((penta_pipe_kernel<KM, true>), pgrid, dim3(p.threads), plds, c->stream, A, F); break;
    if (F.decide) {
      switch (p.K) {
        IDTO_PIPE_DEC_KERNELS(PIPE_DEC_CASE)
        default: return NoKernel("deciding penta_pipe_kernel", p.K);
      }
    } else {
      switch (p.K) {
        IDTO_PIPE_KERNELS(PIPE_CASE)
        default: return NoKernel("penta_pipe_kernel", p.K);
      }
    }
#undef PIPE_CASE
#undef PIPE_DEC_CASE
    HIP_OK(hipGetLastError());
    return 0;
  }
  A.rowcnt = c->nd_rowcnt; A.ndbuf = c->nd_buf;
  { static const int wt = [] { const char* e = std::getenv("IDTO_ND_WT"); return e ? std::atoi(e) : 0; }(); A.wt_rows = wt; }   // (measurement aid)
  ++c->nd_launches;
  c->last_solver = 2;
  {  // I/O wavefronts of a chain workgroup (penta_ldl_body: NW = 4, one elimination wavefront, three helpers)
    const int nhelp = 4 - p.gj_waves, io_first = (nhelp > 2) ? p.gj_waves + 1 : p.gj_waves;
    A.rowunit = (unsigned long long)(4 - io_first);
    A.rowtarget = c->nd_launches * A.rowunit;
  }
  ++c->epoch;
  if (++c->fact_id == 0) c->fact_id = 1;
  A.epoch = c->epoch; A.status = c->status_dev; A.fact_id = c->fact_id; A.pstride = c->pstride;
  A.ts = c->solver_debug ? c->dbg : nullptr;
  // (back substitution in recursion form, penta_pipe.h chain_recursion_tail: the plan then asks for the whole LDS)
  if (p.rec_tail) { A.rec_tail = p.rec_tail; A.lds_doubles = p.lds / (int)sizeof(double); A.wst = c->nd_wst; }
  const dim3 grid(p.grid, c->batch);
  switch (p.K) {
#define ND_CASE(KM) case KM: hipLaunchKernelGGL((penta_nd_kernel<KM, false>), grid, dim3(p.threads), p.lds, c->stream, A); break;
    IDTO_ND_KERNELS(ND_CASE)
#undef ND_CASE
    default: return NoKernel("penta_nd_kernel", p.K);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

// the launch the plan names; penta_ldl_kernel (one or two workgroups) here
static int LaunchLdl(idto_hip_ctx* c, const SolverPlan& p, const double* b, double sign, double* xo, bool factor_only, const SolverExtras& ex) {
  if (ex.assemble && !(p.can_assemble && (!ex.decide || p.can_decide))) { g_err = "the planned solver launch cannot carry the assembly / the decision"; return -1; }
  if (p.kind == idto_host::SOLVER_BAND) return LaunchBand(c, p, b, sign, xo, ex);
  if (p.kind == idto_host::SOLVER_ND || p.kind == idto_host::SOLVER_PIPE) return LaunchNd(c, p, b, sign, xo, ex);
  const int n = p.n, k = p.k, m_split = p.m_split, lds = p.lds, nrhs = 1;
  const size_t qq0 = p.qq0;
  b += (size_t)p.r0 * k;
  xo += (size_t)p.r0 * k;
  double* dbg = c->solver_debug ? c->dbg : nullptr;
  const dim3 grid(p.grid, c->batch);
  c->last_solver = 1;
  if (m_split > 0) ++c->epoch;  // (exchange buffer and flags live in the problem's arena)
  if (++c->fact_id == 0) c->fact_id = 1;  // (0 is the initial value of the status word)
#define LDL_ARGS n, k, c->HA + qq0, c->HB + qq0, c->HC + qq0, b, sign, nrhs, xo, c->Ust, c->Hst, c->Est, c->Dst, dbg, \
                 m_split, c->xch, c->flags, c->epoch, c->status_dev, c->fact_id, c->pstride, factor_only ? 1 : 0, c->ldl_npos
#define LDL_CASE(KM, PD, GW) \
  case KM: hipLaunchKernelGGL((penta_ldl_kernel<KM, 256, PD, GW>), grid, dim3(p.threads), lds, c->stream, LDL_ARGS); break;
  switch (p.K) {
    IDTO_LDL_KERNELS(LDL_CASE)
    default: return NoKernel("penta_ldl_kernel", p.K);
  }
#undef LDL_CASE
#undef LDL_ARGS
  HIP_OK(hipGetLastError());
  return 0;
}

// ---- one persistent launch for the whole Gauss-Newton iteration (fused.h)
static int FusedVariant(const idto_hip_ctx* c) {  // instantiated (MAXC, K) combinations: the reference's example models
  if (c->M.nxb || c->M.nstem > 1) return 0;   // (gn_fused_kernel embeds id_eval without the exchange of shared pairs / the stem)
  if (c->capsules || c->cylinders) return 0;   // (capsule and cylinder models: the three-launch path only)
  const int mc = idto_host::FdChainBound(c->maxc);   // (what a FUSED plan names)
  int variant = 0, i = 0;
#define FUSED_IS(MC, KM, PD, GW) ++i; if (mc == MC && c->nq == KM) variant = i;
  IDTO_FUSED_KERNELS(FUSED_IS)
#undef FUSED_IS
  return variant;
}
static bool FusedEligible(const idto_hip_ctx* c) {
  if (!(c->fused && c->batch == 1 && c->weights_diagonal && !c->reference_solver && !c->solver_debug && c->fd_stop == 0 &&
        c->asm_stop == 0 && c->k_begin == 0 && c->k_end == c->N && c->N >= 2 && FusedVariant(c) != 0))
    return false;
  // the nested-dissection solvers and the scalar band factorisation are launches of their own: the three-launch path
  // takes them (the system as it stands - a context's first step still counts block row 0)
  SolverPlan p;
  return Plan(c, c->h_assembled, SolveRequest{}, &p) == 0 && p.kind == idto_host::SOLVER_LDL;
}
static int LaunchFused(idto_hip_ctx* c) {
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_GRADIENT, IDTO_ARR_H_A, IDTO_ARR_H_B,
                   IDTO_ARR_H_C, IDTO_ARR_HBANDS, IDTO_ARR_STEP});
  c->con_ready = false; c->con_begun = false;
  if (!c->h_assembled) {  // x_0 = -g_0 = 0 is not written by the solver (SolverFirstRow)
    HIP_OK(hipMemsetAsync(c->step, 0, (size_t)c->nq * sizeof(double), c->stream));
    c->h_assembled = true;
  }
  SolverPlan p;   // (the chains' geometry: r0, n, m_split and lds_full are the same whichever kernel the plan names)
  if (int rc = Plan(c, true, SolveRequest{}, &p)) return rc;
  idto_host::FdRequest rq;   // the embedded evaluation's mode, chunk, LDS term and chain bound: host/fd_plan.cc
  rq.kind = idto_host::FdRequest::FUSED; rq.mode = 1;
  idto_host::FdPlan fd;
  if (idto_host::PlanFd(FdShapeOf(c), rq, &fd, &g_err)) return -1;
  const int lds = std::max(std::max(fd.lds, c->asm_diag_lds), std::max(p.lds_full, 84 * 1024));
  FusedArgs A;
  A.M = c->M; A.cp = c->cp; A.P = c->P;
  A.q = c->q; A.slab = c->slab; A.slab_stride = c->slab_stride; A.v = c->v; A.a = c->a; A.nplus = c->nplus;
  A.fd_mode = fd.mode; A.fd_echunk = fd.echunk; A.nfd = c->N;
  A.g = c->g; A.HA = c->HA; A.HB = c->HB; A.HC = c->HC; A.nrows = c->N + 1;
  A.n = p.n; A.k = p.k;
  A.sHA = c->HA + p.qq0; A.sHB = c->HB + p.qq0; A.sHC = c->HC + p.qq0;
  A.b = c->g + (size_t)p.r0 * p.k; A.rhs_sign = -1.0; A.x = c->step + (size_t)p.r0 * p.k;
  A.Ust = c->Ust; A.Hst = c->Hst; A.Est = c->Est; A.Dst = c->Dst;
  if (p.m_split > 0) ++c->epoch;
  if (++c->fact_id == 0) c->fact_id = 1;
  A.m_split = p.m_split; A.xch = c->xch; A.flags = c->flags; A.epoch = c->epoch; A.status = c->status_dev;
  A.fact_id = c->fact_id;
  ++c->sync_steps;
  A.sync = c->sync_cnt;
  A.dbg = c->fused_debug ? c->dbg : nullptr;
  A.fd_target = c->sync_steps * (unsigned long long)A.nfd;
  A.asm_target = c->sync_steps * (unsigned long long)(4 * A.nrows);
  const dim3 grid(A.nfd + 4 * A.nrows + (p.m_split > 0 ? 2 : 1));
  c->last_solver = 5;
  c->last_step_kind = 2;
  c->last_assembly = 2;   // (assemble_diag_kernel's rows, run by the launch's assembly workgroups: not what an earlier path left)
  if (TimeBegin(c, 3)) return -2;
#define FUSED_LAUNCH(MC, KM, PD, GW) \
  if (mc == MC && c->nq == KM) { hipLaunchKernelGGL((gn_fused_kernel<MC, KM, PD, GW>), grid, dim3(256), lds, c->stream, A); launched = true; }
  {
    const int mc = fd.maxc;
    bool launched = false;
    IDTO_FUSED_KERNELS(FUSED_LAUNCH)
    if (!launched) return NoKernel("gn_fused_kernel", c->nq);
  }
#undef FUSED_LAUNCH
  HIP_OK(hipGetLastError());
  c->fd_full = true; c->partials_ahead = false;
  c->terms_valid = false;   // (the fused kernel assembles from the slab itself)
  return TimeEnd(c);
}

// gn_small.h: fd + assembly + band solve of a small all-revolute model in ONE workgroup per problem.  What it stands in
// for must be what the two launches would have run: forward differences from the straight-line evaluation, diagonal
// weights, the whole horizon, the scalar band factorisation (BandEligible), nothing switched to a measurement mode.
// p: the plan of the system the launch solves - H's, or the KKT context's with blocks of nq + nu
static bool SmallEligible(const idto_hip_ctx* c, SolverPlan* p) {
  if (c->model_records) return false;   // (the kernel stages the context's one model: idto_hip_set_model_batch)
  if (!c->gn_small || !c->fd_fast || c->gradients_method != 0 || !c->weights_diagonal || c->reference_solver) return false;
  if (c->M.nxb || c->M.nstem > 1) return false;   // (id_eval_fast has no shared pairs and no stem)
  if (!(c->M.fast_shape == 1 || c->M.fast_shape == 5) || c->M.nfloat != 0 || c->nq != c->nv || c->npaths != 1) return false;
  if (!((c->M.fast_shape == 1 && c->nq == 2) || (c->M.fast_shape == 5 && c->nq == 3))) return false;   // (the instantiations)
  if (c->k_begin != 0 || c->k_end != c->N || c->fd_stop || c->asm_stop || c->solver_debug || c->ldl_npos > 0) return false;
  // (the kernel assembles H itself: block row 0 is the identity, the solver starts at row 1)
  return Plan(c, true, WholeStep(c), p) == 0;
}
// tr: inside idto_hip_tr_solve - the launch evaluates the trial point c->q_trial into the output set `alt`, decides, and
// goes on to g, H and the step only for an accepted step (gn_small.h SmallArgs::T); last: tau, cost and decision only
// kkt: with enforced constraints - the step is the banded KKT solve, z into c->kkt's step (gn_small.h SmallArgs::kkt_r0)
// iter: ... and tr_iter_kernel's part for the iterate in front (SmallArgs::I; a second workgroup reads the status words)
static int LaunchSmall(idto_hip_ctx* c, const SolverPlan& p, const TrDecideArgs* tr = nullptr, bool last = false,
                       AltSel alt = AltSel{nullptr, 0, 0}, bool kkt = false, const TrIterArgs* iter = nullptr) {
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_GRADIENT, IDTO_ARR_H_A, IDTO_ARR_H_B,
                   IDTO_ARR_H_C, IDTO_ARR_HBANDS, IDTO_ARR_STEP, IDTO_ARR_COST});
  c->con_ready = false; c->con_begun = false;
  if (!c->h_assembled) {  // x_0 = -g_0 = 0 is not written by the solver (SolverFirstRow)
    HIP_OK(hipMemset2DAsync(c->step, c->pstride, 0, (size_t)c->nq * sizeof(double), (size_t)c->batch, c->stream));
    c->h_assembled = true;
  }
  idto_hip_ctx* sc = kkt ? c->kkt : c;   // whose system the launch solves
  SmallArgs A;
  A.kkt_r0 = p.r0; A.kstride = sc->pstride;
  A.M = c->M; A.cp = c->cp; A.P = c->P; A.q = c->q; A.slab = c->slab; A.slab_stride = c->slab_stride;
  A.v = c->v; A.a = c->a; A.nplus = c->nplus; A.g = c->g; A.HA = c->HA; A.HB = c->HB; A.HC = c->HC;
  A.pstride = c->pstride; A.alt = alt;
  A.T = tr ? *tr : TrDecideArgs{}; A.tau_only = last ? 1 : 0; A.cost_out = c->cost;
  if (iter) A.I = *iter; else { A.I = TrIterArgs{}; A.I.state = nullptr; }
  const unsigned gx = iter ? 2u : 1u;
  if (tr) A.q = c->q_trial;
  BandArgs& B = A.B;
  B.n = p.n; B.k = p.k;
  B.HA = sc->HA + p.qq0; B.HB = sc->HB + p.qq0; B.HC = sc->HC + p.qq0;
  B.b = sc->g + (size_t)p.r0 * p.k; B.rhs_sign = -1.0; B.x = sc->step + (size_t)p.r0 * p.k; B.Dst = sc->Dst;
  ++sc->epoch;
  if (++sc->fact_id == 0) sc->fact_id = 1;
  B.status = sc->status_dev; B.fact_id = sc->fact_id; B.epoch = sc->epoch; B.pstride = sc->pstride;
  B.npos = sc->ldl_npos; B.ts = nullptr;
  A.ts = std::getenv("IDTO_SMALL_STAMPS") ? c->dbg : nullptr;
  A.lds_small = p.lds_small;
  if (sc->small_stage_N != c->N) {   // (once per horizon; the KKT system's table lives in its own context)
    const int qq = p.k * p.k, nb = c->N + 1;
    std::vector<BandStageItem> tab((size_t)band_stage_table(p.n, p.k, 0, 0, 0, 0, nullptr));
    band_stage_table(p.n, p.k, p.r0 * qq, nb * qq + p.r0 * qq, 2 * nb * qq + p.r0 * qq, 3 * nb * qq + p.r0 * p.k, tab.data());
    Release(sc, &sc->small_stage);
    if (Alloc(sc, tab.size(), &sc->small_stage)) return -2;
    HIP_OK(hipMemcpy(sc->small_stage, tab.data(), tab.size() * sizeof(BandStageItem), hipMemcpyHostToDevice));
    sc->small_stage_n = (int)tab.size(); sc->small_stage_N = c->N;
  }
  A.stage = sc->small_stage; A.nstage = sc->small_stage_n;
  c->last_solver = 7;
  c->last_step_kind = 2;
  c->last_assembly = 5;
  if (!tr && TimeBegin(c, 3)) return -2;
  // (256 threads, one wavefront per SIMD: the evaluation needs more than the 256 registers a lane has at two per SIMD -
  // 512 threads spilled 19 / 67 registers to scratch inside it and the step was slower than the two launches)
  {  // the model's shape and band width, the solved system's band width (a KKT context's is wider), the loop's instantiation or the plain step's
    const int shape = c->M.fast_shape, w = 3 * c->nq, ws = 3 * p.k;
    const bool trk = tr || kkt;
    bool launched = false;
#define SMALL_LAUNCH(SH, WM, WSM, TR) \
    if (shape == SH && w == WM && ws == WSM && trk == TR) { hipLaunchKernelGGL((gn_small_kernel<SH, WM, 256, WSM, TR>), dim3(gx * p.grid, c->batch), dim3(p.threads), p.lds, c->stream, A); launched = true; }
    IDTO_SMALL_KERNELS(SMALL_LAUNCH)
#undef SMALL_LAUNCH
    if (!launched) return NoKernel("gn_small_kernel", ws);
  }
  HIP_OK(hipGetLastError());
  c->fd_full = !last; c->partials_ahead = false;
  c->terms_valid = false;   // (no single-record products: a later idto_hip_grad_hess assembles from the slab)
  return tr ? 0 : TimeEnd(c);
}

static int FactorSolve(idto_hip_ctx* c, const double* rhs, int nrhs, double* x, const RhsSource* src,
                       const SolverPlan* planned = nullptr, const SolverExtras& ex = SolverExtras{});
int idto_hip_factor_solve(idto_hip_ctx* c, const double* rhs, int nrhs, double* x) {
  return FactorSolve(c, rhs, nrhs, x, nullptr);
}
// src: the right-hand sides are [g | J^T] read in place (penta_apply.h RhsSource; nrhs > 1), `rhs` is then any valid
// pointer to (N + 1) nq doubles for the factorisation kernel's unused first column
// planned, ex: (idto_hip_gn_step, idto_hip_tr_solve; the solve of -g) the plan the caller has made for this solve and
// what it found the plan's launch can do besides
static int FactorSolve(idto_hip_ctx* c, const double* rhs, int nrhs, double* x, const RhsSource* src, const SolverPlan* planned,
                       const SolverExtras& ex) {
  const bool x0_written = src != nullptr;   // (the substitution kernel zeroes x_0 itself)
  HIP_OK(hipSetDevice(c->device));
  if (!rhs) DropPrefetch(c, {IDTO_ARR_STEP});
  const int n = c->N + 1, k = c->nq;
  const double* b = rhs ? rhs : c->g;
  double* xo = rhs ? x : c->step;
  if (!rhs) nrhs = 1;
  if (nrhs < 1) { g_err = "nrhs < 1"; return -1; }
  if (rhs && c->batch != 1) { g_err = "explicit right-hand sides serve single-problem contexts"; return -1; }
  if (TimeBegin(c, 2)) return -2;
  c->last_step_kind = rhs ? 0 : 1;
  if (c->reference_solver) {
    c->last_solver = 3;
    if (++c->fact_id == 0) c->fact_id = 1;
    hipLaunchKernelGGL(penta_kernel, dim3(1, c->batch), dim3(256), c->penta_lds, c->stream, n, k, c->HA, c->HB, c->HC, b,
                       rhs ? 1.0 : -1.0, xo, c->Kst, c->LUst, c->pivst, c->Yst, c->Zst, c->status_dev, c->fact_id,
                       c->pstride);
    HIP_OK(hipGetLastError());
    if (TimeEnd(c)) return -2;
    if (nrhs > 1) {
      hipLaunchKernelGGL(penta_solve_kernel, dim3(nrhs - 1), dim3(64), c->solve_lds, c->stream, n, k, c->HA, c->Kst,
                         c->LUst, c->pivst, c->Yst, c->Zst, rhs + (size_t)n * k, x + (size_t)n * k);
      HIP_OK(hipGetLastError());
    }
    return 0;
  }
  // block LDL^T: factorise once with the first right-hand side (two-sided when the horizon is
  // long enough; the substitution kernel walks both chains of factors) ...
  // (several right-hand sides: the factorisation stops after its forward pass, every column incl. the first is
  // substituted by penta_apply_kernel - the chains' own back substitution would only delay the others)
  SolverPlan own;
  if (!planned) {
    SolveRequest rq;
    rq.nrhs = nrhs;
    if (int rp = Plan(c, c->h_assembled, rq, &own)) return rp;
    planned = &own;
  }
  const SolverPlan& p = *planned;
  int rc = LaunchLdl(c, p, b, rhs ? 1.0 : -1.0, xo, /*factor_only=*/nrhs > 1, ex);
  const int r0 = p.r0, ns = p.n, K = p.apply_K, m_split = p.m_split;   // the sub-system the launch factorised
  if (r0 && rhs && !x0_written)  // x_0 = rhs_0 for every column (row 0 of H is the identity); the default rhs has g_0 = 0 = x_0
    HIP_OK(hipMemcpy2DAsync(x, (size_t)n * k * sizeof(double), rhs, (size_t)n * k * sizeof(double), (size_t)k * sizeof(double),
                            (size_t)nrhs, hipMemcpyDeviceToDevice, c->stream));
  if (rc) return rc;
  if (nrhs > 1) {
    // ... then substitute the other right-hand sides in parallel: one wavefront each (two, one per chain, when the
    // factorisation was two-sided)
    const int waves = 4, cols = m_split > 0 ? waves / 2 : waves, blocks = (nrhs + cols - 1) / cols;
    const int lds = p.apply_lds;
    const double* b1 = b + (size_t)r0 * k;
    double* x1 = xo + (size_t)r0 * k;
    if (!c->Tst && Alloc(c, idto_host::SolverBufferCounts(k, c->N).apply_t, &c->Tst)) return -2;
    RhsSource RS{};
    if (src) { RS = *src; RS.r0 = r0; }
#define APPLY_LAUNCH(KM)                                                                                          \
    if (KM <= 8) {   /* small blocks: the forward pass reads the row-major factors directly, no transposed copies */ \
      hipLaunchKernelGGL((penta_apply_kernel<KM, true>), dim3(blocks), dim3(64 * waves), lds, c->stream, ns, k, c->Ust, \
                         c->Hst, c->Est, c->Dst, c->Tst, b1, rhs ? 1.0 : -1.0, nrhs, x1, m_split, (size_t)n * k, RS);  \
    } else {                                                                                                        \
      hipLaunchKernelGGL(penta_factor_transpose_kernel<KM>, dim3(ns, 3), dim3(256), 0, c->stream, c->Ust, c->Hst,  \
                         c->Est, c->Tst);                                                                          \
      hipLaunchKernelGGL((penta_apply_kernel<KM, false>), dim3(blocks), dim3(64 * waves), lds, c->stream, ns, k, c->Ust, \
                         c->Hst, c->Est, c->Dst, c->Tst, b1, rhs ? 1.0 : -1.0, nrhs, x1, m_split, (size_t)n * k, RS); \
    }
#define APPLY_CASE(KM) case KM: APPLY_LAUNCH(KM); break;
    switch (K) {
      IDTO_APPLY_KERNELS(APPLY_CASE)
      default: return NoKernel("penta_apply_kernel", K);
    }
#undef APPLY_CASE
#undef APPLY_LAUNCH
    HIP_OK(hipGetLastError());
  }
  return TimeEnd(c);
}

int idto_hip_solve_host(idto_hip_ctx* c, const double* rhs_host, int nrhs, double* x_host) {
  HIP_OK(hipSetDevice(c->device));
  if (!rhs_host || !x_host || nrhs < 1) { g_err = "solve_host: bad arguments"; return -1; }
  if (c->batch != 1) { g_err = "solve_host serves single-problem contexts"; return -1; }
  const size_t count = (size_t)nrhs * (c->N + 1) * c->nq;
  if (EnsureStage(c, count)) return -2;
  c->con_ready = false; c->con_begun = false;  // the staging buffers are shared with the constraint step
  HIP_OK(hipMemcpyAsync(c->stage_rhs, rhs_host, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int rc = idto_hip_factor_solve(c, c->stage_rhs, nrhs, c->stage_x);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(x_host, c->stage_x, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return FactorStatus(c);
}

static void LaunchDenseLdl(idto_hip_ctx* c, double* S, double* L, double* d, double* stat, double* rv, int neq, const double* b,
                           double b_sign, const double* b2);
static std::atomic<long> g_dense_solves{0};
long idto_hip_dense_solve_count() { return g_dense_solves.load(); }   // (tests: which branch of SolveLinearSystemInPlace ran)
#ifdef IDTO_TR_STAMPS
// (measurement build, tools/tr_stamps.py) the trust-region kernels' phase stamps of the last iteration, 100 MHz ticks
extern "C" int idto_hip_debug_tr_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(idto_dev::g_tr_stamps), 64 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif

// SolveLinearSystemInPlace's kDenseLdlt branch (reference optimizer/trajectory_optimizer.cc:2088-2093): H.MakeDense(),
// LDL^T, solve.  The debugging / cross-checking solver of the reference (its default is the block Thomas algorithm): the
// resident bands are spread into an n x n matrix (dense_from_bands_kernel), factorised by the blocked LDL^T of
// dense_ldl.h - one launch per panel of 32 columns, the right-hand side's forward substitution carried along - and
// substituted backwards by one workgroup.  Without pivoting (Eigen's ldlt() pivots on the diagonal): H is positive
// definite whenever the block Thomas branch succeeds; a pivot that is not positive and finite is reported as
// IDTO_HIP_FACTORIZATION_FAILED, where the reference's DRAKE_DEMAND(info() == Success) aborts.
int idto_hip_solve_dense_ldlt(idto_hip_ctx* c, const double* rhs_host, double* x_host) {
  HIP_OK(hipSetDevice(c->device));
  if (!rhs_host || !x_host) { g_err = "solve_dense_ldlt: bad arguments"; return -1; }
  if (c->batch != 1) { g_err = "solve_dense_ldlt serves single-problem contexts"; return -1; }
  const int nblk = c->N + 1, bs = c->nq, n = nblk * bs;
  ++g_dense_solves;
  if (c->dn_n != n) {
    Release(c, &c->dn_S); Release(c, &c->dn_d); Release(c, &c->dn_stat); Release(c, &c->dn_rv);
    c->dn_n = 0;
    if (Alloc(c, 2 * (size_t)n * n, &c->dn_S) || Alloc(c, (size_t)n, &c->dn_d) || Alloc(c, (size_t)2, &c->dn_stat) ||
        Alloc(c, 3 * (size_t)n, &c->dn_rv))   // [r with the finished panels eliminated | y = L^-1 r | x]
      return -2;
    c->dn_n = n;
  }
  if (EnsureStage(c, (size_t)n)) return -2;
  c->con_ready = false; c->con_begun = false;  // the staging buffers are shared with the constraint step
  const double stat0[2] = {std::numeric_limits<double>::infinity(), 0.0};
  HIP_OK(hipMemcpyAsync(c->stage_rhs, rhs_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemcpyAsync(c->dn_stat, stat0, sizeof(stat0), hipMemcpyHostToDevice, c->stream));
  double *S = c->dn_S, *L = c->dn_S + (size_t)n * n, *x = c->dn_rv + 2 * (size_t)n;
  hipLaunchKernelGGL(dense_from_bands_kernel, dim3(nblk), dim3(256), 0, c->stream, c->HA, c->HB, c->HC, nblk, bs, S);
  LaunchDenseLdl(c, S, L, c->dn_d, c->dn_stat, c->dn_rv, n, c->stage_rhs, 1.0, nullptr);
  hipLaunchKernelGGL(dense_ldl_solve_kernel, dim3(1), dim3(512), (n + 512 + DENSE_NB * (DENSE_NB + 1)) * sizeof(double), c->stream,
                     L, n, c->dn_d, c->dn_rv + n, 1.0, (const double*)nullptr, x, 1);
  HIP_OK(hipGetLastError());
  double stat[2];
  HIP_OK(hipMemcpyAsync(x_host, x, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(stat, c->dn_stat, sizeof(stat), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (!(stat[0] > 0.0) || !std::isfinite(stat[1])) {
    g_err = "solve_dense_ldlt: a pivot of the dense LDL^T is not positive and finite";
    return IDTO_HIP_FACTORIZATION_FAILED;
  }
  return 0;
}

// The constrained degrees of freedom on the device: ONE copy, shared by the banded KKT step (which needs nothing else;
// batch contexts included) and by the Schur-complement route.  (Round 4 kept a list per route and each invalidated the
// other's: a resident KKT solve followed by the host loop - the TRF_SINGULAR_S fallback, or SolveFromWarmStart followed
// by EvalLagrangeMultipliers - allocated con_dofs, con_S, con_L, ... again on every alternation, and Alloc never frees:
// an MPC server on that path leaked ~2 MB per re-plan at allegro's size and paid a device-wide synchronisation each time.)
static int DeviceDofs(idto_hip_ctx* c, const int* dofs, int nu, const char* who, bool* changed) {
  if (!dofs || nu < 1 || nu > c->nv) { g_err = std::string(who) + ": bad arguments"; return -1; }
  for (int j = 0; j < nu; ++j)
    if (dofs[j] < 0 || dofs[j] >= c->nv) { g_err = std::string(who) + ": dof index out of range"; return -1; }
  *changed = !(c->con_dofs && c->con_dofs_host.size() == (size_t)nu && std::equal(dofs, dofs + nu, c->con_dofs_host.begin()));
  if (!*changed) return 0;
  if (int rc = c->con_dofs.Ensure((size_t)nu)) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));   // (work that reads the previous set may still be enqueued)
  HIP_OK(hipMemcpy(c->con_dofs, dofs, (size_t)nu * sizeof(int), hipMemcpyHostToDevice));
  c->con_dofs_host.assign(dofs, dofs + nu);
  c->con_nu = nu; c->con_neq = nu * c->N;
  c->con_schur_valid = false;   // (the Schur route's buffers, if any, were sized for another set)
  c->con_begun = false;
  return 0;
}
static int ConstraintDofs(idto_hip_ctx* c, const int* dofs, int nu) {
  bool changed = false;
  return DeviceDofs(c, dofs, nu, "equality constraints", &changed);
}
// the device arrays of the Schur-complement route for this set of degrees of freedom (made again - the superseded ones
// freed - only when the set really changes)
static int ConstraintBuffers(idto_hip_ctx* c, const int* dofs, int nu) {
  if (c->batch != 1) { g_err = "the equality-constraint step serves single-problem contexts"; return -1; }
  bool changed = false;
  if (int rc = DeviceDofs(c, dofs, nu, "constraint_schur", &changed)) return rc;
  const int N = c->N, n = (N + 1) * c->nq, neq = nu * N;
  if (!c->con_schur_valid) {
    // (made again for every new set, zero-filled, not only for a larger one)
    for (Grown<double>* b : {&c->con_S, &c->con_d, &c->con_h, &c->con_L, &c->con_rv}) b->Reset();
    if (c->con_S.Ensure((size_t)neq * neq + neq) ||
        c->con_d.Ensure((size_t)neq) || c->con_h.Ensure((size_t)neq + 2) || c->con_L.Ensure((size_t)neq * neq) ||
        c->con_rv.Ensure(2 * (size_t)neq))   // [r with the finished panels eliminated | y = L^-1 r]
      return -2;
    if (int rc = c->con_pin.Ensure((size_t)neq * neq + neq + 2 * (size_t)n + 2 * (size_t)neq + 4)) return rc;
    c->con_schur_valid = true;
    c->con_begun = false;
  }
  return 0;
}

int idto_hip_constraint_schur_begin(idto_hip_ctx* c, const int* dofs, int nu) {
  HIP_OK(hipSetDevice(c->device));
  if (!dofs || nu < 1 || nu > c->nv) { g_err = "constraint_schur: bad arguments"; return -1; }
  if (c->batch != 1) { g_err = "the equality-constraint step serves single-problem contexts"; return -1; }
  const int N = c->N, n = (N + 1) * c->nq, neq = nu * N;
  if (c->con_begun && c->con_nu == nu && std::equal(dofs, dofs + nu, c->con_dofs_host.begin()))
    return 0;  // already enqueued for the current Hessian
  if (int rc = ConstraintBuffers(c, dofs, nu)) return rc;
  c->con_ready = false; c->con_begun = false;
  if (EnsureStage(c, (size_t)(neq + 1) * n)) return -2;
  // Y = H^-1 [g | J^T]: the right-hand sides are read where they are (g; rows of the slab records), nothing is staged
  RhsSource src{};
  src.slab = c->slab; src.slab_stride = c->slab_stride; src.nu = nu; src.nv = c->nv; src.r0 = 0;
  src.dofs = c->con_dofs; src.g = c->g; src.alt = c->alt_r;
  int rc = FactorSolve(c, c->g, neq + 1, c->stage_x, &src);
  if (rc) return rc;
  hipLaunchKernelGGL(constraint_schur_kernel, dim3(neq), dim3(256), 3 * c->nq * sizeof(double), c->stream, c->slab,
                     c->slab_stride, c->con_dofs, nu, N, c->nq, c->nv, c->stage_x, neq, c->con_S,
                     c->con_S + (size_t)neq * neq, c->alt_r);
  HIP_OK(hipGetLastError());
  c->con_S_factored = false;
  c->con_begun = true;
  return 0;
}

int idto_hip_constraint_schur(idto_hip_ctx* c, const int* dofs, int nu, double* S_host, double* Jy_host) {
  HIP_OK(hipSetDevice(c->device));
  if (!S_host || !Jy_host || !dofs) { g_err = "constraint_schur: bad arguments"; return -1; }
  const bool same = c->con_begun && nu == c->con_nu && std::equal(dofs, dofs + nu, c->con_dofs_host.begin());
  if (!same) {
    int rc = idto_hip_constraint_schur_begin(c, dofs, nu);
    if (rc) return rc;
  }
  const int neq = c->con_neq;
  if (c->con_S_factored) {  // the device factorisation overwrote S: form it again from Y
    hipLaunchKernelGGL(constraint_schur_kernel, dim3(neq), dim3(256), 3 * c->nq * sizeof(double), c->stream, c->slab,
                       c->slab_stride, c->con_dofs, c->con_nu, c->N, c->nq, c->nv, c->stage_x, neq, c->con_S,
                       c->con_S + (size_t)neq * neq, c->alt_r);
    HIP_OK(hipGetLastError());
    c->con_S_factored = false;
  }
  HIP_OK(hipMemcpyAsync(c->con_pin, c->con_S, ((size_t)neq * neq + neq) * sizeof(double), hipMemcpyDeviceToHost,
                        c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(S_host, c->con_pin, (size_t)neq * neq * sizeof(double));
  std::memcpy(Jy_host, c->con_pin + (size_t)neq * neq, (size_t)neq * sizeof(double));
  c->con_ready = true;
  return FactorStatus(c);
}

// S = L D L^T without pivoting, one launch per panel of 32 columns (dense_ldl.h dense_ldl_step_kernel); L -> con_L
// together with the forward substitution of the right-hand side r = b2 + b_sign b (-> con_rv = L^-1 r)
static void LaunchDenseLdl(idto_hip_ctx* c, double* S, double* L, double* d, double* stat, double* rv, int neq, const double* b,
                           double b_sign, const double* b2) {
  for (int j0 = 0; j0 < neq; j0 += DENSE_NB) {
    const int j1 = j0 + DENSE_NB, below = neq > j1 ? neq - j1 : 0;
    const int tiles = below > 0 ? (below + 31) / 32 : 1;
    hipLaunchKernelGGL(dense_ldl_step_kernel, dim3(tiles, tiles), dim3(256), 0, c->stream, S, L, neq, j0, d, stat,
                       b, b_sign, b2, rv, rv + neq);
  }
}
static void LaunchDenseLdl(idto_hip_ctx* c, double* S, int neq, const double* b, double b_sign, const double* b2) {
  LaunchDenseLdl(c, S, c->con_L, c->con_d, c->con_h, c->con_rv, neq, b, b_sign, b2);
}

int idto_hip_constraint_solve(idto_hip_ctx* c, const double* h_host, double* lambda_host, double* step_host,
                              double* jtl_host) {
  HIP_OK(hipSetDevice(c->device));
  if (!c->con_begun) { g_err = "constraint_solve: call idto_hip_constraint_schur_begin for the current Hessian first"; return -1; }
  if (!h_host || !lambda_host || !step_host || !jtl_host) { g_err = "constraint_solve: bad arguments"; return -1; }
  if (c->con_S_factored) { g_err = "constraint_solve: already called for this Hessian"; return -1; }
  const int N = c->N, n = (N + 1) * c->nq, neq = c->con_neq;
  // pinned layout behind [S | Jy]: [min, max | h] up, [min, max | lambda | step | J^T lambda] down
  double* pin = c->con_pin + (size_t)neq * neq + neq;
  pin[0] = std::numeric_limits<double>::infinity(); pin[1] = 0.0;
  std::memcpy(pin + 2, h_host, (size_t)neq * sizeof(double));
  HIP_OK(hipMemcpyAsync(c->con_h, pin, (size_t)(neq + 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  double* S = c->con_S;
  LaunchDenseLdl(c, S, neq, S + (size_t)neq * neq, -1.0, c->con_h + 2);
  c->con_S_factored = true;
  c->con_lambda_at = c->con_lambda + 2;
  // lambda = S^-1 (h - J y_g): the forward substitution went with the factorisation
  hipLaunchKernelGGL(dense_ldl_solve_kernel, dim3(1), dim3(512), (neq + 512 + DENSE_NB * (DENSE_NB + 1)) * sizeof(double), c->stream, c->con_L, neq, c->con_d,
                     c->con_rv + neq, 1.0, (const double*)nullptr, c->con_lambda + 2, 1);
  hipLaunchKernelGGL(constraint_step_kernel, dim3((n + 63) / 64), dim3(64 * STEP_WAVES), (neq + 64 * STEP_WAVES) * sizeof(double), c->stream, c->slab,
                     c->slab_stride, c->con_dofs, c->con_nu, N, c->nq, c->nv, c->stage_x, neq, c->con_lambda + 2,
                     c->con_out, c->con_out + n, c->alt_r);
  HIP_OK(hipGetLastError());
  double* down = pin + neq + 2;
  HIP_OK(hipMemcpyAsync(down, c->con_h, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(down + 2, c->con_lambda + 2, (size_t)neq * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(down + 2 + neq, c->con_out, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->con_ready = true;  // Y is in place for idto_hip_constraint_step (fallback path)
  if (int fs = FactorStatus(c)) return fs;  // H itself was not positive definite
  const double dmin = down[0], dmax = down[1];
  if (!(dmin > 1e-13 * dmax) || !std::isfinite(dmax)) return 1;  // (semi-)singular S: the caller pivots on the host
  std::memcpy(lambda_host, down + 2, (size_t)neq * sizeof(double));
  std::memcpy(step_host, down + 2 + neq, (size_t)n * sizeof(double));
  std::memcpy(jtl_host, down + 2 + neq + n, (size_t)n * sizeof(double));
  return 0;
}

int idto_hip_constraint_step(idto_hip_ctx* c, const double* lambda_host, double* step_host, double* jtl_host) {
  HIP_OK(hipSetDevice(c->device));
  if (!c->con_ready) { g_err = "constraint_step: call idto_hip_constraint_schur for the current Hessian first"; return -1; }
  if (!lambda_host || !step_host || !jtl_host) { g_err = "constraint_step: bad arguments"; return -1; }
  const int N = c->N, n = (N + 1) * c->nq, neq = c->con_neq;
  double* pl = c->con_pin + (size_t)neq * neq + neq;  // [lambda | step | J^T lambda]
  std::memcpy(pl, lambda_host, (size_t)neq * sizeof(double));
  HIP_OK(hipMemcpyAsync(c->con_lambda, pl, (size_t)neq * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->con_lambda_at = c->con_lambda;
  hipLaunchKernelGGL(constraint_step_kernel, dim3((n + 63) / 64), dim3(64 * STEP_WAVES), (neq + 64 * STEP_WAVES) * sizeof(double), c->stream, c->slab,
                     c->slab_stride, c->con_dofs, c->con_nu, N, c->nq, c->nv, c->stage_x, neq, c->con_lambda, c->con_out,
                     c->con_out + n, c->alt_r);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(pl + neq, c->con_out, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(step_host, pl + neq, (size_t)n * sizeof(double));
  std::memcpy(jtl_host, pl + neq + n, (size_t)n * sizeof(double));
  return FactorStatus(c);
}

int idto_hip_set_unactuated_dofs(idto_hip_ctx* c, const int* dofs, int nu) {
  HIP_OK(hipSetDevice(c->device));
  if (nu < 0 || nu > c->nv || (nu > 0 && !dofs)) { g_err = "set_unactuated_dofs: bad arguments"; return -1; }
  for (int j = 0; j < nu; ++j)
    if (dofs[j] < 0 || dofs[j] >= c->nv) { g_err = "set_unactuated_dofs: dof index out of range"; return -1; }
  // (every SolveFromWarmStart sets them: a device allocation and a copy only when the set changes - the allocation alone
  // was 0.1 ms of an MPC re-plan, and stayed allocated until the context went)
  if (nu == c->una_nu && (nu == 0 || (c->una_dofs && std::equal(dofs, dofs + nu, c->una_dofs_host.begin())))) return 0;
  c->una_nu = nu;
  c->una_dofs_host.assign(dofs, dofs + nu);
  if (nu > 0 && Upload(c, dofs, (size_t)nu, &c->una_dofs)) return -2;
  return 0;
}

// ---- device-side trust-region bookkeeping (trust_region.h)
static TrRowsArgs PrepareArgs(idto_hip_ctx* c, int scaling_method, int with_lambda) {
  const int n = (c->N + 1) * c->nq;
  TrRowsArgs A;
  A.nblk = c->N + 1; A.K = c->nq;
  A.HA = c->HA; A.HB = c->HB; A.HC = c->HC; A.g = c->g;
  A.jtl = with_lambda ? c->con_out + n : nullptr;
  A.yin = with_lambda ? c->con_out : c->step;
  A.ysign = with_lambda ? 1.0 : -1.0;
  A.q = c->q; A.scaling_method = scaling_method;
  A.Dprev = c->tr_Dprev; A.D = c->tr_D; A.gt = c->tr_gt; A.w = c->tr_w;
  A.slab = c->slab; A.slab_stride = c->slab_stride; A.tau_off = 3 * c->nv * c->nq;
  A.dofs = with_lambda ? c->con_dofs : c->una_dofs;
  A.nu = with_lambda ? c->con_nu : c->una_nu;
  A.N = c->N;
  A.lambda = with_lambda ? c->con_lambda_at : nullptr;
  A.partial = c->tr_part;
  A.freeze = nullptr;   // (idto_hip_tr_solve points it at the loop's sticky flags)
  A.part_ll = nullptr; A.epoch = 0u; A.dq_old = nullptr;   // (... and these at the hand-over between tr_iter_kernel's workgroups)
  A.kx = TrKkt{};
  return A;
}

static int EnqueuePrepare(idto_hip_ctx* c, int scaling_method, int with_lambda) {
  const int n = (c->N + 1) * c->nq;
  const int lds = tr_rows_lds(c->nq) * (int)sizeof(double);
  hipLaunchKernelGGL(tr_prepare_rows_kernel, dim3(c->N + 1), dim3(256), lds, c->stream,
                     PrepareArgs(c, scaling_method, with_lambda));
  hipLaunchKernelGGL(tr_prepare_sum_kernel, dim3(1), dim3(256), 0, c->stream, c->N + 1, c->tr_part, c->tr_out, c->tr_D,
                     c->tr_Dprev, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(c->tr_pin, c->tr_out, 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return 0;
}

int idto_hip_tr_set_scale_memory(idto_hip_ctx* c, const double* D_prev_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch != 1) { g_err = "tr_set_scale_memory serves single-problem contexts"; return -1; }
  const size_t n = (size_t)(c->N + 1) * c->nq;
  std::vector<double> ones;
  if (!D_prev_host) { ones.assign(n, 1.0); D_prev_host = ones.data(); }
  c->spec_ready = false;   // (a speculative tr_prepare used the previous memory)
  HIP_OK(hipMemcpyAsync(c->tr_Dprev, D_prev_host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));   // (the host buffer may be a temporary)
  return 0;
}

int idto_hip_tr_set_convergence(idto_hip_ctx* c, const double* tolerances) {
  c->tr_conv_on = tolerances != nullptr;
  for (int i = 0; i < 6; ++i) c->tr_conv_tol[i] = tolerances ? tolerances[i] : 0.0;
  return 0;
}

int idto_hip_tr_prepare(idto_hip_ctx* c, int scaling_method, int with_lambda, double* out_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch != 1) { g_err = "tr_prepare serves single-problem contexts"; return -1; }
  if (scaling_method < -1 || scaling_method > 3) { g_err = "tr_prepare: bad scaling method"; return -1; }
  if (with_lambda && (!c->con_ready || !c->con_lambda_at)) {
    g_err = "tr_prepare: multipliers requested but no constraint step is resident";
    return -1;
  }
  if (c->spec_ready && !with_lambda && c->spec_scaling == scaling_method) {
    // the accepted trial point's iteration was enqueued speculatively by idto_hip_tr_trial
    c->spec_ready = false;
  } else {
    c->spec_ready = false;
    if (int rc = EnqueuePrepare(c, scaling_method, with_lambda)) return rc;
  }
  HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(out_host, c->tr_pin, 9 * sizeof(double));
  return FactorStatus(c);
}

int idto_hip_tr_trial(idto_hip_ctx* c, double a, double b, int scaling, int normalize_quaternions, int with_lambda,
                      int speculate_scaling_method, double* out_host) {
  HIP_OK(hipSetDevice(c->device));
  if (c->batch != 1) { g_err = "tr_trial serves single-problem contexts"; return -1; }
  c->spec_pending = false; c->spec_ready = false;
  const int n = (c->N + 1) * c->nq;
  DropPrefetch(c, {IDTO_ARR_V, IDTO_ARR_A, IDTO_ARR_NPLUS, IDTO_ARR_SLAB, IDTO_ARR_COST});
  hipLaunchKernelGGL(tr_trial_kernel, dim3(1), dim3(1024), (size_t)2 * (n + c->N + 1) * sizeof(double), c->stream, n, c->nq, c->tr_D, c->tr_gt,
                     c->tr_w, a, b, scaling, c->q, c->q_trial, c->tr_dq, c->tr_quat,
                     normalize_quaternions ? c->tr_nquat : 0, c->tr_out + 9);
  HIP_OK(hipGetLastError());
  // tau and the cost at the trial point: the same kernels as idto_hip_eval_tau, reading q_trial
  std::swap(c->q, c->q_trial);
  int rc = LaunchFd(c, 0, 0, c->N);
  if (!rc) {
    hipLaunchKernelGGL(cost_kernel, dim3(1), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->q, c->v, c->slab,
                       c->slab_stride, c->cost, c->weights_diagonal ? 1 : 0, (double*)nullptr, (size_t)0, c->tr_out + 11, TrDecideArgs{}, AltSel{nullptr, 0, 0});
    if (with_lambda)
      hipLaunchKernelGGL(tr_hlambda_kernel, dim3(1), dim3(256), 16 * sizeof(double), c->stream, c->slab, c->slab_stride,
                         3 * c->nv * c->nq, c->con_dofs, c->con_nu, c->N, c->con_lambda_at, c->tr_out + 12);
  }
  std::swap(c->q, c->q_trial);
  if (rc) return rc;
  HIP_OK(hipGetLastError());
  c->fd_full = false; c->partials_ahead = false;
  c->trial_resident = true;
  HIP_OK(hipMemcpyAsync(c->tr_pin + 9, c->tr_out + 9, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  const bool speculate = speculate_scaling_method >= -1 && !with_lambda && FusedEligible(c) &&
                         speculate_scaling_method != 1 && speculate_scaling_method != 3;  // (adaptive scalings update D in place)
  if (speculate) {
    // the next iteration on the trial point, before the host has seen its cost: accepted steps (the
    // common case) find g, H, the Newton step and the inner products ready; a rejected step costs
    // one more idto_hip_gn_step on the old q
    if (!c->spec_ev) HIP_OK(hipEventCreateWithFlags(&c->spec_ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(c->spec_ev, c->stream));
    std::swap(c->q, c->q_trial);
    int rs = LaunchFused(c);
    if (!rs) rs = EnqueuePrepare(c, speculate_scaling_method, 0);
    std::swap(c->q, c->q_trial);
    if (rs) return rs;
    c->spec_pending = true;
    c->spec_scaling = speculate_scaling_method;
    HIP_OK(hipEventSynchronize(c->spec_ev));   // the trial point's scalars only
  } else {
    HIP_OK(hipStreamSynchronize(c->stream));
  }
  out_host[0] = c->tr_pin[9];    // dq . dq
  out_host[1] = c->tr_pin[10];   // g~ . D^-1 dq
  out_host[2] = c->tr_pin[11];   // cost at q + dq
  out_host[3] = with_lambda ? c->tr_pin[12] : 0.0;  // h(q + dq) . lambda
  return 0;
}

int idto_hip_tr_accept(idto_hip_ctx* c) {
  if (!c->trial_resident) { g_err = "tr_accept: no trial point is resident"; return -1; }
  std::swap(c->q, c->q_trial);   // v, a, tau, N+ and the cost in device memory already belong to it
  c->trial_resident = false;
  c->spec_ready = c->spec_pending;   // ... and so does the speculative iteration, if one was enqueued
  c->spec_pending = false;
  c->con_ready = false; c->con_begun = false;
  DropPrefetch(c, {IDTO_ARR_Q});
  return 0;
}

int idto_hip_tr_reject(idto_hip_ctx* c) {
  // the trial point is dropped: v, a, tau (and, after a speculative launch, the partials, g, H and the
  // Newton step) in device memory do not belong to the resident q any more
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  return 0;
}

// The solver-only context of the KKT system [H J^T; J 0] (kkt.h): block size nq + nu, the parent's horizon, stream and
// solver options; only what LaunchLdl / FactorStatus touch is allocated.
static int MakeKkt(idto_hip_ctx* c, int nu) {
  if (c->kkt && c->kkt_nu == nu) return 0;
  if (c->kkt) { idto_hip_destroy(c->kkt); c->kkt = nullptr; }
  const int K = c->nq + nu, N = c->N, B = c->batch;
  if (K > 32) { g_err = "tr_solve: nq + nu <= 32 for the banded equality-constraint step"; return -1; }
  std::unique_ptr<idto_hip_ctx> k(new idto_hip_ctx);
  k->device = c->device; k->stream = c->stream; k->own_stream = false;
  k->batch = B; k->nq = K; k->nv = 0; k->N = N; k->dt = c->dt;
  // (seven workgroups for allegro's 29 x 29 blocks: 0.46 -> 0.29 ms per iteration; the small systems stay on two - the
  // nested-dissection order buys them 3 us and costs acrobot's multipliers a digit: 2e-8 against 3e-9)
  // (these two as they are when the context is made; the options of the table follow the parent from then on)
  k->two_sided = c->two_sided; k->solver_nd = c->solver_nd && (K == 29 || K == 8); k->solver_pipe = false; k->fused = false; k->asm_in_solver = false;
  k->solver_debug = c->kkt_debug;
#define X(name, kind, access, env, to_kkt, to_child) if (to_kkt) OptAssign(k->name, OPT_INT, c->name);
  IDTO_OPTIONS(X)
#undef X
  k->h_assembled = true;      // block row 0 is decoupled (q_0 is no variable, mu_0 a dummy): the chains start at row 1
  k->ldl_npos = c->nq;
  // one arena per problem, as in idto_hip_create_batch: the solver kernels take the problem from blockIdx.y
  if (PointIntoArena(k.get(), idto_host::ARENA_KKT, "hipMalloc (KKT context) failed") ||
      AllocStatusWords(k.get(), "hipHostMalloc (KKT solver status) failed")) {
    idto_hip_destroy(k.release());
    return -2;
  }
  c->kkt = k.release(); c->kkt_nu = nu;
  return 0;
}

static bool AsmInSolver(const idto_hip_ctx* c, SolverPlan* p);
namespace {
// idto_hip_tr_solve_batch_fetch's outputs beyond rows and radii (a batch of more than one problem)
struct TrBatchFetch {
  int only_best;
  double* out[5];   // q, v, tau, dq, w: [batch][...] or - only_best - [1][...]; any may be null
  double* final_cost; int* status; int* best;
  const MpcTickHook* mpc = nullptr;   // idto_hip_mpc_batch_replan: the store behind the gather, its doubles behind the fetch's
};
// One call of the device-resident trust-region loop: its parameters and where the results go.
// Delta0s / Delta_out: one radius per problem of the context; rows_host: [batch][iterations][TRR_COUNT]
struct TrRequest {
  int iterations, scaling_method, scaling, normalize_quaternions;
  const double* Delta0s; double Delta_max, eta; const int* constrained_dofs; int nu;
  double* rows_host; double* Delta_out;
  double* const* fetch = nullptr;         // idto_hip_tr_solve_fetch: q, v, tau, dq, w of the one problem; any may be null
  const TrBatchFetch* bfetch = nullptr;   // idto_hip_tr_solve_batch_fetch
};
// What is loop-invariant of the way through TrSolve
struct TrRoute {
  bool use_kkt, lookahead, adaptive, tr_small, tr_fold_fits;
  SolverPlan small_plan;   // of the system the small models' launch solves: H's, or the KKT context's
  int passes; TrConvergence conv;
};
inline size_t TrRowDoubles(const TrRequest& rq) { return (size_t)rq.iterations * TRR_COUNT; }   // of one problem's rows
// The fetching entry points' argument checks, `who` the message's prefix; missing: the required arrays when one is null.  (TrPlanRoute keeps its two, tr_resident_ok between them.)
int TrCheckArgs(const char* who, const TrRequest& rq, const char* missing) {
  if (missing) { g_err = std::string(who) + ": " + missing + " are required"; return -1; }
  if (rq.nu < 0 || (rq.nu > 0 && !rq.constrained_dofs)) { g_err = std::string(who) + ": bad constraint arguments"; return -1; }
  if (rq.iterations <= 0) { g_err = std::string(who) + ": iterations must be positive"; return -1; }
  return 0;
}
// Do these enforced constraints take the banded KKT step (kkt.h), the one route that serves a batch?  Blocks of nq + nu up to
// the 30 x 30 instantiation of the two-workgroup factorisation: allegro's 23 + 6, N = 60, 0.523 against 0.665 ms per iteration with
// the Schur-complement chain; the 32 x 32 one needs a third elimination wavefront and spills: 442 against 245 us at N = 20.
bool TrKktRoute(const idto_hip_ctx* c, int nu) {
  return nu > 0 && c->con_kkt && idto_host::SolverBlockSize(c->nq + nu, true) <= 30 && c->weights_diagonal;
}
// the fetches' staging on the device and its pinned mirror, grown on demand
int EnsureFetch(idto_hip_ctx* c, size_t total) { return c->fetch.Ensure(total, total); }
// where the batch fetch's parts lie in that staging (tr_fetch.h)
TrFetchLayout BatchFetchLayout(const idto_hip_ctx* c, const TrRequest& rq) {
  const TrBatchFetch* bf = rq.bfetch;
  return TrFetchLayout::Make(c->batch, TRS_COUNT, TrRowDoubles(rq), c->N, c->nq, c->nv, bf->only_best != 0, true,
                             bf->mpc ? bf->mpc->nguess : 0, bf->mpc ? bf->mpc->nplans : 0);
}
// The refusals in front of everything that is enqueued, and the decisions that need nothing of the device
int TrPlanRoute(idto_hip_ctx* c, const TrRequest& rq, TrRoute* rt) {
  if (rq.bfetch && c->batch == 1) { g_err = "tr_solve: the batch fetch serves batches of more than one problem"; return -1; }
  TRACE("hip: tr_solve begins");
  if (rq.iterations <= 0) { g_err = "tr_solve: iterations must be positive"; return -1; }
  if (!c->tr_resident_ok) {
    g_err = "tr_solve: the iteration kernel's workgroups timed out on this context before (option tr_resident_ok): use "
            "idto_hip_tr_prepare / trial / accept / reject";
    return -1;
  }
  if (rq.nu < 0 || (rq.nu > 0 && !rq.constrained_dofs)) { g_err = "tr_solve: bad constraint arguments"; return -1; }
  if (rq.nu > 0 && !c->weights_diagonal) { g_err = "tr_solve: enforced constraints need diagonal cost weights"; return -1; }
  // (the adaptive methods, D = min(D_prev, f(diag H)): tr_iter_kernel keeps D_prev.  A rejected step leaves g and H where they are - the gated
  // assembly - so the next iteration forms min(D, f(diag H)) = D again: the memory does not advance, as in the reference, whose cached scale factors belong to the state that did not change.)
  if (rq.scaling_method < -1 || rq.scaling_method > 3) { g_err = "tr_solve: bad scaling method"; return -1; }
  rt->adaptive = rq.scaling_method == 1 || rq.scaling_method == 3;
  // (nu > 0 has diagonal weights here - the refusal above - so that the predicate's own look at them decides nothing)
  rt->use_kkt = TrKktRoute(c, rq.nu);
  rt->lookahead = c->weights_diagonal && c->asm_stop == 0 && c->fd_stop == 0;
  TrConvergence& conv = rt->conv = TrConvergence{};
  conv.on = c->tr_conv_on ? 1 : 0;
  conv.rel_cost = c->tr_conv_tol[0]; conv.abs_cost = c->tr_conv_tol[1]; conv.rel_grad = c->tr_conv_tol[2];
  conv.abs_grad = c->tr_conv_tol[3]; conv.rel_state = c->tr_conv_tol[4]; conv.abs_state = c->tr_conv_tol[5];
  // (with convergence checks the last iteration, too, is followed by g at its iterate: one more pass of the loop
  // body up to tr_iter_kernel, which then only evaluates the criteria)
  rt->passes = rq.iterations + (conv.on ? 1 : 0);
  return 0;
}
// ... and the rest where they stand in the stream, behind g and H of the first iterate: a route's refusals, the KKT context, the output sets, the small launch
int TrPlanLaunches(idto_hip_ctx* c, const TrRequest& rq, TrRoute* rt) {
  const int B = c->batch, nu = rq.nu;
  if (B != 1 && nu > 0 && !rt->use_kkt) { g_err = "tr_solve: enforced constraints on a batch need the banded KKT step (nq + nu <= 30, option con_kkt)"; return -1; }
  int rc = rt->use_kkt ? ConstraintDofs(c, rq.constrained_dofs, nu) : 0;
  if (!rc && rt->use_kkt) rc = MakeKkt(c, nu);
  if (rc) return rc;
  if (B != 1 && !rt->lookahead) { g_err = "tr_solve on a batch context needs the two-set evaluation (diagonal cost weights)"; return -1; }
  if (rt->adaptive && !rt->lookahead) { g_err = "tr_solve: the adaptive scalings need the gated assembly (diagonal cost weights)"; return -1; }
  if (nu > 0 && !rt->lookahead) { g_err = "tr_solve: enforced constraints need the two-set evaluation"; return -1; }
  // from here on the trial point's v, a, N+, tau, partials go to the set the iterate does not occupy (TrSolve's guard clears them)
  if (rt->lookahead) { c->alt_r = AltSel{c->tr_state, c->alt_off, 0}; c->alt_w = AltSel{c->tr_state, c->alt_off, 1}; }
  // (the small models' one-workgroup launch, gn_small.h: unconstrained, or with ONE enforced constraint through the banded
  // KKT step - the instantiations: acrobot 2 + 1, spinner 3 + 1 - whose context the scalar band solver takes)
  rt->tr_small = c->tr_small && rt->lookahead && SmallEligible(c, &rt->small_plan) && c->h_assembled;
  if (rt->tr_small && nu > 0)
    rt->tr_small = rt->use_kkt && nu == 1 && c->kkt->batch == c->batch && Plan(c->kkt, true, WholeStep(c), &rt->small_plan) == 0 &&
                   rt->small_plan.k == c->nq + 1;
  // (the folded iteration's arrays live in the band solver's carve-up)
  rt->tr_fold_fits = rt->tr_small && gn_small_fold_doubles(c->N, c->nq) <= rt->small_plan.lds_small;
  return 0;
}
// The loop's state words - of every problem [Delta, L(q) (resident: the caller evaluated the cost of q), ...] - and the iteration kernel's counter
int TrBegin(idto_hip_ctx* c, const TrRequest& rq) {
  const int B = c->batch;
  // (the larger one first: the previous, smaller one - an earlier solve's launches may read it - is freed behind its device-wide wait)
  if (int rc = c->tr_rows.Ensure((size_t)B * rq.iterations * TRR_COUNT, 0, true)) return rc;
  c->spec_pending = false; c->spec_ready = false; c->trial_resident = false;
  // tr_iter_kernel finds its last workgroup by counter == target: both restart with every solve, so that a
  // launch that failed in an earlier solve cannot leave them out of step
  c->tr_target = 0;
  if (B == 1) {
    // (one problem: one launch sets the state words, the cost among them, and the counter - no wait here, the loop is
    // enqueued while the evaluation of the initial guess still runs)
    static_assert(TRS_COUNT <= 16, "tr_pin holds 16 doubles");
    hipLaunchKernelGGL(tr_begin_kernel, dim3(1), dim3(64), 0, c->stream, c->tr_state, (int)TRS_COUNT, (int)TRS_DELTA,
                       (int)TRS_ACCEPTED, (int)TRS_COST, rq.Delta0s[0], c->cost, c->tr_cnt);
    HIP_OK(hipGetLastError());
    return 0;
  }
  HIP_OK(hipMemset2DAsync(c->tr_cnt, c->pstride, 0, sizeof(unsigned long long), (size_t)B, c->stream));
  std::vector<double> tmp; double* st = nullptr;
  if (rq.bfetch) {   // (pinned words of the context: no wait here - the call's one wait is behind the loop, and every return in between waits too)
    if (int rc = c->bstate_pin.Ensure((size_t)B * TRS_COUNT)) return rc;
    st = c->bstate_pin;
    std::fill(st, st + (size_t)B * TRS_COUNT, 0.0);
  } else { tmp.assign((size_t)B * TRS_COUNT, 0.0); st = tmp.data(); }
  for (int b = 0; b < B; ++b) { st[(size_t)b * TRS_COUNT + TRS_DELTA] = rq.Delta0s[b]; st[(size_t)b * TRS_COUNT + TRS_ACCEPTED] = 1.0; }
  HIP_OK(hipMemcpy2DAsync(c->tr_state, c->pstride, st, TRS_COUNT * sizeof(double), TRS_COUNT * sizeof(double), (size_t)B,
                          hipMemcpyHostToDevice, c->stream));
  if (!rq.bfetch) HIP_OK(hipStreamSynchronize(c->stream));   // (the host buffer is a temporary)
  HIP_OK(hipMemcpy2DAsync(c->tr_state + TRS_COST, c->pstride, c->cost, c->pstride, sizeof(double), (size_t)B,
                          hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// Multipliers of the iterate and H^-1 (g + J^T lambda) (TO.cc:1371-1396, :2139-2149) from ONE banded solve of the KKT system
// (kkt.h): build its bands from H and the slab's rows of J, factorise + solve, take the result apart.  ex: what taking it
// apart needs, for tr_iter_kernel's fold.  built: the assembly of the previous iteration wrote the system along.
int TrMultipliersKkt(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt, int k, bool* built, KktExtractArgs* ex) {
  idto_hip_ctx* kc = c->kkt; const int nu = rq.nu, B = c->batch;
  // (tr_small: from the second iteration on the launch that evaluated, decided and assembled has solved it too)
  const bool solved = rt.tr_small && k > 0;
  const bool was_built = *built;   // (option "kkt_in_asm")
  *built = false;
  KktBuildArgs Kb;
  Kb.N = c->N; Kb.nq = c->nq; Kb.nv = c->nv; Kb.nu = nu; Kb.HA = c->HA; Kb.HB = c->HB; Kb.HC = c->HC; Kb.g = c->g;
  Kb.slab = c->slab; Kb.slab_stride = c->slab_stride; Kb.dofs = c->con_dofs;
  Kb.KA = kc->HA; Kb.KB = kc->HB; Kb.KC = kc->HC; Kb.rhs = kc->g; Kb.alt = c->alt_r;
  Kb.pstride = c->pstride; Kb.kstride = kc->pstride;
  if (!solved) {
    if (!was_built) hipLaunchKernelGGL(kkt_build_kernel, dim3(c->N + 1, B), dim3(256), 0, c->stream, Kb);
    HIP_OK(hipGetLastError());
    if (int rc = idto_hip_factor_solve(kc, nullptr, 1, nullptr)) return rc;
  }
  // (taking z apart - w, J^T lambda, lambda, the multiplier pivots' range - is folded into tr_iter_kernel; option
  // "kkt_fold" 0 keeps kkt_extract_kernel's launch: tests hold the two against each other)
  KktExtractArgs& Ke = *ex;
  Ke.N = c->N; Ke.nq = c->nq; Ke.nv = c->nv; Ke.nu = nu;
  Ke.z = kc->step; Ke.slab = c->slab; Ke.slab_stride = c->slab_stride; Ke.dofs = c->con_dofs;
  Ke.w = c->con_out; Ke.jtl = c->con_out + (size_t)(c->N + 1) * c->nq; Ke.lambda = c->con_lambda;
  Ke.Dinv = kc->Dst; Ke.dstride = idto_host::SolverBlockSize(kc->nq, true); Ke.first_row = idto_host::SolverFirstRow(kc->h_assembled, kc->N);
  Ke.state = c->tr_state; Ke.alt = c->alt_r; Ke.pstride = c->pstride; Ke.kstride = kc->pstride;
  if (!c->kkt_fold) hipLaunchKernelGGL(kkt_extract_kernel, dim3(c->N + 1, B), dim3(64), 0, c->stream, Ke);
  HIP_OK(hipGetLastError());
  c->con_lambda_at = c->con_lambda;
  c->con_ready = false; c->con_begun = false;
  return 0;
}
// Multipliers of the iterate (TO.cc:1371-1396), all on the device: Y = H^-1 [g | J^T], S = J Y_J, J y_g (idto_hip_constraint_schur_begin),
// lambda = S^-1 (h - J y_g) in one workgroup, then H^-1 (g + J^T lambda) and J^T lambda (constraint_step_kernel)
int TrMultipliersSchur(idto_hip_ctx* c, const TrRequest& rq) {
  const int nu = rq.nu, neq = nu * c->N, n = (c->N + 1) * c->nq;
  c->con_begun = false;
  if (int rc = idto_hip_constraint_schur_begin(c, rq.constrained_dofs, nu)) return rc;
  if (neq <= CON_LAMBDA_MAX) {   // S in the LDS of one workgroup
    hipLaunchKernelGGL(constraint_lambda_kernel, dim3(1), dim3(CON_LAMBDA_THREADS),
                       (size_t)con_lambda_lds_doubles(neq) * sizeof(double), c->stream,
                       c->con_S, neq, c->slab, c->slab_stride, 3 * c->nv * c->nq, c->con_dofs, nu, c->con_lambda, c->tr_state,
                       c->alt_r, c->solver_debug ? c->dbg : (double*)nullptr);
    c->con_lambda_at = c->con_lambda;
  } else {                       // the blocked factorisation of dense_ldl.h, as idto_hip_constraint_solve runs it
    hipLaunchKernelGGL(constraint_h_kernel, dim3((neq + 255) / 256), dim3(256), 0, c->stream, c->slab, c->slab_stride,
                       3 * c->nv * c->nq, c->con_dofs, nu, neq, c->con_h, c->alt_r);
    double* S = c->con_S;
    LaunchDenseLdl(c, S, neq, S + (size_t)neq * neq, -1.0, c->con_h + 2);
    c->con_S_factored = true;
    hipLaunchKernelGGL(dense_ldl_solve_kernel, dim3(1), dim3(512), (neq + 512 + DENSE_NB * (DENSE_NB + 1)) * sizeof(double),
                       c->stream, c->con_L, neq, c->con_d, c->con_rv + neq, 1.0, (const double*)nullptr, c->con_lambda + 2, 1);
    hipLaunchKernelGGL(constraint_flag_kernel, dim3(1), dim3(1), 0, c->stream, c->con_h, c->tr_state);
    c->con_lambda_at = c->con_lambda + 2;
  }
  hipLaunchKernelGGL(constraint_step_kernel, dim3((n + 63) / 64), dim3(64 * STEP_WAVES),
                     (neq + 64 * STEP_WAVES) * sizeof(double), c->stream, c->slab, c->slab_stride, c->con_dofs, nu, c->N,
                     c->nq, c->nv, c->stage_x, neq, c->con_lambda_at, c->con_out, c->con_out + n, c->alt_r);
  HIP_OK(hipGetLastError());
  c->con_ready = true;
  return 0;
}
// tr_iter_kernel's arguments for pass k; kkt_ex: the KKT result for the kernel to take apart, or null
TrIterArgs TrIterArgsFor(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt, int k, const KktExtractArgs* kkt_ex) {
  TrIterArgs T;
  T.rows = PrepareArgs(c, rq.scaling_method, rq.nu > 0 ? 1 : 0);
  T.alt = c->alt_r; T.rows.part_ll = c->tr_part_ll; T.part2 = c->tr_part2;
  T.rows.epoch = ++c->tr_epoch;
  if (T.rows.epoch == 0u) T.rows.epoch = ++c->tr_epoch;   // (0 is what an arena that was never written holds)
  T.out = c->tr_out; T.state = c->tr_state; T.n = (c->N + 1) * c->nq; T.nq = c->nq; T.scaling = rq.scaling;
  T.nquat = rq.normalize_quaternions ? c->tr_nquat : 0;
  T.quat = c->tr_quat; T.q_trial = c->q_trial; T.dq = c->tr_dq;
  T.conv = rt.conv; T.conv.rows = c->tr_rows; T.conv.check_only = (k == rq.iterations) ? 1 : 0;
  T.fact_status = c->status_dev; T.fact_id = c->fact_id; T.timeout_status = c->status_dev + 2 * c->batch;   // (the most recent factorisation: this iteration's step)
  if (rt.use_kkt) { T.fact_status = c->kkt->status_dev; T.fact_id = c->kkt->fact_id; T.timeout_status = c->kkt->status_dev + 2 * c->batch; }
  T.rows.freeze = c->tr_state + TRS_FLAGS; T.pstride = c->pstride; T.rows_stride = TrRowDoubles(rq);
  T.kdinv = nullptr; T.kdstride = 0; T.kfirst_row = 0; T.kstride = 0; T.curpre = c->decide_word + 2;
  T.debug_skip_row = c->debug_skip_role >= 100 ? c->debug_skip_role - 100 : -1;
  if (kkt_ex) {
    T.rows.kx.z = kkt_ex->z; T.rows.kx.KK = c->nq + rq.nu; T.rows.kx.nv = c->nv;
    T.rows.kx.w_out = kkt_ex->w; T.rows.kx.jtl_out = kkt_ex->jtl; T.rows.kx.lambda_out = kkt_ex->lambda;
    T.kdinv = kkt_ex->Dinv; T.kdstride = kkt_ex->dstride; T.kfirst_row = kkt_ex->first_row; T.kstride = kkt_ex->kstride;
  }
  return T;
}
// the decision's arguments (cost_kernel's epilogue, or the launch that stands in for it)
TrDecideArgs TrDecideArgsFor(const idto_hip_ctx* c, const TrRequest& rq) {
  const int nu = rq.nu; TrDecideArgs Dc;
  Dc.state = c->tr_state; Dc.out = c->tr_out; Dc.rows = c->tr_rows; Dc.q = c->q; Dc.q_trial = c->q_trial;
  Dc.n = (c->N + 1) * c->nq; Dc.rows_stride = TrRowDoubles(rq); Dc.eta = rq.eta; Dc.Delta_max = rq.Delta_max;
  Dc.eps = 10 * std::numeric_limits<double>::epsilon() / c->P.dt / c->P.dt;   // TO.cc:2024
  Dc.lambda = nu > 0 ? c->con_lambda_at : nullptr; Dc.dofs = nu > 0 ? c->con_dofs : nullptr;
  Dc.nu = nu; Dc.N = c->N; Dc.slab_stride = c->slab_stride; Dc.tau_off = 3 * c->nv * c->nq; Dc.part2 = c->tr_part2; Dc.nblk = c->N + 1;
  return Dc;
}
// tau (with its partials: the trial point is the next iterate unless rejected) and the cost at the trial point, the decision, and - more:
// an iteration follows - g, H and the next step.  fold: tr_iter_kernel's part of this pass for the small launch to take along, or null.
int TrTrialAndNext(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt, const TrDecideArgs& Dc, bool more,
                   const TrIterArgs* fold, bool* kkt_built) {
  const int nu = rq.nu, B = c->batch; const bool lookahead = rt.lookahead;
  // a small all-revolute model: the trial point's evaluation, its cost, the decision and - accepted - g, H and the next
  // step in ONE workgroup of ONE launch (gn_small.h), the bits of the three launches below
  if (rt.tr_small) return LaunchSmall(c, rt.small_plan, &Dc, !more, c->alt_w, nu > 0, fold);
  std::swap(c->q, c->q_trial);
  int rc = LaunchFd(c, (lookahead && more) ? 1 : 0, 0, c->N, c->alt_w);
  c->fd_full = lookahead && more;   // (v, N+ of the trial point = of the iterate the gated assembly runs for)
  // the cost of the trial point and the decision: a launch of their own (cost_kernel), or one more workgroup of the
  // pipelined solver's launch that follows (penta_pipe.h PipeAsm::decide, option "decide_in_solver")
  SolverPlan sp;   // the next solve's, when its launch is to carry the gated assembly
  const bool asm_in_solver = !rc && more && lookahead && nu == 0 && c->h_assembled && AsmInSolver(c, &sp);
  const bool decide_in_solver = asm_in_solver && c->decide_in_solver && sp.can_decide;
  if (!rc && !decide_in_solver)
    hipLaunchKernelGGL(cost_kernel, dim3(1, B), dim3(1024), c->cost_lds, c->stream, c->M, c->P, c->q, c->v, c->slab,
                       c->slab_stride, c->cost, c->weights_diagonal ? 1 : 0, (double*)nullptr, c->pstride,
                       (double*)nullptr, Dc, c->alt_w);
  std::swap(c->q, c->q_trial);
  if (rc) return rc;
  HIP_OK(hipGetLastError());
  if (!more) return 0;
  if (asm_in_solver) {
    // the gated assembly inside the pipelined solver's launch (penta_pipe.h PipeAsm): a problem whose step was
    // rejected keeps g and H and the solver reads them where they are -> the same step
    DropPrefetch(c, {IDTO_ARR_GRADIENT, IDTO_ARR_H_A, IDTO_ARR_H_B, IDTO_ARR_H_C, IDTO_ARR_HBANDS});
    c->con_ready = false; c->con_begun = false;
    SolverExtras ex; ex.assemble = true; ex.gate = c->tr_state + TRS_ACCEPTED; ex.decide = decide_in_solver ? &Dc : nullptr;
    return FactorSolve(c, nullptr, 1, nullptr, nullptr, &sp, ex);
  }
  if (!lookahead) return idto_hip_gn_step(c);   // (dense cost weights: the partials again, at the iterate)
  if (rt.use_kkt && c->kkt_in_asm) {
    // (the next iteration's KKT system written by this assembly: a rejected step keeps g, H - and the system, which the
    // solvers only read)
    idto_hip_ctx* kc = c->kkt;
    KktSink S{};
    S.KA = kc->HA; S.KB = kc->HB; S.KC = kc->HC; S.rhs = kc->g; S.K = c->nq + nu; S.nu = nu; S.slab = c->slab; S.slab_stride = (int)c->slab_stride; S.dofs = c->con_dofs;
    rc = LaunchAssemble(c, c->tr_state + TRS_ACCEPTED, &S, kc->pstride, kkt_built);
  } else {
    rc = LaunchAssemble(c, c->tr_state + TRS_ACCEPTED);
  }
  if (!rc && nu == 0) rc = idto_hip_factor_solve(c, nullptr, 1, nullptr);   // (after a rejection: the same H, g -> the same step)
  return rc;
}
// One problem's code from the status words, after the wait (b < 0: the one problem of a single context).  A multiplier pivot that vanished -
// redundant constraints, TRF_SINGULAR_S in the rows: the caller's pivoted factorisation takes over - leaves garbage in the rows of H behind it,
// whose pivot test then fails as well: next to that flag a KKT pivot failure is no failure; a time-out always is.  (The batch-fetch exit used to ask
// both contexts before it weighed either; it relies on this: with the KKT step the context's own solver ran nothing in this call and tr_iter_kernel's time-out word is the KKT context's.)
int TrFactorVerdict(idto_hip_ctx* c, bool use_kkt, double flags_word, int b) {
  if (use_kkt) {
    const int fs = FactorStatus(c->kkt, b);
    const bool singular = ((int)flags_word & TRF_SINGULAR_S) != 0;
    if (fs == IDTO_HIP_SOLVER_TIMEOUT || (fs && !singular)) return fs;
  }
  return FactorStatus(c, b);
}
// a batch: the problems whose iterate ended up in the other set get it copied over (a single-problem context swaps its pointers instead)
int TrFoldSets(idto_hip_ctx* c) {
  hipLaunchKernelGGL(tr_fold_sets_kernel, dim3(64, c->batch), dim3(256), 0, c->stream, c->v, (size_t)c->alt_off / sizeof(double),
                     c->tr_state, c->pstride);
  HIP_OK(hipGetLastError());
  return 0;
}
// A tick from the plants, behind its wait: the plants' states and status words, which PlantState::tick_pin holds, go to the
// caller, and the host copies of the problems follow the states (as MpcShiftEnqueue moves them for a tick from the host)
void MpcPlantsBack(idto_hip_ctx* c, const MpcTickHook& hook) {
  const int B = c->batch;
  const size_t tick_w = (size_t)(1 + c->nq + c->nv);
  const double* s = hook.plant->tick_pin;
  MpcBatchState* m = hook.m;
  if (hook.plant_status_out) std::memcpy(hook.plant_status_out, s + (size_t)B * tick_w, (size_t)B * 2 * sizeof(int));
  for (int b = 0; b < B; ++b) {
    const double* x0 = s + (size_t)b * tick_w + 1;
    if (hook.x_after_out) std::memcpy(hook.x_after_out + (size_t)b * (tick_w - 1), x0, (tick_w - 1) * sizeof(double));
    if (b < (int)c->host_problems.size()) {
      HostProblemCopy& hp = *c->host_problems[(size_t)b];
      const std::vector<double> old0(hp.q_nom.begin(), hp.q_nom.begin() + c->nq);
      for (int t = 0; t < m->L.n; ++t)
        for (int i = 0; i < c->nq; ++i)
          hp.q_nom[(size_t)t * c->nq + i] = idto_spline::nominal_shift(hp.q_nom[(size_t)t * c->nq + i], m->selector[(size_t)i] != 0, x0[i], old0[(size_t)i]);
      std::copy(x0, x0 + c->nq, hp.q_init.begin());
      std::copy(x0 + c->nq, x0 + c->nq + c->nv, hp.v_init.begin());
    }
  }
  hook.followed = true;
}
// idto_hip_tr_solve_batch_fetch: state words, rows and the iterates of every problem (only_best: of the best one) packed
// by ONE launch, which also chooses the best problem; one copy, one wait (trust_region.h tr_gather_batch_kernel)
int TrFinishBatchFetch(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt) {
  const TrBatchFetch* bfetch = rq.bfetch;
  const MpcTickHook* hook = bfetch->mpc;
  const int B = c->batch;
  const TrFetchLayout L = BatchFetchLayout(c, rq);
  const size_t lds = (size_t)B * (sizeof(double) + sizeof(int));
  if (lds > 60 * 1024) { g_err = "tr_solve_batch_fetch: the batch is too large for the selecting workgroup's LDS"; return -1; }
  if (int erc = EnsureFetch(c, L.total())) return erc;
  TrGatherBatchArgs G;
  G.state = c->tr_state; G.rows = c->tr_rows; G.B = B; G.iterations = rq.iterations; G.nrows = (int)L.nrows; G.only_best = bfetch->only_best ? 1 : 0;
  G.q = c->q; G.v = c->v; G.slab = c->slab; G.dq = c->tr_dq; G.w = c->tr_w; G.nq = c->nq; G.nv = c->nv; G.slab_stride = (int)c->slab_stride;
  G.alt_off = (long long)c->alt_off; G.pstride = c->pstride; G.L = L; G.out = c->fetch.dev;
  hipLaunchKernelGGL(tr_gather_batch_kernel, dim3(TR_GATHER_BATCH_GX + 1, B), dim3(256), lds, c->stream, G);
  HIP_OK(hipGetLastError());
  if (hook) {
    // the tick's new plans: fitted on the device from the loop's result, written to the plane that is not in force and
    // behind the guesses in the same staging buffer (the shift left those there: idto_hip_mpc_batch_replan)
    MpcBatchState* m = hook->m;
    MpcStoreArgs S{};
    S.L = m->L; S.breaks = m->breaks; S.actuated = m->actuated_dev; S.q = c->q; S.q_stride = c->pstride; S.v = c->v; S.v_stride = c->pstride;
    S.tau = c->slab + 3 * (size_t)c->nv * c->nq; S.tau_stride = c->pstride; S.tau_row = (int)c->slab_stride;
    S.state = c->tr_state; S.state_stride = c->pstride; S.alt_off = (long long)c->alt_off;
    S.rows = c->tr_rows; S.iterations = rq.iterations; S.nrows = (int)L.nrows; S.times = m->tick_dev; S.times_stride = 1 + c->nq + c->nv;
    S.plan_old = m->plan[m->cur]; S.plan_new = m->plan[m->cur ^ 1]; S.work = m->work; S.out = c->fetch.dev + L.plans();
    hipLaunchKernelGGL(mpc_store_kernel, dim3((m->L.dims() + 63) / 64, B), dim3(64), 0, c->stream, S);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipMemcpyAsync(c->fetch.pin, c->fetch.dev, L.total() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  const size_t tick_w = (size_t)(1 + c->nq + c->nv);
  if (hook && hook->plant) {   // one more copy back, the plants' states, in front of the tick's one wait
    PlantState* pl = hook->plant;
    if (int erc = pl->tick_pin.Ensure((size_t)B * (tick_w + 1))) return erc;   // (+ two status ints a plant)
    HIP_OK(hipMemcpyAsync(pl->tick_pin, pl->state, (size_t)B * tick_w * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(pl->tick_pin + (size_t)B * tick_w, pl->status, (size_t)B * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  // (behind the copy: the fold only makes the context's first set the iterate's for the calls that follow)
  if (int rc = TrFoldSets(c)) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: tr_solve: waited for the device (every problem's state words, rows and solution back)");
  if (hook && hook->plant) MpcPlantsBack(c, *hook);
  const double* p = c->fetch.pin;
  const int best = *bfetch->best = (int)p[L.header()];
  for (int b = 0; b < B; ++b) { bfetch->final_cost[b] = p[L.final_cost() + b]; bfetch->status[b] = (int)p[L.status() + b]; }
  if (hook && hook->guess_out) std::memcpy(hook->guess_out, p + L.guess(), L.nguess * sizeof(double));
  if (hook && hook->plans_out) std::memcpy(hook->plans_out, p + L.plans(), L.nplans * sizeof(double));
  for (int b = 0; b < B; ++b) {
    if (rq.Delta_out) rq.Delta_out[b] = p[L.state(b) + TRS_DELTA];
    std::memcpy(rq.rows_host + (size_t)b * L.nrows, p + L.rows(b), L.nrows * sizeof(double));
  }
  if (!bfetch->only_best || best >= 0)
    for (size_t t = 0; t < L.slots; ++t)
      for (int i = 0; i < 5; ++i)
        if (bfetch->out[i]) std::memcpy(bfetch->out[i] + t * L.cnt[i], p + L.part(t, i), L.cnt[i] * sizeof(double));
  // every problem's outputs are filled; the return value: a time-out first, else whether any factorisation failed
  int failed = 0;
  for (int b = 0; b < B; ++b) {
    const int fs = TrFactorVerdict(c, rt.use_kkt, p[L.state(b) + TRS_FLAGS], b);
    if (fs == IDTO_HIP_SOLVER_TIMEOUT) return fs;
    if (fs || (bfetch->status[b] & TRF_FACTORIZATION)) failed = IDTO_HIP_FACTORIZATION_FAILED;
  }
  return failed;
}
// idto_hip_tr_solve_batch: the state words of every problem and the rows; the first problem that reports decides the return value
int TrFinishBatch(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt) {
  const int B = c->batch;
  if (int rc = TrFoldSets(c)) return rc;
  std::vector<double> st((size_t)B * TRS_COUNT);
  HIP_OK(hipMemcpy2DAsync(st.data(), TRS_COUNT * sizeof(double), c->tr_state, c->pstride, TRS_COUNT * sizeof(double), (size_t)B,
                          hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  HIP_OK(hipMemcpy(rq.rows_host, c->tr_rows, (size_t)B * TrRowDoubles(rq) * sizeof(double), hipMemcpyDeviceToHost));
  if (rq.Delta_out) for (int b = 0; b < B; ++b) rq.Delta_out[b] = st[(size_t)b * TRS_COUNT + TRS_DELTA];
  for (int b = 0; b < B; ++b)
    if (int fs = TrFactorVerdict(c, rt.use_kkt, st[(size_t)b * TRS_COUNT + TRS_FLAGS], b)) return fs;
  return 0;
}
// the end of both single-problem exits, c->tr_pin holding the state words
int TrFinishSingle(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt) {
  if (rq.Delta_out) *rq.Delta_out = c->tr_pin[TRS_DELTA];
  if (c->tr_pin[TRS_CUR] != 0.0) {   // the iterate's v, a, N+, slab, products ended up in the other set: it is "the" set now
    c->v = at_problem(c->v, (size_t)c->alt_off); c->a = at_problem(c->a, (size_t)c->alt_off); c->nplus = at_problem(c->nplus, (size_t)c->alt_off);
    c->slab = at_problem(c->slab, (size_t)c->alt_off); c->terms = at_problem(c->terms, (size_t)c->alt_off);
    c->alt_off = -c->alt_off;
  }
  return TrFactorVerdict(c, rt.use_kkt, c->tr_pin[TRS_FLAGS], -1);
}
// idto_hip_tr_solve_fetch: the state words, the rows and the solution with them: one gathering launch, one copy, the same wait
int TrFinishFetch(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt) {
  const TrFetchLayout L = TrFetchLayout::Make(1, TRS_COUNT, TrRowDoubles(rq), c->N, c->nq, c->nv, false, false);
  if (int rc = EnsureFetch(c, L.total())) return rc;
  TrGatherArgs G;
  G.state = c->tr_state; G.rows = c->tr_rows; G.alt_off = rt.lookahead ? (long long)c->alt_off : 0; G.L = L; G.out = c->fetch.dev;
  G.q = c->q; G.v = c->v; G.slab = c->slab; G.dq = c->tr_dq; G.w = c->tr_w; G.nq = c->nq; G.nv = c->nv; G.slab_stride = (int)c->slab_stride;
  hipLaunchKernelGGL(tr_gather_kernel, dim3(16), dim3(256), 0, c->stream, G);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(c->fetch.pin, c->fetch.dev, L.total() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  TRACE("hip: tr_solve: gather + one copy enqueued");
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: tr_solve: waited for the device (state words, rows and the solution back)");
  const double* p = c->fetch.pin;
  std::memcpy(c->tr_pin, p + L.state(0), TRS_COUNT * sizeof(double));
  std::memcpy(rq.rows_host, p + L.rows(0), L.nrows * sizeof(double));
  for (int i = 0; i < 5; ++i)
    if (rq.fetch[i]) std::memcpy(rq.fetch[i], p + L.part(0, i), L.cnt[i] * sizeof(double));
  return TrFinishSingle(c, rq, rt);
}
// idto_hip_tr_solve: the state words and the statistics rows with ONE wait (the rows through pinned staging of the context)
int TrFinishRows(idto_hip_ctx* c, const TrRequest& rq, const TrRoute& rt) {
  const size_t nrow = TrRowDoubles(rq);
  if (int rc = c->rows_pin.Ensure(nrow, 64 * TRR_COUNT)) return rc;
  HIP_OK(hipMemcpyAsync(c->tr_pin, c->tr_state, TRS_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(c->rows_pin, c->tr_rows, nrow * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: tr_solve: waited for the device (state words + rows back)");
  std::memcpy(rq.rows_host, c->rows_pin, nrow * sizeof(double));
  return TrFinishSingle(c, rq, rt);
}
// The device-resident trust-region loop: begin, per pass {multipliers, iterate, trial + decision, next step}, finish
int TrSolve(idto_hip_ctx* c, const TrRequest& rq) {
  HIP_OK(hipSetDevice(c->device));
  const int B = c->batch, nu = rq.nu, iterations = rq.iterations;
  TrRoute rt;
  int rc = TrPlanRoute(c, rq, &rt);
  if (!rc) rc = TrBegin(c, rq);
  if (rc) return rc;
  // g, H and the Newton step of the first iterate (with constraints the step comes out of the multiplier chain)
  rc = nu > 0 ? idto_hip_eval_partials(c) : idto_hip_gn_step(c);
  if (!rc && nu > 0) rc = idto_hip_grad_hess(c);
  if (rc) return rc;
  struct AltGuard { idto_hip_ctx* c; ~AltGuard() { c->alt_r.state = nullptr; c->alt_w.state = nullptr; } } alt_guard{c};
  if ((rc = TrPlanLaunches(c, rq, &rt)) != 0) return rc;
  // With the convergence criteria on, the loop is enqueued in chunks of TR_CHUNK iterations and the sticky flags are looked at in between:
  // once a criterion holds (or an iteration failed) the iterations that are left would run every kernel in full - none of fd, cost and the
  // solver reads the flags - only to decide nothing, and a solve that converges after 20 of max_iterations = 500 would take 25 times as
  // long as the loop it replaces (TO.cc:2600-2612 leaves the loop).  Rows of iterations that never ran are zeros.
  constexpr int TR_CHUNK = 8;
  if (rt.conv.on) HIP_OK(hipMemsetAsync(c->tr_rows, 0, (size_t)B * TrRowDoubles(rq) * sizeof(double), c->stream));
  TRACE("hip: tr_solve: loop state enqueued, constraint buffers ready");
  const int lds_iter = (int)sizeof(double) * (tr_rows_lds(c->nq) + TR_NSUM * (c->N + 1) + 3 + TR_NSUM + 3 * c->nq);
  bool kkt_built = false;
  for (int k = 0; k < rt.passes; ++k) {
    if (rt.conv.on && B == 1 && k > 0 && k % TR_CHUNK == 0) {
      HIP_OK(hipMemcpyAsync(c->tr_pin, c->tr_state, TRS_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIP_OK(hipStreamSynchronize(c->stream));
      if (c->tr_pin[TRS_FLAGS] != 0.0) break;
    }
    KktExtractArgs kkt_ex{};
    if (rt.use_kkt) rc = TrMultipliersKkt(c, rq, rt, k, &kkt_built, &kkt_ex);
    else if (nu > 0) rc = TrMultipliersSchur(c, rq);
    if (rc) return rc;
    const TrIterArgs T = TrIterArgsFor(c, rq, rt, k, (rt.use_kkt && c->kkt_fold) ? &kkt_ex : nullptr);
    // (the small models' launch below takes this kernel's part too - option "tr_fold" -: the whole iteration is one launch)
    const bool fold = rt.tr_small && rt.tr_fold_fits && c->tr_fold && k < iterations && T.nquat == 0 && T.rows.nu <= 4;
    if (!fold) hipLaunchKernelGGL(tr_iter_kernel, dim3(c->N + 2, B), dim3(256), lds_iter, c->stream, T);
    HIP_OK(hipGetLastError());
    if (k == iterations) break;   // (the check-only pass)
    const bool more = k + 1 < rt.passes;
    if ((rc = TrTrialAndNext(c, rq, rt, TrDecideArgsFor(c, rq), more, fold ? &T : nullptr, &kkt_built)) != 0) return rc;
    if (!more) break;
  }
  c->fd_full = false; c->partials_ahead = false;
  TRACE("hip: tr_solve: every iteration enqueued");
  if (B != 1) {   // (every problem has its own current set)
    if (c->alt_off <= 0) { g_err = "tr_solve: batch contexts keep their primary output set"; return -1; }
    return rq.bfetch ? TrFinishBatchFetch(c, rq, rt) : TrFinishBatch(c, rq, rt);
  }
  return rq.fetch ? TrFinishFetch(c, rq, rt) : TrFinishRows(c, rq, rt);
}
}  // namespace

int idto_hip_tr_solve(idto_hip_ctx* c, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                      double Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                      double* rows_host, double* Delta_out) {
  if (c->batch != 1) { g_err = "tr_solve serves single-problem contexts (batches: idto_hip_tr_solve_batch)"; return -1; }
  return TrSolve(c, TrRequest{iterations, scaling_method, scaling, normalize_quaternions, &Delta0, Delta_max, eta, constrained_dofs, nu, rows_host, Delta_out});
}

int idto_hip_tr_solve_fetch(idto_hip_ctx* c, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                            double Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                            double* rows_host, double* Delta_out, double* q_out, double* v_out, double* tau_out, double* dq_out,
                            double* w_out) {
  if (c->batch != 1) { g_err = "tr_solve_fetch serves single-problem contexts"; return -1; }
  double* const fetch[5] = {q_out, v_out, tau_out, dq_out, w_out};
  return TrSolve(c, TrRequest{iterations, scaling_method, scaling, normalize_quaternions, &Delta0, Delta_max, eta, constrained_dofs, nu, rows_host, Delta_out, fetch});
}

int idto_hip_tr_solve_batch(idto_hip_ctx* c, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                            const double* Delta0, double Delta_max, double eta, double* rows_host, double* Delta_out) {
  if (!Delta0 || !rows_host) { g_err = "tr_solve_batch: Delta0[batch] and rows_host[batch][iterations][IDTO_TR_ROW] are required"; return -1; }
  return TrSolve(c, TrRequest{iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta, nullptr, 0, rows_host, Delta_out});
}

// The options and the |h| column's degrees of freedom of a batch context, given to the single-problem context that advances one of its
// problems.  (at EVERY call, not only when the child is created - options set on the batch context afterwards, a solver
// stepped down after a time-out must reach the children, or "rows bit for bit those of idto_hip_tr_solve" breaks silently)
static int CopyOptionsToChild(const idto_hip_ctx* c, idto_hip_ctx* ch) {
#define X(name, kind, access, env, to_kkt, to_child) if (to_child) OptAssign(ch->name, OPT_INT, c->name);
  IDTO_OPTIONS(X)
#undef X
  return idto_hip_set_unactuated_dofs(ch, c->una_dofs_host.data(), c->una_nu);
}

// The trust-region loop with ENFORCED equality constraints for every problem of a batch context (BASELINE config 5:
// examples/allegro_hand/allegro_hand.yaml:95 `equality_constraints : true`; reference TO.cc:1267-1396, :2495-2625).
// The multiplier chain of an iteration - H^-1 [g | J^T] for n_eq + 1 right-hand sides, S = J H^-1 J^T, its dense
// factorisation, the step - is a sequence of single-problem launches with buffers of its own (constraints.h, dense_ldl.h,
// penta_apply.h), so the batch runs as one single-problem context per problem (created on first use from the host copies
// of the model and the problems), each advanced by idto_hip_tr_solve on a stream and a host thread of its own: the
// problems' launches overlap on the device, every problem's rows are bit for bit what idto_hip_tr_solve gives it alone,
// and the iterates are written back into the batch's arenas.
int idto_hip_tr_solve_batch_constrained(idto_hip_ctx* c, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                                        const double* Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                                        double* rows_host, double* Delta_out) {
  TrRequest rq{iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta, constrained_dofs, nu, rows_host, Delta_out};
  if (!Delta0 || !rows_host) { g_err = "tr_solve_batch_constrained: Delta0[batch] and rows_host[batch][iterations][IDTO_TR_ROW] are required"; return -1; }
  if (nu <= 0 || !constrained_dofs) { rq.constrained_dofs = nullptr; rq.nu = 0; }   // (idto_hip_tr_solve_batch)
  const int B = c->batch;
  if (B == 1 || rq.nu == 0) return TrSolve(c, rq);
  // the banded KKT step (kkt.h) is a sequence of launches with grid.y = problem like everything else of the loop: one
  // launch set per iteration for the whole batch.  The Schur-complement route (option con_kkt = 0, or nq + nu > 30) is
  // single-problem launches: a child context, stream and host thread per problem.
  if (TrKktRoute(c, nu)) {
    if (int rc = idto_hip_eval_tau(c)) return rc;   // (the loop starts from the cost of the resident q; the other route evaluates it per problem)
    return TrSolve(c, rq);
  }
  if (!c->host_model) { g_err = "tr_solve_batch_constrained: the context keeps no host copy of its model"; return -1; }
  if (c->model_records) {   // (a child context is built from the host copy of the ONE model)
    g_err = "tr_solve_batch_constrained: the child-context route of the constraints (option con_kkt 0, or nq + nu > 30) does "
            "not serve a batch with per-problem models (idto_hip_set_model_batch)";
    return -1;
  }
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->children.resize((size_t)B, nullptr);
  for (int b = 0; b < B; ++b) {
    idto_hip_ctx* ch = c->children[b];
    if (!ch) {
      const int rc = idto_hip_create(&c->host_model->m, &c->host_problems[b]->p, &c->host_contact, c->device, &ch);
      if (rc) return rc;
      c->children[b] = ch;
    }
    if (int rc = CopyOptionsToChild(c, ch)) return rc;
  }
  const size_t qbytes = (size_t)(c->N + 1) * c->nq * sizeof(double);
  std::vector<int> rcs((size_t)B, 0);
  std::vector<std::string> errs((size_t)B);
  auto work = [&](int b) {
    idto_hip_ctx* ch = c->children[b];
    auto fail = [&](int rc, const char* what) { rcs[b] = rc; errs[b] = g_err.empty() ? what : g_err; };
    if (hipSetDevice(c->device) != hipSuccess) return fail(-2, "hipSetDevice failed");
    ch->tr_conv_on = false;
    if (hipMemcpyAsync(ch->q, at_problem(c->q, (size_t)b * c->pstride), qbytes, hipMemcpyDeviceToDevice, ch->stream) != hipSuccess)
      return fail(-2, "copy of the problem's q failed");
    ch->fd_full = false; ch->partials_ahead = false; ch->con_ready = false; ch->con_begun = false; ch->trial_resident = false;
    int rc = idto_hip_eval_tau(ch);
    if (rc) return fail(rc, "eval_tau failed");
    TrRequest one = rq;   // problem b's radius, rows and radius out
    one.Delta0s = Delta0 + b; one.rows_host = rows_host + (size_t)b * iterations * TRR_COUNT; one.Delta_out = Delta_out ? Delta_out + b : nullptr;
    rc = TrSolve(ch, one);
    if (rc) return fail(rc, "tr_solve failed");
    if (hipMemcpyAsync(at_problem(c->q, (size_t)b * c->pstride), ch->q, qbytes, hipMemcpyDeviceToDevice, ch->stream) != hipSuccess ||
        hipStreamSynchronize(ch->stream) != hipSuccess)
      return fail(-2, "copy of the iterate failed");
  };
  std::vector<std::thread> threads;
  for (int b = 1; b < B; ++b) threads.emplace_back(work, b);
  work(0);
  for (auto& t : threads) t.join();
  c->fd_full = false; c->partials_ahead = false; c->trial_resident = false; c->con_ready = false; c->con_begun = false;   // q of every problem moved
  for (int b = 0; b < B; ++b)
    if (rcs[b]) { g_err = "problem " + std::to_string(b) + ": " + errs[b]; return rcs[b]; }
  return 0;
}

// ---- B model-predictive controllers on a batch context (mpc_batch.h)
static int MpcReady(idto_hip_ctx* c, const char* who) {
  if (!c->mpc) { g_err = std::string(who) + ": call idto_hip_mpc_batch_begin on the context first"; return -1; }
  for (idto_hip_ctx* ch : c->children)
    if (ch) {
      g_err = std::string(who) + ": this context has child contexts (the child-context route of idto_hip_tr_solve_batch_constrained "
              "made them), which the shift on the device would leave with the old initial conditions and nominal trajectories";
      return -1;
    }
  return 0;
}

int idto_hip_mpc_batch_begin(idto_hip_ctx* c, const int* selector, const int* actuated_dofs, int nu) {
  if (!selector || !actuated_dofs || nu < 1 || nu > c->nv) { g_err = "mpc_batch_begin: selector[nq] and 1 <= nu <= nv actuated_dofs are required"; return -1; }
  for (int j = 0; j < nu; ++j)
    if (actuated_dofs[j] < 0 || actuated_dofs[j] >= c->nv) { g_err = "mpc_batch_begin: an actuated dof outside [0, nv)"; return -1; }
  if (c->N < 1) { g_err = "mpc_batch_begin: a plan needs at least two knots"; return -1; }
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->mpc.reset();
  auto m = std::make_unique<MpcBatchState>(c);   // (a failure below returns what it has made: the context is left without MPC storage)
  const size_t B = (size_t)c->batch;
  const int n = c->N + 1;
  m->L = MpcPlanLayout{n, c->nq, c->nv, nu};
  m->selector.resize((size_t)c->nq);
  for (int i = 0; i < c->nq; ++i) m->selector[(size_t)i] = selector[i] ? 1 : 0;
  std::vector<double> breaks((size_t)n);
  for (int i = 0; i < n; ++i) breaks[(size_t)i] = i * c->dt;   // StoreOptimizerSolution: time_steps[i] = i * time_step
  const size_t nqa = (size_t)n * c->nq, nva = (size_t)n * c->nv, nta = (size_t)c->N * c->nv, len = m->L.len();
  const size_t tick = B * (size_t)(1 + c->nq + c->nv);
  m->io_count = std::max(std::max(B * (nqa + nva + nta + 1), B * len), 2 * B * nqa);
  if (Upload(c, breaks.data(), breaks.size(), &m->breaks) || Upload(c, m->selector.data(), m->selector.size(), &m->selector_dev) ||
      Upload(c, actuated_dofs, (size_t)nu, &m->actuated_dev) || Alloc(c, B * len, &m->plan[0]) || Alloc(c, B * len, &m->plan[1]) ||
      Alloc(c, B * (size_t)n * m->L.dims(), &m->work) || Alloc(c, tick, &m->tick_dev) || Alloc(c, m->io_count, &m->io_dev))
    return -2;
  if (int rc = m->tick_pin.Ensure(tick)) return rc;
  if (int rc = m->io_pin.Ensure(m->io_count)) return rc;
  c->mpc = std::move(m);
  ++c->mpc_generation;
  return 0;
}

int idto_hip_mpc_batch_store(idto_hip_ctx* c, const double* q, const double* v, const double* tau, const double* start_times,
                             double* plans_out) {
  if (int rc = MpcReady(c, "mpc_batch_store")) return rc;
  if (!q || !v || !tau || !start_times) { g_err = "mpc_batch_store: q, v, tau and start_times are required"; return -1; }
  HIP_OK(hipSetDevice(c->device));
  MpcBatchState* m = c->mpc.get();
  const size_t B = (size_t)c->batch, len = m->L.len();
  const size_t nqa = (size_t)m->L.n * c->nq, nva = (size_t)m->L.n * c->nv, nta = (size_t)c->N * c->nv;
  double* in = m->io_pin;
  std::memcpy(in, q, B * nqa * sizeof(double));
  std::memcpy(in + B * nqa, v, B * nva * sizeof(double));
  std::memcpy(in + B * (nqa + nva), tau, B * nta * sizeof(double));
  std::memcpy(in + B * (nqa + nva + nta), start_times, B * sizeof(double));
  const size_t count = B * (nqa + nva + nta + 1);
  HIP_OK(hipMemcpyAsync(m->io_dev, in, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  MpcStoreArgs S{};
  S.L = m->L; S.breaks = m->breaks; S.actuated = m->actuated_dev;
  S.q = m->io_dev; S.q_stride = nqa * sizeof(double);
  S.v = m->io_dev + B * nqa; S.v_stride = nva * sizeof(double);
  S.tau = m->io_dev + B * (nqa + nva); S.tau_stride = nta * sizeof(double); S.tau_row = c->nv;
  S.state = nullptr; S.state_stride = 0; S.alt_off = 0;
  S.rows = nullptr; S.iterations = 0; S.nrows = 0;
  S.times = m->io_dev + B * (nqa + nva + nta); S.times_stride = 1;
  S.plan_old = m->plan[m->cur]; S.plan_new = m->plan[m->cur]; S.work = m->work;
  S.out = nullptr;
  hipLaunchKernelGGL(mpc_store_kernel, dim3((m->L.dims() + 63) / 64, (unsigned)B), dim3(64), 0, c->stream, S);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(m->io_pin, m->plan[m->cur], B * len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (plans_out) std::memcpy(plans_out, m->io_pin, B * len * sizeof(double));
  return 0;
}

// the copy of times and x0 and the shift, enqueued; guess_dev: [B][(N+1) nq] on the device, or null
static int MpcShiftEnqueue(idto_hip_ctx* c, const double* times, const double* x0, double* guess_dev) {
  MpcBatchState* m = c->mpc.get();
  const int B = c->batch, nq = c->nq, nv = c->nv, n = m->L.n;
  // as idto_hip_set_q_batch + idto_hip_set_problem_batch leave the context
  c->trial_resident = false; c->spec_pending = false; c->spec_ready = false;
  DropPrefetch(c, {IDTO_ARR_Q});
  c->fd_full = false; c->partials_ahead = false;
  c->con_ready = false; c->con_begun = false;
  const size_t w = (size_t)(1 + nq + nv);
  if (times) {   // (null: the plants' kernel, enqueued in front, writes the tick buffer - idto_hip_mpc_batch_tick_plants)
    for (int b = 0; b < B; ++b) {
      double* t = m->tick_pin + (size_t)b * w;
      t[0] = times[b];
      std::memcpy(t + 1, x0 + (size_t)b * (nq + nv), (size_t)(nq + nv) * sizeof(double));
    }
    HIP_OK(hipMemcpyAsync(m->tick_dev, m->tick_pin, (size_t)B * w * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  MpcShiftArgs A{};
  A.L = m->L; A.breaks = m->breaks; A.selector = m->selector_dev; A.time_step = c->dt;
  A.plan = m->plan[m->cur]; A.tick = m->tick_dev;
  A.q = c->q; A.v_init = c->d_vinit; A.q_nom = c->d_qnom; A.pstride = c->pstride;
  A.guess_out = guess_dev;
  hipLaunchKernelGGL(mpc_shift_kernel, dim3(1, B), dim3(256), (size_t)nq * sizeof(double), c->stream, A);
  HIP_OK(hipGetLastError());
  // the host copies of the problems (what a child context would be made from) follow: the same arithmetic, mpc_spline.h
  // (a tick from the plants: behind the wait, when their states are on the host - MpcHostProblemsFollow)
  for (int b = 0; times && b < B && b < (int)c->host_problems.size(); ++b) {
    HostProblemCopy& hp = *c->host_problems[(size_t)b];
    const double* q0 = x0 + (size_t)b * (nq + nv);
    const std::vector<double> old0(hp.q_nom.begin(), hp.q_nom.begin() + nq);
    for (int t = 0; t < n; ++t)
      for (int i = 0; i < nq; ++i)
        hp.q_nom[(size_t)t * nq + i] = idto_spline::nominal_shift(hp.q_nom[(size_t)t * nq + i], m->selector[(size_t)i] != 0, q0[i], old0[(size_t)i]);
    std::copy(q0, q0 + nq, hp.q_init.begin());
    std::copy(q0 + nq, q0 + nq + nv, hp.v_init.begin());
  }
  TRACE("hip: mpc_batch: tick inputs and the shift enqueued");
  return 0;
}

int idto_hip_mpc_batch_shift(idto_hip_ctx* c, const double* times, const double* x0, double* guess_out, double* q_nom_out) {
  if (int rc = MpcReady(c, "mpc_batch_shift")) return rc;
  if (!times || !x0) { g_err = "mpc_batch_shift: times[batch] and x0[batch][nq + nv] are required"; return -1; }
  HIP_OK(hipSetDevice(c->device));
  MpcBatchState* m = c->mpc.get();
  const size_t B = (size_t)c->batch, nqa = (size_t)m->L.n * c->nq;
  int rc = MpcShiftEnqueue(c, times, x0, m->io_dev);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  HIP_OK(hipMemcpyAsync(m->io_pin, m->io_dev, B * nqa * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpy2DAsync(m->io_pin + B * nqa, nqa * sizeof(double), c->d_qnom, c->pstride, nqa * sizeof(double), B,
                          hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (guess_out) std::memcpy(guess_out, m->io_pin, B * nqa * sizeof(double));
  if (q_nom_out) std::memcpy(q_nom_out, m->io_pin + B * nqa, B * nqa * sizeof(double));
  return 0;
}

// The inside of idto_hip_tr_solve_batch_fetch for a batch of more than one problem (rq.bfetch); with its mpc a controllers'
// tick (idto_hip_mpc_batch_replan): the shift and idto_hip_eval_tau in front of the loop, the store behind it.
static int TrSolveBatchFetch(idto_hip_ctx* c, const TrRequest& rq) {
  const TrBatchFetch* bf = rq.bfetch;
  if (rq.nu > 0 && !TrKktRoute(c, rq.nu)) {
    g_err = "tr_solve_batch_fetch: these enforced constraints take the child-context route of idto_hip_tr_solve_batch_constrained "
            "(option con_kkt = 0, nq + nu > 30 or dense cost weights: every problem advanced in a single-problem context of "
            "its own), which has no gathered fetch: use idto_hip_tr_solve_batch_constrained + idto_hip_get_batch";
    return -1;
  }
  HIP_OK(hipSetDevice(c->device));
  int rc = 0;
  if (bf->mpc) {
    // (the guesses go where the one copy back finds them: behind the fetch's own doubles)
    const TrFetchLayout L = BatchFetchLayout(c, rq);
    if ((rc = EnsureFetch(c, L.total())) != 0) return rc;
    rc = MpcShiftEnqueue(c, bf->mpc->times, bf->mpc->x0, c->fetch.dev + L.guess());
  }
  if (!rc && (rq.nu > 0 || bf->mpc))
    rc = idto_hip_eval_tau(c);   // (as idto_hip_tr_solve_batch_constrained: the loop starts from the cost of the resident q)
  if (!rc) rc = TrSolve(c, rq);
  // (a return from inside the loop's enqueueing: the initial state words travel from pinned memory of the context, which the
  // next call rewrites - wait for what is enqueued)
  if (rc < 0) (void)hipStreamSynchronize(c->stream);
  return rc;
}

// A tick's arguments and outputs behind its source of [time, q0, v0]: idto_hip_mpc_batch_replan's, which
// idto_hip_mpc_batch_tick_plants shares
struct MpcReplanArgs {
  int iterations, scaling_method, scaling, normalize_quaternions; const double* Delta0; double Delta_max, eta;
  const int* constrained_dofs; int nu; double* rows_host; double* Delta_out; double *q_out, *v_out, *tau_out, *final_cost;
  int *status, *best; double *guess_out, *plans_out;
};
static TrRequest MpcReplanRequest(const MpcReplanArgs& a) {
  return TrRequest{a.iterations, a.scaling_method, a.scaling, a.normalize_quaternions, a.Delta0, a.Delta_max, a.eta, a.constrained_dofs, a.nu, a.rows_host, a.Delta_out};
}
// what a tick refuses, before any device work (from_plants: times and x0 are not arguments)
static int MpcReplanCheck(idto_hip_ctx* c, const char* who, const MpcReplanArgs& a, bool from_plants, bool tick_missing) {
  if (int rc = MpcReady(c, who)) return rc;
  const bool missing = tick_missing || !a.Delta0 || !a.rows_host || !a.final_cost || !a.status || !a.best;
  const char* need = from_plants ? "Delta0[batch], rows_host[batch][iterations][IDTO_TR_ROW], final_cost[batch], status[batch] and best"
                                 : "times[batch], x0[batch][nq + nv], Delta0[batch], rows_host[batch][iterations][IDTO_TR_ROW], "
                                   "final_cost[batch], status[batch] and best";
  if (int rc = TrCheckArgs(who, MpcReplanRequest(a), missing ? need : nullptr)) return rc;
  if (c->batch < 2) { g_err = std::string(who) + ": serves batches of more than one problem (one controller: idto_hip_tr_solve_fetch)"; return -1; }
  return 0;
}
// the tick itself: the shift from times / x0 (null: from the tick buffer that the plants' kernel wrote), the loop, the store,
// the copies back, the one wait
static int MpcReplanRun(idto_hip_ctx* c, const double* times, const double* x0, const MpcReplanArgs& a, PlantState* plant, double* x_after_out,
                        int* plant_status_out) {
  TrRequest rq = MpcReplanRequest(a);
  MpcBatchState* m = c->mpc.get();
  MpcTickHook hook{m, times, x0, a.guess_out, a.plans_out, (size_t)c->batch * m->L.n * c->nq, (size_t)c->batch * m->L.len()};
  hook.plant = plant; hook.x_after_out = x_after_out; hook.plant_status_out = plant_status_out;
  TrBatchFetch bf{0, {a.q_out, a.v_out, a.tau_out, nullptr, nullptr}, a.final_cost, a.status, a.best, &hook}; rq.bfetch = &bf;
  const int rc = TrSolveBatchFetch(c, rq);
  if (plant && !hook.followed) {
    // the loop returned before its gather (an error, a time-out): the plants have advanced and the device has been shifted all
    // the same - fetch the plants' states and status now, so that the caller and the host copies of the problems have them
    const size_t w = (size_t)(1 + c->nq + c->nv), B = (size_t)c->batch;
    if (plant->tick_pin.Ensure(B * (w + 1)) == 0 && hipStreamSynchronize(c->stream) == hipSuccess &&
        hipMemcpy(plant->tick_pin, plant->state, B * w * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(plant->tick_pin + B * w, plant->status, B * 2 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
      const std::string err = g_err;
      MpcPlantsBack(c, hook);
      g_err = err;
    }
  }
  // the plane the store wrote is in force once the tick counted; a loop that timed out, or a call that failed, leaves every plan
  if (rc == 0 || rc == IDTO_HIP_FACTORIZATION_FAILED) m->cur ^= 1;
  return rc;
}

int idto_hip_mpc_batch_replan(idto_hip_ctx* c, const double* times, const double* x0, int iterations, int scaling_method,
                              int scaling, int normalize_quaternions, const double* Delta0, double Delta_max, double eta,
                              const int* constrained_dofs, int nu, double* rows_host, double* Delta_out, double* q_out,
                              double* v_out, double* tau_out, double* final_cost, int* status, int* best, double* guess_out,
                              double* plans_out) {
  const MpcReplanArgs a{iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta, constrained_dofs, nu, rows_host,
                        Delta_out, q_out, v_out, tau_out, final_cost, status, best, guess_out, plans_out};
  if (int rc = MpcReplanCheck(c, "mpc_batch_replan", a, false, !times || !x0)) return rc;
  return MpcReplanRun(c, times, x0, a, nullptr, nullptr, nullptr);
}

// ---- the plant family's entries (plant_abi.inc, scene_abi.inc, lin_abi.inc, track_abi.inc): what they refuse, the sizes of
// their launches and where a call's arrays lie are host/plant_calls.h's answers about a PlantShape; here is what acts on them
using idto_host::CallPlan;
static idto_host::PlantShape PlantShapeOf(const idto_hip_ctx* c) {
  idto_host::PlantShape s{};
  s.batch = c->batch; s.nq = c->nq; s.nv = c->nv; s.nb = c->M.nb; s.npairs = c->M.npairs; s.ngeoms = c->M.ngeoms; s.blob_n = c->M.blob_n;
  s.nxb = c->M.nxb; s.nstem = c->M.nstem; s.npaths = c->npaths; s.maxc = c->maxc;
  for (const idto_hip_ctx* ch : c->children) s.children |= ch != nullptr;
  s.model_records = c->model_records != nullptr; s.host_model = c->host_tables && c->host_model;
  if (c->mpc) { s.mpc = true; s.mpc_nu = c->mpc->L.nu; s.mpc_n = c->mpc->L.n; s.mpc_len = c->mpc->L.len(); }
  if (const PlantState* p = c->plant.get(); p && p->begun) {
    s.plants_begun = true; s.plant_mode = p->mode; s.plant_nu = p->nu; s.plant_block = p->block; s.plant_lds = p->lds;
    s.plant_record_capacity = p->record_capacity; s.plant_mpc_current = c->mpc_generation == p->mpc_generation;
  }
  return s;
}
// a refusal becomes the entry's message and return code (the message is built only then)
static int Refused(idto_host::Refusal r) {
  if (r.rc) g_err = std::move(r.msg);
  return r.rc;
}
// rec: a parameter record on the host; its DevModel becomes Mb with the tables moved to the record's device copy at `dev`
static void RecordForDevice(const idto_hip_ctx* c, DevModel Mb, const double* dev, double* rec) {
  shift_model(Mb, dev);
  std::memcpy(rec + model_record_devmodel_at((size_t)c->M.blob_n), &Mb, sizeof(DevModel));
}
// Which parameter records a launch reads: the plants' where `models` asks for them, else the context's per-problem records,
// else `own` - the context's own record, or null for a kernel that has the context's model among its arguments.
// b >= 0: problem b's record for every workgroup of the launch (stride 0).
extern "C++" template <class Args>   // (PlantArgs, SceneArgs)
static void SelectRecords(const idto_hip_ctx* c, int models, const double* own, long b, Args* A) {
  const bool plants = models == IDTO_SCENE_MODELS_PLANTS;
  const double* records = plants ? c->plant->records : c->model_records;
  const size_t stride = plants ? c->plant->mstride : c->mstride;
  if (!records) { A->records = own; A->mstride = 0; }
  else if (b >= 0) { A->records = at_problem(records, (size_t)b * stride); A->mstride = 0; }
  else { A->records = records; A->mstride = stride; }
  A->rec_contact = model_record_contact_at((size_t)c->M.blob_n) * sizeof(double);
  A->rec_model = model_record_devmodel_at((size_t)c->M.blob_n) * sizeof(double);
}
// A call's arrays against its plan, in buffer b and its mirror.  PlanStage: an input into the mirror at its device offset;
// PlanUpload: all of them in one copy; PlanFetch: entry e back to its place in the mirror if it was asked for (from: the entry
// that holds it on the device, where e is in the mirror alone); PlanCopyOut, behind the wait: from the mirror to the caller.
static void PlanStage(const CallPlan& p, const GrownBuffer& b, int e, const void* src, size_t bytes) { std::memcpy(b.pin + p.at(e), src, bytes); }
static void PlanStage(const CallPlan& p, const GrownBuffer& b, int e, const double* src) { PlanStage(p, b, e, src, p.count(e) * sizeof(double)); }
static int PlanUpload(idto_hip_ctx* c, const CallPlan& p, const GrownBuffer& b) {
  HIP_OK(hipMemcpyAsync(b.dev, b.pin, p.in_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return 0;
}
static int PlanFetch(idto_hip_ctx* c, const CallPlan& p, const GrownBuffer& b, int e, const void* wanted, int from = -1) {
  if (!wanted || !p.count(e)) return 0;
  HIP_OK(hipMemcpyAsync(b.pin + p.Mirror(e), b.dev + p.at(from < 0 ? e : from), p.count(e) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
static void PlanCopyOut(const CallPlan& p, const GrownBuffer& b, int e, void* out, size_t bytes) { if (out) std::memcpy(out, b.pin + p.Mirror(e), bytes); }
static void PlanCopyOut(const CallPlan& p, const GrownBuffer& b, int e, double* out) { PlanCopyOut(p, b, e, out, p.count(e) * sizeof(double)); }

#include "plant_abi.inc"   // idto_hip_forward_dynamics, idto_hip_plant_*
#include "scene_abi.inc"   // idto_hip_scene_sizes, idto_hip_scene_report
#include "lin_abi.inc"     // idto_hip_lin_sizes, idto_hip_plant_linearize, idto_hip_plant_tvlqr
#include "track_abi.inc"   // idto_hip_plant_track, idto_hip_plant_tvlqr_track

// The batch loop with everything a caller reads afterwards brought back under the loop's one wait, and the best problem
// chosen on the device (trust_region.h tr_gather_batch_kernel).
int idto_hip_tr_solve_batch_fetch(idto_hip_ctx* c, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                                  const double* Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                                  double* rows_host, double* Delta_out, int only_best, double* q_out, double* v_out,
                                  double* tau_out, double* dq_out, double* w_out, double* final_cost, int* status, int* best) {
  TrRequest rq{iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta, constrained_dofs, nu, rows_host, Delta_out};
  const bool missing = !Delta0 || !rows_host || !final_cost || !status || !best;
  if (int rc = TrCheckArgs("tr_solve_batch_fetch", rq, missing ? "Delta0[batch], rows_host[batch][iterations][IDTO_TR_ROW], final_cost[batch], status[batch] and best" : nullptr))
    return rc;
  if (c->batch == 1) {
    // one problem: idto_hip_tr_solve_fetch, and the choice among one made here from what it returned
    double* const fetch[5] = {q_out, v_out, tau_out, dq_out, w_out}; rq.fetch = fetch;
    const int rc = TrSolve(c, rq);
    if (rc < 0 || rc == IDTO_HIP_SOLVER_TIMEOUT) return rc;
    int f = 0;
    for (int k = 0; k < iterations; ++k) f |= (int)rows_host[(size_t)k * TRR_COUNT + TRR_FLAGS];
    final_cost[0] = c->tr_pin[TRS_COST];
    status[0] = f;
    *best = ((f & TR_ELIGIBLE_MASK) == 0 && std::isfinite(final_cost[0])) ? 0 : -1;
    return rc;
  }
  TrBatchFetch bf{only_best ? 1 : 0, {q_out, v_out, tau_out, dq_out, w_out}, final_cost, status, best}; rq.bfetch = &bf;
  return TrSolveBatchFetch(c, rq);
}

#define NCCL_OK(expr)                                                                 \
  do {                                                                                \
    ncclResult_t r_ = (expr);                                                         \
    if (r_ != ncclSuccess) {                                                          \
      g_err = std::string(#expr) + ": " + R->GetErrorString(r_);                      \
      return -4;                                                                      \
    }                                                                                 \
  } while (0)

// the RCCL that got loaded must have the major version of the headers this library was compiled with
static int CommVersionOk() {
  RCCL_OR_FAIL(R);
  int v = 0;
  NCCL_OK(R->GetVersion(&v));
  const int major_rt = v / 10000, major_ct = NCCL_VERSION_CODE / 10000;
  if (major_rt != major_ct) {
    g_err = "librccl version mismatch: compiled against " + std::to_string(NCCL_VERSION_CODE) + ", loaded " + std::to_string(v);
    return -1;
  }
  return 0;
}
static int CommAttach(idto_hip_ctx* c, ncclComm_t comm, int rank, int world) {
  if (c->batch != 1) { g_err = "the sharded iteration serves single-problem contexts"; return -1; }
  if (world < 1 || world > IDTO_SLAB_PAD || rank < 0 || rank >= world) { g_err = "bad rank / world size"; return -1; }
  c->comm = comm; c->comm_rank = rank; c->comm_world = world;
  c->comm_per = (c->N + world - 1) / world;
  const int lo = std::min(c->N, rank * c->comm_per);
  return idto_hip_set_shard(c, lo, std::min(c->N, lo + c->comm_per));
}

int idto_hip_comm_unique_id(char* id_out, int bytes) {
  if (int rc = CommVersionOk()) return rc;
  if (!id_out || bytes < (int)sizeof(ncclUniqueId)) { g_err = "comm_unique_id: buffer of at least 128 bytes required"; return -1; }
  RCCL_OR_FAIL(R);
  ncclUniqueId id;
  NCCL_OK(R->GetUniqueId(&id));
  std::memcpy(id_out, &id, sizeof id);
  return 0;
}

int idto_hip_comm_init(idto_hip_ctx* c, const char* unique_id, int rank, int world) {
  HIP_OK(hipSetDevice(c->device));
  if (c->comm) { g_err = "comm_init: the context already belongs to a communicator"; return -1; }
  if (int rc = CommVersionOk()) return rc;
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof id);
  ncclComm_t comm = nullptr;
  RCCL_OR_FAIL(R);
  NCCL_OK(R->CommInitRank(&comm, world, id, rank));
  return CommAttach(c, comm, rank, world);
}

int idto_hip_comm_init_all(idto_hip_ctx** ctxs, int n) {
  if (!ctxs || n < 1 || n > IDTO_SLAB_PAD) { g_err = "comm_init_all: bad arguments"; return -1; }
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) {
    if (ctxs[i]->comm) { g_err = "comm_init_all: a context already belongs to a communicator"; return -1; }
    devs[i] = ctxs[i]->device;
  }
  if (int rc = CommVersionOk()) return rc;
  std::vector<ncclComm_t> comms(n, nullptr);
  RCCL_OR_FAIL(R);
  NCCL_OK(R->CommInitAll(comms.data(), n, devs.data()));
  for (int i = 0; i < n; ++i)
    if (int rc = CommAttach(ctxs[i], comms[i], i, n)) return rc;
  return 0;
}

int idto_hip_comm_destroy(idto_hip_ctx* c) {
  if (c->comm) {
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    RCCL_OR_FAIL(R);
    NCCL_OK(R->CommDestroy(c->comm));
    c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1;
    return idto_hip_set_shard(c, 0, c->N);
  }
  return 0;
}

// in place: rank r's records start at r * per * stride of the receive buffer, which is where its
// fd_kernel wrote them
static int AllGatherSlab(idto_hip_ctx* c) {
  const size_t count = (size_t)c->comm_per * c->slab_stride;
  RCCL_OR_FAIL(R);
  NCCL_OK(R->AllGather(c->slab + (size_t)c->comm_rank * count, c->slab, count, ncclDouble, c->comm, c->stream));
  return 0;
}

int idto_hip_allgather_slab(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  if (!c->comm) { g_err = "allgather_slab: call idto_hip_comm_init first"; return -1; }
  DropPrefetch(c, {IDTO_ARR_SLAB});
  return AllGatherSlab(c);
}

int idto_hip_gn_step_sharded(idto_hip_ctx* c) {
  if (!c->comm) { g_err = "gn_step_sharded: call idto_hip_comm_init first"; return -1; }
  int rc = idto_hip_eval_partials(c);   // this rank's k-range
  if (rc) return rc;
  rc = idto_hip_allgather_slab(c);      // RCCL, on the context's stream
  if (rc) return rc;
  rc = idto_hip_grad_hess(c);           // every rank assembles and solves redundantly: identical bits, no second collective
  if (rc) return rc;
  return idto_hip_factor_solve(c, nullptr, 1, nullptr);
}

int idto_hip_eval_partials_multi(idto_hip_ctx** ctxs, int n) {
  // one process driving n devices (communicator from idto_hip_comm_init_all): every device's
  // finite-difference kernel covers its k-range, the all-gathers of all ranks go into one group
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]->comm) { g_err = "eval_partials_multi: call idto_hip_comm_init_all first"; return -1; }
    if (int rc = idto_hip_eval_partials(ctxs[i])) return rc;
  }
  RCCL_OR_FAIL(R);
  NCCL_OK(R->GroupStart());
  for (int i = 0; i < n; ++i) {
    HIP_OK(hipSetDevice(ctxs[i]->device));
    DropPrefetch(ctxs[i], {IDTO_ARR_SLAB});
    if (int rc = AllGatherSlab(ctxs[i])) { (void)R->GroupEnd(); return rc; }
  }
  NCCL_OK(R->GroupEnd());
  return 0;
}

int idto_hip_gn_step_multi(idto_hip_ctx** ctxs, int n) {
  if (int rc = idto_hip_eval_partials_multi(ctxs, n)) return rc;
  for (int i = 0; i < n; ++i) {
    if (int rc = idto_hip_grad_hess(ctxs[i])) return rc;
    if (int rc = idto_hip_factor_solve(ctxs[i], nullptr, 1, nullptr)) return rc;
  }
  return 0;
}

// Which RCCL the process resolved (RcclState: a copy the process had mapped already - torch's bundled one when torch was
// imported first - else the loader's).  Any is fine as long as the major version is the one of the headers this library
// was compiled against: checked where a communicator is created (CommVersionOk), reported here for the bench line.
int idto_hip_rccl_info(char* path_out, int path_cap, int* version_out) {
  RCCL_OR_FAIL(R);
  int v = 0;
  NCCL_OK(R->GetVersion(&v));
  if (version_out) *version_out = v;
  if (path_out && path_cap > 0) std::snprintf(path_out, (size_t)path_cap, "%s", R->path.c_str());
  return 0;
}

int idto_hip_get_option(idto_hip_ctx* c, const char* name, int* value) {
  // the computed ones, read-only
  if (std::strcmp(name, "rccl_version") == 0) { return idto_hip_rccl_info(nullptr, 0, value); }
  if (std::strcmp(name, "kkt_last_solver") == 0) { *value = c->kkt ? c->kkt->last_solver : 0; return 0; }
  if (std::strcmp(name, "fast_shape") == 0) { *value = c->M.fast_shape; return 0; }   // id_fast.h: 0 none, 1 acrobot, 2 hopper, 3 mini_cheetah, 4 allegro_hand, 5 spinner, 6 free object + one 7-body arm
  if (std::strcmp(name, "model_batch") == 0) { *value = c->model_records ? 1 : 0; return 0; }   // idto_hip_set_model_batch has switched the context to per-problem records
#define X(nm, kind, access, env, to_kkt, to_child) if (((access) & OPT_GET) && std::strcmp(name, #nm) == 0) { *value = c->nm; return 0; }
  IDTO_OPTIONS(X)
#undef X
  g_err = std::string("unknown option ") + name;
  return -1;
}

int idto_hip_set_option(idto_hip_ctx* c, const char* name, int value) {
  // (2: the stamps of the KKT context's solver - the constrained step's banded solve - are what IDTO_ARR_DEBUG returns)
  if (std::strcmp(name, "solver_debug") == 0) { c->solver_debug = value == 1; c->kkt_debug = value == 2; if (c->kkt) c->kkt->solver_debug = c->kkt_debug; return 0; }
  // (below 16 block rows nd_split leaves a joiner chains of three rows with one row of their own: untested, not offered)
  if (std::strcmp(name, "nd_min_rows") == 0) value = std::max(16, value);
  if (std::strcmp(name, "ls_waves") == 0 && (value < 0 || value > IDTO_LS_MAX_CANDIDATES)) { g_err = "ls_waves: 0 (planned) .. IDTO_LS_MAX_CANDIDATES candidates per wave"; return -1; }
  if (std::strcmp(name, "gradients_method") == 0 && (value < 0 || value > 2)) { g_err = "gradients_method: 0 forward, 1 central, 2 central4 (autodiff needs Drake)"; return -1; }
  if (std::strcmp(name, "asm_fold") == 0) c->terms_valid = false;
#define X(nm, kind, access, env, to_kkt, to_child)             \
  if (((access) & OPT_SET) && std::strcmp(name, #nm) == 0) {     \
    OptAssign(c->nm, kind, value);                             \
    if (to_kkt && c->kkt) OptAssign(c->kkt->nm, OPT_INT, c->nm); \
    return 0;                                                  \
  }
  IDTO_OPTIONS(X)
#undef X
  g_err = std::string("unknown option ") + name;
  return -1;
}

// Can idto_hip_gn_step's solve carry the assembly (the conditions of LaunchAssemble's products path; *p: the plan of
// that solve, made for the bands as they will be once they count as assembled)?  p->can_decide: ... and the decision on
// the trust-region loop's trial point
static bool AsmInSolver(const idto_hip_ctx* c, SolverPlan* p) {
  if (!(c->asm_in_solver && c->solver_pipe && !c->reference_solver)) return false;
  if (!(c->weights_diagonal && c->terms_valid && c->fd_full && c->asm_stop == 0)) return false;
  return Plan(c, true, SolveRequest{}, p) == 0 && p->can_assemble;
}

int idto_hip_gn_step(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  if (c->spec_ready) return 0;   // already enqueued for this q by idto_hip_tr_trial (speculation)
  c->spec_pending = false;
  SolverPlan p;
  if (FusedEligible(c)) return LaunchFused(c);
  if (SmallEligible(c, &p)) return LaunchSmall(c, p);
  int rc = idto_hip_eval_partials(c);
  if (rc) return rc;
  if (AsmInSolver(c, &p)) {
    // two launches: the pipelined solver's grid carries the assembly (LaunchNd).  LaunchAssemble's bookkeeping:
    DropPrefetch(c, {IDTO_ARR_GRADIENT, IDTO_ARR_H_A, IDTO_ARR_H_B, IDTO_ARR_H_C, IDTO_ARR_HBANDS});
    if (!c->h_assembled) {
      HIP_OK(hipMemset2DAsync(c->step, c->pstride, 0, (size_t)c->nq * sizeof(double), (size_t)c->batch, c->stream));
      c->h_assembled = true;
    }
    c->con_ready = false; c->con_begun = false;
    SolverExtras ex;
    ex.assemble = true;
    return FactorSolve(c, nullptr, 1, nullptr, nullptr, &p, ex);
  }
  rc = idto_hip_grad_hess(c);
  if (rc) return rc;
  return idto_hip_factor_solve(c, nullptr, 1, nullptr);
}

int idto_hip_timing_enable(idto_hip_ctx* c, int enable) {
  c->timing = enable != 0;
  c->timing_stride = enable > 1 ? enable : 1;  // enable = s > 1: sample every s-th launch
  for (unsigned& t : c->timing_tick) t = 0;
  return 0;
}
int idto_hip_timing_reset(idto_hip_ctx* c) {
  if (TimeDrain(c)) return -2;
  for (int i = 0; i < 4; ++i) { c->tsum[i] = 0; c->tcnt[i] = 0; }
  return 0;
}
int idto_hip_timing_get(idto_hip_ctx* c, int which, double* avg_ms, int* launches) {
  if (which < 0 || which > 3) { g_err = "bad kernel index"; return -1; }
  if (TimeDrain(c)) return -2;
  *launches = c->tcnt[which];
  *avg_ms = c->tcnt[which] ? c->tsum[which] / c->tcnt[which] : 0.0;
  return 0;
}

int idto_hip_sync(idto_hip_ctx* c) {
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

// (every array id, its place and its count: host/context_layout.h IDTO_ARRAYS; the constraint step's two are sized by the
// constraints in force)
long idto_hip_array_size(idto_hip_ctx* c, int what) {
  if (what == IDTO_ARR_CON_S) return c->con_S ? (long)c->con_neq * c->con_neq + c->con_neq : -1;
  if (what == IDTO_ARR_CON_LAMBDA) return (c->con_lambda_at && c->con_neq > 0) ? (long)c->con_neq : -1;
  return idto_host::ArrayLookup(what, c->nq, c->nv, c->N).count;
}
int idto_hip_slab_stride(idto_hip_ctx* c) { return c->slab_stride; }

}  // extern "C"
namespace {
void* DevPtr(idto_hip_ctx* c, int what) {
  if (what == IDTO_ARR_DEBUG && c->kkt_debug && c->kkt) return c->kkt->dbg;
  if (what == IDTO_ARR_CON_S) return c->con_S;
  if (what == IDTO_ARR_CON_LAMBDA) return const_cast<double*>(c->con_lambda_at);
  switch (what) {
#define A(id, field, count) case id: return c->field;
#define S(id, at, width)    // (tau and the three partials live strided inside the slab: SlabRows)
#define O(id)
    IDTO_ARRAYS(A, S, O)
#undef A
#undef S
#undef O
    default: return nullptr;
  }
}
// is the array rows of the slab's records?  *at, *width: doubles into a record, doubles of a row
bool SlabRows(const idto_hip_ctx* c, int what, size_t* at, size_t* width) {
  const idto_host::ArrayInfo ai = idto_host::ArrayLookup(what, c->nq, c->nv, c->N);
  *at = ai.at; *width = ai.width;
  return ai.where == idto_host::ArrayInfo::SLAB_ROWS;
}
}  // namespace
extern "C" {

void* idto_hip_device_ptr(idto_hip_ctx* c, int what) {
  // a caller holding a pointer to the Hessian bands may overwrite them: from here on the solver
  // treats H as a general symmetric block penta-diagonal matrix (no identity block row 0 assumed)
  // until idto_hip_grad_hess assembles it again
  if (what == IDTO_ARR_H_A || what == IDTO_ARR_H_B || what == IDTO_ARR_H_C || what == IDTO_ARR_HBANDS)
    c->h_assembled = false;
  if (what == IDTO_ARR_SLAB) c->terms_valid = false;   // (records written from outside: assemble from the slab)
  return DevPtr(c, what);
}

int idto_hip_prefetch(idto_hip_ctx* c, int what) {
  HIP_OK(hipSetDevice(c->device));
  const long count = idto_hip_array_size(c, what);
  void* p = DevPtr(c, what);
  if (count < 0 || !p) { g_err = "prefetch: array is not contiguous in device memory"; return -1; }
  if (!c->side) HIP_OK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  // slot: the one already holding `what`, else a free one
  idto_hip_ctx::Prefetch* slot = nullptr;
  for (auto& pf : c->pre) if (pf.what == what) slot = &pf;
  if (!slot) for (auto& pf : c->pre) if (pf.what < 0 && !slot) slot = &pf;
  if (!slot) { g_err = "prefetch: at most 4 different arrays"; return -1; }
  if (slot->what != what) {  // lay the staging area out again (rare: first use of an array)
    HIP_OK(hipStreamSynchronize(c->side));
    slot->what = what; slot->count = (size_t)count;
    size_t total = 0;
    for (auto& pf : c->pre) if (pf.what >= 0) { pf.off = total; total += pf.count; pf.pending = false; }
    if (int rc = c->pre_pin.Ensure(total)) return rc;
    if (!slot->ev) HIP_OK(hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming));
  }
  HIP_OK(hipEventRecord(slot->ev, c->stream));
  HIP_OK(hipStreamWaitEvent(c->side, slot->ev, 0));
  HIP_OK(hipMemcpyAsync(c->pre_pin + slot->off, p, slot->count * sizeof(double), hipMemcpyDeviceToHost, c->side));
  slot->pending = true;
  return 0;
}

int idto_hip_get(idto_hip_ctx* c, int what, double* out) {
  HIP_OK(hipSetDevice(c->device));
  for (auto& pf : c->pre)
    if (pf.what == what && pf.pending) {  // the copy was enqueued earlier: wait for it alone
      HIP_OK(hipStreamSynchronize(c->side));
      std::memcpy(out, c->pre_pin + pf.off, pf.count * sizeof(double));
      pf.pending = false;
      return (what == IDTO_ARR_STEP) ? FactorStatus(c) : 0;
    }
  return idto_hip_get_batch(c, what, 0, out);
}

int idto_hip_get_batch(idto_hip_ctx* c, int what, int pb, double* out) {
  HIP_OK(hipSetDevice(c->device));
  if (pb < 0 || pb >= c->batch) { g_err = "problem index outside the batch"; return -1; }
  HIP_OK(hipStreamSynchronize(c->stream));
  const long count = idto_hip_array_size(c, what);
  if (count < 0) { g_err = "unknown array id"; return -1; }
  const size_t po = (size_t)pb * c->pstride;
  size_t off = 0, width = 0;
  if (SlabRows(c, what, &off, &width)) {
    HIP_OK(hipMemcpy2D(out, width * sizeof(double), at_problem(c->slab, po) + off, (size_t)c->slab_stride * sizeof(double),
                       width * sizeof(double), c->N, hipMemcpyDeviceToHost));
    return 0;
  }
  void* p = DevPtr(c, what);
  HIP_OK(hipMemcpy(out, at_problem(static_cast<char*>(p), po), (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
  if (what != IDTO_ARR_STEP) return 0;
  int fs = FactorStatus(c, pb);
  // a launch whose waits between workgroups ran out: FactorStatus has stepped the context down, the Gauss-Newton
  // step is computed again (at most once per variant that can time out)
  for (int attempt = 0; fs == IDTO_HIP_SOLVER_TIMEOUT && attempt < 4 && c->last_step_kind != 0; ++attempt) {
    const int rc = (c->last_step_kind == 2) ? idto_hip_gn_step(c) : idto_hip_factor_solve(c, nullptr, 1, nullptr);
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, at_problem(static_cast<char*>(p), po), (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    fs = FactorStatus(c, pb);
  }
  return fs;
}

int idto_hip_get_many(idto_hip_ctx* c, int n, const int* what, double* const* out) {
  HIP_OK(hipSetDevice(c->device));
  if (n < 0 || (n > 0 && (!what || !out))) { g_err = "get_many: bad arguments"; return -1; }
  if (c->batch != 1) { g_err = "get_many serves single-problem contexts"; return -1; }
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const long count = idto_hip_array_size(c, what[i]);
    if (count < 0 || what[i] == IDTO_ARR_STEP) { g_err = "get_many: unknown array id (or IDTO_ARR_STEP: use idto_hip_get)"; return -1; }
    off[i + 1] = off[i] + (size_t)count;
  }
  if (int rc = c->many_pin.Ensure(off[n], 1)) return rc;
  for (int i = 0; i < n; ++i) {
    const int w = what[i];
    for (auto& pf : c->pre) if (pf.what == w) pf.pending = false;   // (a staged copy of it is superseded)
    double* dst = c->many_pin + off[i];
    size_t o = 0, width = 0;
    if (SlabRows(c, w, &o, &width)) {   // rows of the slab's records
      HIP_OK(hipMemcpy2DAsync(dst, width * sizeof(double), c->slab + o, (size_t)c->slab_stride * sizeof(double), width * sizeof(double),
                              c->N, hipMemcpyDeviceToHost, c->stream));
    } else {
      HIP_OK(hipMemcpyAsync(dst, DevPtr(c, w), (off[i + 1] - off[i]) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
  }
  TRACE("hip: get_many: copies enqueued");
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: get_many: waited");
  for (int i = 0; i < n; ++i) std::memcpy(out[i], c->many_pin + off[i], (off[i + 1] - off[i]) * sizeof(double));
  return 0;
}

int idto_hip_solver_status(idto_hip_ctx* c, int* failed, int* failed_rows_total) {
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  const volatile unsigned* st = c->status_pin;
  int any = 0, rows = 0;
  for (int b = 0; b < c->batch; ++b) {
    any |= (c->fact_id != 0 && st[2 * b] == c->fact_id) ? 1 : 0;
    rows += (int)st[2 * b + 1];
  }
  if (failed) *failed = any;
  if (failed_rows_total) *failed_rows_total = rows;
  return 0;
}

int idto_hip_solver_status_batch(idto_hip_ctx* c, int* failed) {
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  const volatile unsigned* st = c->status_pin;
  for (int b = 0; b < c->batch; ++b) failed[b] = (c->fact_id != 0 && st[2 * b] == c->fact_id) ? 1 : 0;
  return 0;
}

int idto_hip_gn_step_batch(idto_hip_ctx* c) { return idto_hip_gn_step(c); }

int idto_hip_math_probe(int device, const double* x, int n, double* sq, double* rc, double* sn, double* cs, double* ex,
                        double* lg) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_err = "no HIP device available"; return -3; }
  HIP_OK(hipSetDevice(device));
  double* d[7];
  for (int i = 0; i < 7; ++i) HIP_OK(hipMalloc((void**)&d[i], (size_t)n * sizeof(double)));
  HIP_OK(hipMemcpy(d[0], x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d[0], n, d[1], d[2], d[3], d[4], d[5], d[6]);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  double* outs[6] = {sq, rc, sn, cs, ex, lg};
  for (int i = 0; i < 6; ++i) HIP_OK(hipMemcpy(outs[i], d[i + 1], (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < 7; ++i) (void)hipFree(d[i]);
  return 0;
}

}  // extern "C"
