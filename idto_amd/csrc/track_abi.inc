// track_abi.inc — the C-ABI of the plants under the time-varying LQR law (include/idto_hip.h idto_hip_plant_track,
// idto_hip_plant_tvlqr_track): host code only, included by idto_hip.hip inside its extern "C" block behind lin_abi.inc, whose
// helpers it uses (LinEnsure for the context's own parameter record, LinCheck, LinRun and its hook, LinFinite; PlantBlock's
// rule, PlantServes; Alloc, Release, EnsurePinned, HIP_OK, TRACE).  The kernel is plant.h's track_kernel, in track_launch.hip.

#define IDTO_TRACK_MAX_ROLLOUTS 65536   /* batch * nrollouts: the workgroups of one launch */

static int TrackLdsBytes(const idto_hip_ctx* c, int threads, int nu) {
  const size_t d = (size_t)plant_lds_doubles(c->nq, c->nv, c->M.blob_n, c->M.nxb, c->M.nstem, c->npaths, threads) + plant_law_doubles(c->nq, c->nv, nu);
  return d > (size_t)1 << 24 ? 1 << 27 : (int)(d * sizeof(double));
}
// PlantBlock's rule with the law's LDS beside the block's
static int TrackBlock(const idto_hip_ctx* c, int nu) {
  int t = std::min(256, (((c->nv + 1) * c->npaths + 63) / 64) * 64);
  while (t > 64 && TrackLdsBytes(c, t, nu) > 160 * 1024) t -= 64;
  return t;
}

// The feature's storage, made at the first call: one device buffer and its pinned staging, grown on demand (the context's
// own parameter record is lin_abi.inc's, made by LinEnsure)
static int TrackEnsure(idto_hip_ctx* c, const std::string& who, size_t dev_count, size_t pin_count) {
  if (int rc = LinEnsure(c, who, 0, 0)) return rc;
  if (!c->track) {
    // (a launch above 64 KiB of dynamic LDS needs the opt-in, per instantiation)
    if (const hipError_t e = track_set_max_lds(160 * 1024); e != hipSuccess) {
      (void)hipGetLastError();
      g_err = who + ": hipFuncSetAttribute (160 KiB of dynamic LDS for track_kernel) failed: " + hipGetErrorString(e);
      return -2;
    }
    c->track = new TrackState();
  }
  TrackState* s = c->track;
  if (s->dev_cap < dev_count) {
    HIP_OK(hipStreamSynchronize(c->stream));
    Release(c, &s->dev); s->dev_cap = 0;
    if (Alloc(c, dev_count, &s->dev)) return -2;
    s->dev_cap = dev_count;
  }
  return EnsurePinned(&s->pin, &s->pin_cap, pin_count);
}

// a call's arguments beside the gains
struct TrackCall {
  int S, substeps; double h; int models, nu; const int* actuated;
  const double* x_nom; const double* tau_nom; int R; const double* x0; int max_launch_substeps;
  double* x_out; double* u_out; double* dx_out; int* status_out;
};

// every refusal, before any device work (own_K: the call brings its gains, K - the second entry's are the device's)
static int TrackCheck(idto_hip_ctx* c, const std::string& who, const TrackCall& a, bool own_K, const double* K) {
  if (a.S < 1) { g_err = who + ": nsteps must be >= 1"; return -1; }
  if (a.R < 1) { g_err = who + ": nrollouts must be >= 1"; return -1; }
  if (!a.x_nom || !a.tau_nom || !a.x0 || !a.actuated || (own_K && !K)) {
    g_err = who + ": x_nom[batch][nsteps + 1][nq + nv], tau_nom[batch][nsteps][nv], x0[batch][nrollouts][nq + nv], actuated[nu]" +
            (own_K ? " and K[batch][nsteps][nu * n]" : "") + " are required";
    return -1;
  }
  if ((long long)c->batch * a.R > IDTO_TRACK_MAX_ROLLOUTS) {
    g_err = who + ": batch * nrollouts = " + std::to_string((long long)c->batch * a.R) + " rollouts, more than " + std::to_string(IDTO_TRACK_MAX_ROLLOUTS) + " in one call";
    return -1;
  }
  if (a.substeps < 1 || a.substeps > IDTO_PLANT_MAX_SUBSTEPS) { g_err = who + ": substeps must be in [1, 4096] (a single launch stays short on a shared device)"; return -1; }
  if (a.max_launch_substeps != 0 && (a.max_launch_substeps < a.substeps || a.max_launch_substeps > IDTO_PLANT_MAX_SUBSTEPS)) {
    g_err = who + ": max_launch_substeps is 0 or in [substeps, 4096] (a launch holds whole control steps)"; return -1;
  }
  if (!(a.h > 0.0) || !std::isfinite(a.h)) { g_err = who + ": the substep h must be > 0 and finite"; return -1; }
  if (a.models != IDTO_SCENE_MODELS_PROBLEMS && a.models != IDTO_SCENE_MODELS_PLANTS) {
    g_err = who + ": models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS"; return -1;
  }
  if (a.models == IDTO_SCENE_MODELS_PLANTS && (!c->plant || !c->plant->begun)) {
    g_err = who + ": the plants' models were asked for: call idto_hip_plant_begin on the context first"; return -1;
  }
  for (idto_hip_ctx* ch : c->children)
    if (ch) { g_err = who + ": this context has child contexts (the child-context route of idto_hip_tr_solve_batch_constrained made them)"; return -1; }
  if (int rc = PlantServes(c, who.c_str())) return rc;
  if (a.nu < 1 || a.nu > c->nv) { g_err = who + ": nu must be in [1, nv]"; return -1; }
  for (int i = 0; i < a.nu; ++i)
    if (a.actuated[i] < 0 || a.actuated[i] >= c->nv) { g_err = who + ": actuated[" + std::to_string(i) + "] is not a velocity index in [0, nv)"; return -1; }
  const size_t B = (size_t)c->batch, S = (size_t)a.S, w = (size_t)(c->nq + c->nv), nv = (size_t)c->nv;
  if (int rc = LinFinite(who, "x_nom", a.x_nom, B * (S + 1) * w)) return rc;
  if (int rc = LinFinite(who, "tau_nom", a.tau_nom, B * S * nv)) return rc;
  if (int rc = LinFinite(who, "x0", a.x0, B * (size_t)a.R * w)) return rc;
  if (TrackLdsBytes(c, TrackBlock(c, a.nu), a.nu) > 160 * 1024) { g_err = who + ": the model, a substep's evaluations and the law's K_t do not fit the 160 KiB of LDS"; return -1; }
  return 0;
}

// Where a call's arrays lie in the feature's device buffer: [inputs | the rollouts' states | outputs], each part on a 64-byte
// boundary.  The status words are zeroed by the inputs' upload: a launch skips a rollout whose word is not 0.
struct TrackPlan {
  size_t o_x, o_tau, o_K, o_act, o_state, o_st, in_n, out0, o_xo, o_u, o_dx, total;
  size_t n_xo, n_u, n_dx, n_st;
};
static TrackPlan TrackLayout(const idto_hip_ctx* c, const TrackCall& a, bool own_K) {
  const size_t B = (size_t)c->batch, S = (size_t)a.S, R = (size_t)a.R, w = (size_t)(c->nq + c->nv), nv = (size_t)c->nv, n = 2 * nv, nu = (size_t)a.nu;
  TrackPlan p{};
  size_t at = 0;
  auto take = [&](size_t count) { const size_t o = at; at += (count + 7) / 8 * 8; return o; };
  p.n_xo = B * R * S * w; p.n_u = B * R * S * nu; p.n_dx = B * R * (S + 1) * n; p.n_st = B * R;   // (two ints a rollout)
  p.o_x = take(B * (S + 1) * w); p.o_tau = take(B * S * nv); p.o_K = take(own_K ? B * S * nu * n : 0); p.o_act = take((nu + 1) / 2);
  p.o_state = take(B * R * (1 + w)); p.o_st = take(p.n_st); p.in_n = at;
  p.out0 = at;
  p.o_xo = take(p.n_xo); p.o_u = take(p.n_u); p.o_dx = take(p.n_dx);
  p.total = at;
  return p;
}

// the inputs' upload and every launch, enqueued; K_dev: the gains on the device, or null for the call's own (K_host)
static int TrackEnqueue(idto_hip_ctx* c, const std::string& who, const TrackCall& a, const TrackPlan& p, const double* K_host, const double* K_dev) {
  TrackState* T = c->track;
  const size_t B = (size_t)c->batch, S = (size_t)a.S, R = (size_t)a.R, w = (size_t)(c->nq + c->nv), nv = (size_t)c->nv, n = 2 * nv, nu = (size_t)a.nu;
  std::memcpy(T->pin + p.o_x, a.x_nom, B * (S + 1) * w * sizeof(double));
  std::memcpy(T->pin + p.o_tau, a.tau_nom, B * S * nv * sizeof(double));
  if (K_host) std::memcpy(T->pin + p.o_K, K_host, B * S * nu * n * sizeof(double));
  std::memcpy(T->pin + p.o_act, a.actuated, nu * sizeof(int));
  for (size_t r = 0; r < B * R; ++r) {   // [t = 0, q, v]: plant_kernel's state
    double* s = T->pin + p.o_state + r * (1 + w);
    s[0] = 0.0;
    std::memcpy(s + 1, a.x0 + r * w, w * sizeof(double));
  }
  std::memset(T->pin + p.o_st, 0, p.n_st * sizeof(double));
  HIP_OK(hipMemcpyAsync(T->dev, T->pin, p.in_n * sizeof(double), hipMemcpyHostToDevice, c->stream));

  const int block = TrackBlock(c, a.nu);
  PlantLaunch pl{};
  pl.plants = (int)(B * R); pl.block = block; pl.lds = TrackLdsBytes(c, block, a.nu); pl.stream = c->stream;
  pl.maxc = c->maxc; pl.nxb = c->M.nxb; pl.nstem = c->M.nstem;
  PlantArgs& A = pl.args;
  if (a.models == IDTO_SCENE_MODELS_PLANTS) { A.records = c->plant->records; A.mstride = c->plant->mstride; }
  else if (c->model_records) { A.records = c->model_records; A.mstride = c->mstride; }
  else { A.records = c->lin->record; A.mstride = 0; }
  A.rec_contact = model_record_contact_at((size_t)c->M.blob_n) * sizeof(double);
  A.rec_model = model_record_devmodel_at((size_t)c->M.blob_n) * sizeof(double);
  A.state = T->dev + p.o_state; A.h = a.h; A.substeps = a.S * a.substeps;   // (the rollout's: plant.h TrackArgs)
  A.record_every = a.substeps; A.record = T->dev + p.o_xo;
  A.status = reinterpret_cast<int*>(T->dev + p.o_st);
  TrackArgs t{};
  t.R = a.R; t.S = a.S; t.m = a.substeps; t.nu = a.nu;
  t.actuated = reinterpret_cast<const int*>(T->dev + p.o_act);
  t.x_nom = T->dev + p.o_x; t.tau_nom = T->dev + p.o_tau; t.K = K_dev ? K_dev : T->dev + p.o_K;
  t.u_out = T->dev + p.o_u; t.dx_out = T->dev + p.o_dx;
  // whole steps of at most max_launch_substeps substeps a launch: never more than IDTO_PLANT_MAX_SUBSTEPS
  const int per_launch = (a.max_launch_substeps ? a.max_launch_substeps : IDTO_PLANT_MAX_SUBSTEPS) / a.substeps;
  int launches = 0;
  for (int first = 0; first < a.S; first += per_launch, ++launches) {
    t.first_step = first; t.steps = std::min(per_launch, a.S - first);
    track_launch(pl, t);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
      (void)hipStreamSynchronize(c->stream);
      g_err = who + ": the launch of track_kernel failed: " + hipGetErrorString(e);
      return -2;
    }
  }
  TRACE("hip: plant_track: the rollouts enqueued");
  // (the inputs' copy is in front of the launches on the stream: the staging is free again) - only what was asked for comes back
  auto fetch = [&](bool on, size_t o, size_t count) {
    return on ? hipMemcpyAsync(T->pin + (o - p.out0), T->dev + o, count * sizeof(double), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIP_OK(fetch(a.x_out, p.o_xo, p.n_xo));
  HIP_OK(fetch(a.u_out, p.o_u, p.n_u));
  HIP_OK(fetch(a.dx_out, p.o_dx, p.n_dx));
  HIP_OK(hipMemcpyAsync(T->pin + (p.total - p.out0), T->dev + p.o_st, p.n_st * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return 0;
}

// behind the wait: the outputs, with NaN in the rows of a rollout that lie behind its last completed step
static void TrackFinish(idto_hip_ctx* c, const TrackCall& a, const TrackPlan& p) {
  const TrackState* T = c->track;
  const size_t B = (size_t)c->batch, S = (size_t)a.S, R = (size_t)a.R, w = (size_t)(c->nq + c->nv), n = 2 * (size_t)c->nv, nu = (size_t)a.nu;
  auto back = [&](size_t o) { return T->pin + (o - p.out0); };
  const int* status = reinterpret_cast<const int*>(back(p.total));
  if (a.x_out) std::memcpy(a.x_out, back(p.o_xo), p.n_xo * sizeof(double));
  if (a.u_out) std::memcpy(a.u_out, back(p.o_u), p.n_u * sizeof(double));
  if (a.dx_out) std::memcpy(a.dx_out, back(p.o_dx), p.n_dx * sizeof(double));
  if (a.status_out) std::memcpy(a.status_out, status, 2 * B * R * sizeof(int));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t r = 0; r < B * R; ++r) {
    const size_t steps = (size_t)status[2 * r + 1] / (size_t)a.substeps;   // completed steps: the law of step `steps` ran if steps < S
    if (a.x_out) std::fill(a.x_out + (r * S + steps) * w, a.x_out + (r + 1) * S * w, nan);
    if (a.u_out) std::fill(a.u_out + (r * S + steps) * nu, a.u_out + (r + 1) * S * nu, nan);
    if (a.dx_out && steps < S) std::fill(a.dx_out + (r * (S + 1) + steps + 1) * n, a.dx_out + (r + 1) * (S + 1) * n, nan);
  }
}

int idto_hip_plant_track(idto_hip_ctx* c, int nsteps, int substeps, double h, int models, int nu, const int* actuated, const double* x_nom,
                         const double* tau_nom, const double* K, int nrollouts, const double* x0, int max_launch_substeps, double* x_out,
                         double* u_out, double* dx_out, int* status_out) {
  const std::string who = "plant_track";
  const TrackCall a{nsteps, substeps, h, models, nu, actuated, x_nom, tau_nom, nrollouts, x0, max_launch_substeps, x_out, u_out, dx_out, status_out};
  if (int rc = TrackCheck(c, who, a, true, K)) return rc;
  HIP_OK(hipSetDevice(c->device));
  const TrackPlan p = TrackLayout(c, a, true);
  if (int rc = TrackEnsure(c, who, p.total, std::max(p.in_n, p.total - p.out0 + p.n_st))) return rc;
  if (int rc = TrackEnqueue(c, who, a, p, K, nullptr)) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: plant_track: waited for the device");
  TrackFinish(c, a, p);
  return 0;
}

int idto_hip_plant_tvlqr_track(idto_hip_ctx* c, int nsteps, const double* x, const double* tau, double h, int substeps, double eps, int models,
                               int nu, const int* actuated, const double* Q, const double* R, const double* Qf, int nrollouts, const double* x0,
                               int max_launch_substeps, double* x_next_out, double* A_out, double* B_out, int* status_out, double* K_out,
                               double* P_out, int* lqr_status_out, double* x_out, double* u_out, double* dx_out, int* track_status_out) {
  const std::string who = "plant_tvlqr_track";
  const TrackCall a{nsteps, substeps, h, models, nu, actuated, x, tau, nrollouts, x0, max_launch_substeps, x_out, u_out, dx_out, track_status_out};
  if (int rc = TrackCheck(c, who, a, false, nullptr)) return rc;
  // the linearisations are about the first nsteps of the nsteps + 1 states of every problem
  const size_t B = (size_t)c->batch, S = (size_t)nsteps, w = (size_t)(c->nq + c->nv);
  std::vector<double> x_lin(B * S * w);
  for (size_t b = 0; b < B; ++b) std::memcpy(x_lin.data() + b * S * w, x + b * (S + 1) * w, S * w * sizeof(double));
  const LinTv tv{nu, actuated, Q, R, Qf, K_out, P_out, lqr_status_out};
  if (int rc = LinCheck(c, who, nsteps, x_lin.data(), tau, h, substeps, eps, models, &tv)) return rc;
  HIP_OK(hipSetDevice(c->device));
  const TrackPlan p = TrackLayout(c, a, false);
  if (int rc = TrackEnsure(c, who, p.total, std::max(p.in_n, p.total - p.out0 + p.n_st))) return rc;
  const LinThen then{[&](const double* K_dev) { return TrackEnqueue(c, who, a, p, nullptr, K_dev); }, [&]() { TrackFinish(c, a, p); }};
  return LinRun(c, who, nsteps, x_lin.data(), tau, h, substeps, eps, models, &tv, x_next_out, A_out, B_out, status_out, &then);
}
