// track_abi.inc — the C-ABI of the plants under the time-varying LQR law (include/idto_hip.h idto_hip_plant_track,
// idto_hip_plant_tvlqr_track): host code only, included by idto_hip.hip inside its extern "C" block behind lin_abi.inc, whose
// helpers it uses (LinEnsure for the context's own parameter record, LinRun and its hook; PlantShapeOf, Refused, SelectRecords,
// GrownEnsure, Plan*; HIP_OK, TRACE).  What an entry refuses, the rollouts' block and LDS and where a call's arrays lie are
// host/plant_calls.h's.  The kernel is plant.h's track_kernel, in track_launch.hip.

using idto_host::TrackCall;

// The feature's storage, made at the first call: one device buffer and its pinned mirror, grown on demand (the context's
// own parameter record is lin_abi.inc's, made by LinEnsure)
static int TrackEnsure(idto_hip_ctx* c, const std::string& who, const CallPlan& p) {
  if (int rc = LinEnsure(c, who, 0, 0)) return rc;
  if (!c->track) {
    // (a launch above 64 KiB of dynamic LDS needs the opt-in, per instantiation)
    if (const hipError_t e = track_set_max_lds(idto_host::kPlantMaxLds); e != hipSuccess) {
      (void)hipGetLastError();
      g_err = who + ": hipFuncSetAttribute (160 KiB of dynamic LDS for track_kernel) failed: " + hipGetErrorString(e);
      return -2;
    }
    c->track = std::make_unique<GrownBuffer>();
  }
  return GrownEnsure(c, c->track.get(), p.total, p.pinned);
}

// the inputs' upload and every launch, enqueued, then the fetch of what was asked for; K_dev: the gains on the device, or null
// for the call's own (K_host).  The status words are zeroed by the upload: a launch skips a rollout whose word is not 0.
static int TrackEnqueue(idto_hip_ctx* c, const std::string& who, const TrackCall& a, const CallPlan& p, const double* K_host, const double* K_dev) {
  namespace tk = idto_host::track;
  const GrownBuffer& T = *c->track;
  const idto_host::PlantShape s = PlantShapeOf(c);
  const size_t B = (size_t)c->batch, R = (size_t)a.R, w = (size_t)(c->nq + c->nv), nu = (size_t)a.nu;
  PlanStage(p, T, tk::x_nom, a.x_nom);
  PlanStage(p, T, tk::tau_nom, a.tau_nom);
  if (K_host) PlanStage(p, T, tk::K, K_host);
  PlanStage(p, T, tk::actuated, a.actuated, nu * sizeof(int));
  for (size_t r = 0; r < B * R; ++r) {   // [t = 0, q, v]: plant_kernel's state
    double* st = T.pin + p.at(tk::state) + r * (1 + w);
    st[0] = 0.0;
    std::memcpy(st + 1, a.x0 + r * w, w * sizeof(double));
  }
  std::memset(T.pin + p.at(tk::status), 0, p.count(tk::status) * sizeof(double));
  if (int rc = PlanUpload(c, p, T)) return rc;

  const size_t law = plant_law_doubles(c->nq, c->nv, a.nu);
  PlantLaunch pl{};
  pl.plants = (int)(B * R); pl.block = idto_host::PlantBlock(s, 0, law); pl.lds = idto_host::PlantLdsBytes(s, pl.block, law); pl.stream = c->stream;
  pl.maxc = c->maxc; pl.nxb = c->M.nxb; pl.nstem = c->M.nstem;
  PlantArgs& A = pl.args;
  SelectRecords(c, a.models, c->lin->record, -1, &A);
  A.state = T.dev + p.at(tk::state); A.h = a.h; A.substeps = a.S * a.substeps;   // (the rollout's: plant.h TrackArgs)
  A.record_every = a.substeps; A.record = T.dev + p.at(tk::x_out);
  A.status = reinterpret_cast<int*>(T.dev + p.at(tk::status));
  TrackArgs t{};
  t.R = a.R; t.S = a.S; t.m = a.substeps; t.nu = a.nu;
  t.actuated = reinterpret_cast<const int*>(T.dev + p.at(tk::actuated));
  t.x_nom = T.dev + p.at(tk::x_nom); t.tau_nom = T.dev + p.at(tk::tau_nom); t.K = K_dev ? K_dev : T.dev + p.at(tk::K);
  t.u_out = T.dev + p.at(tk::u_out); t.dx_out = T.dev + p.at(tk::dx_out);
  // whole steps of at most max_launch_substeps substeps a launch: never more than IDTO_PLANT_MAX_SUBSTEPS
  const int per_launch = (a.max_launch_substeps ? a.max_launch_substeps : IDTO_PLANT_MAX_SUBSTEPS) / a.substeps;
  for (int first = 0; first < a.S; first += per_launch) {
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
  if (int rc = PlanFetch(c, p, T, tk::x_out, a.x_out)) return rc;
  if (int rc = PlanFetch(c, p, T, tk::u_out, a.u_out)) return rc;
  if (int rc = PlanFetch(c, p, T, tk::dx_out, a.dx_out)) return rc;
  return PlanFetch(c, p, T, tk::status_back, &T, tk::status);   // (always: TrackFinish reads the completed steps)
}

// behind the wait: the outputs, with NaN in the rows of a rollout that lie behind its last completed step
static void TrackFinish(idto_hip_ctx* c, const TrackCall& a, const CallPlan& p) {
  namespace tk = idto_host::track;
  const GrownBuffer& T = *c->track;
  const size_t B = (size_t)c->batch, S = (size_t)a.S, R = (size_t)a.R, w = (size_t)(c->nq + c->nv), n = 2 * (size_t)c->nv, nu = (size_t)a.nu;
  const int* status = reinterpret_cast<const int*>(T.pin + p.Mirror(tk::status_back));
  PlanCopyOut(p, T, tk::x_out, a.x_out);
  PlanCopyOut(p, T, tk::u_out, a.u_out);
  PlanCopyOut(p, T, tk::dx_out, a.dx_out);
  PlanCopyOut(p, T, tk::status_back, a.status_out, 2 * B * R * sizeof(int));
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
  const idto_host::PlantShape s = PlantShapeOf(c);
  if (int rc = Refused(idto_host::RefuseTrack(s, who.c_str(), a, true, K))) return rc;
  HIP_OK(hipSetDevice(c->device));
  const CallPlan p = idto_host::PlanTrack(s, nsteps, nrollouts, nu, true);
  if (int rc = TrackEnsure(c, who, p)) return rc;
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
  const idto_host::PlantShape s = PlantShapeOf(c);
  if (int rc = Refused(idto_host::RefuseTrack(s, who.c_str(), a, false, nullptr))) return rc;
  // the linearisations are about the first nsteps of the nsteps + 1 states of every problem
  const size_t B = (size_t)c->batch, S = (size_t)nsteps, w = (size_t)(c->nq + c->nv);
  std::vector<double> x_lin(B * S * w);
  for (size_t b = 0; b < B; ++b) std::memcpy(x_lin.data() + b * S * w, x + b * (S + 1) * w, S * w * sizeof(double));
  const LinTv tv{nu, actuated, Q, R, Qf, K_out, P_out, lqr_status_out};
  if (int rc = Refused(idto_host::RefuseLin(s, who.c_str(), nsteps, x_lin.data(), tau, h, substeps, eps, models, &tv))) return rc;
  HIP_OK(hipSetDevice(c->device));
  const CallPlan p = idto_host::PlanTrack(s, nsteps, nrollouts, nu, false);
  if (int rc = TrackEnsure(c, who, p)) return rc;
  const LinThen then{[&](const double* K_dev) { return TrackEnqueue(c, who, a, p, nullptr, K_dev); }, [&]() { TrackFinish(c, a, p); }};
  return LinRun(c, who, nsteps, x_lin.data(), tau, h, substeps, eps, models, &tv, x_next_out, A_out, B_out, status_out, &then);
}
