// lin_abi.inc — the C-ABI of the plants' linearisation and the time-varying LQR gains (include/idto_hip.h idto_hip_lin_sizes,
// idto_hip_plant_linearize, idto_hip_plant_tvlqr): host code only, included by idto_hip.hip inside its extern "C" block behind
// plant_abi.inc and scene_abi.inc, where the helpers it uses (PlantShapeOf, Refused, RecordForDevice, SelectRecords, GrownEnsure,
// Plan*; Alloc, Release, HIP_OK, TRACE) are defined.  What an entry refuses, the rollouts' block and LDS and where a call's
// arrays lie are host/plant_calls.h's.  The kernels are plant_lin.h's, in lin_launch.hip; the rollouts are plant_kernel's,
// through plant_launch.

static_assert(PLANT_OK == 0, "lin_difference_kernel takes a status word of 0 for a rollout that ended well");

using idto_host::LinTv;

int idto_hip_lin_sizes(idto_hip_ctx* c, int nstates, int nu, int* n, int* columns, long* x_next_count, long* A_count, long* B_count,
                       long* K_count, long* P_count) {
  const long B = c->batch, S = nstates, nn = 2 * c->nv;
  if (n) *n = (int)nn;
  if (columns) *columns = lin_columns(c->nv);
  if (x_next_count) *x_next_count = B * S * (c->nq + c->nv);
  if (A_count) *A_count = B * S * nn * nn;
  if (B_count) *B_count = B * S * nn * c->nv;
  if (K_count) *K_count = B * S * nu * nn;
  if (P_count) *P_count = B * (S + 1) * nn * nn;
  return 0;
}

// The feature's storage, made at the first call: the context's own parameter record where the context has none per problem,
// then one device buffer and its pinned mirror, grown on demand
static int LinEnsure(idto_hip_ctx* c, const std::string& who, size_t dev_count, size_t pin_count) {
  if (!c->lin) {
    if (!c->host_tables || !c->host_model) { g_err = who + ": the context keeps no host copy of its model"; return -1; }
    auto s = std::make_unique<LinState>();
    // (built once and kept for the context's life: host_model and host_contact are written at creation only - an entry that
    // changed either later would have to rebuild this record, as idto_hip_set_model_batch rewrites the context's records)
    std::vector<double> rec = idto_host::ModelRecord(&c->host_model->m, *c->host_tables, c->host_contact);
    if (Alloc(c, rec.size(), &s->record)) return -2;
    RecordForDevice(c, c->M, s->record, rec.data());
    if (hipMemcpy(s->record, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = who + ": hipMemcpy (the parameter record) failed"; Release(c, &s->record); return -2;
    }
    // (a launch above 64 KiB of dynamic LDS needs the opt-in)
    hipError_t e = plant_set_max_lds(idto_host::kPlantMaxLds);
    if (e == hipSuccess) e = tvlqr_set_max_lds(idto_host::kPlantMaxLds);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      g_err = who + ": hipFuncSetAttribute (160 KiB of dynamic LDS) failed: " + hipGetErrorString(e);
      Release(c, &s->record);
      return -2;
    }
    c->lin = std::move(s);
  }
  return GrownEnsure(c, &c->lin->buf, dev_count, pin_count);
}

// What a caller enqueues behind LinRun's launches and in front of its one wait (track_abi.inc: the rollouts under the gains):
// enqueue gets the device's K [B][S][nu * n] where tvlqr_kernel leaves it, finish runs behind the wait
struct LinThen {
  std::function<int(const double* K_dev)> enqueue;
  std::function<void()> finish;
};

// the call has passed idto_host::RefuseLin: layout, upload, the launches, the fetch of what was asked for, one wait, copy-out
static int LinRun(idto_hip_ctx* c, const std::string& who, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                  int models, const LinTv* tv, double* x_next_out, double* A_out, double* B_out, int* status_out, const LinThen* then = nullptr) {
  namespace ln = idto_host::lin;
  const idto_host::PlantShape s = PlantShapeOf(c);
  const int P = lin_columns(c->nv);
  const size_t B = (size_t)c->batch, nv = (size_t)c->nv, w = (size_t)(c->nq + c->nv), n = 2 * nv, SP = (size_t)nstates * (size_t)P;
  const size_t nu = tv ? (size_t)tv->nu : 0;
  const int block = idto_host::PlantBlock(s, 0, 0), plant_lds = idto_host::PlantLdsBytes(s, block, 0);

  HIP_OK(hipSetDevice(c->device));
  const CallPlan p = idto_host::PlanLin(s, nstates, tv != nullptr, tv ? tv->nu : 0);
  if (int rc = LinEnsure(c, who, p.total, p.pinned)) return rc;
  const GrownBuffer& L = c->lin->buf;
  PlanStage(p, L, ln::x, x);
  PlanStage(p, L, ln::tau, tau);
  if (tv) {
    PlanStage(p, L, ln::Q, tv->Q);
    PlanStage(p, L, ln::R, tv->R);
    PlanStage(p, L, ln::Qf, tv->Qf);
    PlanStage(p, L, ln::actuated, tv->actuated, nu * sizeof(int));
  }
  if (int rc = PlanUpload(c, p, L)) return rc;
  auto launched = [&](const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    (void)hipStreamSynchronize(c->stream);
    g_err = who + ": the launch of " + what + " failed: " + hipGetErrorString(e);
    return -2;
  };
  LinArgs a{};
  a.S = nstates; a.P = P; a.nb = c->M.nb; a.nq = c->nq; a.nv = c->nv;
  a.jtype = c->M.jtype; a.qstart = c->M.qstart; a.vstart = c->M.vstart;
  a.x = L.dev + p.at(ln::x); a.tau = L.dev + p.at(ln::tau); a.eps = eps; a.two_eps = 2.0 * eps;
  a.pstate = L.dev + p.at(ln::pstate); a.ptau = L.dev + p.at(ln::ptau); a.pstatus = reinterpret_cast<int*>(L.dev + p.at(ln::pstatus));
  a.x_next = L.dev + p.at(ln::x_next); a.A = L.dev + p.at(ln::A); a.Bm = L.dev + p.at(ln::Bm); a.status = reinterpret_cast<int*>(L.dev + p.at(ln::status));
  lin_perturb_launch(a, c->batch, c->stream);
  if (int rc = launched("lin_perturb_kernel")) return rc;
  for (size_t b = 0; b < B; ++b) {   // the rollouts: plant_kernel in hold mode, every workgroup on problem b's one record
    PlantLaunch pl{};
    pl.plants = (int)SP; pl.block = block; pl.lds = plant_lds; pl.stream = c->stream;
    pl.maxc = c->maxc; pl.nxb = c->M.nxb; pl.nstem = c->M.nstem;
    PlantArgs& A = pl.args;
    SelectRecords(c, models, c->lin->record, (long)b, &A);
    A.state = a.pstate + b * SP * (1 + w); A.tau = a.ptau + b * SP * nv; A.h = h; A.substeps = substeps;
    A.status = reinterpret_cast<int*>(L.dev + p.at(ln::pstatus)) + 2 * b * SP;
    plant_launch(pl);
    if (int rc = launched("plant_kernel")) return rc;
  }
  lin_difference_launch(a, c->batch, c->stream);
  if (int rc = launched("lin_difference_kernel")) return rc;
  if (tv) {
    TvlqrArgs t{};
    t.S = nstates; t.nv = c->nv; t.nu = tv->nu; t.actuated = reinterpret_cast<const int*>(L.dev + p.at(ln::actuated));
    t.A = a.A; t.Bm = a.Bm; t.Q = L.dev + p.at(ln::Q); t.R = L.dev + p.at(ln::R); t.Qf = L.dev + p.at(ln::Qf);
    t.K = L.dev + p.at(ln::K); t.P = L.dev + p.at(ln::P); t.status = reinterpret_cast<int*>(L.dev + p.at(ln::lqr_status));
    tvlqr_launch(t, c->batch, (int)(tvlqr_lds_doubles((int)n, (int)nu) * sizeof(double)), c->stream);
    if (int rc = launched("tvlqr_kernel")) return rc;
  }
  if (then)
    if (int rc = then->enqueue(L.dev + p.at(ln::K))) { (void)hipStreamSynchronize(c->stream); return rc; }
  // (the inputs' copy is in front of the launches on the stream: the staging is free again) - only what was asked for comes back
  void* const outs[] = {x_next_out, A_out, B_out, status_out, tv ? tv->K_out : nullptr, tv ? tv->P_out : nullptr, tv ? tv->lqr_status_out : nullptr};
  for (int e = ln::x_next; e < ln::count; ++e)
    if (int rc = PlanFetch(c, p, L, e, outs[e - ln::x_next])) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: plant_linearize: waited for the device");
  if (then) then->finish();
  for (int e = ln::x_next; e < ln::count; ++e)
    PlanCopyOut(p, L, e, outs[e - ln::x_next], e == ln::lqr_status ? B * sizeof(int) : p.count(e) * sizeof(double));
  return 0;
}

int idto_hip_plant_linearize(idto_hip_ctx* c, int nstates, const double* x, const double* tau, double h, int substeps, double eps, int models,
                             double* x_next_out, double* A_out, double* B_out, int* status_out) {
  if (int rc = Refused(idto_host::RefuseLin(PlantShapeOf(c), "plant_linearize", nstates, x, tau, h, substeps, eps, models, nullptr))) return rc;
  return LinRun(c, "plant_linearize", nstates, x, tau, h, substeps, eps, models, nullptr, x_next_out, A_out, B_out, status_out);
}

int idto_hip_plant_tvlqr(idto_hip_ctx* c, int nstates, const double* x, const double* tau, double h, int substeps, double eps, int models, int nu,
                         const int* actuated, const double* Q, const double* R, const double* Qf, double* x_next_out, double* A_out,
                         double* B_out, int* status_out, double* K_out, double* P_out, int* lqr_status_out) {
  const LinTv tv{nu, actuated, Q, R, Qf, K_out, P_out, lqr_status_out};
  if (int rc = Refused(idto_host::RefuseLin(PlantShapeOf(c), "plant_tvlqr", nstates, x, tau, h, substeps, eps, models, &tv))) return rc;
  return LinRun(c, "plant_tvlqr", nstates, x, tau, h, substeps, eps, models, &tv, x_next_out, A_out, B_out, status_out);
}
