// lin_abi.inc — the C-ABI of the plants' linearisation and the time-varying LQR gains (include/idto_hip.h idto_hip_lin_sizes,
// idto_hip_plant_linearize, idto_hip_plant_tvlqr): host code only, included by idto_hip.hip inside its extern "C" block behind
// plant_abi.inc and scene_abi.inc, whose helpers it uses (PlantBlock, PlantLdsBytes, PlantServes; Alloc, Release, EnsurePinned,
// HIP_OK, TRACE).  The kernels are plant_lin.h's, in lin_launch.hip; the rollouts are plant_kernel's, through plant_launch.

static_assert(PLANT_OK == 0, "lin_difference_kernel takes a status word of 0 for a rollout that ended well");

#define IDTO_LIN_MAX_COLUMNS 65536   /* S * P of one problem: a plant_kernel launch of at most that many workgroups */

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
// then one device buffer and its pinned staging, grown on demand
static int LinEnsure(idto_hip_ctx* c, const std::string& who, size_t dev_count, size_t pin_count) {
  if (!c->lin) {
    if (!c->host_tables || !c->host_model) { g_err = who + ": the context keeps no host copy of its model"; return -1; }
    auto s = std::make_unique<LinState>();
    // (built once and kept for the context's life: host_model and host_contact are written at creation only - an entry that
    // changed either later would have to rebuild this record, as idto_hip_set_model_batch rewrites the context's records)
    std::vector<double> rec = idto_host::ModelRecord(&c->host_model->m, *c->host_tables, c->host_contact);
    if (Alloc(c, rec.size(), &s->record)) return -2;
    DevModel Mb = c->M;
    shift_model(Mb, s->record);
    std::memcpy(rec.data() + model_record_devmodel_at((size_t)c->M.blob_n), &Mb, sizeof(DevModel));
    if (hipMemcpy(s->record, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = who + ": hipMemcpy (the parameter record) failed"; Release(c, &s->record); return -2;
    }
    // (a launch above 64 KiB of dynamic LDS needs the opt-in)
    hipError_t e = plant_set_max_lds(160 * 1024);
    if (e == hipSuccess) e = tvlqr_set_max_lds(160 * 1024);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      g_err = who + ": hipFuncSetAttribute (160 KiB of dynamic LDS) failed: " + hipGetErrorString(e);
      Release(c, &s->record);
      return -2;
    }
    c->lin = s.release();
  }
  LinState* s = c->lin;
  if (s->dev_cap < dev_count) {
    HIP_OK(hipStreamSynchronize(c->stream));
    Release(c, &s->dev); s->dev_cap = 0;
    if (Alloc(c, dev_count, &s->dev)) return -2;
    s->dev_cap = dev_count;
  }
  return EnsurePinned(&s->pin, &s->pin_cap, pin_count);
}

// what idto_hip_plant_tvlqr has beside idto_hip_plant_linearize's arguments
struct LinTv {
  int nu; const int* actuated; const double* Q; const double* R; const double* Qf;
  double* K_out; double* P_out; int* lqr_status_out;
};

static int LinFinite(const std::string& who, const char* what, const double* p, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(p[i])) { g_err = who + ": " + what + " is not finite at index " + std::to_string(i); return -1; }
  return 0;
}

// What a caller enqueues behind LinRun's launches and in front of its one wait (track_abi.inc: the rollouts under the gains):
// enqueue gets the device's K [B][S][nu * n] where tvlqr_kernel leaves it, finish runs behind the wait
struct LinThen {
  std::function<int(const double* K_dev)> enqueue;
  std::function<void()> finish;
};

// every refusal of LinRun, before any device work
static int LinCheck(idto_hip_ctx* c, const std::string& who, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                    int models, const LinTv* tv) {
  if (!x || !tau) { g_err = who + ": x[batch][nstates][nq + nv] and tau[batch][nstates][nv] are required"; return -1; }
  if (nstates < 1) { g_err = who + ": nstates must be >= 1"; return -1; }
  if (substeps < 1 || substeps > IDTO_PLANT_MAX_SUBSTEPS) { g_err = who + ": substeps must be in [1, 4096] (a single launch stays short on a shared device)"; return -1; }
  if (!(h > 0.0) || !std::isfinite(h)) { g_err = who + ": the substep h must be > 0 and finite"; return -1; }
  if (!(eps > 0.0) || !std::isfinite(eps)) { g_err = who + ": eps must be > 0 and finite"; return -1; }
  if (models != IDTO_SCENE_MODELS_PROBLEMS && models != IDTO_SCENE_MODELS_PLANTS) {
    g_err = who + ": models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS"; return -1;
  }
  if (models == IDTO_SCENE_MODELS_PLANTS && (!c->plant || !c->plant->begun)) {
    g_err = who + ": the plants' models were asked for: call idto_hip_plant_begin on the context first"; return -1;
  }
  for (idto_hip_ctx* ch : c->children)
    if (ch) { g_err = who + ": this context has child contexts (the child-context route of idto_hip_tr_solve_batch_constrained made them)"; return -1; }
  if (int rc = PlantServes(c, who.c_str())) return rc;
  const int P = lin_columns(c->nv);
  if ((long long)nstates * P > IDTO_LIN_MAX_COLUMNS) {
    g_err = who + ": nstates * (1 + 6 nv) = " + std::to_string((long long)nstates * P) + " columns, more than " + std::to_string(IDTO_LIN_MAX_COLUMNS) + " in one call";
    return -1;
  }
  const size_t B = (size_t)c->batch, S = (size_t)nstates, nq = (size_t)c->nq, nv = (size_t)c->nv, w = nq + nv, n = 2 * nv;
  const size_t nu = tv ? (size_t)tv->nu : 0;
  if (tv) {
    if (tv->nu < 1 || tv->nu > c->nv) { g_err = who + ": nu must be in [1, nv]"; return -1; }
    if (!tv->actuated || !tv->Q || !tv->R || !tv->Qf) { g_err = who + ": actuated[nu], Q[n * n], R[nu * nu] and Qf[n * n] are required"; return -1; }
    for (size_t i = 0; i < nu; ++i)
      if (tv->actuated[i] < 0 || tv->actuated[i] >= c->nv) { g_err = who + ": actuated[" + std::to_string(i) + "] is not a velocity index in [0, nv)"; return -1; }
    if (int rc = LinFinite(who, "Q", tv->Q, n * n)) return rc;
    if (int rc = LinFinite(who, "R", tv->R, nu * nu)) return rc;
    if (int rc = LinFinite(who, "Qf", tv->Qf, n * n)) return rc;
    if (tvlqr_lds_doubles((int)n, (int)nu) * sizeof(double) > 160 * 1024) {
      g_err = who + ": the Riccati step's matrices (5 n^2 + 4 n nu + 2 nu^2 + nu doubles, n = 2 nv) do not fit the 160 KiB of LDS"; return -1;
    }
  }
  if (int rc = LinFinite(who, "x", x, B * S * w)) return rc;
  if (int rc = LinFinite(who, "tau", tau, B * S * nv)) return rc;
  if (PlantLdsBytes(c, PlantBlock(c, 0, false), false) > 160 * 1024) { g_err = who + ": the model and a substep's evaluations do not fit the 160 KiB of LDS"; return -1; }
  return 0;
}

static int LinRun(idto_hip_ctx* c, const std::string& who, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                  int models, const LinTv* tv, double* x_next_out, double* A_out, double* B_out, int* status_out, const LinThen* then = nullptr) {
  if (int rc = LinCheck(c, who, nstates, x, tau, h, substeps, eps, models, tv)) return rc;
  const int P = lin_columns(c->nv);
  const size_t B = (size_t)c->batch, S = (size_t)nstates, nq = (size_t)c->nq, nv = (size_t)c->nv, w = nq + nv, n = 2 * nv, SP = S * (size_t)P;
  const size_t nu = tv ? (size_t)tv->nu : 0;
  const int block = PlantBlock(c, 0, false), plant_lds = PlantLdsBytes(c, block, false);

  HIP_OK(hipSetDevice(c->device));
  // one device buffer: [inputs | the columns' plants | outputs], each part on a 64-byte boundary
  size_t at = 0;
  auto take = [&](size_t count) { const size_t o = at; at += (count + 7) / 8 * 8; return o; };
  const size_t o_x = take(B * S * w), o_tau = take(B * S * nv), o_Q = take(tv ? n * n : 0), o_R = take(nu * nu), o_Qf = take(tv ? n * n : 0),
               o_act = take((nu + 1) / 2), in_n = at;
  const size_t o_ps = take(B * SP * (1 + w)), o_pt = take(B * SP * nv), o_pst = take(B * SP), out0 = at;
  const size_t n_xn = B * S * w, n_A = B * S * n * n, n_B = B * S * n * nv, n_st = B * S, n_K = tv ? B * S * nu * n : 0,
               n_P = tv ? B * (S + 1) * n * n : 0, n_lst = tv ? (B + 1) / 2 : 0;
  const size_t o_xn = take(n_xn), o_A = take(n_A), o_B = take(n_B), o_st = take(n_st), o_K = take(n_K), o_P = take(n_P), o_lst = take(n_lst);
  if (int rc = LinEnsure(c, who, at, std::max(in_n, at - out0))) return rc;
  LinState* L = c->lin;
  std::memcpy(L->pin + o_x, x, B * S * w * sizeof(double));
  std::memcpy(L->pin + o_tau, tau, B * S * nv * sizeof(double));
  if (tv) {
    std::memcpy(L->pin + o_Q, tv->Q, n * n * sizeof(double));
    std::memcpy(L->pin + o_R, tv->R, nu * nu * sizeof(double));
    std::memcpy(L->pin + o_Qf, tv->Qf, n * n * sizeof(double));
    std::memcpy(L->pin + o_act, tv->actuated, nu * sizeof(int));
  }
  HIP_OK(hipMemcpyAsync(L->dev, L->pin, in_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
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
  a.x = L->dev + o_x; a.tau = L->dev + o_tau; a.eps = eps; a.two_eps = 2.0 * eps;
  a.pstate = L->dev + o_ps; a.ptau = L->dev + o_pt; a.pstatus = reinterpret_cast<int*>(L->dev + o_pst);
  a.x_next = L->dev + o_xn; a.A = L->dev + o_A; a.Bm = L->dev + o_B; a.status = reinterpret_cast<int*>(L->dev + o_st);
  lin_perturb_launch(a, c->batch, c->stream);
  if (int rc = launched("lin_perturb_kernel")) return rc;
  for (size_t b = 0; b < B; ++b) {   // the rollouts: plant_kernel in hold mode, every workgroup on problem b's one record
    PlantLaunch pl{};
    pl.plants = (int)SP; pl.block = block; pl.lds = plant_lds; pl.stream = c->stream;
    pl.maxc = c->maxc; pl.nxb = c->M.nxb; pl.nstem = c->M.nstem;
    PlantArgs& A = pl.args;
    if (models == IDTO_SCENE_MODELS_PLANTS) A.records = at_problem(c->plant->records, b * c->plant->mstride);
    else A.records = c->model_records ? at_problem(c->model_records, b * c->mstride) : L->record;
    A.mstride = 0;
    A.rec_contact = model_record_contact_at((size_t)c->M.blob_n) * sizeof(double);
    A.rec_model = model_record_devmodel_at((size_t)c->M.blob_n) * sizeof(double);
    A.state = a.pstate + b * SP * (1 + w); A.tau = a.ptau + b * SP * nv; A.h = h; A.substeps = substeps;
    A.status = reinterpret_cast<int*>(L->dev + o_pst) + 2 * b * SP;
    plant_launch(pl);
    if (int rc = launched("plant_kernel")) return rc;
  }
  lin_difference_launch(a, c->batch, c->stream);
  if (int rc = launched("lin_difference_kernel")) return rc;
  if (tv) {
    TvlqrArgs t{};
    t.S = nstates; t.nv = c->nv; t.nu = tv->nu; t.actuated = reinterpret_cast<const int*>(L->dev + o_act);
    t.A = a.A; t.Bm = a.Bm; t.Q = L->dev + o_Q; t.R = L->dev + o_R; t.Qf = L->dev + o_Qf;
    t.K = L->dev + o_K; t.P = L->dev + o_P; t.status = reinterpret_cast<int*>(L->dev + o_lst);
    tvlqr_launch(t, c->batch, (int)(tvlqr_lds_doubles((int)n, (int)nu) * sizeof(double)), c->stream);
    if (int rc = launched("tvlqr_kernel")) return rc;
  }
  if (then)
    if (int rc = then->enqueue(L->dev + o_K)) { (void)hipStreamSynchronize(c->stream); return rc; }
  // (the inputs' copy is in front of the launches on the stream: the staging is free again) - only what was asked for comes back
  auto fetch = [&](bool on, size_t o, size_t count) {
    return on && count ? hipMemcpyAsync(L->pin + (o - out0), L->dev + o, count * sizeof(double), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIP_OK(fetch(x_next_out, o_xn, n_xn));
  HIP_OK(fetch(A_out, o_A, n_A));
  HIP_OK(fetch(B_out, o_B, n_B));
  HIP_OK(fetch(status_out, o_st, n_st));
  if (tv) {
    HIP_OK(fetch(tv->K_out, o_K, n_K));
    HIP_OK(fetch(tv->P_out, o_P, n_P));
    HIP_OK(fetch(tv->lqr_status_out, o_lst, n_lst));
  }
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: plant_linearize: waited for the device");
  if (then) then->finish();
  auto back = [&](size_t o) { return L->pin + (o - out0); };
  if (x_next_out) std::memcpy(x_next_out, back(o_xn), n_xn * sizeof(double));
  if (A_out) std::memcpy(A_out, back(o_A), n_A * sizeof(double));
  if (B_out) std::memcpy(B_out, back(o_B), n_B * sizeof(double));
  if (status_out) std::memcpy(status_out, back(o_st), 2 * B * S * sizeof(int));
  if (tv) {
    if (tv->K_out) std::memcpy(tv->K_out, back(o_K), n_K * sizeof(double));
    if (tv->P_out) std::memcpy(tv->P_out, back(o_P), n_P * sizeof(double));
    if (tv->lqr_status_out) std::memcpy(tv->lqr_status_out, back(o_lst), B * sizeof(int));
  }
  return 0;
}

int idto_hip_plant_linearize(idto_hip_ctx* c, int nstates, const double* x, const double* tau, double h, int substeps, double eps, int models,
                             double* x_next_out, double* A_out, double* B_out, int* status_out) {
  return LinRun(c, "plant_linearize", nstates, x, tau, h, substeps, eps, models, nullptr, x_next_out, A_out, B_out, status_out);
}

int idto_hip_plant_tvlqr(idto_hip_ctx* c, int nstates, const double* x, const double* tau, double h, int substeps, double eps, int models, int nu,
                         const int* actuated, const double* Q, const double* R, const double* Qf, double* x_next_out, double* A_out,
                         double* B_out, int* status_out, double* K_out, double* P_out, int* lqr_status_out) {
  const LinTv tv{nu, actuated, Q, R, Qf, K_out, P_out, lqr_status_out};
  return LinRun(c, "plant_tvlqr", nstates, x, tau, h, substeps, eps, models, &tv, x_next_out, A_out, B_out, status_out);
}
