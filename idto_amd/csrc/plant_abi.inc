// plant_abi.inc — the C-ABI of the plants on the device (include/idto_hip.h idto_hip_forward_dynamics, idto_hip_plant_*):
// host code only, included by idto_hip.hip inside its extern "C" block, where idto_hip_ctx and the helpers it uses
// (PlantShapeOf, Refused, RecordForDevice, SelectRecords; Alloc, Release, UploadStage, HIP_OK, TRACE) are defined.
// What an entry refuses, the block and LDS of a launch and the storage's layout are host/plant_calls.h's.  The kernel is
// plant.h's, its instantiations plant_launch.hip's.

// The plants' one allocation, every plant's parameter record the context's (the base model's, or the context's record b)
static int PlantAllocate(idto_hip_ctx* c, const idto_plant_params_t& prm) {
  const idto_host::PlantShape s = PlantShapeOf(c);
  const bool pd = prm.mode == IDTO_PLANT_PD_PLUS;
  if (int rc = Refused(idto_host::RefusePlantStorage(s, prm.block_threads, pd))) return rc;
  const size_t beside = pd ? idto_host::PlantPdDoubles(s) : 0;
  const int B = c->batch, nq = c->nq, nv = c->nv, nu = pd ? c->mpc->L.nu : 0;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));   // (a record upload of the context's may be in flight; the old storage may be in use)
  c->plant.reset();
  auto p = std::make_unique<PlantState>(c);
  p->nu = nu; p->mpc_generation = c->mpc_generation; p->h = prm.h; p->mode = prm.mode; p->feed_forward = prm.feed_forward;
  p->block = idto_host::PlantBlock(s, prm.block_threads, beside); p->lds = idto_host::PlantLdsBytes(s, p->block, beside);
  p->record_capacity = idto_host::PlantRecordCapacity(prm.record_capacity);
  const std::vector<double> base_record = idto_host::ModelRecord(&c->host_model->m, *c->host_tables, c->host_contact);
  const size_t rec_n = base_record.size();
  if (c->model_records && c->mstride != rec_n * sizeof(double)) { g_err = "plant_begin: the context's parameter records have another size"; return -1; }
  p->mstride = rec_n * sizeof(double);
  const CallPlan L = idto_host::PlanPlantStorage(s, rec_n, prm.record_capacity, nu);
  if (Alloc(c, L.total, &p->base)) return -2;
  namespace ps = idto_host::plant_storage;
  p->records = p->base + L.at(ps::records); p->state = p->base + L.at(ps::state); p->tau = p->base + L.at(ps::tau); p->record = p->base + L.at(ps::record);
  p->fd_x = p->base + L.at(ps::fd_x); p->fd_a = p->base + L.at(ps::fd_a); p->fd_M = p->base + L.at(ps::fd_M); p->fd_bias = p->base + L.at(ps::fd_bias);
  p->Kp = p->base + L.at(ps::Kp); p->Kd = p->base + L.at(ps::Kd); p->status = reinterpret_cast<int*>(p->base + L.at(ps::status));
  p->fd_pinned = L.pinned;
  std::vector<double> all((size_t)B * rec_n);
  if (c->model_records) {
    if (hipMemcpy(all.data(), c->model_records, all.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
      g_err = "plant_begin: hipMemcpy (the context's parameter records) failed"; return -2;
    }
  }
  const size_t mat = model_record_devmodel_at((size_t)c->M.blob_n);
  for (int b = 0; b < B; ++b) {
    double* rec = all.data() + (size_t)b * rec_n;
    DevModel Mb = c->M;
    if (c->model_records) std::memcpy(&Mb, rec + mat, sizeof(DevModel));   // (its tables: the context's record b - moved below)
    else std::copy(base_record.begin(), base_record.end(), rec);
    RecordForDevice(c, Mb, p->records + (size_t)b * rec_n, rec);
  }
  bool ok = hipMemcpy(p->records, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && pd) ok = hipMemcpy(p->Kp, prm.Kp, (size_t)nu * nq * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                     hipMemcpy(p->Kd, prm.Kd, (size_t)nu * nv * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { g_err = "plant_begin: hipMemcpy (parameter records, gains) failed"; return -2; }
  // (a launch above 64 KiB of dynamic LDS needs the opt-in: an instantiation that did not get it would fail at its launch)
  if (const hipError_t e = plant_set_max_lds(idto_host::kPlantMaxLds); e != hipSuccess) {
    (void)hipGetLastError();
    g_err = std::string("plant_begin: hipFuncSetAttribute (160 KiB of dynamic LDS for plant_kernel) failed: ") + hipGetErrorString(e);
    return -2;
  }
  c->plant = std::move(p);
  return 0;
}

int idto_hip_plant_begin(idto_hip_ctx* c, const idto_plant_params_t* prm) {
  if (int rc = Refused(idto_host::RefusePlantBegin(PlantShapeOf(c), prm))) return rc;
  const int rc = PlantAllocate(c, *prm);
  if (rc == 0) c->plant->begun = true;
  return rc;
}

int idto_hip_plant_set_model(idto_hip_ctx* c, int b, const idto_model_t* model, const idto_contact_params_t* contact) {
  if (int rc = Refused(idto_host::RefusePlantSetModel(PlantShapeOf(c), b))) return rc;
  const idto_model_t* base = &c->host_model->m;
  std::vector<double> record;
  if (int rc = idto_host::BuildModelVariant(base, *c->host_tables, b, model ? model : base, contact ? *contact : c->host_contact, &record, &g_err))
    return rc;
  PlantState* p = c->plant.get();
  if (record.size() * sizeof(double) != p->mstride) { g_err = "plant_set_model: the record has another size than the plants' records"; return -1; }
  HIP_OK(hipSetDevice(c->device));
  double* dev = at_problem(p->records, (size_t)b * p->mstride);
  DevModel Mb = c->M;
  for (int i = 0; i < 3; ++i) Mb.gravity[i] = (model ? model : base)->gravity[i];
  RecordForDevice(c, Mb, dev, record.data());
  // (behind whatever the context has enqueued: a launch in flight keeps the record it started with)
  HIP_OK(hipMemcpyAsync(dev, record.data(), p->mstride, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

int idto_hip_plant_set_state(idto_hip_ctx* c, const double* times, const double* x) {
  if (int rc = Refused(idto_host::RefusePlantSetState(PlantShapeOf(c), times, x))) return rc;
  HIP_OK(hipSetDevice(c->device));
  const size_t w = (size_t)(1 + c->nq + c->nv);
  std::vector<double> s((size_t)c->batch * w);
  for (int b = 0; b < c->batch; ++b) {
    s[(size_t)b * w] = times[b];
    std::memcpy(s.data() + (size_t)b * w + 1, x + (size_t)b * (w - 1), (w - 1) * sizeof(double));
  }
  HIP_OK(hipMemcpyAsync(c->plant->state, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

int idto_hip_plant_get_state(idto_hip_ctx* c, double* times_out, double* x_out) {
  if (int rc = Refused(idto_host::RefusePlantsBegun(PlantShapeOf(c), "plant_get_state"))) return rc;
  HIP_OK(hipSetDevice(c->device));
  const size_t w = (size_t)(1 + c->nq + c->nv);
  std::vector<double> s((size_t)c->batch * w);
  HIP_OK(hipMemcpyAsync(s.data(), c->plant->state, s.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  for (int b = 0; b < c->batch; ++b) {
    if (times_out) times_out[b] = s[(size_t)b * w];
    if (x_out) std::memcpy(x_out + (size_t)b * (w - 1), s.data() + (size_t)b * w + 1, (w - 1) * sizeof(double));
  }
  return 0;
}

// plant_kernel's arguments that every launch on the plants' records shares, and the launch
static PlantArgs PlantCommonArgs(const idto_hip_ctx* c) {
  PlantArgs A{};
  SelectRecords(c, IDTO_SCENE_MODELS_PLANTS, nullptr, -1, &A);
  A.status = c->plant->status; A.h = c->plant->h;
  return A;
}
static int PlantEnqueue(idto_hip_ctx* c, const PlantArgs& A, int lds) {
  PlantLaunch L{};
  L.plants = c->batch; L.block = c->plant->block; L.lds = lds; L.stream = c->stream; L.args = A;
  L.maxc = c->maxc; L.nxb = c->M.nxb; L.nstem = c->M.nstem;
  plant_launch(L);
  HIP_OK(hipGetLastError());
  return 0;
}

int idto_hip_forward_dynamics(idto_hip_ctx* c, const double* x, const double* tau_applied, double* a_out, double* M_out, double* bias_out) {
  const idto_host::PlantShape s = PlantShapeOf(c);
  if (int rc = Refused(idto_host::RefuseForwardDynamics(s, x, tau_applied, a_out))) return rc;
  if (!c->plant) {   // (a context that never began a plant: the storage with default parameters)
    idto_plant_params_t prm{};
    prm.h = 1.0; prm.mode = IDTO_PLANT_HOLD;
    if (int rc = PlantAllocate(c, prm)) return rc;
  }
  HIP_OK(hipSetDevice(c->device));
  PlantState* p = c->plant.get();
  const size_t B = (size_t)c->batch, nq = (size_t)c->nq, nv = (size_t)c->nv;
  // (fd_a, fd_M, fd_bias lie next to each other, each padded to 64 bytes: one copy back, then the status words)
  const size_t span = (size_t)(p->fd_bias + B * nv - p->fd_a);
  if (int rc = p->pin.Ensure(p->fd_pinned)) return rc;
  std::memcpy(p->pin, x, B * (nq + nv) * sizeof(double));
  std::memcpy(p->pin + B * (nq + nv), tau_applied, B * nv * sizeof(double));
  HIP_OK(hipMemcpyAsync(p->fd_x, p->pin, B * (nq + nv) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemcpyAsync(p->tau, p->pin + B * (nq + nv), B * nv * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PlantArgs A = PlantCommonArgs(c);
  A.state = p->fd_x; A.tau = p->tau; A.fd = 1; A.substeps = 1;
  A.a_out = p->fd_a; A.M_out = p->fd_M; A.bias_out = p->fd_bias;
  if (int rc = PlantEnqueue(c, A, idto_host::PlantLdsBytes(s, p->block, 0))) { (void)hipStreamSynchronize(c->stream); return rc; }
  const double* back = p->pin;   // (the inputs' copies are in front of the launch on the stream: the staging is free again)
  const int* status = reinterpret_cast<const int*>(p->pin + span);
  HIP_OK(hipMemcpyAsync(p->pin, p->fd_a, span * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(p->pin + span, p->status, 2 * B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: forward_dynamics: waited for the device (a, M and the bias back)");
  std::memcpy(a_out, back, B * nv * sizeof(double));
  if (M_out) std::memcpy(M_out, back + (p->fd_M - p->fd_a), B * nv * nv * sizeof(double));
  if (bias_out) std::memcpy(bias_out, back + (p->fd_bias - p->fd_a), B * nv * sizeof(double));
  for (size_t b = 0; b < B; ++b)
    if (status[2 * b] != PLANT_OK) {
      g_err = "forward_dynamics: plant " + std::to_string(b) + (status[2 * b] == PLANT_PIVOT ? ": a pivot of the mass matrix' LDL^T is not > 0 and finite"
                                                                                              : ": a non-finite state or torque") + " (its a_out is not valid)";
      return -1;
    }
  return 0;
}

// the torque's upload (hold mode) and the launch, enqueued; tick_out: where the final [t, q, v] go as well, or null
static int PlantStepEnqueue(idto_hip_ctx* c, int substeps, const double* tau_hold, int record_every, int nrec, double* tick_out) {
  PlantState* p = c->plant.get();
  const bool pd = p->mode == IDTO_PLANT_PD_PLUS;
  const size_t B = (size_t)c->batch, nv = (size_t)c->nv;
  PlantArgs A = PlantCommonArgs(c);
  A.state = p->state; A.tau = p->tau; A.substeps = substeps; A.tick_out = tick_out;
  A.record_every = nrec ? record_every : 0; A.record = nrec ? p->record : nullptr;
  if (pd) {
    const MpcBatchState* m = c->mpc.get();
    A.pd = 1; A.n = m->L.n; A.nu = m->L.nu; A.feed_forward = p->feed_forward;
    A.breaks = m->breaks; A.plan = m->plan[m->cur]; A.plan_len = m->L.len();
    for (int s = 0; s < 3; ++s) { A.plan_y[s] = m->L.y(s); A.plan_m[s] = m->L.m(s); }
    A.Kp = p->Kp; A.Kd = p->Kd; A.actuated = m->actuated_dev;
  } else {   // (from pinned staging taken in turn: a call without outputs does not wait)
    char* buf = nullptr; int slot = 0;
    if (int rc = UploadStage(c, B * nv * sizeof(double), &buf, &slot)) return rc;
    std::memcpy(buf, tau_hold, B * nv * sizeof(double));
    HIP_OK(hipMemcpyAsync(p->tau, buf, B * nv * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipEventRecord(c->up_ev[slot], c->stream));
  }
  if (int rc = PlantEnqueue(c, A, p->lds)) { (void)hipStreamSynchronize(c->stream); return rc; }
  TRACE("hip: plant_step: the substeps enqueued (one launch)");
  return 0;
}

int idto_hip_plant_step(idto_hip_ctx* c, int substeps, const double* tau_hold, int record_every, double* x_record_out, int* status_out) {
  int nrec = 0;
  if (int rc = Refused(idto_host::RefusePlantStep(PlantShapeOf(c), "plant_step", substeps, tau_hold, record_every, x_record_out != nullptr, &nrec))) return rc;
  HIP_OK(hipSetDevice(c->device));
  PlantState* p = c->plant.get();
  const size_t B = (size_t)c->batch, nq = (size_t)c->nq, nv = (size_t)c->nv;
  if (int rc = PlantStepEnqueue(c, substeps, tau_hold, record_every, nrec, nullptr)) return rc;
  if (!x_record_out && !status_out) return 0;
  const size_t rec_count = B * (size_t)nrec * (nq + nv);
  if (int rc = p->pin.Ensure(rec_count + B)) return rc;
  if (rec_count) HIP_OK(hipMemcpyAsync(p->pin, p->record, rec_count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(p->pin + rec_count, p->status, 2 * B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: plant_step: waited for the device (the recorded states and the status back)");
  if (x_record_out) std::memcpy(x_record_out, p->pin, rec_count * sizeof(double));
  if (status_out) std::memcpy(status_out, p->pin + rec_count, 2 * B * sizeof(int));
  return 0;
}

int idto_hip_mpc_batch_tick_plants(idto_hip_ctx* c, int substeps, int iterations, int scaling_method, int scaling, int normalize_quaternions,
                                   const double* Delta0, double Delta_max, double eta, const int* constrained_dofs, int nu,
                                   double* rows_host, double* Delta_out, double* q_out, double* v_out, double* tau_out,
                                   double* final_cost, int* status, int* best, double* guess_out, double* plans_out,
                                   double* x_after_out, int* plant_status_out) {
  const MpcReplanArgs a{iterations, scaling_method, scaling, normalize_quaternions, Delta0, Delta_max, eta, constrained_dofs, nu, rows_host,
                        Delta_out, q_out, v_out, tau_out, final_cost, status, best, guess_out, plans_out};
  // every refusal first: the tick's (idto_hip_mpc_batch_replan's own), then the step's
  if (int rc = MpcReplanCheck(c, "mpc_batch_tick_plants", a, true, false)) return rc;
  if (int rc = Refused(idto_host::RefuseTickPlantsStep(PlantShapeOf(c), substeps))) return rc;
  HIP_OK(hipSetDevice(c->device));
  // the plants' substeps under PD+ on the current plans; the kernel's last act writes the tick buffer that mpc_shift_kernel reads
  if (int rc = PlantStepEnqueue(c, substeps, nullptr, 0, 0, c->mpc->tick_dev)) return rc;
  return MpcReplanRun(c, nullptr, nullptr, a, c->plant.get(), x_after_out, plant_status_out);
}
