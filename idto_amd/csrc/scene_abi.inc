// scene_abi.inc — the C-ABI of the scene report (include/idto_hip.h idto_hip_scene_sizes, idto_hip_scene_report): host code
// only, included by idto_hip.hip inside its extern "C" block beside plant_abi.inc, where idto_hip_ctx and the helpers it
// uses (Alloc, Release, EnsurePinned, HIP_OK, TRACE) are defined.  The kernel is scene_report.h's, its instantiations
// scene_launch.hip's.

int idto_hip_scene_sizes(idto_hip_ctx* c, int* nbodies, int* npairs, int* body_doubles, int* pair_doubles) {
  if (nbodies) *nbodies = c->M.nb;
  if (npairs) *npairs = c->M.npairs;
  if (body_doubles) *body_doubles = IDTO_SCENE_BODY_DOUBLES;
  if (pair_doubles) *pair_doubles = IDTO_SCENE_PAIR_DOUBLES;
  return 0;
}

// The report's storage, made at the first report: the body of every geometry (one table per context: the topology is shared
// by the problems of a batch), then the states and the outputs of a call, grown on demand
static int SceneEnsure(idto_hip_ctx* c, size_t in_count, size_t out_count) {
  if (!c->scene) {
    if (!c->host_model) { g_err = "scene_report: the context keeps no host copy of its model"; return -1; }
    auto s = std::make_unique<SceneState>();
    const int ng = c->M.ngeoms;
    if (Alloc(c, (size_t)ng, &s->geom_body)) return -2;
    if (ng > 0 && hipMemcpy(s->geom_body, c->host_model->m.geom_body, (size_t)ng * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = "scene_report: hipMemcpy (the geometries' bodies) failed"; Release(c, &s->geom_body); return -2;
    }
    // (a launch above 64 KiB of dynamic LDS needs the opt-in)
    if (const hipError_t e = scene_set_max_lds(160 * 1024); e != hipSuccess) {
      (void)hipGetLastError();
      g_err = std::string("scene_report: hipFuncSetAttribute (160 KiB of dynamic LDS for scene_kernel) failed: ") + hipGetErrorString(e);
      Release(c, &s->geom_body);
      return -2;
    }
    c->scene = s.release();
  }
  SceneState* s = c->scene;
  if (s->in_cap < in_count) {
    HIP_OK(hipStreamSynchronize(c->stream));
    Release(c, &s->in); s->in_cap = 0;
    if (Alloc(c, in_count, &s->in)) return -2;
    s->in_cap = in_count;
  }
  if (s->out_cap < out_count) {
    HIP_OK(hipStreamSynchronize(c->stream));
    Release(c, &s->out); s->out_cap = 0;
    if (Alloc(c, out_count, &s->out)) return -2;
    s->out_cap = out_count;
  }
  return EnsurePinned(&s->pin, &s->pin_cap, std::max(in_count, out_count));
}

int idto_hip_scene_report(idto_hip_ctx* c, int nstates, const double* x, int models, double* bodies_out, double* pairs_out,
                          double* tau_contact_out, double* tau_pairs_out) {
  // ---- every refusal, before any device work
  if (!x) { g_err = "scene_report: x[batch][nstates][nq + nv] is required"; return -1; }
  if (nstates < 1) { g_err = "scene_report: nstates must be >= 1"; return -1; }
  if (!bodies_out && !pairs_out && !tau_contact_out && !tau_pairs_out) { g_err = "scene_report: every output is NULL: nothing to report"; return -1; }
  if (models != IDTO_SCENE_MODELS_PROBLEMS && models != IDTO_SCENE_MODELS_PLANTS) {
    g_err = "scene_report: models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS"; return -1;
  }
  if (models == IDTO_SCENE_MODELS_PLANTS && (!c->plant || !c->plant->begun)) {
    g_err = "scene_report: the plants' models were asked for: call idto_hip_plant_begin on the context first"; return -1;
  }
  if (nstates > (1 << 20)) { g_err = "scene_report: more than 1048576 states in one call"; return -1; }
  const size_t B = (size_t)c->batch, S = (size_t)nstates, w = (size_t)(c->nq + c->nv);
  const size_t nb = (size_t)c->M.nb, np = (size_t)c->M.npairs, nv = (size_t)c->nv;
  for (size_t b = 0; b < B; ++b)
    for (size_t s = 0; s < S; ++s)
      for (size_t i = 0; i < w; ++i)
        if (!std::isfinite(x[(b * S + s) * w + i])) {
          g_err = "scene_report: x is not finite at problem " + std::to_string(b) + ", state " + std::to_string(s) + ", index " + std::to_string(i);
          return -1;
        }
  const size_t lds = scene_lds_doubles(c->M.nb, c->nq, c->nv, c->M.npairs, c->M.blob_n) * sizeof(double);
  if (lds > 160 * 1024) { g_err = "scene_report: the model, its bodies' records and its pairs' rows do not fit the 160 KiB of LDS"; return -1; }

  HIP_OK(hipSetDevice(c->device));
  // the outputs' places in one device buffer, each on a 64-byte boundary
  size_t at = 0;
  auto take = [&](bool on, size_t count) { const size_t o = at; if (on) at += (count + 7) / 8 * 8; return o; };
  const size_t n_bodies = B * S * nb * IDTO_SCENE_BODY_DOUBLES, n_pairs = B * S * np * IDTO_SCENE_PAIR_DOUBLES, n_tau = B * S * nv,
               n_rows = B * S * np * nv;
  const size_t o_bodies = take(bodies_out, n_bodies), o_pairs = take(pairs_out, n_pairs), o_tau = take(tau_contact_out, n_tau),
               o_rows = take(tau_pairs_out, n_rows);
  if (int rc = SceneEnsure(c, B * S * w, std::max<size_t>(at, 8))) return rc;
  SceneState* sc = c->scene;
  std::memcpy(sc->pin, x, B * S * w * sizeof(double));
  HIP_OK(hipMemcpyAsync(sc->in, sc->pin, B * S * w * sizeof(double), hipMemcpyHostToDevice, c->stream));
  SceneLaunch L{};
  L.nstates = nstates; L.batch = c->batch; L.block = scene_block(c->M.nb, c->nv, c->M.npairs); L.lds = (int)lds; L.stream = c->stream;
  SceneArgs& A = L.args;
  if (models == IDTO_SCENE_MODELS_PLANTS) { A.records = c->plant->records; A.mstride = c->plant->mstride; }
  else if (c->model_records) { A.records = c->model_records; A.mstride = c->mstride; }
  A.rec_contact = model_record_contact_at((size_t)c->M.blob_n) * sizeof(double);
  A.rec_model = model_record_devmodel_at((size_t)c->M.blob_n) * sizeof(double);
  A.M = c->M; A.cp = c->cp;
  A.geom_body = sc->geom_body; A.x = sc->in; A.nstates = nstates;
  A.bodies = bodies_out ? sc->out + o_bodies : nullptr;
  A.pairs = pairs_out ? sc->out + o_pairs : nullptr;
  A.tau_contact = tau_contact_out ? sc->out + o_tau : nullptr;
  A.tau_pairs = tau_pairs_out ? sc->out + o_rows : nullptr;
  scene_launch(L);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    g_err = std::string("scene_report: the launch failed: ") + hipGetErrorString(e);
    return -2;
  }
  // (the states' copy is in front of the launch on the stream: the staging is free again)
  if (at) HIP_OK(hipMemcpyAsync(sc->pin, sc->out, at * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: scene_report: waited for the device");
  if (bodies_out) std::memcpy(bodies_out, sc->pin + o_bodies, n_bodies * sizeof(double));
  if (pairs_out) std::memcpy(pairs_out, sc->pin + o_pairs, n_pairs * sizeof(double));
  if (tau_contact_out) std::memcpy(tau_contact_out, sc->pin + o_tau, n_tau * sizeof(double));
  if (tau_pairs_out) std::memcpy(tau_pairs_out, sc->pin + o_rows, n_rows * sizeof(double));
  return 0;
}
