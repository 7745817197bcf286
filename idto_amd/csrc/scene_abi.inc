// scene_abi.inc — the C-ABI of the scene report (include/idto_hip.h idto_hip_scene_sizes, idto_hip_scene_report): host code
// only, included by idto_hip.hip inside its extern "C" block beside plant_abi.inc, where idto_hip_ctx and the helpers it
// uses (PlantShapeOf, Refused, SelectRecords, GrownEnsure, PlanCopyOut; Alloc, Release, HIP_OK, TRACE) are defined.  What the
// entry refuses and where its outputs lie are host/plant_calls.h's.  The kernel is scene_report.h's, its instantiations
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
static int SceneEnsure(idto_hip_ctx* c, const CallPlan& p) {
  if (!c->scene) {
    if (!c->host_model) { g_err = "scene_report: the context keeps no host copy of its model"; return -1; }
    auto s = std::make_unique<SceneState>();
    const int ng = c->M.ngeoms;
    if (Alloc(c, (size_t)ng, &s->geom_body)) return -2;
    if (ng > 0 && hipMemcpy(s->geom_body, c->host_model->m.geom_body, (size_t)ng * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      g_err = "scene_report: hipMemcpy (the geometries' bodies) failed"; Release(c, &s->geom_body); return -2;
    }
    // (a launch above 64 KiB of dynamic LDS needs the opt-in)
    if (const hipError_t e = scene_set_max_lds(idto_host::kPlantMaxLds); e != hipSuccess) {
      (void)hipGetLastError();
      g_err = std::string("scene_report: hipFuncSetAttribute (160 KiB of dynamic LDS for scene_kernel) failed: ") + hipGetErrorString(e);
      Release(c, &s->geom_body);
      return -2;
    }
    c->scene = std::move(s);
  }
  if (int rc = GrownEnsure(c, &c->scene->in, p.in_n, p.pinned)) return rc;
  return GrownEnsure(c, &c->scene->out, std::max<size_t>(p.total, 8), 0);
}

int idto_hip_scene_report(idto_hip_ctx* c, int nstates, const double* x, int models, double* bodies_out, double* pairs_out,
                          double* tau_contact_out, double* tau_pairs_out) {
  namespace sn = idto_host::scene;
  double* const outs[sn::count] = {bodies_out, pairs_out, tau_contact_out, tau_pairs_out};
  unsigned mask = 0;
  for (int e = 0; e < sn::count; ++e) mask |= outs[e] ? 1u << e : 0u;
  const idto_host::PlantShape s = PlantShapeOf(c);
  if (int rc = Refused(idto_host::RefuseSceneReport(s, nstates, x, models, mask))) return rc;
  const CallPlan p = idto_host::PlanScene(s, nstates, mask);

  HIP_OK(hipSetDevice(c->device));
  if (int rc = SceneEnsure(c, p)) return rc;
  SceneState* sc = c->scene.get();
  std::memcpy(sc->in.pin, x, p.in_n * sizeof(double));
  HIP_OK(hipMemcpyAsync(sc->in.dev, sc->in.pin, p.in_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  SceneLaunch L{};
  L.nstates = nstates; L.batch = c->batch; L.block = scene_block(c->M.nb, c->nv, c->M.npairs); L.stream = c->stream;
  L.lds = (int)(scene_lds_doubles(c->M.nb, c->nq, c->nv, c->M.npairs, c->M.blob_n) * sizeof(double));
  SceneArgs& A = L.args;
  SelectRecords(c, models, nullptr, -1, &A);
  A.M = c->M; A.cp = c->cp;
  A.geom_body = sc->geom_body; A.x = sc->in.dev; A.nstates = nstates;
  double** const args[sn::count] = {&A.bodies, &A.pairs, &A.tau_contact, &A.tau_pairs};
  for (int e = 0; e < sn::count; ++e) *args[e] = outs[e] ? sc->out.dev + p.at(e) : nullptr;
  scene_launch(L);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    g_err = std::string("scene_report: the launch failed: ") + hipGetErrorString(e);
    return -2;
  }
  // (the states' copy is in front of the launch on the stream: the staging is free again)
  if (p.total) HIP_OK(hipMemcpyAsync(sc->in.pin, sc->out.dev, p.total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  TRACE("hip: scene_report: waited for the device");
  for (int e = 0; e < sn::count; ++e) PlanCopyOut(p, sc->in, e, outs[e]);
  return 0;
}
