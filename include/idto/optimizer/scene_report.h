// scene_report.h — where the bodies are and what the contact pairs do along a trajectory: what the reference's users read
// from the plant's context behind EvalPlantContext (reference optimizer/trajectory_optimizer.h:452) - body poses, spatial
// velocities, signed-distance pairs, contact results -, here from one launch of the device (include/idto_hip.h
// idto_hip_scene_report).  SceneReport is a plain struct of vectors; Scene is a view on any optimizer's device context, as
// examples::mpc::Plants is: it owns nothing but the report's storage inside the context.
#pragma once

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "idto_hip.h"

namespace idto {
namespace optimizer {

struct SceneReport {
  int batch = 0, nstates = 0, nbodies = 0, npairs = 0, nv = 0;
  std::vector<double> bodies;        // [batch][nstates][nbodies][IDTO_SCENE_BODY_DOUBLES]
  std::vector<double> pairs;         // [batch][nstates][npairs][IDTO_SCENE_PAIR_DOUBLES]
  std::vector<double> tau_contact;   // [batch][nstates][nv]
  std::vector<double> tau_pairs;     // [batch][nstates][npairs][nv], empty unless asked for

  // a body's 18 doubles: R_WB row-major, p, w, v (world frame, body origin)
  const double* body(int state, int body_index, int problem = 0) const {
    return bodies.data() + (((std::size_t)problem * nstates + state) * nbodies + body_index) * IDTO_SCENE_BODY_DOUBLES;
  }
  const double* R_WB(int state, int body_index, int problem = 0) const { return body(state, body_index, problem); }
  const double* p_WB(int state, int body_index, int problem = 0) const { return body(state, body_index, problem) + 9; }
  const double* w_WB(int state, int body_index, int problem = 0) const { return body(state, body_index, problem) + 12; }
  const double* v_WB(int state, int body_index, int problem = 0) const { return body(state, body_index, problem) + 15; }
  // a pair's 20 doubles, at the offsets IDTO_SCENE_PAIR_*
  const double* pair(int state, int pair_index, int problem = 0) const {
    return pairs.data() + (((std::size_t)problem * nstates + state) * npairs + pair_index) * IDTO_SCENE_PAIR_DOUBLES;
  }
  bool active(int state, int pair_index, int problem = 0) const { return pair(state, pair_index, problem)[IDTO_SCENE_PAIR_ACTIVE] != 0.0; }
  double phi(int state, int pair_index, int problem = 0) const { return pair(state, pair_index, problem)[IDTO_SCENE_PAIR_PHI]; }
  double fn(int state, int pair_index, int problem = 0) const { return pair(state, pair_index, problem)[IDTO_SCENE_PAIR_FN]; }
  const double* force(int state, int pair_index, int problem = 0) const { return pair(state, pair_index, problem) + IDTO_SCENE_PAIR_F; }
  const double* contact_torque(int state, int problem = 0) const {
    return tau_contact.data() + ((std::size_t)problem * nstates + state) * nv;
  }
};

class Scene {
 public:
  explicit Scene(idto_hip_ctx* context) : ctx_(context) {   // e.g. optimizer.device_context()
    if (!context) throw std::invalid_argument("Scene: a device context is required");
  }
  // x [batch][nstates][nq + nv]; models: IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS.  One launch, one wait; throws
  // std::runtime_error with the library's refusal
  SceneReport Report(int nstates, const double* x, int nv, int models = IDTO_SCENE_MODELS_PROBLEMS, bool pair_rows = false) const {
    SceneReport r;
    int bd = 0, pd = 0;
    Ok(idto_hip_scene_sizes(ctx_, &r.nbodies, &r.npairs, &bd, &pd));
    r.batch = idto_hip_batch_size(ctx_); r.nstates = nstates > 0 ? nstates : 0; r.nv = nv;
    const std::size_t n = (std::size_t)r.batch * r.nstates;
    r.bodies.resize(n * r.nbodies * bd); r.pairs.resize(n * r.npairs * pd); r.tau_contact.resize(n * nv);
    if (pair_rows) r.tau_pairs.resize(n * r.npairs * nv);
    // (empty vectors still hand over a non-null pointer: an output is "asked for" by its pointer)
    double none = 0.0;
    auto at = [&](std::vector<double>& v) { return v.empty() ? &none : v.data(); };
    Ok(idto_hip_scene_report(ctx_, nstates, x, models, at(r.bodies), at(r.pairs), at(r.tau_contact), pair_rows ? at(r.tau_pairs) : nullptr));
    return r;
  }

 private:
  static void Ok(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("Scene: ") + idto_hip_last_error());
  }
  idto_hip_ctx* ctx_;
};

}  // namespace optimizer
}  // namespace idto
