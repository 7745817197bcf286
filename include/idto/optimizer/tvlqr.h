// tvlqr.h — the local feedback law that belongs to a plan: the plant's linearisation x+ ~ f(x*, u*) + A_t dx + B_t du about the
// states of a trajectory, and the gains K_t, cost-to-go P_t of the finite-horizon LQR problem along them, from one pass of
// the device (include/idto_hip.h idto_hip_plant_linearize, idto_hip_plant_tvlqr).  f is the plants' own map - `substeps`
// semi-implicit Euler substeps of h under a held torque, with the optimizer's contact model -, so the law stabilises what
// examples::mpc::Plants simulates.  Deviations are in tangent coordinates dx = [dtheta (nv); dv (nv)], n = 2 nv: a floating
// joint's quaternion deviates by three angular components in the world frame, as its velocity does.
// PlantLinearization and TvlqrGains are plain structs; Linearizer is a view on any optimizer's device context, as Scene is.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "idto/optimizer/types.h"
#include "idto_hip.h"

namespace idto {
namespace optimizer {

struct PlantLinearization {
  int batch = 0, nstates = 0, nq = 0, nv = 0;
  std::vector<VectorXd> x_next;   // [batch * nstates]: f(x_s, tau_s) = [q; v]
  std::vector<MatrixXd> A;        // [batch * nstates]: n x n
  std::vector<MatrixXd> B;        // [batch * nstates]: n x nv
  std::vector<int> status;        // [batch * nstates][2]: {0, 0}, or {the rollout's code, the column}: A, B, x_next of the state are NaN
  std::size_t at(int state, int problem = 0) const { return (std::size_t)problem * nstates + state; }
  bool ok() const {
    for (int s : status) if (s != 0) return false;
    return true;
  }
};

struct TvlqrGains {
  PlantLinearization lin;
  std::vector<int> actuated;      // [nu] the velocity indices of u: the columns Bu of B
  std::vector<MatrixXd> K;        // [batch * nstates]: nu x n; u = u_nom - K_t [q (-) q_nom; v - v_nom]
  std::vector<MatrixXd> P;        // [batch * (nstates + 1)]: n x n, P_S = Qf
  std::vector<int> status;        // [batch]: 0, or 1 + t: K and P from t downward are NaN
  const MatrixXd& cost_to_go(int t, int problem = 0) const { return P[(std::size_t)problem * (lin.nstates + 1) + t]; }
};

class Linearizer {
 public:
  explicit Linearizer(idto_hip_ctx* context) : ctx_(context) {   // e.g. optimizer.device_context()
    if (!context) throw std::invalid_argument("Linearizer: a device context is required");
  }
  // x [batch][nstates][nq + nv], tau [batch][nstates][nv].  Throws std::runtime_error with the library's refusal.
  PlantLinearization Linearize(int nstates, const double* x, const double* tau, int nq, int nv, double h, int substeps,
                               double eps = IDTO_LIN_EPS_DEFAULT, int models = IDTO_SCENE_MODELS_PROBLEMS) const {
    Raw r = Sized(nstates, nq, nv, 0);
    Ok(idto_hip_plant_linearize(ctx_, nstates, x, tau, h, substeps, eps, models, r.xn.data(), r.A.data(), r.B.data(), r.status.data()));
    return Unpack(r, nstates, nq, nv);
  }
  // Q, Qf [n x n], R [nu x nu] symmetric, in tangent coordinates
  TvlqrGains Gains(int nstates, const double* x, const double* tau, int nq, int nv, double h, int substeps, const std::vector<int>& actuated,
                   const MatrixXd& Q, const MatrixXd& R, const MatrixXd& Qf, double eps = IDTO_LIN_EPS_DEFAULT,
                   int models = IDTO_SCENE_MODELS_PROBLEMS) const {
    const int n = 2 * nv, nu = (int)actuated.size();
    if (Q.rows() != n || Q.cols() != n || Qf.rows() != n || Qf.cols() != n || R.rows() != nu || R.cols() != nu)
      throw std::invalid_argument("Tvlqr: Q and Qf are 2 nv x 2 nv, R is nu x nu");
    Raw r = Sized(nstates, nq, nv, nu);
    TvlqrGains g;
    g.status.assign((std::size_t)r.batch, 0);
    Ok(idto_hip_plant_tvlqr(ctx_, nstates, x, tau, h, substeps, eps, models, nu, actuated.data(), Q.data(), R.data(), Qf.data(), r.xn.data(),
                            r.A.data(), r.B.data(), r.status.data(), r.K.data(), r.P.data(), g.status.data()));
    g.lin = Unpack(r, nstates, nq, nv);
    g.actuated = actuated;
    Split(r.K, nu, n, &g.K);
    Split(r.P, n, n, &g.P);
    return g;
  }

 protected:   // (idto/optimizer/tracking.h Tracker lays its call's arrays out with the same helpers)
  struct Raw { int batch = 0; std::vector<double> xn, A, B, K, P; std::vector<int> status; };
  Raw Sized(int nstates, int nq, int nv, int nu) const {
    Raw r;
    r.batch = idto_hip_batch_size(ctx_);
    const std::size_t BS = (std::size_t)r.batch * (nstates > 0 ? nstates : 0), n = 2 * (std::size_t)nv;
    // (an empty vector still hands over a non-null pointer: the library refuses nstates < 1 by name)
    r.xn.resize(BS * (nq + nv) + 1); r.A.resize(BS * n * n + 1); r.B.resize(BS * n * nv + 1); r.status.resize(2 * BS + 1);
    r.K.resize(BS * nu * n + 1); r.P.resize((BS + r.batch) * n * n + 1);
    return r;
  }
  static void Split(const std::vector<double>& flat, int rows, int cols, std::vector<MatrixXd>* out) {
    const std::size_t each = (std::size_t)rows * cols, count = each ? (flat.size() - 1) / each : 0;
    out->assign(count, MatrixXd(rows, cols));
    for (std::size_t k = 0; k < count; ++k) std::copy(flat.begin() + k * each, flat.begin() + (k + 1) * each, (*out)[k].data());
  }
  static PlantLinearization Unpack(const Raw& r, int nstates, int nq, int nv) {
    PlantLinearization l;
    l.batch = r.batch; l.nstates = nstates; l.nq = nq; l.nv = nv;
    const std::size_t BS = (std::size_t)r.batch * nstates, w = (std::size_t)nq + nv;
    l.x_next.resize(BS);
    for (std::size_t k = 0; k < BS; ++k) l.x_next[k].assign(r.xn.begin() + k * w, r.xn.begin() + (k + 1) * w);
    Split(r.A, 2 * nv, 2 * nv, &l.A);
    Split(r.B, 2 * nv, nv, &l.B);
    l.status.assign(r.status.begin(), r.status.begin() + 2 * BS);
    return l;
  }
  static void Ok(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("Linearizer: ") + idto_hip_last_error());
  }
  idto_hip_ctx* ctx_;
};

// blkdiag(Qtheta, Qv): the state weight in tangent coordinates from its two nv x nv blocks
inline MatrixXd TangentWeight(const MatrixXd& Qtheta, const MatrixXd& Qv) {
  const int nv = Qtheta.rows();
  if (Qtheta.cols() != nv || Qv.rows() != nv || Qv.cols() != nv) throw std::invalid_argument("Tvlqr: Qtheta and Qv are nv x nv");
  MatrixXd Q(2 * nv, 2 * nv);
  for (int j = 0; j < nv; ++j)
    for (int i = 0; i < nv; ++i) { Q(i, j) = Qtheta(i, j); Q(nv + i, nv + j) = Qv(i, j); }
  return Q;
}

// time_step / h as a substep count; throws unless it is an integer >= 1 to 1e-9
inline int SubstepsPerStep(double time_step, double h) {
  const double r = time_step / h, k = std::round(r);
  if (!(h > 0.0) || !std::isfinite(r) || k < 1.0 || std::fabs(r - k) > 1e-9)
    throw std::invalid_argument("Tvlqr: time_step / h = " + std::to_string(r) + " is not a whole number of substeps");
  return (int)k;
}

}  // namespace optimizer
}  // namespace idto
