// tracking.h — a plan's feedback law at work: rollouts of the plants' own map under u_t = u*_t - K_t [q (-) q*_t; v - v*_t], the
// torque formed at the start of a control step and held over its substeps, from given initial states - the gains of tvlqr.h
// computed and run in ONE pass of the device with one wait (include/idto_hip.h idto_hip_plant_tvlqr_track).  The question it
// answers: does the plan plus K_t bring a perturbed robot back?  TrackedRollouts is a plain struct; Tracker is a view on any
// optimizer's device context, as Linearizer is.
#pragma once

#include "idto/optimizer/tvlqr.h"

namespace idto {
namespace optimizer {

struct TrackedRollouts {
  TvlqrGains gains;               // the law's K_t, P_t and the linearisation they are about
  int batch = 0, nrollouts = 0, nsteps = 0, nq = 0, nv = 0, nu = 0;
  std::vector<VectorXd> x;        // [batch * nrollouts * nsteps]: the state [q; v] behind step t
  std::vector<VectorXd> u;        // [batch * nrollouts * nsteps]: the control in front of step t (nu)
  std::vector<VectorXd> dx;       // [batch * nrollouts * (nsteps + 1)]: the deviation in front of step t, the final state's last (2 nv)
  std::vector<int> status;        // [batch * nrollouts][2]: {code, substeps completed}; rows behind the last completed step are NaN
  std::size_t at(int step, int rollout, int problem = 0) const { return ((std::size_t)problem * nrollouts + rollout) * nsteps + step; }
  const VectorXd& deviation(int step, int rollout, int problem = 0) const {
    return dx[((std::size_t)problem * nrollouts + rollout) * (nsteps + 1) + step];
  }
  bool ok() const {
    for (std::size_t r = 0; r < status.size() / 2; ++r) if (status[2 * r] != 0) return false;
    return true;
  }
};

class Tracker : public Linearizer {
 public:
  explicit Tracker(idto_hip_ctx* context) : Linearizer(context) {}
  // x [batch][nsteps + 1][nq + nv] the nominal states, tau [batch][nsteps][nv] the nominal torque (all nv components),
  // x0 [batch][nrollouts][nq + nv]; Q, Qf [n x n], R [nu x nu] symmetric, in tangent coordinates
  TrackedRollouts Track(int nsteps, const double* x, const double* tau, int nq, int nv, double h, int substeps, const std::vector<int>& actuated,
                        const MatrixXd& Q, const MatrixXd& R, const MatrixXd& Qf, int nrollouts, const double* x0,
                        double eps = IDTO_LIN_EPS_DEFAULT, int models = IDTO_SCENE_MODELS_PROBLEMS) const {
    const int n = 2 * nv, nu = (int)actuated.size();
    if (Q.rows() != n || Q.cols() != n || Qf.rows() != n || Qf.cols() != n || R.rows() != nu || R.cols() != nu)
      throw std::invalid_argument("Track: Q and Qf are 2 nv x 2 nv, R is nu x nu");
    Raw r = Sized(nsteps, nq, nv, nu);
    TrackedRollouts out;
    out.batch = r.batch; out.nrollouts = nrollouts; out.nsteps = nsteps; out.nq = nq; out.nv = nv; out.nu = nu;
    const std::size_t BR = (std::size_t)r.batch * (nrollouts > 0 ? nrollouts : 0), S = nsteps > 0 ? nsteps : 0, w = (std::size_t)nq + nv;
    std::vector<double> xo(BR * S * w + 1), uo(BR * S * nu + 1), dxo(BR * (S + 1) * n + 1);
    out.status.assign(2 * BR + 1, 0);
    out.gains.status.assign((std::size_t)r.batch, 0);
    Ok(idto_hip_plant_tvlqr_track(ctx_, nsteps, x, tau, h, substeps, eps, models, nu, actuated.data(), Q.data(), R.data(), Qf.data(), nrollouts,
                                  x0, 0, r.xn.data(), r.A.data(), r.B.data(), r.status.data(), r.K.data(), r.P.data(), out.gains.status.data(),
                                  xo.data(), uo.data(), dxo.data(), out.status.data()));
    out.status.resize(2 * BR);
    out.gains.lin = Unpack(r, nsteps, nq, nv);
    out.gains.actuated = actuated;
    Split(r.K, nu, n, &out.gains.K);
    Split(r.P, n, n, &out.gains.P);
    Rows(xo, BR * S, w, &out.x);
    Rows(uo, BR * S, nu, &out.u);
    Rows(dxo, BR * (S + 1), n, &out.dx);
    return out;
  }

 private:
  static void Rows(const std::vector<double>& flat, std::size_t count, std::size_t width, std::vector<VectorXd>* out) {
    out->resize(count);
    for (std::size_t k = 0; k < count; ++k) (*out)[k].assign(flat.begin() + k * width, flat.begin() + (k + 1) * width);
  }
};

}  // namespace optimizer
}  // namespace idto
