// A C++ consumer of TrajectoryOptimizer::Track (include/idto/optimizer/tracking.h) with no Python in the process: the pendulum
// at N = 5, a few iterations of Solve towards the upright position, then the time-varying LQR gains about the solution and two
// rollouts under them from perturbed initial states, in substeps of time_step / 4 - one pass of the device.  It prints the
// solution and everything the call returned with 17 significant digits; tests/test_gpu_plant_track.py runs it on the GPU and
// holds the printed numbers to the Python route on the same states.
//
// usage: track_pendulum <path to pendulum.model>
#include <cstdio>
#include <string>
#include <vector>

#include "idto/model_file.h"
#include "idto/optimizer/trajectory_optimizer.h"

using namespace idto::optimizer;

static void row(const char* name, int t, const double* p, std::size_t n) {
  std::printf("%s %d", name, t);
  for (std::size_t i = 0; i < n; ++i) std::printf(" %.17g", p[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: track_pendulum <pendulum.model>\n"); return 2; }
  try {
    const idto::ModelFile mf = idto::ModelFile::Load(argv[1]);
    const int N = 5, nq = mf.nq, nv = mf.nv, R = 2;
    const double dt = 0.05;
    ProblemDefinition prob;
    prob.num_steps = N;
    prob.q_init = {2.9};
    prob.v_init = {0.1};
    prob.Qq = MatrixXd::Diagonal({1.0});
    prob.Qv = MatrixXd::Diagonal({1.0});
    prob.R = MatrixXd::Diagonal({0.1});
    prob.Qf_q = MatrixXd::Diagonal({100.0});
    prob.Qf_v = MatrixXd::Diagonal({1.0});
    for (int t = 0; t <= N; ++t) { prob.q_nom.push_back({3.1415}); prob.v_nom.push_back({0.0}); }
    SolverParameters params;
    params.max_iterations = 3;
    params.scaling = false;
    params.equality_constraints = false;
    params.verbose = false;
    TrajectoryOptimizer<double> opt(mf.c_model(), dt, prob, params);
    std::vector<VectorXd> q_guess((std::size_t)N + 1, prob.q_init);
    TrajectoryOptimizerSolution<double> solution;
    TrajectoryOptimizerStats<double> stats;
    opt.Solve(q_guess, &solution, &stats);
    for (int t = 0; t <= N; ++t) { row("q", t, solution.q[t].data(), nq); row("v", t, solution.v[t].data(), nv); }
    for (int t = 0; t < N; ++t) row("tau", t, solution.tau[t].data(), nv);

    const MatrixXd Qtheta = MatrixXd::Diagonal({10.0}), Qv = MatrixXd::Diagonal({1.0});
    const MatrixXd Qf_theta = MatrixXd::Diagonal({100.0}), Qf_v = MatrixXd::Diagonal({10.0});
    const std::vector<int> act = opt.actuated_dofs();
    std::printf("actuated");
    for (int j : act) std::printf(" %d", j);
    std::printf("\n");
    const MatrixXd Rw = MatrixXd::Diagonal(VectorXd(act.size(), 0.1));
    std::vector<VectorXd> x0s;
    for (int r = 0; r < R; ++r) {
      VectorXd x0 = {solution.q[0][0] + 0.01 * (r + 1), solution.v[0][0] - 0.02 * (r + 1)};
      row("x0", r, x0.data(), (std::size_t)nq + nv);
      x0s.push_back(x0);
    }
    const TrackedRollouts tr = opt.Track(solution, dt / 4, Qtheta, Qv, Rw, Qf_theta, Qf_v, x0s);
    std::printf("lqr_status %d lin_ok %d track_ok %d\n", tr.gains.status[0], (int)tr.gains.lin.ok(), (int)tr.ok());
    const std::size_t n = 2 * (std::size_t)nv;
    for (int t = 0; t < N; ++t) row("K", t, tr.gains.K[(std::size_t)t].data(), act.size() * n);
    for (int r = 0; r < R; ++r) {
      std::printf("status %d %d %d\n", r, tr.status[2 * r], tr.status[2 * r + 1]);
      for (int t = 0; t < N; ++t) {
        row("x", r * N + t, tr.x[tr.at(t, r)].data(), (std::size_t)nq + nv);
        row("u", r * N + t, tr.u[tr.at(t, r)].data(), act.size());
      }
      for (int t = 0; t <= N; ++t) row("dx", r * (N + 1) + t, tr.deviation(t, r).data(), n);
    }
    // the gains inside are Tvlqr's
    const TvlqrGains g = opt.Tvlqr(solution, dt / 4, Qtheta, Qv, Rw, Qf_theta, Qf_v);
    bool same = g.status == tr.gains.status && g.K.size() == tr.gains.K.size();
    for (std::size_t t = 0; same && t < g.K.size(); ++t)
      for (std::size_t i = 0; i < act.size() * n; ++i) same = same && g.K[t].data()[i] == tr.gains.K[t].data()[i];
    std::printf("tvlqr_same %d\n", (int)same);
    // a substep that does not divide the time step is refused
    try {
      opt.Track(solution, dt / 4.5, Qtheta, Qv, Rw, Qf_theta, Qf_v, x0s);
      std::printf("refused 0\n");
    } catch (const std::invalid_argument& e) {
      std::printf("refused 1 %s\n", e.what());
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "track_pendulum: %s\n", e.what());
    return 1;
  }
}
