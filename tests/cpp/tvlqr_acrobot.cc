// A C++ consumer of TrajectoryOptimizer::Tvlqr and ::LinearizePlant (include/idto/optimizer/tvlqr.h) with no Python in the
// process: the acrobot example's problem at N = 5, a few iterations of Solve, then the time-varying LQR gains about the
// solution in substeps of time_step / 4.  It prints the solution and everything the call returned with 17 significant
// digits; tests/test_gpu_tvlqr_cpp.py runs it on the GPU and holds the printed numbers to the Python route on the same states.
//
// usage: tvlqr_acrobot <path to acrobot.model>
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
  if (argc < 2) { std::fprintf(stderr, "usage: tvlqr_acrobot <acrobot.model>\n"); return 2; }
  try {
    const idto::ModelFile mf = idto::ModelFile::Load(argv[1]);
    const int N = 5, nq = mf.nq, nv = mf.nv;
    const double dt = 0.05;
    ProblemDefinition prob;
    prob.num_steps = N;
    prob.q_init = {0.3, -0.2};
    prob.v_init = {0.0, 0.1};
    prob.Qq = MatrixXd::Diagonal({1.0, 1.0});
    prob.Qv = MatrixXd::Diagonal({1.0, 1.0});
    prob.R = MatrixXd::Diagonal({1e3, 0.1});
    prob.Qf_q = MatrixXd::Diagonal({100.0, 100.0});
    prob.Qf_v = MatrixXd::Diagonal({1.0, 1.0});
    for (int t = 0; t <= N; ++t) { prob.q_nom.push_back({3.1415, 0.0}); prob.v_nom.push_back({0.0, 0.0}); }
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

    const MatrixXd Qtheta = MatrixXd::Diagonal({10.0, 10.0}), Qv = MatrixXd::Diagonal({1.0, 1.0});
    const MatrixXd Qf_theta = MatrixXd::Diagonal({100.0, 100.0}), Qf_v = MatrixXd::Diagonal({10.0, 10.0});
    const std::vector<int> act = opt.actuated_dofs();
    std::printf("actuated");
    for (int j : act) std::printf(" %d", j);
    std::printf("\n");
    const MatrixXd R = MatrixXd::Diagonal(VectorXd(act.size(), 0.1));
    const TvlqrGains g = opt.Tvlqr(solution, dt / 4, Qtheta, Qv, R, Qf_theta, Qf_v);
    std::printf("lqr_status %d lin_ok %d\n", g.status[0], (int)g.lin.ok());
    const std::size_t n = 2 * (std::size_t)nv;
    for (int t = 0; t < N; ++t) {
      row("x_next", t, g.lin.x_next[g.lin.at(t)].data(), (std::size_t)nq + nv);
      row("A", t, g.lin.A[g.lin.at(t)].data(), n * n);
      row("B", t, g.lin.B[g.lin.at(t)].data(), n * nv);
      row("K", t, g.K[(std::size_t)t].data(), act.size() * n);
    }
    for (int t = 0; t <= N; ++t) row("P", t, g.cost_to_go(t).data(), n * n);
    // LinearizePlant on the same states is the linearisation inside
    std::vector<VectorXd> q(solution.q.begin(), solution.q.begin() + N), v(solution.v.begin(), solution.v.begin() + N);
    const PlantLinearization l = opt.LinearizePlant(q, v, solution.tau, dt / 4, 4);
    bool same = l.ok() && l.status == g.lin.status;
    for (int t = 0; t < N && same; ++t) {
      for (std::size_t i = 0; i < n * n; ++i) same = same && l.A[(std::size_t)t].data()[i] == g.lin.A[(std::size_t)t].data()[i];
      for (std::size_t i = 0; i < n * nv; ++i) same = same && l.B[(std::size_t)t].data()[i] == g.lin.B[(std::size_t)t].data()[i];
      same = same && l.x_next[(std::size_t)t] == g.lin.x_next[(std::size_t)t];
    }
    std::printf("linearize_plant_same %d\n", (int)same);
    // a substep that does not divide the time step is refused
    try {
      opt.Tvlqr(solution, dt / 4.5, Qtheta, Qv, R, Qf_theta, Qf_v);
      std::printf("refused 0\n");
    } catch (const std::invalid_argument& e) {
      std::printf("refused 1 %s\n", e.what());
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "tvlqr_acrobot: %s\n", e.what());
    return 1;
  }
}
