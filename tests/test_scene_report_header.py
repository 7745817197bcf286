"""include/idto/optimizer/scene_report.h without a GPU: the header is self-contained C++17, SceneReport's accessors address the
layouts of include/idto_hip.h (IDTO_SCENE_BODY_DOUBLES, IDTO_SCENE_PAIR_*), and TrajectoryOptimizer declares EvalScene."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "idto/optimizer/trajectory_optimizer.h"
using idto::optimizer::SceneReport;
int main() {
  static_assert(IDTO_SCENE_BODY_DOUBLES == 18 && IDTO_SCENE_PAIR_DOUBLES == 20 && IDTO_SCENE_PAIR_PAD == 19, "layout");
  static_assert(IDTO_SCENE_PAIR_F + 3 == IDTO_SCENE_PAIR_PAD && IDTO_SCENE_PAIR_VT + 3 == IDTO_SCENE_PAIR_FN, "layout");
  SceneReport r;
  r.batch = 2; r.nstates = 3; r.nbodies = 4; r.npairs = 5; r.nv = 6;
  r.bodies.resize(2 * 3 * 4 * 18); r.pairs.resize(2 * 3 * 5 * 20); r.tau_contact.resize(2 * 3 * 6);
  for (size_t i = 0; i < r.bodies.size(); ++i) r.bodies[i] = (double)i;
  for (size_t i = 0; i < r.pairs.size(); ++i) r.pairs[i] = (double)i;
  for (size_t i = 0; i < r.tau_contact.size(); ++i) r.tau_contact[i] = (double)i;
  const size_t b = ((1 * 3 + 2) * 4 + 3) * 18, p = ((1 * 3 + 2) * 5 + 4) * 20;
  bool ok = r.R_WB(2, 3, 1)[0] == (double)b && r.p_WB(2, 3, 1)[0] == (double)(b + 9) && r.w_WB(2, 3, 1)[0] == (double)(b + 12) &&
            r.v_WB(2, 3, 1)[2] == (double)(b + 17);
  ok = ok && r.phi(2, 4, 1) == (double)(p + 1) && r.fn(2, 4, 1) == (double)(p + 15) && r.force(2, 4, 1)[2] == (double)(p + 18) &&
       r.active(2, 4, 1) && !r.active(0, 0, 0) && r.contact_torque(2, 1)[5] == (double)((1 * 3 + 2) * 6 + 5);
  // (declared: the optimizer's entry points and the view)
  using TO = idto::optimizer::TrajectoryOptimizer<double>;
  SceneReport (TO::*by_states)(const std::vector<idto::optimizer::VectorXd>&, const std::vector<idto::optimizer::VectorXd>&, bool) const = &TO::EvalScene;
  SceneReport (TO::*by_solution)(const idto::optimizer::TrajectoryOptimizerSolution<double>&, bool) const = &TO::EvalScene;
  return ok && by_states && by_solution && sizeof(idto::optimizer::Scene) > 0 ? 0 : 1;
}
'''


def test_scene_report_header_and_accessors(tmp_path):
    src = tmp_path / "t.cc"
    src.write_text(SRC)
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", os.path.join(ROOT, "idto_amd"), "-lidto_opt", "-lidto_hip", "-Wl,-rpath," + os.path.join(ROOT, "idto_amd")])
    assert subprocess.call([str(exe)]) == 0
