// cylinder_host_check.cc — signed_distance of csrc/id_eval.h, the unmodified device text, compiled for the host and called
// on the queries of a file: the sphere-cylinder rule of include/idto_model.h at states that need the sphere's centre bit
// for bit in the cylinder's frame (r == 0, the dr == dz tie, c.z == 0), which no model's kinematics delivers.  Built and
// run by tests/test_cylinder_host.py with the address and undefined-behaviour sanitizers; the comparison with the numpy
// restatement (tests/cylinder_ref.py) is made there.
//
// usage: cylinder_host_check QUERIES     a query: typeA RA[9] pA[3] sizeA[3] typeB RB[9] pB[3] sizeB[3]
// One line per query: valid phi n[3] Ca[3] Cb[3], the doubles with 17 significant digits.
#include <hip/hip_runtime.h>

#include "lane_emu/host_model.h"

namespace idto_dev {
constexpr size_t kLdsDoubles = 64;
alignas(64) double lds[kLdsDoubles];
}  // namespace idto_dev

using namespace lane_emu;

namespace {
struct Side {
  int type;
  idto_dev::M3 R;
  idto_dev::V3 p, s;
};
Side read_side(Tokens& in) {
  Side g;
  g.type = in.integer();
  for (int i = 0; i < 9; ++i) g.R.m[i] = in.num();
  const std::vector<double> v = in.nums(6);
  g.p = idto_dev::mk(v[0], v[1], v[2]);
  g.s = idto_dev::mk(v[3], v[4], v[5]);
  return g;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) die("usage: cylinder_host_check QUERIES");
  Tokens in(argv[1]);
  while (in.more()) {
    const Side A = read_side(in), B = read_side(in);
    const idto_dev::SdResult r = idto_dev::signed_distance(A.type, A.R, A.p, A.s, B.type, B.R, B.p, B.s);
    std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", (int)r.valid, r.phi, r.n.x, r.n.y, r.n.z,
                r.Ca.x, r.Ca.y, r.Ca.z, r.Cb.x, r.Cb.y, r.Cb.z);
  }
  return 0;
}
