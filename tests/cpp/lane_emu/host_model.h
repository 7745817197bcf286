// lane_emu/host_model.h — TEST INFRASTRUCTURE shared by tests/cpp/id_eval_host_check.cc and plant_body_host_check.cc: a
// model file as the DevModel the kernels read (built from host/model_tables.cc's tables exactly as idto_hip.hip
// UploadModel builds it, the pointers being host pointers), the CPU oracle on a model file, and the reader of the
// whitespace-separated case files that the Python side writes.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "host/model_batch.h"
#include "host/model_tables.h"
#include "id_eval.h"
#include "idto/model_file.h"
#include "rigid_body.h"

namespace lane_emu {

[[noreturn]] inline void die(const std::string& what) {
  std::fprintf(stderr, "FAILED: %s\n", what.c_str());
  std::exit(2);
}

struct HostModel {
  idto::ModelFile mf;
  idto_host::ModelTables t;
  idto_dev::DevModel M;
  int maxc = 1;
  // the two X-macro lists, then the scalars: idto_hip.hip UploadModel
  void Point(const double* bd) {
    const int* bi = reinterpret_cast<const int*>(bd);
    M.blob = bd; M.blob_n = (int)t.blob.size();
#define X(name) M.name = bd + t.at.name;
    IDTO_MODEL_DOUBLE_TABLES(X)
#undef X
#define X(name) M.name = bi + t.at.name;
    IDTO_MODEL_INT_TABLES(X)
#undef X
  }
  explicit HostModel(const std::string& path) : mf(idto::ModelFile::Load(path)) {
    const idto_model_t m = mf.c_model();
    std::string err;
    if (idto_host::BuildModelTables(&m, &t, &err)) die(path + ": " + err);
    std::memset(&M, 0, sizeof(M));
    Point(t.blob.data());
    M.nb = m.nbodies; M.nq = m.nq; M.nv = m.nv; M.npaths = m.npaths; M.common_body = m.common_body;
    M.ngeoms = m.ngeoms; M.npairs = m.npairs; M.maxpp = t.maxpp;
    for (int i = 0; i < 3; ++i) M.gravity[i] = m.gravity[i];
    M.nfloat = t.nfloat;
    for (int i = 0; i < 4; ++i) { M.float_qs[i] = t.float_qs[i]; M.float_vs[i] = t.float_vs[i]; }
    M.fast_shape = t.fast_shape; M.fast_lo = t.fast_lo; M.fast_n = t.fast_n; M.f_maxpp = t.f_maxpp;
    M.gslots = t.gslots; M.gcommon = t.gcommon; M.gstem = t.gstem; M.nxb = t.nxb; M.nstem = t.nstem;
    maxc = t.maxc;
  }
  // the instantiation fd_launch.hip / plant_launch.hip pick for the generic evaluation: by nstem, nxb and maxc
  const char* Instantiation() const {
    if (M.nstem > 1) return "8xs";
    if (M.nxb) return "8x";
    return maxc <= 2 ? "2" : (maxc <= 3 ? "3" : (maxc <= 4 ? "4" : "8"));
  }
};

// the contact parameters as the device reads them (host/model_batch.h: the threshold's one expression) and as the oracle does
inline idto_dev::DevContact DevContactOf(const double c[5]) {
  idto_contact_params_t p{};
  p.contact_stiffness = c[0]; p.dissipation_velocity = c[1]; p.stiction_velocity = c[2]; p.friction_coefficient = c[3];
  p.smoothing_factor = c[4];
  double v[6];
  idto_host::ContactValues(p, v);
  return idto_dev::DevContact{v[0], v[1], v[2], v[3], v[4], v[5]};
}
inline std::unique_ptr<oracle::Dynamics> OracleOf(const std::string& path, const double c[5]) {
  const idto::ModelFile mf = idto::ModelFile::Load(path);
  auto d = std::make_unique<oracle::Dynamics>();
  d->model.FromC(mf.c_model());
  d->contact.k = c[0]; d->contact.vd = c[1]; d->contact.vs = c[2]; d->contact.mu = c[3]; d->contact.sigma = c[4];
  d->contact.Finalize();
  return d;
}

struct Tokens {
  std::vector<std::string> tok;
  size_t pos = 0;
  explicit Tokens(const std::string& path) {
    std::ifstream in(path);
    if (!in) die("cannot open " + path);
    std::stringstream ss;
    ss << in.rdbuf();
    for (std::string t; ss >> t;) tok.push_back(t);
  }
  bool more() const { return pos < tok.size(); }
  const std::string& next() {
    if (pos >= tok.size()) die("the case file ends early");
    return tok[pos++];
  }
  void expect(const char* s) {
    const std::string& t = next();
    if (t != s) die(std::string("the case file: expected '") + s + "', got '" + t + "'");
  }
  double num() { return std::strtod(next().c_str(), nullptr); }   // ("nan" and "inf" included)
  int integer() { return std::atoi(next().c_str()); }
  std::vector<double> nums(int n) { std::vector<double> v(n); for (double& x : v) x = num(); return v; }
};

// a == b as bits would have it for the numbers that occur: both NaN counts as equal, -0 == +0 as the tests' `==` does
inline bool same(double a, double b) { return a == b || (a != a && b != b); }
inline bool same(const double* a, const double* b, int n) {
  for (int i = 0; i < n; ++i) if (!same(a[i], b[i])) return false;
  return true;
}

}  // namespace lane_emu
