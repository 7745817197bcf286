// lin_host.cc — csrc/plant_tangent.h and csrc/tvlqr_step.h compiled for the host, as a stand-alone program that the tests
// drive through files (tests/lin_cases.py): the perturbed columns of a linearisation, the central difference of their
// rollouts, the Riccati recursion and the feedback law - the text that lin_perturb_kernel, lin_difference_kernel and
// tvlqr_kernel (csrc/plant_lin.h) compile for the device.  build.sh builds it as build/lin_host; the CPU tests compile it
// again with the address and undefined-behaviour sanitizers.
//
// usage: lin_host MODE IN OUT - IN and OUT are flat files of doubles (integers travel as doubles):
//   perturb     IN: nb nq nv eps | jtype[nb] qstart[nb] vstart[nb] | x[nq + nv] tau[nv]
//               OUT: [P][nq + nv + nv]: every column's q, v, tau
//   difference  IN: nb nq nv eps | jtype qstart vstart | finals [P][nq + nv]
//               OUT: A [n * n], B [n * nv] column-major
//   tvlqr       IN: S nv nu | actuated[nu] | A [S][n * n] B [S][n * nv] Q [n * n] R [nu * nu] Qf [n * n]
//               OUT: status | K [S][nu * n] | P [S + 1][n * n]
//   control     IN: nb nq nv nu | jtype qstart vstart | K [nu * n] x_nom[nq + nv] u_nom[nu] x[nq + nv]
//               OUT: u[nu]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tvlqr_step.h"

using namespace idto_plant;

static bool read_all(const char* path, std::vector<double>* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out->resize((size_t)bytes / sizeof(double));
  const size_t got = std::fread(out->data(), sizeof(double), out->size(), f);
  std::fclose(f);
  return got == out->size();
}
static bool write_all(const char* path, const std::vector<double>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const size_t put = std::fwrite(v.data(), sizeof(double), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}
static int fail(const char* what) { std::fprintf(stderr, "lin_host: %s\n", what); return 2; }

struct Tables { std::vector<int> jtype, qstart, vstart; };
static const double* read_tables(const double* p, int nb, Tables* t) {
  for (std::vector<int>* v : {&t->jtype, &t->qstart, &t->vstart}) {
    v->resize((size_t)nb);
    for (int i = 0; i < nb; ++i) (*v)[(size_t)i] = (int)p[i];
    p += nb;
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 4) return fail("usage: lin_host perturb|difference|tvlqr|control IN OUT");
  const std::string mode = argv[1];
  std::vector<double> in, out;
  if (!read_all(argv[2], &in)) return fail("cannot read IN");
  if (mode == "perturb" || mode == "difference") {
    if (in.size() < 4) return fail("IN is too short");
    const int nb = (int)in[0], nq = (int)in[1], nv = (int)in[2], w = nq + nv, n = 2 * nv, P = lin_columns(nv);
    const double eps = in[3];
    Tables t;
    if (in.size() < 4 + 3 * (size_t)nb) return fail("IN is too short");
    const double* p = read_tables(in.data() + 4, nb, &t);
    const size_t head = 4 + 3 * (size_t)nb;
    if (mode == "perturb") {
      if (in.size() != head + (size_t)w + nv) return fail("perturb: IN has the wrong size");
      const double* x = p;
      const double* tau = p + w;
      out.assign((size_t)P * (w + nv), 0.0);
      for (int col = 0; col < P; ++col) {
        double* c = out.data() + (size_t)col * (w + nv);
        for (int b = 0; b < nb; ++b) lin_perturb_body(t.jtype[b], t.qstart[b], t.vstart[b], nq, nv, col, eps, x, tau, c, c + nq, c + w);
      }
    } else {
      if (in.size() != head + (size_t)P * w) return fail("difference: IN has the wrong size");
      const double two_eps = 2.0 * eps;
      out.assign((size_t)n * n + (size_t)n * nv, 0.0);
      for (int j = 0; j < 3 * nv; ++j) {
        const double* xp = p + (size_t)(1 + 2 * j) * w;
        const double* xm = p + (size_t)(2 + 2 * j) * w;
        for (int b = 0; b < nb; ++b) lin_difference_body(t.jtype[b], t.qstart[b], t.vstart[b], nq, nv, two_eps, xp, xm, out.data() + (size_t)j * n);
      }
    }
  } else if (mode == "tvlqr") {
    if (in.size() < 3) return fail("IN is too short");
    const int S = (int)in[0], nv = (int)in[1], nu = (int)in[2], n = 2 * nv;
    const size_t nn = (size_t)n * n, want = 3 + (size_t)nu + S * nn + (size_t)S * n * nv + 2 * nn + (size_t)nu * nu;
    if (S < 1 || nv < 1 || nu < 1 || nu > nv || in.size() != want) return fail("tvlqr: IN has the wrong size");
    std::vector<int> act((size_t)nu);
    for (int i = 0; i < nu; ++i) {
      act[(size_t)i] = (int)in[3 + (size_t)i];
      if (act[(size_t)i] < 0 || act[(size_t)i] >= nv) return fail("tvlqr: an actuated index outside [0, nv)");
    }
    const double* A = in.data() + 3 + nu;
    const double* B = A + S * nn;
    const double* Q = B + (size_t)S * n * nv;
    const double* R = Q + nn;
    const double* Qf = R + (size_t)nu * nu;
    out.assign(1 + (size_t)S * nu * n + (size_t)(S + 1) * nn, 0.0);
    std::vector<double> work((size_t)tvlqr_step_work(n, nu) + nn + (size_t)n * nu);
    out[0] = (double)tvlqr_recursion(S, nv, nu, act.data(), A, B, Q, R, Qf, out.data() + 1, out.data() + 1 + (size_t)S * nu * n, work.data());
  } else if (mode == "control") {
    if (in.size() < 4) return fail("IN is too short");
    const int nb = (int)in[0], nq = (int)in[1], nv = (int)in[2], nu = (int)in[3], w = nq + nv, n = 2 * nv;
    if (in.size() != 4 + 3 * (size_t)nb + (size_t)nu * n + 2 * (size_t)w + nu) return fail("control: IN has the wrong size");
    Tables t;
    const double* K = read_tables(in.data() + 4, nb, &t);
    const double* x_nom = K + (size_t)nu * n;
    const double* u_nom = x_nom + w;
    const double* x = u_nom + nu;
    std::vector<double> dx((size_t)n);
    out.assign((size_t)nu, 0.0);
    tvlqr_control(nb, t.jtype.data(), t.qstart.data(), t.vstart.data(), nq, nv, nu, K, x_nom, u_nom, x, dx.data(), out.data());
  } else {
    return fail("unknown mode");
  }
  if (!write_all(argv[3], out)) return fail("cannot write OUT");
  return 0;
}
