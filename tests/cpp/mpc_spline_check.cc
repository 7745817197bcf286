// mpc_spline_check.cc — csrc/mpc_spline.h on the CPU, as a stand-alone program (tests/test_mpc_spline.py builds it with
// the address and undefined-behaviour sanitizers and runs it):
//   * against tests/golden/mpc_spline.json + .f64 - what idto_mpc_spline_eval returned BEFORE the header existed - with ==;
//   * against the spline's defining properties over seeded inputs: it interpolates the knots, the first and second
//     derivatives are continuous at the interior knots, the third at the second and the second-to-last knot (not-a-knot),
//     two knots give the line and three the parabola, times outside the breaks evaluate at the nearest break;
//   * the nominal shift with a selector of mixed entries: an entry that is not selected comes back bit for bit;
//   * the guess time and the control rows.
// Tolerances of the property checks (the golden check has none): a piece's k-th derivative is of the size Y / h^k (Y = max |y|,
// h = the smallest interval) and comes out of a diagonally dominant tridiagonal solve plus a handful of operations: round-off
// of a modest multiple of eps Y / h^k.  The bound is 1e-9 Y / h^k = 4.5e6 eps: far above that, and far below the O(1) x Y / h^k
// by which a wrong coefficient, a swapped interval or a natural instead of a not-a-knot end condition is off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "mpc_spline.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                                          \
  do {                                                                            \
    if (!(cond)) {                                                                \
      if (++g_fail <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                             \
  } while (0)

struct Spline {
  int n = 0, dim = 0;
  std::vector<double> t, y, m, w;
  int Fit() {
    m.assign((size_t)n * dim, 0.0);
    w.assign((size_t)n * dim, 0.0);
    int rc = 0;
    for (int c = 0; c < dim; ++c) rc |= idto_spline::spline_fit(t.data(), n, y.data() + c, m.data() + c, w.data() + c, dim);
    return rc;
  }
  double Value(int c, double time) const { return idto_spline::spline_value(t.data(), n, y.data() + c, m.data() + c, dim, time); }
  // the k-th derivative (k = 0 .. 3) of piece i at the offset s from its left break
  double Piece(int i, int c, double s, int k) const {
    const double h = t[i + 1] - t[i];
    const double y0 = y[(size_t)i * dim + c], y1 = y[(size_t)(i + 1) * dim + c];
    const double m0 = m[(size_t)i * dim + c], m1 = m[(size_t)(i + 1) * dim + c];
    const double d = (y1 - y0) / h, c2 = (3 * d - 2 * m0 - m1) / h, c3 = (m0 + m1 - 2 * d) / (h * h);
    if (k == 0) return y0 + s * (m0 + s * (c2 + s * c3));
    if (k == 1) return m0 + s * (2 * c2 + 3 * s * c3);
    if (k == 2) return 2 * c2 + 6 * s * c3;
    return 6 * c3;
  }
};

// tests/golden/mpc_spline.f64 holds the numbers - per case, from its offset in doubles, breaks[n], knots[n][dim], times[nt],
// values[nt][dim] as little-endian float64 -, the command line the index of mpc_spline.json: n dim nt offset per case
int CheckGolden(const char* data_path, int nargs, char** args) {
  std::ifstream fd(data_path, std::ios::binary);
  if (!fd || nargs % 4 != 0) { std::printf("cannot read %s, or an index that is not n dim nt offset per case\n", data_path); return -1; }
  std::stringstream sd;
  sd << fd.rdbuf();
  const std::string raw = sd.str();
  std::vector<double> D(raw.size() / sizeof(double));
  std::memcpy(D.data(), raw.data(), D.size() * sizeof(double));
  long long values = 0;
  for (int cs = 0; cs < nargs / 4; ++cs) {
    Spline sp;
    sp.n = std::atoi(args[4 * cs]); sp.dim = std::atoi(args[4 * cs + 1]);
    const int nt = std::atoi(args[4 * cs + 2]);
    const size_t off = (size_t)std::atoll(args[4 * cs + 3]), nk = (size_t)sp.n * sp.dim, nv = (size_t)nt * sp.dim;
    if (sp.n < 2 || sp.dim < 1 || nt < 1 || off + sp.n + nk + nt + nv > D.size()) { std::printf("golden case %d: outside the data\n", cs); return -1; }
    const double* p = D.data() + off;
    sp.t.assign(p, p + sp.n); p += sp.n;
    sp.y.assign(p, p + nk); p += nk;
    const std::vector<double> times(p, p + nt), want(p + nt, p + nt + nv);
    CHECK(sp.Fit() == 0, "golden case %d: singular", cs);
    for (int k = 0; k < nt; ++k)
      for (int c = 0; c < sp.dim; ++c, ++values) {
        const double got = sp.Value(c, times[k]);
        CHECK(got == want[(size_t)k * sp.dim + c], "golden case %d (n %d dim %d) time %d comp %d: %.17g != %.17g", cs, sp.n, sp.dim, k, c,
              got, want[(size_t)k * sp.dim + c]);
      }
  }
  std::printf("golden: %d cases, %lld values\n", nargs / 4, values);
  return (values == 10902) ? nargs / 4 : -1;
}

Spline Seeded(std::mt19937_64& rng, int n, int dim, int kind) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::normal_distribution<double> g(0.0, 1.0);
  Spline sp;
  sp.n = n; sp.dim = dim;
  sp.t.resize(n);
  double acc = -0.25;
  for (int i = 0; i < n; ++i) {
    if (kind == 0) sp.t[i] = i * 0.05;
    else if (kind == 1) sp.t[i] = i * 0.01;
    else { acc += 0.003 + 0.197 * u(rng); sp.t[i] = acc; }
  }
  sp.y.resize((size_t)n * dim);
  for (int c = 0; c < dim; ++c) {
    const double scale = (c % 3 == 0) ? 1e-3 : (c % 3 == 1 ? 1.0 : 40.0);
    for (int i = 0; i < n; ++i) sp.y[(size_t)i * dim + c] = scale * g(rng);
  }
  return sp;
}

void CheckProperties() {
  std::mt19937_64 rng(7321);
  const double rel = 1e-9;
  for (int n : {2, 3, 4, 5, 6, 7, 21, 41})
    for (int dim : {1, 3, 19})
      for (int kind = 0; kind < 3; ++kind) {
        Spline sp = Seeded(rng, n, dim, kind);
        CHECK(sp.Fit() == 0, "n %d: singular", n);
        double hmin = 1e300;
        for (int i = 0; i + 1 < n; ++i) hmin = std::fmin(hmin, sp.t[i + 1] - sp.t[i]);
        for (int c = 0; c < dim; ++c) {
          double Y = 0;
          for (int i = 0; i < n; ++i) Y = std::fmax(Y, std::fabs(sp.y[(size_t)i * dim + c]));
          const double tol[4] = {rel * Y, rel * Y / hmin, rel * Y / (hmin * hmin), rel * Y / (hmin * hmin * hmin)};
          // the knots: a piece starts at its left knot's value exactly (s = 0) and ends at the right knot's to round-off
          for (int i = 0; i < n; ++i) {
            const double at = sp.Value(c, sp.t[i]);
            if (i + 1 < n) CHECK(at == sp.y[(size_t)i * dim + c], "n %d knot %d: value %.17g, knot %.17g", n, i, at, sp.y[(size_t)i * dim + c]);
            else CHECK(std::fabs(at - sp.y[(size_t)i * dim + c]) <= tol[0], "n %d last knot: off by %.3g", n, at - sp.y[(size_t)i * dim + c]);
          }
          for (int i = 0; i + 2 < n; ++i) {   // interior knot i + 1: pieces i and i + 1
            const double h = sp.t[i + 1] - sp.t[i];
            for (int k = 0; k <= 2; ++k) {
              const double gap = sp.Piece(i, c, h, k) - sp.Piece(i + 1, c, 0.0, k);
              CHECK(std::fabs(gap) <= tol[k], "n %d dim %d kind %d knot %d: derivative %d jumps by %.3g (tol %.3g)", n, dim, kind, i + 1, k, gap, tol[k]);
            }
          }
          if (n >= 4) {   // not-a-knot: the third derivative is continuous at the second and the second-to-last knot
            const double g0 = sp.Piece(0, c, 0, 3) - sp.Piece(1, c, 0, 3), g1 = sp.Piece(n - 3, c, 0, 3) - sp.Piece(n - 2, c, 0, 3);
            CHECK(std::fabs(g0) <= tol[3] && std::fabs(g1) <= tol[3], "n %d dim %d kind %d: third derivative jumps by %.3g / %.3g (tol %.3g)", n, dim,
                  kind, g0, g1, tol[3]);
          }
          if (n == 2) {   // the line: both knot derivatives are the slope, the cubic and quadratic coefficients vanish
            const double d = (sp.y[dim + c] - sp.y[c]) / (sp.t[1] - sp.t[0]);
            CHECK(sp.m[c] == d && sp.m[dim + c] == d, "n 2: knot derivatives are not the slope");
            const double mid = 0.5 * (sp.t[0] + sp.t[1]);
            CHECK(std::fabs(sp.Value(c, mid) - (sp.y[c] + d * (mid - sp.t[0]))) <= tol[0], "n 2: not the line");
          }
          if (n == 3) {   // the parabola through the three points (Lagrange form), no cubic term
            CHECK(std::fabs(sp.Piece(0, c, 0, 3)) <= tol[3] && std::fabs(sp.Piece(1, c, 0, 3)) <= tol[3], "n 3: a cubic term");
            const double t0 = sp.t[0], t1 = sp.t[1], t2 = sp.t[2], y0 = sp.y[c], y1 = sp.y[dim + c], y2 = sp.y[2 * dim + c];
            for (double f : {0.13, 0.5, 0.77, 1.31, 1.9}) {
              const double x = t0 + f * 0.5 * (t2 - t0);
              const double L = y0 * (x - t1) * (x - t2) / ((t0 - t1) * (t0 - t2)) + y1 * (x - t0) * (x - t2) / ((t1 - t0) * (t1 - t2)) +
                               y2 * (x - t0) * (x - t1) / ((t2 - t0) * (t2 - t1));
              // (Lagrange's own round-off grows with the ratio of the two intervals: the non-uniform kind's bound)
              CHECK(std::fabs(sp.Value(c, x) - L) <= tol[0] * ((t2 - t0) / hmin) * ((t2 - t0) / hmin), "n 3 kind %d: not the parabola: %.3g", kind,
                    sp.Value(c, x) - L);
            }
          }
          // the clamp: outside the breaks' range the value is the one at the nearest break, bit for bit
          CHECK(sp.Value(c, sp.t[0] - 0.37) == sp.Value(c, sp.t[0]) && sp.Value(c, sp.t[0] - 1e9) == sp.Value(c, sp.t[0]), "n %d: below the range", n);
          CHECK(sp.Value(c, sp.t[n - 1] + 1.9) == sp.Value(c, sp.t[n - 1]) && sp.Value(c, 1e300) == sp.Value(c, sp.t[n - 1]), "n %d: above the range", n);
        }
        // the interval of a time on a knot is the one that begins there; of the last knot, the last one
        for (int i = 0; i < n; ++i) {
          double x = sp.t[i];
          const int iv = idto_spline::spline_interval(sp.t.data(), n, &x);
          CHECK(iv == (i < n - 1 ? i : n - 2) && x == sp.t[i], "n %d: knot %d falls into interval %d", n, i, iv);
        }
        double below = sp.t[0] - 1.0, above = sp.t[n - 1] + 1.0;
        CHECK(idto_spline::spline_interval(sp.t.data(), n, &below) == 0 && below == sp.t[0], "clamp below");
        CHECK(idto_spline::spline_interval(sp.t.data(), n, &above) == n - 2 && above == sp.t[n - 1], "clamp above");
      }
}

void CheckShell() {
  std::mt19937_64 rng(99);
  std::normal_distribution<double> g(0.0, 1.0);
  // the nominal shift, selector of mixed entries
  const int nq = 7, rows = 5;
  const bool sel[nq] = {true, false, false, true, false, true, false};
  std::vector<double> q_nom((size_t)rows * nq), q0(nq);
  for (double& x : q_nom) x = g(rng);
  for (double& x : q0) x = 3 * g(rng);
  q_nom[1] = 0.0;   // (an exact zero that is not selected)
  const std::vector<double> before = q_nom;
  const std::vector<double> old0(before.begin(), before.begin() + nq);
  for (int t = 0; t < rows; ++t)
    for (int i = 0; i < nq; ++i) q_nom[(size_t)t * nq + i] = idto_spline::nominal_shift(q_nom[(size_t)t * nq + i], sel[i], q0[i], old0[i]);
  for (int t = 0; t < rows; ++t)
    for (int i = 0; i < nq; ++i) {
      const double now = q_nom[(size_t)t * nq + i], was = before[(size_t)t * nq + i];
      if (!sel[i]) CHECK(std::memcmp(&now, &was, sizeof now) == 0, "shift: entry (%d, %d) is not selected and changed", t, i);
      else CHECK(now == was + 1.0 * (q0[i] - old0[i]) && now != was, "shift: entry (%d, %d)", t, i);
    }
  for (int i = 0; i < nq; ++i)
    if (sel[i]) CHECK(std::fabs(q_nom[i] - q0[i]) <= 4e-16 * (std::fabs(q0[i]) + std::fabs(old0[i])), "shift: row 0 of a selected entry is not q0");
  // the guess time: start + i * dt in that order
  const double start = 0.123456789, dt = 0.05;
  for (int i = 0; i < 50; ++i) {
    const double prod = i * dt;
    CHECK(idto_spline::guess_time(start, i, dt) == start + prod, "guess_time %d", i);
  }
  // control rows: min(i, N - 1) of N = knots - 1 rows of torques
  for (int knots : {2, 3, 4, 21})
    for (int i = 0; i < knots; ++i) CHECK(idto_spline::control_row(i, knots) == (i < knots - 2 ? i : knots - 2), "control_row(%d, %d)", i, knots);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: mpc_spline_check tests/golden/mpc_spline.f64 {n dim nt offset}\n"); return 2; }
  const int cases = CheckGolden(argv[1], argc - 2, argv + 2);
  if (cases != 54) { std::printf("FAIL: %d golden cases read, 54 expected\n", cases); return 1; }
  CheckProperties();
  CheckShell();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("ok: mpc_spline.h agrees with the recorded values and has its defining properties\n");
  return 0;
}
