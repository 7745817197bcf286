// plant_step_check.cc — csrc/plant_step.h on the CPU, stand-alone (tests/test_plant_step.py compiles it with the address
// and undefined-behaviour sanitizers and runs it).  What it checks, and with which bounds:
//   1. plant_ldlt_solve on SPD systems of order 1, 2, 3, 19, 23 (A = G G^T + n I, G uniform in [-1, 1]): the solution put
//      back into the matrix, |A x - b|_inf <= 8 n eps (|A|_inf |x|_inf + |b|_inf) - the backward bound of an LDL^T of an
//      SPD matrix is c n eps |A| |x| with a modest c; and the row form driven pivot by pivot, the way a lane per row
//      drives it, gives the serial form's bits (==).
//   2. an indefinite matrix returns the index of its first non-positive pivot, a NaN entry the pivot it reaches.
//   3. N+(q) N(q) v = v for random unit quaternions, N+ the block L(2 q~)^T (I - q~ q~^T) / |q| of the kernels' nplus_block
//      restated here: within 16 eps |v|_inf (a dozen products and sums of numbers of size <= 2 |v|).
//   4. after plant_advance the quaternion of a floating joint has norm 1 within 4 eps (the norm's sum and root: 1.5 eps, the
//      division: 0.5 eps, this check's own norm: 1.5 eps), the other joints are the plain
//      Euler expressions (==), and v+ = v + h a (==).
//   5. plant_time(t0, s, h) == t0 + s * h, and differs from the accumulated sum where that one has drifted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "plant_step.h"

using namespace idto_plant;

static int g_fail = 0;
#define CHECK(cond, ...)                                                      \
  do {                                                                        \
    if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

static unsigned long long g_seed = 0x9E3779B97F4A7C15ull;
static double uni() {   // (-1, 1)
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return ((double)(g_seed >> 11) / 9007199254740992.0) * 2.0 - 1.0;
}
static const double eps = std::numeric_limits<double>::epsilon();

static void spd(int n, std::vector<double>* A) {
  std::vector<double> G((size_t)n * n);
  for (double& g : G) g = uni();
  A->assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = (i == j) ? (double)n : 0.0;
      for (int k = 0; k < n; ++k) s += G[(size_t)k * n + i] * G[(size_t)k * n + j];
      (*A)[(size_t)j * n + i] = s;
    }
}

static void check_solves() {
  for (int n : {1, 2, 3, 19, 23}) {
    std::vector<double> A, b((size_t)n), work((size_t)n);
    spd(n, &A);
    for (double& x : b) x = 10.0 * uni();
    std::vector<double> F = A, x = b;
    const int piv = plant_ldlt_solve(F.data(), n, x.data(), work.data());
    CHECK(piv == -1, "order %d: pivot %d refused", n, piv);
    double an = 0, xn = 0, bn = 0, res = 0;
    for (int i = 0; i < n; ++i) {
      double row = 0, r = -b[(size_t)i];
      for (int j = 0; j < n; ++j) { row += std::fabs(A[(size_t)j * n + i]); r += A[(size_t)j * n + i] * x[(size_t)j]; }
      an = std::fmax(an, row); xn = std::fmax(xn, std::fabs(x[(size_t)i])); bn = std::fmax(bn, std::fabs(b[(size_t)i]));
      res = std::fmax(res, std::fabs(r));
    }
    CHECK(res <= 8.0 * n * eps * (an * xn + bn), "order %d: residual %.3e", n, res);
    // the upper triangle is never read: NaN there, and the rows driven the way the device drives them, last row first
    std::vector<double> L = A, y = b, col((size_t)n);
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) L[(size_t)j * n + i] = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < n; ++k) {
      const double d = L[(size_t)k * n + k];
      for (int i = k + 1; i < n; ++i) col[(size_t)i] = L[(size_t)k * n + i];
      for (int i = n - 1; i > k; --i) plant_ldlt_row(L.data(), n, y.data(), col.data(), d, k, i);
    }
    for (int i = n - 1; i >= 0; --i) y[(size_t)i] = y[(size_t)i] / L[(size_t)i * n + i];
    for (int k = n - 1; k >= 1; --k) {
      for (int i = k - 1; i >= 0; --i) plant_ldlt_back_row(L.data(), n, y.data(), y[(size_t)k], k, i);
    }
    for (int i = 0; i < n; ++i) CHECK(y[(size_t)i] == x[(size_t)i], "order %d: row form differs in entry %d", n, i);
  }
}

static void check_refusals() {
  const int n = 5;
  std::vector<double> A, b((size_t)n, 1.0), work((size_t)n);
  spd(n, &A);
  std::vector<double> F = A, x = b;
  F[(size_t)2 * n + 2] = -100.0;   // pivot 2 goes negative whatever the first two eliminations subtract
  CHECK(plant_ldlt_solve(F.data(), n, x.data(), work.data()) == 2, "indefinite matrix: wrong pivot");
  F = A; x = b;
  F[(size_t)1 * n + 3] = std::numeric_limits<double>::quiet_NaN();   // entry (3, 1): reaches pivot 3 behind pivot 1
  CHECK(plant_ldlt_solve(F.data(), n, x.data(), work.data()) == 3, "NaN entry: wrong pivot");
  F = A; x = b;
  F[0] = std::numeric_limits<double>::infinity();
  CHECK(plant_ldlt_solve(F.data(), n, x.data(), work.data()) == 0, "infinite pivot accepted");
  F = A; x = b;
  F[0] = 0.0;
  CHECK(plant_ldlt_solve(F.data(), n, x.data(), work.data()) == 0, "zero pivot accepted");
}

// the 3 x 4 block of N+ for the quaternion qq (any norm): acc(r, c) = sum_i LT(r, i) D(i, c), as the kernels form it
static void nplus_quat(const double* qq, double N[3][4]) {
  const double nrm = std::sqrt(((qq[0] * qq[0] + qq[1] * qq[1]) + qq[2] * qq[2]) + qq[3] * qq[3]);
  const double t[4] = {qq[0] / nrm, qq[1] / nrm, qq[2] / nrm, qq[3] / nrm};
  const double w2 = 2.0 * t[0], x2 = 2.0 * t[1], y2 = 2.0 * t[2], z2 = 2.0 * t[3];
  const double LT[3][4] = {{-x2, w2, -z2, y2}, {-y2, z2, w2, -x2}, {-z2, -y2, x2, w2}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double acc = 0;
      for (int i = 0; i < 4; ++i) acc += LT[r][i] * (((i == c ? 1.0 : 0.0) - t[i] * t[c]) / nrm);
      N[r][c] = acc;
    }
}

static void check_qdot_and_advance() {
  for (int trial = 0; trial < 200; ++trial) {
    // a model of three bodies: revolute (q 0, v 0), floating (q 1..7, v 1..6), planar (q 8..10, v 7..9)
    const int jtype[3] = {IDTO_JOINT_REVOLUTE, IDTO_JOINT_FLOATING, IDTO_JOINT_PLANAR}, qstart[3] = {0, 1, 8}, vstart[3] = {0, 1, 7};
    double q[11], v[10], a[10], qdot[11];
    for (double& x : q) x = uni();
    for (double& x : v) x = 3.0 * uni();
    for (double& x : a) x = 30.0 * uni();
    double nrm = std::sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + q[4] * q[4]);
    for (int i = 1; i <= 4; ++i) q[i] /= nrm;
    for (int b = 0; b < 3; ++b) plant_qdot(jtype[b], qstart[b], vstart[b], q, v, qdot);
    double N[3][4], vn = 0;
    nplus_quat(q + 1, N);
    for (int r = 0; r < 3; ++r) vn = std::fmax(vn, std::fabs(v[1 + r]));
    for (int r = 0; r < 3; ++r) {
      double s = 0;
      for (int c = 0; c < 4; ++c) s += N[r][c] * qdot[1 + c];
      CHECK(std::fabs(s - v[1 + r]) <= 16 * eps * vn, "N+ N v: row %d off by %.3e", r, std::fabs(s - v[1 + r]));
    }
    for (int i = 0; i < 3; ++i) CHECK(qdot[5 + i] == v[4 + i], "floating joint: position rate");
    CHECK(qdot[0] == v[0] && qdot[8] == v[7] && qdot[9] == v[8] && qdot[10] == v[9], "identity joints");

    const double h = 1e-3 * (1.5 + uni());
    double q1[11], v1[10];
    for (int i = 0; i < 11; ++i) q1[i] = q[i];
    for (int i = 0; i < 10; ++i) v1[i] = v[i];
    plant_advance(3, jtype, qstart, vstart, h, q1, v1, a, qdot);
    for (int i = 0; i < 10; ++i) CHECK(v1[i] == v[i] + h * a[i], "v+ entry %d", i);
    nrm = std::sqrt(((q1[1] * q1[1] + q1[2] * q1[2]) + q1[3] * q1[3]) + q1[4] * q1[4]);
    CHECK(std::fabs(nrm - 1.0) <= 4 * eps, "quaternion norm %.17g after the step", nrm);
    CHECK(q1[0] == q[0] + h * v1[0], "revolute q+");
    for (int i = 0; i < 3; ++i) {
      CHECK(q1[8 + i] == q[8 + i] + h * v1[7 + i], "planar q+");
      CHECK(q1[5 + i] == q[5 + i] + h * v1[4 + i], "floating position q+");
    }
  }
}

static void check_time() {
  const double t0 = 0.3, h = 1e-3 / 3;
  double acc = t0;
  bool drifted = false;
  for (int s = 0; s <= 4096; ++s) {
    const double t = plant_time(t0, s, h);
    CHECK(t == t0 + (double)s * h, "plant_time at %d", s);
    drifted = drifted || t != acc;
    acc += h;
  }
  CHECK(drifted, "the accumulated time never left the formula's: the check shows nothing");
  CHECK(plant_finite(1.0) && plant_finite(-0.0) && !plant_finite(std::numeric_limits<double>::infinity()) &&
        !plant_finite(-std::numeric_limits<double>::infinity()) && !plant_finite(std::numeric_limits<double>::quiet_NaN()), "plant_finite");
}

static void check_pd_plus() {
  const int nu = 2, nq = 3, nv = 3, act[2] = {2, 0};
  const double Kp[6] = {1, 2, 3, 4, 5, 6}, Kd[6] = {0.5, 0.25, 0.125, 7, 8, 9};
  const double q[3] = {0.1, 0.2, 0.3}, v[3] = {1, 2, 3}, qn[3] = {0.4, 0.1, 0.9}, vn[3] = {0, 1, 5}, un[2] = {10, 20};
  double tau[3];
  plant_pd_plus(Kp, Kd, nu, nq, nv, act, q, v, qn, vn, true, un, tau);
  for (int r = 0; r < nu; ++r) {
    const double p = (Kp[r * 3] * (qn[0] - q[0]) + Kp[r * 3 + 1] * (qn[1] - q[1])) + Kp[r * 3 + 2] * (qn[2] - q[2]);
    const double d = (Kd[r * 3] * (vn[0] - v[0]) + Kd[r * 3 + 1] * (vn[1] - v[1])) + Kd[r * 3 + 2] * (vn[2] - v[2]);
    CHECK(tau[act[r]] == (p + d) + un[r], "PD+ row %d", r);
  }
  CHECK(tau[1] == 0.0, "an unactuated dof got a torque");
  plant_pd_plus(Kp, Kd, nu, nq, nv, act, q, v, qn, vn, false, nullptr, tau);
  const double p0 = (Kp[0] * (qn[0] - q[0]) + Kp[1] * (qn[1] - q[1])) + Kp[2] * (qn[2] - q[2]);
  const double d0 = (Kd[0] * (vn[0] - v[0]) + Kd[1] * (vn[1] - v[1])) + Kd[2] * (vn[2] - v[2]);
  CHECK(tau[2] == p0 + d0, "PD without the nominal control");
}

int main() {
  check_solves();
  check_refusals();
  check_qdot_and_advance();
  check_time();
  check_pd_plus();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("\nok: plant_step.h\n");
  return 0;
}
