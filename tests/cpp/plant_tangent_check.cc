// plant_tangent_check.cc — csrc/plant_tangent.h on the CPU, stand-alone (tests/test_plant_tangent.py compiles it with the
// address and undefined-behaviour sanitizers and runs it).  What it checks, and with which bounds:
//   1. tangent_sub(tangent_add(q, d), q) == d for revolute, prismatic and planar joints at values where q + d - q is exact
//      (dyadic q and d of comparable size: every sum and difference is representable).
//   2. the same for a floating joint at random unit quaternions and |d| = 1e-6 (angular and linear parts each): within 1e-11
//      per component - what tangent_sub drops is cubic, |d|^3 / 8 = 1.3e-19 from the normalisation of 1 + |d|^2 / 4 plus
//      |d|^3 / 24 against the exact logarithm; the rest is the round-off of a dozen operations on entries of size <= 1, a few
//      1e-16 absolute.
//   3. tangent_add(q, 0) == q bit for bit for quaternions whose norm expression evaluates to exactly 1 - the identity, and those
//      of 200 random ones, normalised with plant_advance_body's expression up to four times, that reach it (at least a quarter
//      must: the norm expression of a normalised quaternion is 1 within 2 ulp, and no quotient moves where it is 1).  For the
//      others the quotient by a norm of 1 +- 2 ulp moves an entry by at most 4 eps.
//   4. the branch d.w < 0: tangent_sub(-(q (+) d), q) == tangent_sub(q (+) d, q) bit for bit (q and -q are one rotation), with
//      d.w < 0 asserted for the first.
//   5. lin_perturb_body's columns: column 0 is (x, tau) bit for bit; the pair of component k differs from it in that component
//      alone (velocity, torque: x +- eps exactly; position of a revolute joint: q +- eps exactly); lin_difference_body of a
//      column pair of the identity map gives the unit vector e_k within 1e-10 (eps / eps: the round-off of q + eps - (q - eps)
//      at |q| <= 4 is 4 * 2^-52 / (2 eps) = 7e-11).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plant_tangent.h"

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
static bool same(const double* a, const double* b, int n) { return std::memcmp(a, b, (size_t)n * sizeof(double)) == 0; }

static double norm_expr(const double* q) { return __builtin_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }
// a random normalised quaternion; *rounds: the normalisations it took until its norm expression was exactly 1 (4: it is not)
static void unit_quaternion(double* q, int* rounds) {
  for (int i = 0; i < 4; ++i) q[i] = uni();
  for (*rounds = 0; *rounds < 4 && norm_expr(q) != 1.0; ++*rounds) {
    const double nrm = norm_expr(q);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
  }
}

static void check_plain_joints() {
  for (int jt : {IDTO_JOINT_REVOLUTE, IDTO_JOINT_PRISMATIC, IDTO_JOINT_PLANAR}) {
    const int nj = plant_joint_nv(jt);
    CHECK(nj == plant_joint_nq(jt), "joint %d: nq != nv", jt);
    // (the joint sits in the middle of longer vectors: qs = 2, vs = 1)
    double q[8] = {9, 9, 0.75, -1.5, 0.25, 9, 9, 9}, d[8] = {7, 0.125, -0.5, 0.375, 7, 7, 7, 7}, out[8], qdot[8], back[8];
    for (double& x : out) x = 5.0;
    for (double& x : back) x = 5.0;
    tangent_add(jt, 2, 1, q, d, out, qdot);
    for (int i = 0; i < nj; ++i) CHECK(out[2 + i] == q[2 + i] + d[1 + i], "joint %d: add", jt);
    CHECK(out[1] == 5.0 && out[2 + nj] == 5.0, "joint %d: add wrote outside its entries", jt);
    tangent_sub(jt, 2, 1, out, q, back);
    for (int i = 0; i < nj; ++i) CHECK(back[1 + i] == d[1 + i], "joint %d: sub(add(q, d), q) != d", jt);
    CHECK(back[0] == 5.0 && back[1 + nj] == 5.0, "joint %d: sub wrote outside its entries", jt);
  }
}

static void check_floating() {
  const int jt = IDTO_JOINT_FLOATING;
  double worst = 0.0;
  int exact = 0, negative = 0;
  for (int trial = 0; trial < 200; ++trial) {
    double q[7], d[6], out[7], qdot[7], back[6];
    int rounds;
    unit_quaternion(q, &rounds);
    for (int i = 0; i < 3; ++i) q[4 + i] = 2.0 * uni();
    // |d_angular| = |d_linear| = 1e-6
    double na = 0, nl = 0;
    for (int i = 0; i < 6; ++i) d[i] = uni();
    for (int i = 0; i < 3; ++i) { na += d[i] * d[i]; nl += d[3 + i] * d[3 + i]; }
    for (int i = 0; i < 3; ++i) { d[i] *= 1e-6 / std::sqrt(na); d[3 + i] *= 1e-6 / std::sqrt(nl); }
    tangent_add(jt, 0, 0, q, d, out, qdot);
    CHECK(std::fabs(norm_expr(out) - 1.0) <= 4 * 2.3e-16, "floating: add left a norm of 1 + %.3e", norm_expr(out) - 1.0);
    tangent_sub(jt, 0, 0, out, q, back);
    for (int i = 0; i < 6; ++i) {
      const double e = std::fabs(back[i] - d[i]);
      worst = e > worst ? e : worst;
      CHECK(e <= 1e-11, "floating trial %d component %d: sub(add(q, d), q) - d = %.3e", trial, i, back[i] - d[i]);
    }
    // 3. d = 0
    double zero[6] = {0, 0, 0, 0, 0, 0}, same_q[7];
    tangent_add(jt, 0, 0, q, zero, same_q, qdot);
    if (norm_expr(q) == 1.0) {
      ++exact;
      CHECK(same(same_q, q, 7), "floating trial %d: add(q, 0) != q", trial);
    } else {
      for (int i = 0; i < 7; ++i) CHECK(std::fabs(same_q[i] - q[i]) <= 4 * 2.3e-16, "floating trial %d: add(q, 0)[%d] - q = %.3e", trial, i, same_q[i] - q[i]);
      CHECK(same(same_q + 4, q + 4, 3), "floating trial %d: add(q, 0) moved the position", trial);
    }
    // 4. the other sign of the same rotation
    double neg[7], back_neg[6];
    for (int i = 0; i < 4; ++i) neg[i] = -out[i];
    for (int i = 4; i < 7; ++i) neg[i] = out[i];
    const double dw = ((neg[0] * q[0] + neg[1] * q[1]) + neg[2] * q[2]) + neg[3] * q[3];
    CHECK(dw < 0.0, "floating trial %d: the negated quaternion does not take the d.w < 0 branch", trial);
    negative += dw < 0.0;
    tangent_sub(jt, 0, 0, neg, q, back_neg);
    CHECK(same(back_neg, back, 6), "floating trial %d: sub(-(q + d), q) != sub(q + d, q)", trial);
  }
  CHECK(exact >= 50, "only %d of 200 quaternions have a norm expression of exactly 1", exact);
  CHECK(negative == 200, "the d.w < 0 branch ran %d times of 200", negative);
  double id[7] = {1, 0, 0, 0, 0.5, -0.25, 2}, zero[6] = {0, 0, 0, 0, 0, 0}, out[7], qdot[7];
  tangent_add(jt, 0, 0, id, zero, out, qdot);
  CHECK(same(out, id, 7), "add(identity, 0) != identity");
  std::printf("floating: worst |sub(add(q, d), q) - d| = %.3e at |d| = 1e-6 (bound 1e-11); %d of 200 quaternions with a norm expression of exactly 1\n", worst, exact);
}

static void check_columns() {
  // a floating body and two revolute joints: nq = 9, nv = 8
  const int nb = 3, nq = 9, nv = 8, w = nq + nv, n = 2 * nv, P = lin_columns(nv);
  const int jtype[nb] = {IDTO_JOINT_FLOATING, IDTO_JOINT_REVOLUTE, IDTO_JOINT_REVOLUTE}, qstart[nb] = {0, 7, 8}, vstart[nb] = {0, 6, 7};
  const double eps = 6.0554544523933395e-06, two_eps = 2.0 * eps;
  CHECK(P == 49, "lin_columns(8) = %d", P);
  std::vector<double> x((size_t)w), tau((size_t)nv);
  int rounds;
  unit_quaternion(x.data(), &rounds);
  for (int i = 4; i < w; ++i) x[(size_t)i] = 2.0 * uni();
  for (double& t : tau) t = 2.0 * uni();
  std::vector<double> cols((size_t)P * (w + nv));
  for (int col = 0; col < P; ++col) {
    double* c = cols.data() + (size_t)col * (w + nv);
    for (int b = 0; b < nb; ++b) lin_perturb_body(jtype[b], qstart[b], vstart[b], nq, nv, col, eps, x.data(), tau.data(), c, c + nq, c + w);
  }
  CHECK(same(cols.data(), x.data(), w) && same(cols.data() + w, tau.data(), nv), "column 0 is not (x, tau)");
  for (int k = 0; k < 3 * nv; ++k)
    for (int sgn = 0; sgn < 2; ++sgn) {
      const double* c = cols.data() + (size_t)(1 + 2 * k + sgn) * (w + nv);
      const double e = sgn ? -eps : eps;
      const int kind = k / nv, comp = k % nv;
      for (int i = 0; i < nv; ++i) {
        CHECK(c[nq + i] == ((kind == 1 && i == comp) ? x[(size_t)(nq + i)] + e : x[(size_t)(nq + i)]), "column of k = %d: v[%d]", k, i);
        CHECK(c[w + i] == ((kind == 2 && i == comp) ? tau[(size_t)i] + e : tau[(size_t)i]), "column of k = %d: tau[%d]", k, i);
      }
      if (kind != 0) { CHECK(same(c, x.data(), nq), "column of k = %d moved q", k); continue; }
      if (comp >= 6) {   // a revolute joint's position
        for (int i = 0; i < nq; ++i) CHECK(c[i] == ((i == 7 + comp - 6) ? x[(size_t)i] + e : x[(size_t)i]), "column of k = %d: q[%d]", k, i);
      } else if (comp >= 3) {   // the floating body's position
        for (int i = 0; i < nq; ++i) CHECK(c[i] == ((i == 4 + comp - 3) ? x[(size_t)i] + e : x[(size_t)i]), "column of k = %d: q[%d]", k, i);
      } else {
        CHECK(same(c + 4, x.data() + 4, nq - 4), "an angular column moved a position");
        CHECK(!same(c, x.data(), 4), "an angular column left the quaternion alone");
      }
    }
  // the identity map: the final states are the columns' own [q; v] - dx columns give e_k, torque columns 0
  for (int k = 0; k < 3 * nv; ++k) {
    std::vector<double> dst((size_t)n, 5.0);
    const double* xp = cols.data() + (size_t)(1 + 2 * k) * (w + nv);
    const double* xm = cols.data() + (size_t)(2 + 2 * k) * (w + nv);
    for (int b = 0; b < nb; ++b) lin_difference_body(jtype[b], qstart[b], vstart[b], nq, nv, two_eps, xp, xm, dst.data());
    for (int i = 0; i < n; ++i) {
      const double want = (k < n && i == k) ? 1.0 : 0.0;
      CHECK(std::fabs(dst[(size_t)i] - want) <= 1e-10, "identity map: column %d row %d = %.17g", k, i, dst[(size_t)i]);
    }
  }
}

int main() {
  check_plain_joints();
  check_floating();
  check_columns();
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("\nok: plant_tangent.h has its defining properties\n");
  return 0;
}
