// track_body_host_check.cc — csrc/plant.h plant_body<..., LAW = true>, the unmodified device text of track_kernel's body, run on
// the host as a whole block (tests/cpp/lane_emu: a lane is an OS thread, __syncthreads and the exchange points are barriers):
// the law's staging and its carve-up behind the exchange areas inside exactly the bytes the host would request
// (plant_lds_doubles + plant_law_doubles), the law on wavefront 0, the rollout's substep count over two launches.  Held with ==
// to the serial composition, step by step: csrc/tvlqr_step.h tvlqr_control, then the host rollout of plant_body_host_check.cc
// (the oracle's bias and mass matrix, csrc/plant_step.h's solve and step) under the resulting torque.  Built and run by
// tests/test_track_body_host.py with the address and undefined-behaviour sanitizers and a second time with the thread
// sanitizer.  What this can and cannot show: lane_emu/hip/hip_runtime.h.
//
// usage: track_body_host_check CASEFILE...     a case file (written by the test), one problem:
//   label NAME  dev MODEL  orc MODEL  contact k vd vs mu sigma  h H  blocks n T...  (0: what the host's rule gives)
//   S  m  R  nu  actuated[nu]
//   x_nom[S + 1][nq + nv]  tau_nom[S][nv]  K[S][nu * n] column-major  x0[R][nq + nv]
// Per block size the R rollouts run as blockIdx 0 ... R - 1 in TWO launches, steps [0, 1) and [1, S).  One line per (label,
// instantiation, block) with `equal/compared` rollouts; the `edump LO HI` line is plant_body_host_check.cc's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "lane_emu/host_model.h"
#include "plant.h"

namespace idto_dev {
constexpr size_t kLdsDoubles = (size_t)1 << 16;   // (160 KiB are 20480; the rest is poisoned like everything behind a request)
alignas(64) double lds[kLdsDoubles];
}  // namespace idto_dev

using namespace lane_emu;
using idto_dev::DevContact;
using idto_dev::DevModel;
using idto_dev::PlantArgs;
using idto_dev::TrackArgs;

namespace {

constexpr int kLdsLimit = 160 * 1024;
int failures = 0;

size_t lds_doubles(const DevModel& M, int threads, int nu) {
  return (size_t)idto_dev::plant_lds_doubles(M.nq, M.nv, M.blob_n, M.nxb, M.nstem, M.npaths, threads) + idto_dev::plant_law_doubles(M.nq, M.nv, nu);
}
// track_abi.inc TrackBlock's rule, restated
int track_block(const DevModel& M, int forced, int nu) {
  int t = forced ? forced : std::min(256, (((M.nv + 1) * M.npaths + 63) / 64) * 64);
  while (t > 64 && lds_doubles(M, t, nu) * sizeof(double) > (size_t)kLdsLimit) t -= 64;
  return t;
}

template <int MAXC, bool XCH, bool STEM>
void run_block(const DevModel& M, const DevContact& cp, const PlantArgs& A, const TrackArgs& T, int b, int threads) {
  launch(b, threads, [&]() { idto_dev::plant_body<MAXC, XCH, STEM, true>(M, cp, A, (int)blockIdx.x, &T); });
}
// track_launch.hip's dispatch: by nstem, nxb and maxc
void launch_rollouts(const HostModel& h, const DevContact& cp, const PlantArgs& A, const TrackArgs& T, int threads, size_t usable) {
  const DevModel& M = h.M;
  for (int b = 0; b < T.R; ++b) {
    lds_prepare(idto_dev::lds, idto_dev::kLdsDoubles, usable);
    if (M.nstem > 1) run_block<8, true, true>(M, cp, A, T, b, threads);
    else if (M.nxb) run_block<8, true, false>(M, cp, A, T, b, threads);
    else if (h.maxc <= 2) run_block<2, false, false>(M, cp, A, T, b, threads);
    else if (h.maxc <= 3) run_block<3, false, false>(M, cp, A, T, b, threads);
    else if (h.maxc <= 4) run_block<4, false, false>(M, cp, A, T, b, threads);
    else run_block<8, false, false>(M, cp, A, T, b, threads);
    lds_release(idto_dev::lds, idto_dev::kLdsDoubles);
  }
}

// a substep on the host: the oracle's bias and columns, plant_step.h's serial solve and step
bool host_substep(const oracle::Dynamics& d, const DevModel& M, double h, double* q, double* v, const double* tau) {
  const int nv = M.nv;
  std::vector<double> Mm((size_t)nv * nv), c(nv), a(nv), zero(nv, 0.0), e(nv, 0.0), work(nv), qdot(M.nq);
  for (int j = 0; j < nv; ++j) {
    e[j] = 1.0;
    d.InverseDynamics(q, zero.data(), e.data(), false, &Mm[(size_t)j * nv]);
    e[j] = 0.0;
  }
  d.InverseDynamics(q, v, zero.data(), true, c.data());
  for (int i = 0; i < nv; ++i) a[i] = tau[i] - c[i];
  if (idto_plant::plant_ldlt_solve(Mm.data(), nv, a.data(), work.data()) != -1) return false;
  idto_plant::plant_advance(M.nb, M.jtype, M.qstart, M.vstart, h, q, v, a.data(), qdot.data());
  return true;
}

void run_case(const std::string& path) {
  Tokens in(path);
  in.expect("label"); const std::string label = in.next();
  in.expect("dev"); const HostModel hm(in.next());
  in.expect("orc"); const std::string orc = in.next();
  in.expect("contact"); const std::vector<double> cv = in.nums(5);
  in.expect("h"); const double h = in.num();
  in.expect("blocks");
  std::vector<int> blocks(in.integer());
  for (int& b : blocks) b = in.integer();
  const DevModel& M = hm.M;
  const int nq = M.nq, nv = M.nv, w = nq + nv, n = 2 * nv;
  const int S = in.integer(), m = in.integer(), R = in.integer(), nu = in.integer();
  std::vector<int> act(nu);
  for (int& a : act) a = in.integer();
  const std::vector<double> x_nom = in.nums((S + 1) * w), tau_nom = in.nums(S * nv), K = in.nums(S * nu * n), x0 = in.nums(R * w);
  if (in.more()) die(path + ": tokens behind x0");
  if (S < 2) die(path + ": two launches need S >= 2");
  const DevContact cp = DevContactOf(cv.data());
  const std::unique_ptr<oracle::Dynamics> d = OracleOf(orc, cv.data());
  if (d->model.nq != nq || d->model.nv != nv || d->contact.threshold != cp.threshold) die(path + ": the oracle's model or threshold is not the device's");
  const double* edump = idto_dev::lds + 3 * nq + 6 * nv;   // (plant.h's carve-up: plant_body_host_check.cc)
  std::printf("edump %p %p\n", (const void*)edump, (const void*)(edump + nv));

  // ---- the serial composition, once
  std::vector<double> xr((size_t)R * S * w), ur((size_t)R * S * nu), dxr((size_t)R * (S + 1) * n);
  for (int r = 0; r < R; ++r) {
    std::vector<double> x(x0.begin() + (size_t)r * w, x0.begin() + (size_t)(r + 1) * w), tau(nv), unom(nu), dx(n);
    for (int t = 0; t < S; ++t) {
      for (int i = 0; i < nv; ++i) tau[i] = tau_nom[(size_t)t * nv + i];
      for (int c = 0; c < nu; ++c) unom[c] = tau[act[c]];
      double* u = &ur[((size_t)r * S + t) * nu];
      idto_plant::tvlqr_control(M.nb, M.jtype, M.qstart, M.vstart, nq, nv, nu, &K[(size_t)t * nu * n], &x_nom[(size_t)t * w], unom.data(), x.data(),
                                &dxr[((size_t)r * (S + 1) + t) * n], u);
      for (int c = 0; c < nu; ++c) tau[act[c]] = u[c];
      for (int s = 0; s < m; ++s)
        if (!host_substep(*d, M, h, x.data(), x.data() + nq, tau.data())) die(label + ": the host rollout met a failed pivot");
      std::copy(x.begin(), x.end(), &xr[((size_t)r * S + t) * w]);
    }
    std::vector<double> u(nu);   // (row S of dx: the law's deviation against x*_S, its control unused)
    idto_plant::tvlqr_control(M.nb, M.jtype, M.qstart, M.vstart, nq, nv, nu, &K[0], &x_nom[(size_t)S * w], unom.data(), x.data(),
                              &dxr[((size_t)r * (S + 1) + S) * n], u.data());
  }

  for (int forced : blocks) {
    if (forced && lds_doubles(M, forced, nu) * sizeof(double) > (size_t)kLdsLimit) {
      std::printf("%s %s nofit %d\n", label.c_str(), hm.Instantiation(), forced);
      continue;
    }
    const int T = track_block(M, forced, nu), groups = T / M.npaths, rounds = (nv + 1 + groups - 1) / groups;
    const size_t usable = lds_doubles(M, T, nu);
    std::vector<double> state((size_t)R * (1 + w)), xo((size_t)R * S * w, NAN), uo((size_t)R * S * nu, NAN), dxo((size_t)R * (S + 1) * n, NAN);
    std::vector<int> status(2 * R, 0);
    for (int r = 0; r < R; ++r) {
      state[(size_t)r * (1 + w)] = 0.0;
      std::copy(x0.begin() + (size_t)r * w, x0.begin() + (size_t)(r + 1) * w, &state[(size_t)r * (1 + w) + 1]);
    }
    PlantArgs A{};
    A.state = state.data(); A.h = h; A.substeps = S * m; A.record_every = m; A.record = xo.data(); A.status = status.data();
    TrackArgs L{};
    L.R = R; L.S = S; L.m = m; L.nu = nu; L.actuated = act.data();
    L.x_nom = x_nom.data(); L.tau_nom = tau_nom.data(); L.K = K.data(); L.u_out = uo.data(); L.dx_out = dxo.data();
    L.first_step = 0; L.steps = 1;
    launch_rollouts(hm, cp, A, L, T, usable);
    bool mid = true;   // between the launches: a step done, its words say so, nothing behind it written
    for (int r = 0; r < R; ++r) mid = mid && status[2 * r] == 0 && status[2 * r + 1] == m && std::isnan(xo[((size_t)r * S + 1) * w]);
    L.first_step = 1; L.steps = S - 1;
    launch_rollouts(hm, cp, A, L, T, usable);
    int ok = 0;
    for (int r = 0; r < R; ++r) {
      const bool e = mid && status[2 * r] == 0 && status[2 * r + 1] == S * m && same(&xo[(size_t)r * S * w], &xr[(size_t)r * S * w], S * w) &&
                     same(&uo[(size_t)r * S * nu], &ur[(size_t)r * S * nu], S * nu) &&
                     same(&dxo[(size_t)r * (S + 1) * n], &dxr[(size_t)r * (S + 1) * n], (S + 1) * n) &&
                     same(&state[(size_t)r * (1 + w) + 1], &xr[((size_t)r * S + S - 1) * w], w);
      if (!e) std::fprintf(stderr, "%s block %d rollout %d: differs (status %d %d)\n", label.c_str(), T, r, status[2 * r], status[2 * r + 1]);
      ok += e;
    }
    // a rollout whose word is not 0 is left alone by a launch
    {
      std::vector<int> st2 = {idto_dev::PLANT_NONFINITE, m};
      std::vector<double> s2(state.begin(), state.begin() + 1 + w), x2((size_t)S * w, -3.0), u2((size_t)S * nu, -3.0), d2((size_t)(S + 1) * n, -3.0);
      const std::vector<double> s2_0 = s2;
      PlantArgs A2 = A; A2.state = s2.data(); A2.record = x2.data(); A2.status = st2.data();
      TrackArgs L2 = L; L2.R = 1; L2.u_out = u2.data(); L2.dx_out = d2.data();
      launch_rollouts(hm, cp, A2, L2, T, usable);
      const bool untouched = st2[0] == idto_dev::PLANT_NONFINITE && st2[1] == m && s2 == s2_0 &&
                             std::all_of(x2.begin(), x2.end(), [](double v) { return v == -3.0; }) &&
                             std::all_of(u2.begin(), u2.end(), [](double v) { return v == -3.0; }) &&
                             std::all_of(d2.begin(), d2.end(), [](double v) { return v == -3.0; });
      if (!untouched) { std::fprintf(stderr, "%s block %d: a launch touched a rollout that had ended\n", label.c_str(), T); ok = -1; }
    }
    std::printf("%s %s track %d rounds=%d %d/%d\n", label.c_str(), hm.Instantiation(), T, rounds, ok, R);
    if (ok != R) ++failures;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) die("usage: track_body_host_check CASEFILE...");
  for (int i = 1; i < argc; ++i) run_case(argv[i]);
  if (failures) std::printf("FAILED: %d lines\n", failures);
  else std::printf("ok: every line equal\n");
  return failures ? 1 : 0;
}
