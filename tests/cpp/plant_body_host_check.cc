// plant_body_host_check.cc — csrc/plant.h plant_body, the unmodified device text, run on the host as a whole block
// (tests/cpp/lane_emu: a lane is an OS thread, __syncthreads and the exchange points are barriers): the LDS carve-up as
// written inside the bytes the host would request, the rounds, the dump row, the solve and the step on wavefront 0.  Held
// with == to the CPU oracle (mass matrix, bias) and to csrc/plant_step.h / mpc_spline.h run serially on the oracle's numbers
// (acceleration, hold rollout, PD+).  Built and run by tests/test_plant_body_host.py with the address and undefined-
// behaviour sanitizers and a second time with the thread sanitizer.  What this can and cannot show:
// lane_emu/hip/hip_runtime.h.
//
// usage: plant_body_host_check CASEFILE...     a case file (written by the test):
//   label NAME  dev MODEL  orc MODEL  contact k vd vs mu sigma  h H  kind finite|nonfinite|pivot
//   default_block T (0: not asserted)  blocks n T...  (0: what PlantBlock's rule gives)
//   pd 0|1 [nu  actuated[nu]  Kp[nu * nq]  Kd[nu * nv]  feed_forward]
//   plants B, then B times: t0 q[nq] v[nv] tau[nv]
// finite: per block size forward dynamics, a hold rollout of 3 substeps recorded every substep and (pd) 2 substeps of PD+
// on a plan of 3 knots that this program writes; plant b runs as blockIdx b with a record (a copy of the blob) of its own.
// nonfinite: status (2, 0) and the state untouched; pivot: status (1, 0) and the state untouched, in both launches.
// A block size whose LDS does not fit 160 KiB prints `nofit`.  One line per (label, instantiation, mode, block) with
// `equal/compared` plants; `edump LO HI` lines give the address range of the write-only dump row of the surplus groups
// (the one place where lanes race by design: the thread-sanitizer leg accepts write-write reports inside it, nothing else).
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

namespace {

constexpr int kLdsLimit = 160 * 1024;
int failures = 0;

struct Pd {
  int on = 0, nu = 0, ff = 0;
  std::vector<int> act;
  std::vector<double> Kp, Kd;
};
struct Plant { double t0; std::vector<double> q, v, tau; };
struct Case {
  std::string label, kind;
  double h;
  Pd pd;
  std::vector<Plant> plants;
};

// PlantBlock's rule (plant_abi.inc), restated from plant_lds_doubles
int lds_bytes(const DevModel& M, int threads, size_t pd_doubles) {
  return (int)(((size_t)idto_dev::plant_lds_doubles(M.nq, M.nv, M.blob_n, M.nxb, M.nstem, M.npaths, threads) + pd_doubles) * sizeof(double));
}
int plant_block(const DevModel& M, int forced, size_t pd_doubles) {
  int t = forced ? forced : std::min(256, (((M.nv + 1) * M.npaths + 63) / 64) * 64);
  while (t > 64 && lds_bytes(M, t, pd_doubles) > kLdsLimit) t -= 64;
  return t;
}

template <int MAXC, bool XCH, bool STEM>
void run_block(const DevModel& M, const DevContact& cp, const PlantArgs& A, int b, int threads) {
  launch(b, threads, [&]() { idto_dev::plant_body<MAXC, XCH, STEM>(M, cp, A, (int)blockIdx.x); });
}
// plant_launch.hip's dispatch: by nstem, nxb and maxc
void launch_plants(const HostModel& h, const std::vector<DevModel>& Ms, const DevContact& cp, const PlantArgs& A, int B, int threads,
                   size_t usable) {
  for (int b = 0; b < B; ++b) {
    lds_prepare(idto_dev::lds, idto_dev::kLdsDoubles, usable);
    const DevModel& M = Ms[b];
    if (M.nstem > 1) run_block<8, true, true>(M, cp, A, b, threads);
    else if (M.nxb) run_block<8, true, false>(M, cp, A, b, threads);
    else if (h.maxc <= 2) run_block<2, false, false>(M, cp, A, b, threads);
    else if (h.maxc <= 3) run_block<3, false, false>(M, cp, A, b, threads);
    else if (h.maxc <= 4) run_block<4, false, false>(M, cp, A, b, threads);
    else run_block<8, false, false>(M, cp, A, b, threads);
    lds_release(idto_dev::lds, idto_dev::kLdsDoubles);
  }
}

// the host restatement: the oracle's bias and columns, plant_step.h's serial solve
struct HostFd { std::vector<double> M, c, a; int piv; };
HostFd host_fd(const oracle::Dynamics& d, const double* q, const double* v, const double* tau) {
  const int nv = d.model.nv;
  HostFd r;
  r.M.resize((size_t)nv * nv); r.c.resize(nv); r.a.resize(nv);
  std::vector<double> zero(nv, 0.0), e(nv, 0.0), work(nv), A;
  for (int j = 0; j < nv; ++j) {
    e[j] = 1.0;
    d.InverseDynamics(q, zero.data(), e.data(), false, &r.M[(size_t)j * nv]);
    e[j] = 0.0;
  }
  d.InverseDynamics(q, v, zero.data(), true, r.c.data());
  A = r.M;
  for (int i = 0; i < nv; ++i) r.a[i] = tau[i] - r.c[i];
  r.piv = idto_plant::plant_ldlt_solve(A.data(), nv, r.a.data(), work.data());
  return r;
}

void report(const Case& c, const char* inst, const char* mode, int block, int rounds, int ok, int n) {
  std::printf("%s %s %s %d rounds=%d %d/%d\n", c.label.c_str(), inst, mode, block, rounds, ok, n);
  if (ok != n) ++failures;
}
bool check(bool ok, const Case& c, const char* mode, int block, int b, const char* what) {
  static int shown = 0;
  if (!ok && shown++ < 12) std::fprintf(stderr, "%s %s block %d plant %d: %s differs\n", c.label.c_str(), mode, block, b, what);
  return ok;
}
// per plant and column of the mass matrix, what differs (the evidence a failing run leaves)
void describe(const Case& c, int block, int b, const double* M, const double* Mref, const double* bias, const double* cref, int nv) {
  std::fprintf(stderr, "%s block %d plant %d: bias %s;", c.label.c_str(), block, b, same(bias, cref, nv) ? "equal" : "DIFFERS");
  for (int j = 0; j < nv; ++j) {
    double worst = 0.0;
    for (int i = 0; i < nv; ++i) worst = std::max(worst, std::fabs(M[(size_t)j * nv + i] - Mref[(size_t)j * nv + i]));
    if (!same(M + (size_t)j * nv, Mref + (size_t)j * nv, nv)) std::fprintf(stderr, " column %d off by %.3e;", j, worst);
  }
  std::fprintf(stderr, "\n");
}

void run_finite(const Case& c, const HostModel& h, const std::vector<DevModel>& Ms, const DevContact& cp, const oracle::Dynamics& d,
                int forced) {
  const DevModel& M = h.M;
  const int nq = M.nq, nv = M.nv, B = (int)c.plants.size(), w = 1 + nq + nv;
  const char* inst = h.Instantiation();
  if (forced && lds_bytes(M, forced, 0) > kLdsLimit) {
    std::printf("%s %s nofit %d\n", c.label.c_str(), inst, forced);
    return;
  }
  const int T = plant_block(M, forced, 0), groups = T / M.npaths, rounds = (nv + 1 + groups - 1) / groups;
  const size_t usable = (size_t)idto_dev::plant_lds_doubles(nq, nv, M.blob_n, M.nxb, M.nstem, M.npaths, T);
  std::vector<int> status(2 * B);
  std::vector<double> tau((size_t)B * nv);
  for (int b = 0; b < B; ++b) std::copy(c.plants[b].tau.begin(), c.plants[b].tau.end(), tau.begin() + (size_t)b * nv);
  PlantArgs A{};
  A.tau = tau.data(); A.h = c.h; A.status = status.data();

  // ---- forward dynamics
  {
    std::vector<double> x((size_t)B * (nq + nv)), a((size_t)B * nv, NAN), Mo((size_t)B * nv * nv, NAN), bias((size_t)B * nv, NAN);
    for (int b = 0; b < B; ++b) {
      std::copy(c.plants[b].q.begin(), c.plants[b].q.end(), x.begin() + (size_t)b * (nq + nv));
      std::copy(c.plants[b].v.begin(), c.plants[b].v.end(), x.begin() + (size_t)b * (nq + nv) + nq);
    }
    const std::vector<double> x0 = x;
    PlantArgs F = A;
    F.state = x.data(); F.fd = 1; F.substeps = 1; F.a_out = a.data(); F.M_out = Mo.data(); F.bias_out = bias.data();
    std::fill(status.begin(), status.end(), -7);
    launch_plants(h, Ms, cp, F, B, T, usable);
    int ok = 0;
    for (int b = 0; b < B; ++b) {
      const HostFd r = host_fd(d, c.plants[b].q.data(), c.plants[b].v.data(), c.plants[b].tau.data());
      bool e = check(r.piv == -1, c, "fd", T, b, "the host's pivot");
      const bool em = same(&Mo[(size_t)b * nv * nv], r.M.data(), nv * nv), eb = same(&bias[(size_t)b * nv], r.c.data(), nv);
      if (!em || !eb) describe(c, T, b, &Mo[(size_t)b * nv * nv], r.M.data(), &bias[(size_t)b * nv], r.c.data(), nv);
      e = check(em, c, "fd", T, b, "M_out") && e;
      e = check(eb, c, "fd", T, b, "bias_out") && e;
      e = check(same(&a[(size_t)b * nv], r.a.data(), nv), c, "fd", T, b, "a_out") && e;
      e = check(status[2 * b] == 0 && status[2 * b + 1] == 0, c, "fd", T, b, "status") && e;
      ok += e;
    }
    if (!check(x == x0, c, "fd", T, -1, "the caller's x (forward dynamics leaves it alone)")) ++failures;
    report(c, inst, "fd", T, rounds, ok, B);
  }

  // ---- hold: 3 substeps, recorded every substep
  {
    const int S = 3;
    std::vector<double> state((size_t)B * w), tick((size_t)B * w, NAN), rec((size_t)B * S * (nq + nv), NAN);
    for (int b = 0; b < B; ++b) {
      double* s = &state[(size_t)b * w];
      s[0] = c.plants[b].t0;
      std::copy(c.plants[b].q.begin(), c.plants[b].q.end(), s + 1);
      std::copy(c.plants[b].v.begin(), c.plants[b].v.end(), s + 1 + nq);
    }
    PlantArgs H = A;
    H.state = state.data(); H.substeps = S; H.record_every = 1; H.record = rec.data(); H.tick_out = tick.data();
    std::fill(status.begin(), status.end(), -7);
    launch_plants(h, Ms, cp, H, B, T, usable);
    int ok = 0;
    for (int b = 0; b < B; ++b) {
      std::vector<double> q = c.plants[b].q, v = c.plants[b].v, qdot(nq);
      bool e = true;
      for (int s = 0; s < S; ++s) {
        const HostFd r = host_fd(d, q.data(), v.data(), c.plants[b].tau.data());
        idto_plant::plant_advance(M.nb, M.jtype, M.qstart, M.vstart, c.h, q.data(), v.data(), r.a.data(), qdot.data());
        const double* got = &rec[((size_t)b * S + s) * (nq + nv)];
        e = check(same(got, q.data(), nq) && same(got + nq, v.data(), nv), c, "hold", T, b, "a recorded state") && e;
      }
      const double t_end = idto_plant::plant_time(c.plants[b].t0, S, c.h);
      for (const double* out : {&state[(size_t)b * w], &tick[(size_t)b * w]})
        e = check(out[0] == t_end && same(out + 1, q.data(), nq) && same(out + 1 + nq, v.data(), nv), c, "hold", T, b, "the final [t, q, v] / tick_out") && e;
      e = check(status[2 * b] == 0 && status[2 * b + 1] == S, c, "hold", T, b, "status") && e;
      ok += e;
    }
    report(c, inst, "hold", T, rounds, ok, B);
  }

  // ---- PD+: 2 substeps on a plan of 3 knots
  if (c.pd.on) {
    const int S = 2, n = 3, nu = c.pd.nu;
    const int dims[3] = {nq, nv, nu};
    size_t y[3], m[3], len = 8;   // [0] the plan's start time, then per spline the values and the knot derivatives
    for (int sp = 0; sp < 3; ++sp) { y[sp] = len; len += (size_t)n * dims[sp]; m[sp] = len; len += (size_t)n * dims[sp]; }
    const size_t pd_doubles = idto_dev::plant_pd_doubles(nq, nv, nu, n, len);
    if (lds_bytes(M, T, pd_doubles) > kLdsLimit) die(c.label + ": PD+ does not fit beside the block");
    const double breaks[3] = {0.0, 0.0013, 0.0031};   // (the substeps at 0.4, 1.4 ms: two intervals are visited)
    std::vector<double> plan((size_t)B * len, 0.0), work((size_t)n * (nq + nv + nu));
    unsigned long long lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; };
    for (int b = 0; b < B; ++b) {
      double* p = &plan[(size_t)b * len];
      p[0] = c.plants[b].t0 - 0.0004;
      for (int sp = 0; sp < 3; ++sp)
        for (int k = 0; k < n; ++k)
          for (int i = 0; i < dims[sp]; ++i) {
            const double base = sp == 0 ? c.plants[b].q[i] : (sp == 1 ? c.plants[b].v[i] : 0.0);
            p[y[sp] + (size_t)k * dims[sp] + i] = base + 0.05 * rnd();
          }
      for (int sp = 0; sp < 3; ++sp)
        for (int i = 0; i < dims[sp]; ++i)
          if (idto_spline::spline_fit(breaks, n, p + y[sp] + i, p + m[sp] + i, work.data(), dims[sp])) die("spline_fit");
    }
    std::vector<double> state((size_t)B * w), tick((size_t)B * w, NAN), rec((size_t)B * S * (nq + nv), NAN);
    for (int b = 0; b < B; ++b) {
      double* s = &state[(size_t)b * w];
      s[0] = c.plants[b].t0;
      std::copy(c.plants[b].q.begin(), c.plants[b].q.end(), s + 1);
      std::copy(c.plants[b].v.begin(), c.plants[b].v.end(), s + 1 + nq);
    }
    PlantArgs P = A;
    P.tau = nullptr; P.state = state.data(); P.substeps = S; P.record_every = 1; P.record = rec.data(); P.tick_out = tick.data();
    P.pd = 1; P.n = n; P.nu = nu; P.feed_forward = c.pd.ff; P.breaks = breaks; P.plan = plan.data(); P.plan_len = len;
    for (int sp = 0; sp < 3; ++sp) { P.plan_y[sp] = y[sp]; P.plan_m[sp] = m[sp]; }
    P.Kp = c.pd.Kp.data(); P.Kd = c.pd.Kd.data(); P.actuated = c.pd.act.data();
    std::fill(status.begin(), status.end(), -7);
    launch_plants(h, Ms, cp, P, B, T, usable + pd_doubles);
    int ok = 0;
    for (int b = 0; b < B; ++b) {
      const double* p = &plan[(size_t)b * len];
      std::vector<double> q = c.plants[b].q, v = c.plants[b].v, qdot(nq), nom(nq + nv + nu), tau_pd(nv);
      bool e = true;
      for (int s = 0; s < S; ++s) {
        const double t = idto_plant::plant_time(c.plants[b].t0, s, c.h) - p[0];
        for (int sp = 0, j = 0; sp < 3; ++sp)
          for (int i = 0; i < dims[sp]; ++i, ++j) nom[j] = idto_spline::spline_value(breaks, n, p + y[sp] + i, p + m[sp] + i, dims[sp], t);
        idto_plant::plant_pd_plus(c.pd.Kp.data(), c.pd.Kd.data(), nu, nq, nv, c.pd.act.data(), q.data(), v.data(), nom.data(), nom.data() + nq,
                                  c.pd.ff != 0, nom.data() + nq + nv, tau_pd.data());
        const HostFd r = host_fd(d, q.data(), v.data(), tau_pd.data());
        idto_plant::plant_advance(M.nb, M.jtype, M.qstart, M.vstart, c.h, q.data(), v.data(), r.a.data(), qdot.data());
        const double* got = &rec[((size_t)b * S + s) * (nq + nv)];
        e = check(same(got, q.data(), nq) && same(got + nq, v.data(), nv), c, "pd", T, b, "a recorded state") && e;
      }
      const double t_end = idto_plant::plant_time(c.plants[b].t0, S, c.h);
      for (const double* out : {&state[(size_t)b * w], &tick[(size_t)b * w]})
        e = check(out[0] == t_end && same(out + 1, q.data(), nq) && same(out + 1 + nq, v.data(), nv), c, "pd", T, b, "the final [t, q, v] / tick_out") && e;
      e = check(status[2 * b] == 0 && status[2 * b + 1] == S, c, "pd", T, b, "status") && e;
      ok += e;
    }
    report(c, inst, "pd", T, rounds, ok, B);
  }
}

// a NaN among the inputs: (2, 0); a zero pivot: (1, 0) - the state untouched, whatever the launch
void run_status(const Case& c, const HostModel& h, const std::vector<DevModel>& Ms, const DevContact& cp, int forced) {
  const DevModel& M = h.M;
  const int nq = M.nq, nv = M.nv, B = (int)c.plants.size(), w = 1 + nq + nv;
  const int T = plant_block(M, forced, 0), groups = T / M.npaths, rounds = (nv + 1 + groups - 1) / groups;
  const size_t usable = (size_t)idto_dev::plant_lds_doubles(nq, nv, M.blob_n, M.nxb, M.nstem, M.npaths, T);
  const int want = c.kind == "nonfinite" ? idto_dev::PLANT_NONFINITE : idto_dev::PLANT_PIVOT;
  std::vector<int> status(2 * B, -7);
  std::vector<double> tau((size_t)B * nv), state((size_t)B * w), tick((size_t)B * w, NAN), rec((size_t)B * 3 * (nq + nv), NAN);
  for (int b = 0; b < B; ++b) {
    std::copy(c.plants[b].tau.begin(), c.plants[b].tau.end(), tau.begin() + (size_t)b * nv);
    double* s = &state[(size_t)b * w];
    s[0] = c.plants[b].t0;
    std::copy(c.plants[b].q.begin(), c.plants[b].q.end(), s + 1);
    std::copy(c.plants[b].v.begin(), c.plants[b].v.end(), s + 1 + nq);
  }
  const std::vector<double> state0 = state;
  PlantArgs A{};
  A.tau = tau.data(); A.h = c.h; A.status = status.data();
  A.state = state.data(); A.substeps = 3; A.record_every = 1; A.record = rec.data(); A.tick_out = tick.data();
  launch_plants(h, Ms, cp, A, B, T, usable);
  int ok = 0;
  for (int b = 0; b < B; ++b) {
    bool e = check(status[2 * b] == want && status[2 * b + 1] == 0, c, c.kind.c_str(), T, b, "status");
    e = check(same(&state[(size_t)b * w], &state0[(size_t)b * w], w), c, c.kind.c_str(), T, b, "the state (it must be untouched)") && e;
    e = check(same(&tick[(size_t)b * w], &state0[(size_t)b * w], w), c, c.kind.c_str(), T, b, "tick_out") && e;
    ok += e;
  }
  report(c, h.Instantiation(), c.kind.c_str(), T, rounds, ok, B);
  // forward dynamics: the same code, a_out not written
  std::vector<double> x((size_t)B * (nq + nv)), a((size_t)B * nv, -3.0);
  for (int b = 0; b < B; ++b) std::copy(&state0[(size_t)b * w + 1], &state0[(size_t)b * w + w], x.begin() + (size_t)b * (nq + nv));
  PlantArgs F{};
  F.tau = tau.data(); F.h = c.h; F.status = status.data(); F.state = x.data(); F.fd = 1; F.substeps = 1; F.a_out = a.data();
  std::fill(status.begin(), status.end(), -7);
  launch_plants(h, Ms, cp, F, B, T, usable);
  ok = 0;
  for (int b = 0; b < B; ++b) {
    bool e = check(status[2 * b] == want && status[2 * b + 1] == 0, c, "fd", T, b, "status");
    for (int i = 0; i < nv; ++i) e = check(a[(size_t)b * nv + i] == -3.0, c, "fd", T, b, "a_out (not valid, not written)") && e;
    ok += e;
  }
  report(c, h.Instantiation(), (c.kind + "_fd").c_str(), T, rounds, ok, B);
}

void run_case(const std::string& path) {
  Tokens in(path);
  Case c;
  in.expect("label"); c.label = in.next();
  in.expect("dev"); const HostModel h(in.next());
  in.expect("orc"); const std::string orc = in.next();
  in.expect("contact"); const std::vector<double> cv = in.nums(5);
  in.expect("h"); c.h = in.num();
  in.expect("kind"); c.kind = in.next();
  in.expect("default_block"); const int default_block = in.integer();
  in.expect("blocks");
  std::vector<int> blocks(in.integer());
  for (int& b : blocks) b = in.integer();
  const int nq = h.M.nq, nv = h.M.nv;
  in.expect("pd"); c.pd.on = in.integer();
  if (c.pd.on) {
    c.pd.nu = in.integer();
    c.pd.act.resize(c.pd.nu);
    for (int& a : c.pd.act) a = in.integer();
    c.pd.Kp = in.nums(c.pd.nu * nq); c.pd.Kd = in.nums(c.pd.nu * nv);
    c.pd.ff = in.integer();
  }
  in.expect("plants"); c.plants.resize(in.integer());
  for (Plant& p : c.plants) { p.t0 = in.num(); p.q = in.nums(nq); p.v = in.nums(nv); p.tau = in.nums(nv); }
  if (in.more()) die(path + ": tokens behind the last plant");
  const DevContact cp = DevContactOf(cv.data());
  const std::unique_ptr<oracle::Dynamics> d = OracleOf(orc, cv.data());
  if (d->model.nq != nq || d->model.nv != nv || d->contact.threshold != cp.threshold) die(path + ": the oracle's model or threshold is not the device's");
  if (default_block && plant_block(h.M, 0, 0) != default_block)
    die(c.label + ": PlantBlock's rule gives " + std::to_string(plant_block(h.M, 0, 0)) + " threads, not " + std::to_string(default_block));
  // a record per plant: a copy of the blob, the DevModel's tables moved to it (plant_abi.inc PlantAllocate)
  std::vector<std::vector<double>> blobs(c.plants.size(), h.t.blob);
  std::vector<DevModel> Ms(c.plants.size(), h.M);
  for (size_t b = 0; b < Ms.size(); ++b) idto_dev::shift_model(Ms[b], blobs[b].data());
  // the dump row: behind q, qn, qdot, v, vn, zero, tau_app, rhs, col (plant.h's carve-up)
  const double* edump = idto_dev::lds + 3 * nq + 6 * nv;
  std::printf("edump %p %p\n", (const void*)edump, (const void*)(edump + nv));
  for (int forced : blocks) {
    if (c.kind == "finite") run_finite(c, h, Ms, cp, *d, forced);
    else run_status(c, h, Ms, cp, forced);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) die("usage: plant_body_host_check CASEFILE...");
  for (int i = 1; i < argc; ++i) run_case(argv[i]);
  if (failures) std::printf("FAILED: %d lines\n", failures);
  else std::printf("ok: every line equal\n");
  return failures ? 1 : 0;
}
