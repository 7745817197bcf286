// id_eval_host_check.cc — csrc/id_eval.h, the unmodified device text, run on the host lane by lane (tests/cpp/lane_emu:
// a lane is an OS thread, a wavefront's exchange points are barriers) and held to oracle::Dynamics::InverseDynamics bit
// for bit.  Built and run by tests/test_id_eval_host.py with the address and undefined-behaviour sanitizers, and a second
// time with the thread sanitizer.  What this can and cannot show: lane_emu/hip/hip_runtime.h.
//
// usage: id_eval_host_check CASEFILE...     a case file (written by the test):
//   label NAME  dev MODEL  orc MODEL|-  chain MODEL|-  contact k vd vs mu sigma  golden 0|1  states S
//   then S times: q[nq] v[nv] a[nv], and with golden 1: tau[nv] scale
// `dev` is evaluated by the instantiation that fd_launch.hip / plant_launch.hip pick for it (by nstem, nxb, maxc):
//   - orc: every result == the oracle on that model file
//   - chain: every result == the same evaluation of that model (a chain form of dev) through ITS instantiation
//   - golden: |tau - the stored tau|_inf / scale <= 1e-7 in `full` mode (a model the oracle cannot express)
// Per state: `full` ID(q, v, a), and all nv mass-matrix columns ID(q, 0, e_j) in both input layouts that exist - fd_body's
// (a row of zeros, a row e_j per evaluation) and the plant's (one shared zero row, the window ramp + (nv - ee) of a row of
// zeros around a one).  The evaluations run G groups of npaths lanes side by side in one wavefront, each group with an
// exchange area of its own that starts as NaN and is never cleared: the first three rounds run, in every group, `full`
// on a state, a column of it, and `full` again on the same area - what the rounds of fd_body and plant_body do.
// One line per (label, instantiation, mode) with `equal/compared`; exit status 1 if any differs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "lane_emu/host_model.h"

namespace idto_dev {
constexpr size_t kLdsDoubles = (size_t)1 << 22;
alignas(64) double lds[kLdsDoubles];
}  // namespace idto_dev

using namespace lane_emu;
using idto_dev::DevContact;
using idto_dev::DevModel;

namespace {

struct Job {
  bool full;
  const double *q, *v, *a;
  double* out;
};

template <int MAXC, bool XCH, bool STEM>
void run_rounds(const DevModel& M, const DevContact& cp, int G, const std::vector<std::vector<Job>>& rounds, double* xs,
                int xeval, double* dump) {
  const int K = M.npaths, nv = M.nv;
  launch(0, G * K, [&]() {
    const int tid = threadIdx.x, g = tid / K, path = tid % K;
    for (const std::vector<Job>& round : rounds) {
      const bool mine = g < (int)round.size();
      const Job& j = round[mine ? g : 0];
      double* dst = mine ? j.out : dump + (size_t)g * nv;   // (a surplus group re-runs job 0 into a row of its own)
      if constexpr (XCH) idto_dev::id_eval<MAXC, true, STEM>(M, cp, path, j.full, j.q, j.v, j.a, dst, xs + (size_t)g * xeval);
      else idto_dev::id_eval<MAXC>(M, cp, path, j.full, j.q, j.v, j.a, dst);
    }
  });
}

void dispatch(const HostModel& h, const DevContact& cp, int G, const std::vector<std::vector<Job>>& rounds, double* xs, int xeval,
              double* dump) {
  const DevModel& M = h.M;
  if (M.nstem > 1) run_rounds<8, true, true>(M, cp, G, rounds, xs, xeval, dump);
  else if (M.nxb) run_rounds<8, true, false>(M, cp, G, rounds, xs, xeval, dump);
  else if (h.maxc <= 2) run_rounds<2, false, false>(M, cp, G, rounds, xs, xeval, dump);
  else if (h.maxc <= 3) run_rounds<3, false, false>(M, cp, G, rounds, xs, xeval, dump);
  else if (h.maxc <= 4) run_rounds<4, false, false>(M, cp, G, rounds, xs, xeval, dump);
  else run_rounds<8, false, false>(M, cp, G, rounds, xs, xeval, dump);
}

struct State { std::vector<double> q, v, a, tau; double scale = 1.0; };

// every result of one model on the case's states, copied out of the emulated LDS
struct Results {
  int S = 0, nv = 0, G = 0;
  std::vector<double> full, colfd, colplant;   // [S][nv], [S][nv][nv] (column j of state s at (s * nv + j) * nv)
  std::vector<double> seq;                     // [G][3][nv]: full of state g % S, column g % nv of it, full again
};

Results evaluate(const HostModel& h, const DevContact& cp, const std::vector<State>& states) {
  const DevModel& M = h.M;
  const int nq = M.nq, nv = M.nv, K = M.npaths, S = (int)states.size();
  const int G = std::max(2, std::min(kWave / K, 8));
  const int xeval = idto_dev::xch_eval_doubles(M.nxb, M.nstem);
  // the carve-up of the emulated LDS
  double* lds = idto_dev::lds;
  size_t at = 0;
  auto take = [&](size_t n) { double* p = lds + at; at += n; return p; };
  double* zero = take(nv);                 // the plant's shared zero row
  double* ramp = take(2 * nv - 1);         // the plant's: zeros around a one
  double* zfd = take(nv);                  // fd_body's row of zeros
  double* eye = take((size_t)nv * nv);     // fd_body's rows e_j
  double* sq = take((size_t)S * nq);
  double* sv = take((size_t)S * nv);
  double* sa = take((size_t)S * nv);
  double* o_full = take((size_t)S * nv);
  double* o_colfd = take((size_t)S * nv * nv);
  double* o_colplant = take((size_t)S * nv * nv);
  double* o_seq = take((size_t)G * 3 * nv);
  double* dump = take((size_t)G * nv);
  double* xs = take((size_t)G * xeval);    // starts as NaN, never cleared
  lds_prepare(lds, idto_dev::kLdsDoubles, at);
  for (int i = 0; i < nv; ++i) zero[i] = zfd[i] = 0.0;
  for (int i = 0; i < 2 * nv - 1; ++i) ramp[i] = (i == nv - 1) ? 1.0 : 0.0;
  for (int i = 0; i < nv * nv; ++i) eye[i] = (i / nv == i % nv) ? 1.0 : 0.0;
  for (int s = 0; s < S; ++s) {
    std::copy(states[s].q.begin(), states[s].q.end(), sq + (size_t)s * nq);
    std::copy(states[s].v.begin(), states[s].v.end(), sv + (size_t)s * nv);
    std::copy(states[s].a.begin(), states[s].a.end(), sa + (size_t)s * nv);
  }
  std::vector<std::vector<Job>> rounds(3);
  for (int g = 0; g < G; ++g) {
    const int s = g % S, j = g % nv, ee = 1 + j;
    rounds[0].push_back(Job{true, sq + (size_t)s * nq, sv + (size_t)s * nv, sa + (size_t)s * nv, o_seq + ((size_t)g * 3 + 0) * nv});
    rounds[1].push_back(Job{false, sq + (size_t)s * nq, zero, ramp + (nv - ee), o_seq + ((size_t)g * 3 + 1) * nv});
    rounds[2].push_back(Job{true, sq + (size_t)s * nq, sv + (size_t)s * nv, sa + (size_t)s * nv, o_seq + ((size_t)g * 3 + 2) * nv});
  }
  std::vector<Job> flat;
  for (int s = 0; s < S; ++s) {
    const double* q = sq + (size_t)s * nq;
    flat.push_back(Job{true, q, sv + (size_t)s * nv, sa + (size_t)s * nv, o_full + (size_t)s * nv});
    for (int j = 0; j < nv; ++j) {
      const int ee = 1 + j;
      flat.push_back(Job{false, q, zfd, eye + (size_t)j * nv, o_colfd + ((size_t)s * nv + j) * nv});
      flat.push_back(Job{false, q, zero, ramp + (nv - ee), o_colplant + ((size_t)s * nv + j) * nv});
    }
  }
  for (size_t i = 0; i < flat.size(); i += G) rounds.emplace_back(flat.begin() + i, flat.begin() + std::min(flat.size(), i + G));
  dispatch(h, cp, G, rounds, xs, xeval, dump);
  Results r;
  r.S = S; r.nv = nv; r.G = G;
  r.full.assign(o_full, o_full + (size_t)S * nv);
  r.colfd.assign(o_colfd, o_colfd + (size_t)S * nv * nv);
  r.colplant.assign(o_colplant, o_colplant + (size_t)S * nv * nv);
  r.seq.assign(o_seq, o_seq + (size_t)G * 3 * nv);
  lds_release(lds, idto_dev::kLdsDoubles);
  return r;
}

int failures = 0;
void report(const std::string& label, const char* inst, const char* mode, int ok, int n) {
  std::printf("%s %s %s %d/%d\n", label.c_str(), inst, mode, ok, n);
  if (ok != n) ++failures;
}
void complain(const std::string& label, const char* mode, int s, int j, const double* got, const double* want, int nv) {
  static int shown = 0;
  if (shown++ >= 8) return;
  double worst = 0.0;
  int at = 0;
  for (int i = 0; i < nv; ++i) {
    const double d = std::fabs(got[i] - want[i]);
    if (!(d <= worst)) { worst = d; at = i; }
  }
  std::fprintf(stderr, "%s %s: state %d column %d differs, most in entry %d: %.17g, wanted %.17g\n", label.c_str(), mode, s, j, at, got[at], want[at]);
}

// `got` against `want` (both Results on the same states), == throughout
void compare(const std::string& label, const char* inst, const std::string& suffix, const Results& got, const Results& want) {
  const int S = got.S, nv = got.nv;
  int ok[4] = {0, 0, 0, 0};
  for (int s = 0; s < S; ++s) {
    const bool e = same(&got.full[(size_t)s * nv], &want.full[(size_t)s * nv], nv);
    ok[0] += e;
    if (!e) complain(label, "full", s, -1, &got.full[(size_t)s * nv], &want.full[(size_t)s * nv], nv);
    for (int j = 0; j < nv; ++j) {
      const size_t o = ((size_t)s * nv + j) * nv;
      const bool a = same(&got.colfd[o], &want.colfd[o], nv), b = same(&got.colplant[o], &want.colfd[o], nv);
      ok[1] += a; ok[2] += b;
      if (!a) complain(label, "columns_fd", s, j, &got.colfd[o], &want.colfd[o], nv);
      if (!b) complain(label, "columns_plant", s, j, &got.colplant[o], &want.colfd[o], nv);
    }
  }
  // the exchange sequence: group g ran full on state g % S, column g % nv of it, full again, all on one exchange area
  for (int g = 0; g < got.G; ++g) {
    const int s = g % S, j = g % nv;
    const double* w[3] = {&want.full[(size_t)s * nv], &want.colfd[((size_t)s * nv + j) * nv], &want.full[(size_t)s * nv]};
    bool e = true;
    for (int k = 0; k < 3; ++k) {
      const bool ek = same(&got.seq[((size_t)g * 3 + k) * nv], w[k], nv);
      if (!ek) complain(label, "sequence", s, k, &got.seq[((size_t)g * 3 + k) * nv], w[k], nv);
      e = e && ek;
    }
    ok[3] += e;
  }
  report(label, inst, ("full" + suffix).c_str(), ok[0], S);
  report(label, inst, ("columns_fd" + suffix).c_str(), ok[1], S * nv);
  report(label, inst, ("columns_plant" + suffix).c_str(), ok[2], S * nv);
  report(label, inst, ("sequence" + suffix).c_str(), ok[3], got.G);
}

void run_case(const std::string& path) {
  Tokens in(path);
  in.expect("label"); const std::string label = in.next();
  in.expect("dev"); const std::string dev = in.next();
  in.expect("orc"); const std::string orc = in.next();
  in.expect("chain"); const std::string chain = in.next();
  in.expect("contact"); const std::vector<double> c = in.nums(5);
  in.expect("golden"); const bool golden = in.integer() != 0;
  in.expect("states"); const int S = in.integer();
  const HostModel h(dev);
  const int nq = h.M.nq, nv = h.M.nv;
  std::vector<State> states(S);
  for (State& st : states) {
    st.q = in.nums(nq); st.v = in.nums(nv); st.a = in.nums(nv);
    if (golden) { st.tau = in.nums(nv); st.scale = in.num(); }
  }
  if (in.more()) die(path + ": tokens behind the last state");
  const DevContact cp = DevContactOf(c.data());
  const Results got = evaluate(h, cp, states);
  const char* inst = h.Instantiation();
  if (orc != "-") {
    const std::unique_ptr<oracle::Dynamics> d = OracleOf(orc, c.data());
    if (d->model.nq != nq || d->model.nv != nv) die(path + ": the oracle's model has other sizes");
    if (d->contact.threshold != cp.threshold) die(path + ": the oracle's contact threshold is not the device's");
    Results want;
    want.S = S; want.nv = nv; want.G = got.G;
    want.full.resize((size_t)S * nv); want.colfd.resize((size_t)S * nv * nv);
    std::vector<double> zero(nv, 0.0), e(nv, 0.0);
    for (int s = 0; s < S; ++s) {
      d->InverseDynamics(states[s].q.data(), states[s].v.data(), states[s].a.data(), true, &want.full[(size_t)s * nv]);
      for (int j = 0; j < nv; ++j) {
        e[j] = 1.0;
        d->InverseDynamics(states[s].q.data(), zero.data(), e.data(), false, &want.colfd[((size_t)s * nv + j) * nv]);
        e[j] = 0.0;
      }
    }
    compare(label, inst, "", got, want);
  }
  if (chain != "-") {
    const HostModel hc(chain);
    if (hc.M.nq != nq || hc.M.nv != nv) die(path + ": the chain form has other sizes");
    const Results want = evaluate(hc, cp, states);
    compare(label, inst, std::string("==chain") + hc.Instantiation(), got, want);
  }
  if (golden) {
    int ok = 0;
    double worst = 0.0;
    for (int s = 0; s < S; ++s) {
      double err = 0.0;
      for (int i = 0; i < nv; ++i) {
        const double d = std::fabs(got.full[(size_t)s * nv + i] - states[s].tau[i]) / states[s].scale;
        if (!(d <= err)) err = d;
      }
      if (!(err <= worst)) worst = err;
      ok += err <= 1e-7;
      if (!(err <= 1e-7)) std::fprintf(stderr, "%s golden: state %d is %.3e of its scale off the stored tau\n", label.c_str(), s, err);
    }
    std::fprintf(stderr, "%s golden: worst |tau - stored| / scale %.3e\n", label.c_str(), worst);
    report(label, inst, "golden", ok, S);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) die("usage: id_eval_host_check CASEFILE...");
  for (int i = 1; i < argc; ++i) run_case(argv[i]);
  if (failures) std::printf("FAILED: %d lines\n", failures);
  else std::printf("ok: every line equal\n");
  return failures ? 1 : 0;
}
