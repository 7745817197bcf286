// scene_report_host_check.cc — csrc/scene_report.h scene_block_body, the unmodified device text, run on the host as a whole
// block (tests/cpp/lane_emu: a lane is an OS thread, __syncthreads a barrier) inside exactly the LDS the launch would request:
// everything behind it is poisoned for the address sanitizer, everything inside starts as NaN.  Built and run by
// tests/test_scene_report_host.py with the address and undefined-behaviour sanitizers and a second time with the thread
// sanitizer (a missing barrier is a data race).  What this can and cannot show: lane_emu/hip/hip_runtime.h.
//
// usage: scene_report_host_check CASEFILE...     a case file (written by the test):
//   label NAME  dev MODEL  orc MODEL|-  contact k vd vs mu sigma  dump PATH|-  states S, then S times: q[nq] v[nv]
// (orc -: a model the oracle cannot express, as it is: the forces and tau_sum lines alone, and the dump)
// The states run as a batch of two problems - problem 1 takes them in reverse order - on the grid (S, 2).  All with ==:
//   bodies    every body's R, p, w, v against oracle::Dynamics::Kinematics
//   pairs     every pair's phi, n, Ca, Cb against oracle::SignedDistance on the oracle's geometry poses, active against
//             phi <= threshold, the padding 0, an inactive pair's fn and f zero
//   forces    every ACTIVE pair's f and the moments cross(pAC, -f), cross(pBC, f) against contact_pair (id_eval.h) on the same
//             two BodyStates
//   body_sums the per-body sums of those wrenches against oracle::Dynamics::ContactForces, accumulated in the order of
//             ascending pair index from +0 per body, the common body per path and then the butterfly
//   tau_sum   tau_contact against the ascending sum of tau_pairs from +0; an inactive pair's row all zero
// One line per (label, check) with equal/compared, then `LABEL identity X`: the largest |tau_contact - (ID without pairs -
// ID with pairs)| / max(1, |tau|_inf) over the states, the oracle's two inverse dynamics at a = 0 (printed, not judged here).
// dump: bodies | pairs | tau_contact | tau_pairs of problem 0 as raw doubles, for the fixtures' test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "lane_emu/host_model.h"
#include "scene_report.h"

namespace idto_dev {
constexpr size_t kLdsDoubles = (size_t)1 << 16;
alignas(64) double lds[kLdsDoubles];
}  // namespace idto_dev

using namespace lane_emu;
using idto_dev::BodyState;
using idto_dev::DevContact;
using idto_dev::DevModel;
using idto_dev::SceneArgs;

namespace {

int failures = 0;

void report(const std::string& label, const char* what, long ok, long n) {
  std::printf("%s %s %ld/%ld\n", label.c_str(), what, ok, n);
  if (ok != n) ++failures;
}
bool note(bool ok, const std::string& label, int b, int s, int k, const char* what) {
  static int shown = 0;
  if (!ok && shown++ < 16) std::fprintf(stderr, "%s problem %d state %d item %d: %s differs\n", label.c_str(), b, s, k, what);
  return ok;
}
bool eq3(const double* a, oracle::V3 b) { return same(a[0], b.x) && same(a[1], b.y) && same(a[2], b.z); }
bool eq3(idto_dev::V3 a, oracle::V3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
oracle::V3 v3(const double* a) { return oracle::V3{a[0], a[1], a[2]}; }

BodyState state_of(const double* bodies, int body) {
  if (body >= 0) return idto_dev::get_state(bodies + (size_t)body * idto_dev::SCENE_BODY);
  BodyState w;
  w.R = idto_dev::ident3(); w.p = idto_dev::mk(0, 0, 0); w.w = w.p; w.v = w.p;
  return w;
}

struct Outputs { std::vector<double> bodies, pairs, tau, rows; };

// the grid (S, B): a block per state and problem, each inside exactly the LDS the launch would request
Outputs run_blocks(const HostModel& h, const DevContact& cp, const std::vector<double>& x, int B, int S) {
  const DevModel& M = h.M;
  const int nq = M.nq, nv = M.nv, nb = M.nb, np = M.npairs;
  const idto_model_t cm = h.mf.c_model();
  Outputs o;
  o.bodies.assign((size_t)B * S * nb * idto_dev::SCENE_BODY, NAN); o.pairs.assign((size_t)B * S * np * idto_dev::SCENE_PAIR, NAN);
  o.tau.assign((size_t)B * S * nv, NAN); o.rows.assign((size_t)B * S * np * nv, NAN);
  SceneArgs A{};
  A.M = M; A.cp = cp; A.geom_body = cm.geom_body; A.x = x.data(); A.nstates = S;
  A.bodies = o.bodies.data(); A.pairs = o.pairs.data(); A.tau_contact = o.tau.data(); A.tau_pairs = o.rows.data();
  const int threads = idto_dev::scene_block(nb, nv, np);
  const size_t usable = idto_dev::scene_lds_doubles(nb, nq, nv, np, M.blob_n);
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < S; ++s) {
      lds_prepare(idto_dev::lds, idto_dev::kLdsDoubles, usable);
      launch(s, threads, [&]() { idto_dev::scene_block_body(M, cp, A, (int)blockIdx.x, b); });
      lds_release(idto_dev::lds, idto_dev::kLdsDoubles);
    }
  return o;
}

// problem 0's bodies | pairs | tau_contact | tau_pairs as raw doubles
void write_dump(const std::string& dump, const Outputs& o, int S, int nb, int np, int nv) {
  if (dump == "-") return;
  std::FILE* f = std::fopen(dump.c_str(), "wb");
  if (!f) die("cannot write " + dump);
  const size_t one[4] = {(size_t)S * nb * idto_dev::SCENE_BODY, (size_t)S * np * idto_dev::SCENE_PAIR, (size_t)S * nv, (size_t)S * np * nv};
  const double* src[4] = {o.bodies.data(), o.pairs.data(), o.tau.data(), o.rows.data()};
  for (int i = 0; i < 4; ++i)
    if (one[i] && std::fwrite(src[i], sizeof(double), one[i], f) != one[i]) die("short write to " + dump);
  std::fclose(f);
}

// orc "-": a model that the oracle cannot express (capsules with length, the per-body gravity switch) as it is - the checks
// that need no oracle (forces against contact_pair, tau_sum) and the dump for the independent fixtures
void run_as_it_is(const std::string& label, const HostModel& h, const DevContact& cp, const std::vector<double>& x, int S,
                  const std::string& dump) {
  const DevModel& M = h.M;
  const int nv = M.nv, nb = M.nb, np = M.npairs, B = 2, BD = idto_dev::SCENE_BODY, PD = idto_dev::SCENE_PAIR;
  const idto_model_t cm = h.mf.c_model();
  const Outputs o = run_blocks(h, cp, x, B, S);
  long ok_f = 0, n_f = 0, ok_t = 0, n_t = 0;
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < S; ++s) {
      const size_t st = (size_t)b * S + s;
      const double* bo = o.bodies.data() + st * nb * BD;
      const double* ro = o.rows.data() + st * np * nv;
      for (int pi = 0; pi < np; ++pi) {
        const double* r = o.pairs.data() + (st * np + pi) * PD;
        if (r[IDTO_SCENE_PAIR_ACTIVE] != 1.0) continue;
        ++n_f;
        const BodyState SA = state_of(bo, cm.geom_body[M.pair_ga[pi]]), SB = state_of(bo, cm.geom_body[M.pair_gb[pi]]);
        const idto_dev::PairForce pf = idto_dev::contact_pair(M, cp, M.pair_ga[pi], M.pair_gb[pi], SA, SB);
        const oracle::V3 f = v3(r + IDTO_SCENE_PAIR_F), mf = oracle::V3{-f.x, -f.y, -f.z};
        const oracle::V3 pC = (v3(r + IDTO_SCENE_PAIR_CA) + v3(r + IDTO_SCENE_PAIR_CB)) * 0.5;
        const oracle::V3 pAC = pC - oracle::V3{SA.p.x, SA.p.y, SA.p.z}, pBC = pC - oracle::V3{SB.p.x, SB.p.y, SB.p.z};
        ok_f += note(pf.active && eq3(pf.fB, f) && eq3(pf.fA, mf) && eq3(pf.nA, oracle::cross(pAC, mf)) && eq3(pf.nB, oracle::cross(pBC, f)),
                     label, b, s, pi, "an active pair's f or moments (contact_pair)");
      }
      bool e = true;
      for (int j = 0; j < nv; ++j) {
        double sum = 0.0;
        for (int pi = 0; pi < np; ++pi) sum = sum + ro[(size_t)pi * nv + j];
        e = note(same(sum, o.tau[st * nv + j]), label, b, s, j, "tau_contact (the ascending sum of tau_pairs)") && e;
      }
      ok_t += e; ++n_t;
    }
  report(label, "forces", ok_f, n_f);
  report(label, "tau_sum", ok_t, n_t);
  write_dump(dump, o, S, nb, np, nv);
}

void run_case(const std::string& path) {
  Tokens in(path);
  in.expect("label"); const std::string label = in.next();
  in.expect("dev"); const HostModel h(in.next());
  in.expect("orc"); const std::string orc = in.next();
  in.expect("contact"); const std::vector<double> cv = in.nums(5);
  in.expect("dump"); const std::string dump = in.next();
  in.expect("states"); const int S = in.integer();
  const DevModel& M = h.M;
  const int nq = M.nq, nv = M.nv, nb = M.nb, np = M.npairs, w = nq + nv, B = 2;
  std::vector<double> x((size_t)B * S * w);
  for (int s = 0; s < S; ++s) {
    const std::vector<double> qv = in.nums(w);
    std::copy(qv.begin(), qv.end(), x.begin() + (size_t)s * w);
    std::copy(qv.begin(), qv.end(), x.begin() + ((size_t)S + (S - 1 - s)) * w);
  }
  if (in.more()) die(path + ": tokens behind the last state");
  const DevContact cp = DevContactOf(cv.data());
  if (orc == "-") return run_as_it_is(label, h, cp, x, S, dump);
  const std::unique_ptr<oracle::Dynamics> d = OracleOf(orc, cv.data());
  const oracle::Model& om = d->model;
  if (om.nq != nq || om.nv != nv || om.nb != nb || om.npairs != np || d->contact.threshold != cp.threshold)
    die(path + ": the oracle's model or threshold is not the device's");
  oracle::Dynamics pairless = *d;
  pairless.model.npairs = 0;
  const idto_model_t cm = h.mf.c_model();
  const int BD = idto_dev::SCENE_BODY, PD = idto_dev::SCENE_PAIR;
  const Outputs out = run_blocks(h, cp, x, B, S);
  const std::vector<double>&bodies = out.bodies, &pairs = out.pairs, &tau = out.tau, &rows = out.rows;

  long ok_b = 0, n_b = 0, ok_p = 0, n_p = 0, ok_f = 0, n_f = 0, ok_s = 0, n_s = 0, ok_t = 0, n_t = 0;
  double identity = 0.0;
  const std::vector<double> zero(nv, 0.0);
  const oracle::V3 z3{0, 0, 0};
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < S; ++s) {
      const size_t st = (size_t)b * S + s;
      const double* q = x.data() + st * w;
      const double* v = q + nq;
      const double* bo = bodies.data() + st * nb * BD;
      const double* po = pairs.data() + st * np * PD;
      const double* to = tau.data() + st * nv;
      const double* ro = rows.data() + st * np * nv;
      std::vector<oracle::BodyKin> kin;
      d->Kinematics(q, v, zero.data(), &kin);
      for (int i = 0; i < nb; ++i, ++n_b) {
        const double* r = bo + (size_t)i * BD;
        ok_b += note(same(r, kin[i].R.m, 9) && eq3(r + 9, kin[i].p) && eq3(r + 12, kin[i].w) && eq3(r + 15, kin[i].v), label, b, s, i, "a body's R, p, w, v");
      }
      // ---- pairs: geometry against the oracle, forces against contact_pair, the sums against ContactForces
      std::vector<oracle::Wrench> ext(nb);
      oracle::V3 cf[IDTO_MAX_PATHS], cn[IDTO_MAX_PATHS];
      for (int k = 0; k < IDTO_MAX_PATHS; ++k) cf[k] = cn[k] = z3;
      for (int pi = 0; pi < np; ++pi, ++n_p) {
        const double* r = po + (size_t)pi * PD;
        const int ga = om.pair_a[pi], gb = om.pair_b[pi], ba = om.geom_body[ga], bb = om.geom_body[gb];
        const oracle::M3 RbA = ba < 0 ? oracle::Identity3() : kin[ba].R, RbB = bb < 0 ? oracle::Identity3() : kin[bb].R;
        const oracle::V3 pbA = ba < 0 ? z3 : kin[ba].p, pbB = bb < 0 ? z3 : kin[bb].p;
        const oracle::SignedDistanceResult sd =
            oracle::SignedDistance(om.geom_type[ga], RbA * om.geom_R[ga], pbA + RbA * om.geom_p[ga], om.geom_size[ga], om.geom_type[gb],
                                   RbB * om.geom_R[gb], pbB + RbB * om.geom_p[gb], om.geom_size[gb]);
        const bool active = r[IDTO_SCENE_PAIR_ACTIVE] == 1.0;
        bool e = same(r[IDTO_SCENE_PAIR_PHI], sd.phi) && eq3(r + IDTO_SCENE_PAIR_N, sd.n) && eq3(r + IDTO_SCENE_PAIR_CA, sd.Ca) &&
                 eq3(r + IDTO_SCENE_PAIR_CB, sd.Cb);
        e = note(e, label, b, s, pi, "a pair's phi, n, Ca, Cb");
        e = note((r[IDTO_SCENE_PAIR_ACTIVE] == 1.0 || r[IDTO_SCENE_PAIR_ACTIVE] == 0.0) && active == (sd.phi <= d->contact.threshold) &&
                     r[IDTO_SCENE_PAIR_PAD] == 0.0, label, b, s, pi, "a pair's active flag or padding") && e;
        if (!active) {
          bool zf = r[IDTO_SCENE_PAIR_FN] == 0.0;
          for (int i = 0; i < 3; ++i) zf = zf && r[IDTO_SCENE_PAIR_F + i] == 0.0;
          for (int j = 0; j < nv; ++j) zf = zf && ro[(size_t)pi * nv + j] == 0.0;
          e = note(zf, label, b, s, pi, "an inactive pair's fn, f or row (not zero)") && e;
        }
        ok_p += e;
        if (!active) continue;
        ++n_f;
        const BodyState SA = state_of(bo, cm.geom_body[h.M.pair_ga[pi]]), SB = state_of(bo, cm.geom_body[h.M.pair_gb[pi]]);
        const idto_dev::PairForce pf = idto_dev::contact_pair(M, cp, M.pair_ga[pi], M.pair_gb[pi], SA, SB);
        const oracle::V3 f = v3(r + IDTO_SCENE_PAIR_F), mf = oracle::V3{-f.x, -f.y, -f.z};
        const oracle::V3 pC = (v3(r + IDTO_SCENE_PAIR_CA) + v3(r + IDTO_SCENE_PAIR_CB)) * 0.5;
        const oracle::V3 pAC = pC - pbA, pBC = pC - pbB;
        const oracle::V3 nA = oracle::cross(pAC, mf), nB = oracle::cross(pBC, f);
        ok_f += note(pf.active && eq3(pf.fB, f) && eq3(pf.fA, mf) && eq3(pf.nA, nA) && eq3(pf.nB, nB), label, b, s, pi,
                     "an active pair's f or moments (contact_pair)");
        const int path = om.pair_path[pi];
        if (ba >= 0) {
          if (ba == om.common_body) { cf[path] = cf[path] + mf; cn[path] = cn[path] + nA; }
          else { ext[ba].f = ext[ba].f + mf; ext[ba].n = ext[ba].n + nA; }
        }
        if (bb >= 0) {
          if (bb == om.common_body) { cf[path] = cf[path] + f; cn[path] = cn[path] + nB; }
          else { ext[bb].f = ext[bb].f + f; ext[bb].n = ext[bb].n + nB; }
        }
      }
      if (om.common_body >= 0) {
        ext[om.common_body].f = oracle::TreeSum(cf, om.npaths);
        ext[om.common_body].n = oracle::TreeSum(cn, om.npaths);
      }
      if (np > 0) {
        std::vector<oracle::Wrench> want;
        d->ContactForces(kin, &want);
        bool e = true;
        for (int i = 0; i < nb; ++i)
          e = note(same(&ext[i].f.x, &want[i].f.x, 3) && same(&ext[i].n.x, &want[i].n.x, 3), label, b, s, i, "a body's contact wrench (ContactForces)") && e;
        ok_s += e; ++n_s;
      }
      // ---- tau_contact: the ascending sum of the rows, and the identity with the oracle's two inverse dynamics
      bool e = true;
      for (int j = 0; j < nv; ++j) {
        double sum = 0.0;
        for (int pi = 0; pi < np; ++pi) sum = sum + ro[(size_t)pi * nv + j];
        e = note(same(sum, to[j]), label, b, s, j, "tau_contact (the ascending sum of tau_pairs)") && e;
      }
      ok_t += e; ++n_t;
      std::vector<double> with(nv), without(nv);
      d->InverseDynamics(q, v, zero.data(), true, with.data());
      pairless.InverseDynamics(q, v, zero.data(), true, without.data());
      double scale = 1.0, worst = 0.0;
      for (int j = 0; j < nv; ++j) scale = std::max(scale, std::max(std::fabs(with[j]), std::fabs(without[j])));
      for (int j = 0; j < nv; ++j) worst = std::max(worst, std::fabs(to[j] - (without[j] - with[j])));
      if (!(worst / scale <= identity)) identity = worst / scale;   // (a NaN sticks)
    }
  report(label, "bodies", ok_b, n_b);
  report(label, "pairs", ok_p, n_p);
  report(label, "forces", ok_f, n_f);
  report(label, "body_sums", ok_s, n_s);
  report(label, "tau_sum", ok_t, n_t);
  std::printf("%s identity %.3e\n", label.c_str(), identity);
  write_dump(dump, out, S, nb, np, nv);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) die("usage: scene_report_host_check CASEFILE...");
  for (int i = 1; i < argc; ++i) run_case(argv[i]);
  if (failures) std::printf("FAILED: %d lines\n", failures);
  else std::printf("ok: every line equal\n");
  return failures ? 1 : 0;
}
