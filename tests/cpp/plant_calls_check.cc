// plant_calls_check.cc — csrc/host/plant_calls.cc on the CPU, under the address and undefined-behaviour sanitizers
// (tests/test_plant_calls.py compiles and runs it): every layout of tests/golden/plant_call_layouts.txt line by line, the one
// block and LDS rule against the two pairs it replaced, and every refusal of every entry by its exact message - with
// double-fault calls that pin the order of the checks - beside one accepted call per entry.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "host/plant_calls.h"
#include "plant_sizes.h"

using namespace idto_host;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static PlantShape Shape(int batch, int nq, int nv) {
  PlantShape s{};
  s.batch = batch; s.nq = nq; s.nv = nv; s.nb = 2; s.npairs = 1; s.ngeoms = 2; s.blob_n = 120; s.nxb = 0; s.nstem = 0; s.npaths = 1; s.maxc = 2;
  s.host_model = true;
  return s;
}

// ---- layouts

static std::string Format(const std::string& head, const CallPlan& p) {
  std::ostringstream o;
  o << head << " :";
  for (const CallEntry& e : p.entries) o << " " << e.name << "@" << e.offset << "+" << e.count;
  o << " | in_n=" << p.in_n << " out0=" << p.out0 << " total=" << p.total << " pinned=" << p.pinned;
  return o.str();
}

static void Layouts(const char* golden) {
  std::ifstream in(golden);
  CHECK(in.good(), "cannot read %s", golden);
  std::map<std::string, int> seen;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    const std::string head = line.substr(0, line.find(" :"));
    std::istringstream h(head);
    std::string kind;
    int a[7] = {0, 0, 0, 0, 0, 0, 0};
    h >> kind;
    for (int& v : a) h >> v;
    PlantShape s = Shape(a[0], a[1], a[2]);
    CallPlan p;
    if (kind == "storage") p = PlanPlantStorage(s, (size_t)a[3], a[4], a[5]);
    else if (kind == "scene") { s.nb = a[3]; s.npairs = a[4]; p = PlanScene(s, a[5], (unsigned)a[6]); }
    else if (kind == "lin") p = PlanLin(s, a[3], a[4] != 0, a[5]);
    else if (kind == "track") p = PlanTrack(s, a[3], a[4], a[5], a[6] != 0);
    else CHECK(false, "unknown kind in: %s", line.c_str());
    const std::string mine = Format(head, p);
    CHECK(mine == line, "layout differs\n  recorded: %s\n  planned:  %s", line.c_str(), mine.c_str());
    // what every kernel pointer relies on: 64-byte boundaries, no overlap on the device, the mirror holds what lands in it
    size_t end = 0;
    for (const CallEntry& e : p.entries) {
      if ((kind == "storage" || kind == "track") && &e == &p.entries.back()) continue;   // (status_back: a place in the mirror alone)
      CHECK(e.offset % 8 == 0 && e.offset >= end && e.offset + e.count <= p.total, "%s: entry %s", head.c_str(), e.name);
      end = e.offset + e.count;
    }
    CHECK(p.pinned >= p.in_n && p.pinned >= p.entries.back().offset + p.entries.back().count - p.out0, "%s: the mirror is too small", head.c_str());
    ++seen[kind];
  }
  // 2 shapes x 2 batches x (capacity 2 x nu 3 | S 2 x 15 masks | S 2 x (off, nu 1, nu nv) | S 2 x R 2 x nu 2 x own_K 2)
  CHECK(seen["storage"] == 24 && seen["scene"] == 120 && seen["lin"] == 24 && seen["track"] == 64, "lines: %d storage, %d scene, %d lin, %d track",
        seen["storage"], seen["scene"], seen["lin"], seen["track"]);
  CHECK(PlantRecordCapacity(0) == 64 && PlantRecordCapacity(5) == 5, "record_capacity 0 is 64");
  // plant_storage / scene / lin / track name the entries in the tables' order
  CHECK(std::string(PlanLin(Shape(1, 2, 2), 1, true, 1).entries[lin::lqr_status].name) == "lqr_status" && lin::count == 16, "lin's names");
  CHECK(std::string(PlanTrack(Shape(1, 2, 2), 1, 1, 1, true).entries[track::status_back].name) == "status_back", "track's names");
  CHECK(std::string(PlanPlantStorage(Shape(1, 2, 2), 9, 0, 0).entries[plant_storage::status_back].name) == "status_back", "the storage's names");
  CHECK(std::string(PlanScene(Shape(1, 2, 2), 1, 15).entries[scene::tau_pairs].name) == "tau_pairs" && scene::count == 4, "the scene's names");
}

// ---- the block and LDS rule against the two pairs it replaced (restated from plant_abi.inc and track_abi.inc as they stood)

static int OldPlantLdsBytes(const PlantShape& c, int threads, bool pd) {
  size_t d = (size_t)idto_dev::plant_lds_doubles(c.nq, c.nv, c.blob_n, c.nxb, c.nstem, c.npaths, threads);
  if (pd) d += idto_dev::plant_pd_doubles(c.nq, c.nv, c.mpc_nu, c.mpc_n, c.mpc_len);
  return d > (size_t)1 << 24 ? 1 << 27 : (int)(d * sizeof(double));
}
static int OldPlantBlock(const PlantShape& c, int forced, bool pd) {
  int t = forced ? forced : std::min(256, (((c.nv + 1) * c.npaths + 63) / 64) * 64);
  while (t > 64 && OldPlantLdsBytes(c, t, pd) > 160 * 1024) t -= 64;
  return t;
}
static int OldTrackLdsBytes(const PlantShape& c, int threads, int nu) {
  const size_t d = (size_t)idto_dev::plant_lds_doubles(c.nq, c.nv, c.blob_n, c.nxb, c.nstem, c.npaths, threads) + idto_dev::plant_law_doubles(c.nq, c.nv, nu);
  return d > (size_t)1 << 24 ? 1 << 27 : (int)(d * sizeof(double));
}
static int OldTrackBlock(const PlantShape& c, int nu) {
  int t = std::min(256, (((c.nv + 1) * c.npaths + 63) / 64) * 64);
  while (t > 64 && OldTrackLdsBytes(c, t, nu) > 160 * 1024) t -= 64;
  return t;
}

static int g_block_cases = 0;
static void BlockAndLds() {
  for (int shape = 0; shape < 2; ++shape)
    for (int batch : {1, 3})
      for (int variant = 0; variant < 3; ++variant) {   // plain | shared pairs and a stem, eight paths | an exchange that makes the block shrink
        PlantShape s = Shape(batch, shape ? 7 : 2, shape ? 6 : 2);
        if (variant >= 1) { s.nxb = 9; s.nstem = 3; s.npaths = 8; }
        if (variant == 2) s.nxb = 40;   // (984 doubles an evaluation: 32 and 24 concurrent ones do not fit, 16 do)
        s.mpc = true; s.mpc_nu = s.nv; s.mpc_n = 7; s.mpc_len = 3 * 7 * (size_t)(s.nq + 2 * s.nv);
        for (int threads = 64; threads <= 256; threads += 64)
          for (int nu : {1, s.nv}) {
            const size_t law = idto_dev::plant_law_doubles(s.nq, s.nv, nu);
            CHECK(PlantLdsBytes(s, threads, 0) == OldPlantLdsBytes(s, threads, false), "LDS, hold");
            CHECK(PlantLdsBytes(s, threads, PlantPdDoubles(s)) == OldPlantLdsBytes(s, threads, true), "LDS, PD+");
            CHECK(PlantLdsBytes(s, threads, law) == OldTrackLdsBytes(s, threads, nu), "LDS, the law");
            for (int forced : {0, threads}) {
              CHECK(PlantBlock(s, forced, 0) == OldPlantBlock(s, forced, false), "block, hold");
              CHECK(PlantBlock(s, forced, PlantPdDoubles(s)) == OldPlantBlock(s, forced, true), "block, PD+");
            }
            CHECK(PlantBlock(s, 0, law) == OldTrackBlock(s, nu), "block, the law");
            ++g_block_cases;
          }
        if (variant == 2) CHECK(PlantBlock(s, 256, 0) == 128 && PlantLdsBytes(s, 192, 0) > kPlantMaxLds, "the block shrinks to fit: %d", PlantBlock(s, 256, 0));
      }
  PlantShape big = Shape(1, 2, 2);
  big.blob_n = 1 << 25;   // beyond 2^24 doubles: the guard, not an int that wrapped
  CHECK(PlantLdsBytes(big, 64, 0) == 1 << 27 && PlantLdsBytes(big, 64, 5) == 1 << 27 && PlantBlock(big, 0, 0) == 64, "the overflow guard");
}

// ---- refusals

static std::map<std::string, int> g_refused, g_accepted;
static void Expect(const char* entry, const Refusal& r, const std::string& msg, int line) {
  if (msg.empty()) {
    ++g_accepted[entry];
    if (r.rc != 0 || !r.msg.empty()) { ++g_fail; std::printf("FAIL line %d: %s refused a valid call: %s\n", line, entry, r.msg.c_str()); }
  } else {
    ++g_refused[entry];
    if (r.rc != -1 || r.msg != msg) { ++g_fail; std::printf("FAIL line %d: %s\n  expected: %s\n  got (%d): %s\n", line, entry, msg.c_str(), r.rc, r.msg.c_str()); }
  }
}
#define EXPECT(entry, refusal, msg) Expect(entry, refusal, msg, __LINE__)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const char* kChildren = ": this context has child contexts (the child-context route of idto_hip_tr_solve_batch_constrained made them)";
static const char* kSubsteps = ": substeps must be in [1, 4096] (a single launch stays short on a shared device)";
static const char* kBegin = ": call idto_hip_plant_begin on the context first";
static const char* kModels = ": models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS";
static const char* kPlantsAsked = ": the plants' models were asked for: call idto_hip_plant_begin on the context first";
static const char* kServes = ": nv > 64 (the solve of M a = tau - c runs a lane per row on one wavefront)";
static const char* kH = ": the substep h must be > 0 and finite";
static std::string W(const char* who, const char* rest) { return std::string(who) + rest; }

static PlantShape Begun(PlantShape s, int mode) {
  s.plants_begun = true; s.plant_mode = mode; s.plant_record_capacity = 5; s.plant_block = 64;
  if (mode == IDTO_PLANT_PD_PLUS) {
    s.mpc = true; s.mpc_nu = 1; s.mpc_n = 4; s.mpc_len = 40; s.plant_nu = 1; s.plant_mpc_current = true;
    s.plant_lds = PlantLdsBytes(s, 64, PlantPdDoubles(s));
  } else {
    s.plant_lds = PlantLdsBytes(s, 64, 0);
  }
  return s;
}

static void PlantEntries() {
  const PlantShape s = Shape(2, 2, 2);
  PlantShape kids = s; kids.children = true;
  PlantShape wide = s; wide.nv = 65;
  PlantShape heavy = s; heavy.blob_n = 30000;   // 240 KB of model: no block fits
  // plant_begin
  const char* e = "plant_begin";
  idto_plant_params_t ok{};
  ok.h = 1e-3; ok.mode = IDTO_PLANT_HOLD;
  auto with = [&](auto edit) { idto_plant_params_t p = ok; edit(p); return p; };
  idto_plant_params_t p;
  EXPECT(e, RefusePlantBegin(s, nullptr), "plant_begin: parameters are required");
  EXPECT(e, RefusePlantBegin(kids, &ok), W(e, kChildren));
  for (double h : {0.0, -1.0, kInf, kNan}) { p = with([&](auto& q) { q.h = h; }); EXPECT(e, RefusePlantBegin(s, &p), "plant_begin: the substep h must be > 0"); }
  p = with([](auto& q) { q.mode = 2; }); EXPECT(e, RefusePlantBegin(s, &p), "plant_begin: mode is IDTO_PLANT_HOLD or IDTO_PLANT_PD_PLUS");
  EXPECT(e, RefusePlantBegin(wide, &ok), W(e, kServes));
  for (int t : {32, 100, 320, -64}) { p = with([&](auto& q) { q.block_threads = t; }); EXPECT(e, RefusePlantBegin(s, &p), "plant_begin: block_threads is 0, 64, 128, 192 or 256"); }
  p = with([](auto& q) { q.record_capacity = -1; }); EXPECT(e, RefusePlantBegin(s, &p), "plant_begin: record_capacity must not be negative");
  idto_plant_params_t pd = ok;
  double Kp[2] = {1, 2}, Kd[2] = {3, 4};
  pd.mode = IDTO_PLANT_PD_PLUS; pd.Kp = Kp; pd.kp_size = 2; pd.Kd = Kd; pd.kd_size = 2;
  EXPECT(e, RefusePlantBegin(s, &pd), "plant_begin: PD+ needs the stored plans: call idto_hip_mpc_batch_begin (and idto_hip_mpc_batch_store) on the context first");
  PlantShape m = s; m.mpc = true; m.mpc_nu = 1; m.mpc_n = 4; m.mpc_len = 40;
  const char* sizes = "plant_begin: gains of the wrong size: Kp is [nu][nq] = 2 and Kd [nu][nv] = 2 doubles";
  p = pd; p.Kp = nullptr; EXPECT(e, RefusePlantBegin(m, &p), sizes);
  p = pd; p.Kd = nullptr; EXPECT(e, RefusePlantBegin(m, &p), sizes);
  p = pd; p.kp_size = 3; EXPECT(e, RefusePlantBegin(m, &p), sizes);
  p = pd; p.kd_size = 1; EXPECT(e, RefusePlantBegin(m, &p), sizes);
  Kp[1] = kNan; EXPECT(e, RefusePlantBegin(m, &pd), "plant_begin: a gain in Kp is not finite");
  Kd[0] = kInf; EXPECT(e, RefusePlantBegin(m, &pd), "plant_begin: a gain in Kp is not finite");   // (both: Kp's first)
  Kp[1] = 2; EXPECT(e, RefusePlantBegin(m, &pd), "plant_begin: a gain in Kd is not finite");
  Kd[0] = 3;
  PlantShape nohost = s; nohost.host_model = false;
  EXPECT(e, RefusePlantStorage(nohost, 0, false), "plant_begin: the context keeps no host copy of its model");
  EXPECT(e, RefusePlantStorage(heavy, 0, false), "plant_begin: the model, a substep's evaluations and the plan do not fit the 160 KiB of LDS");
  PlantShape plans = m; plans.mpc_len = 25000;   // the plans alone are beyond the LDS
  EXPECT(e, RefusePlantStorage(plans, 64, true), "plant_begin: the model, a substep's evaluations and the plan do not fit the 160 KiB of LDS");
  nohost.blob_n = 30000; EXPECT(e, RefusePlantStorage(nohost, 0, false), "plant_begin: the context keeps no host copy of its model");   // (both)
  p = with([](auto& q) { q.h = 0; q.mode = 7; }); EXPECT(e, RefusePlantBegin(s, &p), "plant_begin: the substep h must be > 0");   // (both)
  p = with([](auto& q) { q.h = 0; }); EXPECT(e, RefusePlantBegin(kids, &p), W(e, kChildren));                                      // (both)
  p = with([](auto& q) { q.mode = 7; q.block_threads = 1; }); EXPECT(e, RefusePlantBegin(wide, &p), "plant_begin: mode is IDTO_PLANT_HOLD or IDTO_PLANT_PD_PLUS");
  EXPECT(e, RefusePlantBegin(s, &ok), ""); EXPECT(e, RefusePlantBegin(m, &pd), ""); EXPECT(e, RefusePlantStorage(m, 0, true), "");
  for (int t : {64, 128, 192, 256}) { p = with([&](auto& q) { q.block_threads = t; q.record_capacity = 5; }); EXPECT(e, RefusePlantBegin(s, &p), ""); }

  const PlantShape hold = Begun(s, IDTO_PLANT_HOLD), pdp = Begun(s, IDTO_PLANT_PD_PLUS);
  const double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // plant_set_model's index, plant_set_state, plant_get_state
  e = "plant_set_model";
  EXPECT(e, RefusePlantSetModel(s, 0), W(e, kBegin));
  EXPECT(e, RefusePlantSetModel(hold, -1), "plant_set_model: plant index outside the batch");
  EXPECT(e, RefusePlantSetModel(hold, 2), "plant_set_model: plant index outside the batch");
  EXPECT(e, RefusePlantSetModel(s, -1), W(e, kBegin)); EXPECT(e, RefusePlantSetModel(s, 2), W(e, kBegin));   // (both)
  EXPECT(e, RefusePlantSetModel(hold, 0), ""); EXPECT(e, RefusePlantSetModel(hold, 1), "");
  e = "plant_set_state";
  EXPECT(e, RefusePlantSetState(s, x, x), W(e, kBegin));
  EXPECT(e, RefusePlantSetState(hold, nullptr, x), "plant_set_state: times[batch] and x[batch][nq + nv] are required");
  EXPECT(e, RefusePlantSetState(hold, x, nullptr), "plant_set_state: times[batch] and x[batch][nq + nv] are required");
  EXPECT(e, RefusePlantSetState(s, nullptr, x), W(e, kBegin)); EXPECT(e, RefusePlantSetState(s, x, nullptr), W(e, kBegin));   // (both)
  EXPECT(e, RefusePlantSetState(hold, x, x), "");
  e = "plant_get_state";
  EXPECT(e, RefusePlantsBegun(s, e), W(e, kBegin)); EXPECT(e, RefusePlantsBegun(pdp, e), "");

  // plant_step
  e = "plant_step";
  int nrec = -1;
  EXPECT(e, RefusePlantStep(s, e, 1, x, 0, false, &nrec), W(e, kBegin));
  for (int n : {0, -3, 4097}) EXPECT(e, RefusePlantStep(hold, e, n, x, 0, false, &nrec), W(e, kSubsteps));
  EXPECT(e, RefusePlantStep(hold, e, 1, nullptr, 0, false, &nrec), "plant_step: hold mode needs tau_hold[batch][nv]");
  EXPECT(e, RefusePlantStep(pdp, e, 1, x, 0, false, &nrec), "plant_step: PD+ forms the torque itself: tau_hold must be NULL");
  const char* again = "plant_step: PD+: idto_hip_mpc_batch_begin was called again after idto_hip_plant_begin (call idto_hip_plant_begin again)";
  PlantShape q = pdp; q.mpc = false; EXPECT(e, RefusePlantStep(q, e, 1, nullptr, 0, false, &nrec), again);
  q = pdp; q.plant_mpc_current = false; EXPECT(e, RefusePlantStep(q, e, 1, nullptr, 0, false, &nrec), again);
  q = pdp; q.mpc_nu = 2; EXPECT(e, RefusePlantStep(q, e, 1, nullptr, 0, false, &nrec), again);
  q = pdp; q.mpc_len = 48; EXPECT(e, RefusePlantStep(q, e, 1, nullptr, 0, false, &nrec), again);
  EXPECT(e, RefusePlantStep(hold, e, 10, x, 0, true, &nrec), "plant_step: record_every must be >= 1 with x_record_out");
  EXPECT(e, RefusePlantStep(hold, e, 12, x, 2, true, &nrec), "plant_step: more recorded states than idto_hip_plant_begin's record_capacity");
  EXPECT(e, RefusePlantStep(s, e, 0, nullptr, 0, true, &nrec), W(e, kBegin));                                            // (all)
  EXPECT(e, RefusePlantStep(hold, e, 0, nullptr, 0, true, &nrec), W(e, kSubsteps));                                      // (three)
  EXPECT(e, RefusePlantStep(hold, e, 1, nullptr, 0, true, &nrec), "plant_step: hold mode needs tau_hold[batch][nv]");   // (two)
  q = pdp; q.mpc = false; EXPECT(e, RefusePlantStep(q, e, 1, x, 0, true, &nrec), "plant_step: PD+ forms the torque itself: tau_hold must be NULL");
  EXPECT(e, RefusePlantStep(hold, e, 11, x, 2, true, &nrec), ""); CHECK(nrec == 5, "plant_step records substeps / record_every states: %d", nrec);
  EXPECT(e, RefusePlantStep(hold, e, 4096, x, 0, false, &nrec), ""); CHECK(nrec == 0, "no record: %d", nrec);
  EXPECT(e, RefusePlantStep(pdp, e, 1, nullptr, 1, true, &nrec), ""); CHECK(nrec == 1, "PD+ records: %d", nrec);
  // idto_hip_mpc_batch_tick_plants' step part
  e = "mpc_batch_tick_plants";
  const char* tracks = "mpc_batch_tick_plants: the plants track the stored plans: idto_hip_plant_begin with IDTO_PLANT_PD_PLUS";
  EXPECT(e, RefuseTickPlantsStep(s, 1), W(e, kBegin));
  EXPECT(e, RefuseTickPlantsStep(hold, 1), tracks);
  EXPECT(e, RefuseTickPlantsStep(pdp, 0), W(e, kSubsteps)); EXPECT(e, RefuseTickPlantsStep(pdp, 4097), W(e, kSubsteps));
  q = pdp; q.plant_mpc_current = false;
  EXPECT(e, RefuseTickPlantsStep(q, 1), "mpc_batch_tick_plants: PD+: idto_hip_mpc_batch_begin was called again after idto_hip_plant_begin (call idto_hip_plant_begin again)");
  EXPECT(e, RefuseTickPlantsStep(s, 0), W(e, kBegin));        // (both)
  EXPECT(e, RefuseTickPlantsStep(hold, 0), tracks);           // (both: the mode's message stands for whatever a hold-mode step refuses)
  EXPECT(e, RefuseTickPlantsStep(q, 0), W(e, kSubsteps));     // (both)
  EXPECT(e, RefuseTickPlantsStep(pdp, 8), "");

  // idto_hip_forward_dynamics
  e = "forward_dynamics";
  const char* fd = "forward_dynamics: x[batch][nq + nv], tau_applied[batch][nv] and a_out[batch][nv] are required";
  EXPECT(e, RefuseForwardDynamics(s, nullptr, x, x), fd); EXPECT(e, RefuseForwardDynamics(s, x, nullptr, x), fd); EXPECT(e, RefuseForwardDynamics(s, x, x, nullptr), fd);
  EXPECT(e, RefuseForwardDynamics(wide, x, x, x), W(e, kServes));
  EXPECT(e, RefuseForwardDynamics(wide, nullptr, x, x), fd); EXPECT(e, RefuseForwardDynamics(wide, x, x, nullptr), fd);   // (both)
  EXPECT(e, RefuseForwardDynamics(s, x, x, x), "");
}

static void SceneEntry() {
  const char* e = "scene_report";
  const PlantShape s = Shape(2, 2, 2), hold = Begun(s, IDTO_PLANT_HOLD);
  std::vector<double> x(2 * 3 * 4, 0.5);
  EXPECT(e, RefuseSceneReport(s, 3, nullptr, 0, 1), "scene_report: x[batch][nstates][nq + nv] is required");
  EXPECT(e, RefuseSceneReport(s, 0, x.data(), 0, 1), "scene_report: nstates must be >= 1");
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), 0, 0), "scene_report: every output is NULL: nothing to report");
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), 2, 1), W(e, kModels)); EXPECT(e, RefuseSceneReport(s, 3, x.data(), -1, 1), W(e, kModels));
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), IDTO_SCENE_MODELS_PLANTS, 1), W(e, kPlantsAsked));
  EXPECT(e, RefuseSceneReport(s, (1 << 20) + 1, x.data(), 0, 1), "scene_report: more than 1048576 states in one call");
  x[(1 * 3 + 2) * 4 + 3] = kNan;
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), 0, 1), "scene_report: x is not finite at problem 1, state 2, index 3");
  x[(0 * 3 + 1) * 4 + 0] = kInf;
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), 0, 1), "scene_report: x is not finite at problem 0, state 1, index 0");   // (the first one)
  PlantShape heavy = s; heavy.blob_n = 30000;
  const char* lds = "scene_report: the model, its bodies' records and its pairs' rows do not fit the 160 KiB of LDS";
  EXPECT(e, RefuseSceneReport(heavy, 3, x.data(), 0, 1), "scene_report: x is not finite at problem 0, state 1, index 0");   // (both)
  EXPECT(e, RefuseSceneReport(s, 0, nullptr, 0, 0), "scene_report: x[batch][nstates][nq + nv] is required");               // (three)
  EXPECT(e, RefuseSceneReport(s, 0, x.data(), 7, 0), "scene_report: nstates must be >= 1");                                 // (three)
  EXPECT(e, RefuseSceneReport(s, 3, x.data(), 7, 1), W(e, kModels));                                                         // (both: models, x)
  EXPECT(e, RefuseSceneReport(s, (1 << 20) + 1, x.data(), IDTO_SCENE_MODELS_PLANTS, 1), W(e, kPlantsAsked));                 // (both)
  std::fill(x.begin(), x.end(), -0.25);
  EXPECT(e, RefuseSceneReport(heavy, 3, x.data(), 0, 1), lds);
  for (unsigned mask = 1; mask < 16; ++mask) EXPECT(e, RefuseSceneReport(s, 3, x.data(), 0, mask), "");
  EXPECT(e, RefuseSceneReport(hold, 1, x.data(), IDTO_SCENE_MODELS_PLANTS, 8), "");
}

// idto_hip_plant_linearize (tv null) and idto_hip_plant_tvlqr
static void LinEntries() {
  const PlantShape s = Shape(2, 2, 2), hold = Begun(s, IDTO_PLANT_HOLD);
  PlantShape kids = s; kids.children = true;
  PlantShape wide = s; wide.nv = 65;
  PlantShape heavy = s; heavy.blob_n = 30000;
  const int S = 3;
  std::vector<double> x(2 * S * 4, 0.5), tau(2 * S * 2, 0.25), Q(16, 1.0), R(4, 1.0), Qf(16, 2.0);
  const int act[2] = {1, 0};
  LinTv tv{2, act, Q.data(), R.data(), Qf.data(), nullptr, nullptr, nullptr};
  for (const LinTv* t : {(const LinTv*)nullptr, (const LinTv*)&tv}) {
    const char* e = t ? "plant_tvlqr" : "plant_linearize";
    auto run = [&](const PlantShape& sh, int nstates, const double* xs, const double* ts, double h, int substeps, double eps, int models) {
      return RefuseLin(sh, e, nstates, xs, ts, h, substeps, eps, models, t);
    };
    const char* req = ": x[batch][nstates][nq + nv] and tau[batch][nstates][nv] are required";
    EXPECT(e, run(s, S, nullptr, tau.data(), 1e-3, 1, 1e-6, 0), W(e, req)); EXPECT(e, run(s, S, x.data(), nullptr, 1e-3, 1, 1e-6, 0), W(e, req));
    EXPECT(e, run(s, 0, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": nstates must be >= 1"));
    for (int n : {0, 4097}) EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, n, 1e-6, 0), W(e, kSubsteps));
    for (double h : {0.0, -1.0, kInf, kNan}) EXPECT(e, run(s, S, x.data(), tau.data(), h, 1, 1e-6, 0), W(e, kH));
    for (double eps : {0.0, -1e-6, kInf, kNan}) EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, eps, 0), W(e, ": eps must be > 0 and finite"));
    EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 2), W(e, kModels));
    EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, IDTO_SCENE_MODELS_PLANTS), W(e, kPlantsAsked));
    EXPECT(e, run(kids, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, kChildren));
    EXPECT(e, run(wide, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, kServes));
    EXPECT(e, run(s, 5042, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": nstates * (1 + 6 nv) = 65546 columns, more than 65536 in one call"));
    x[7] = kNan; EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": x is not finite at index 7"));
    tau[0] = kInf; EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": x is not finite at index 7"));   // (both: x first)
    EXPECT(e, run(heavy, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": x is not finite at index 7"));              // (three)
    x[7] = 0.5; EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": tau is not finite at index 0"));
    tau[0] = 0.25;
    EXPECT(e, run(heavy, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), W(e, ": the model and a substep's evaluations do not fit the 160 KiB of LDS"));
    EXPECT(e, run(s, 0, x.data(), tau.data(), 0.0, 0, 0.0, 2), W(e, ": nstates must be >= 1"));   // (five)
    EXPECT(e, run(s, S, x.data(), tau.data(), 0.0, 0, 0.0, 2), W(e, kSubsteps));                  // (four)
    EXPECT(e, run(s, S, x.data(), tau.data(), 0.0, 1, 0.0, 2), W(e, kH));                         // (three)
    EXPECT(e, run(kids, S, x.data(), tau.data(), 1e-3, 1, 0.0, 2), W(e, ": eps must be > 0 and finite"));   // (three)
    EXPECT(e, run(kids, S, x.data(), tau.data(), 1e-3, 1, 1e-6, IDTO_SCENE_MODELS_PLANTS), W(e, kPlantsAsked));   // (both)
    EXPECT(e, run(s, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0), ""); EXPECT(e, run(hold, 1, x.data(), tau.data(), 0.5, 4096, 1.0, IDTO_SCENE_MODELS_PLANTS), "");
  }
  // what idto_hip_plant_tvlqr adds, in front of the states' own checks
  const char* e = "plant_tvlqr";
  auto run = [&](const PlantShape& sh, const LinTv& t) { return RefuseLin(sh, e, S, x.data(), tau.data(), 1e-3, 1, 1e-6, 0, &t); };
  LinTv t = tv;
  for (int nu : {0, 3, -1}) { t = tv; t.nu = nu; EXPECT(e, run(s, t), "plant_tvlqr: nu must be in [1, nv]"); }
  const char* req = "plant_tvlqr: actuated[nu], Q[n * n], R[nu * nu] and Qf[n * n] are required";
  t = tv; t.actuated = nullptr; EXPECT(e, run(s, t), req); t = tv; t.Q = nullptr; EXPECT(e, run(s, t), req);
  t = tv; t.R = nullptr; EXPECT(e, run(s, t), req); t = tv; t.Qf = nullptr; EXPECT(e, run(s, t), req);
  const int bad[2] = {1, 2}, neg[2] = {-1, 5};
  t = tv; t.actuated = bad; EXPECT(e, run(s, t), "plant_tvlqr: actuated[1] is not a velocity index in [0, nv)");
  t = tv; t.actuated = neg; EXPECT(e, run(s, t), "plant_tvlqr: actuated[0] is not a velocity index in [0, nv)");
  Qf[15] = kNan; EXPECT(e, run(s, tv), "plant_tvlqr: Qf is not finite at index 15");
  R[3] = kInf; EXPECT(e, run(s, tv), "plant_tvlqr: R is not finite at index 3");       // (both: R first)
  Q[5] = kNan; EXPECT(e, run(s, tv), "plant_tvlqr: Q is not finite at index 5");       // (three: Q first)
  t = tv; t.actuated = bad; EXPECT(e, run(s, t), "plant_tvlqr: actuated[1] is not a velocity index in [0, nv)");   // (four)
  t = tv; t.nu = 0; t.Q = nullptr; EXPECT(e, run(s, t), "plant_tvlqr: nu must be in [1, nv]");                      // (both)
  x[0] = kNan; EXPECT(e, run(s, tv), "plant_tvlqr: Q is not finite at index 5");                                    // (the call's own before the states)
  Q[5] = 1; R[3] = 1; Qf[15] = 2; x[0] = 0.5;
  PlantShape riccati = Shape(1, 64, 64);   // n = 128: 5 n^2 doubles alone are 640 KiB
  std::vector<double> bigQ(128 * 128, 1.0), xs(3 * 128, 0.0);
  const LinTv bt{1, act, bigQ.data(), R.data(), bigQ.data(), nullptr, nullptr, nullptr};
  EXPECT(e, RefuseLin(riccati, e, S, xs.data(), xs.data(), 1e-3, 1, 1e-6, 0, &bt),
         "plant_tvlqr: the Riccati step's matrices (5 n^2 + 4 n nu + 2 nu^2 + nu doubles, n = 2 nv) do not fit the 160 KiB of LDS");
  LinTv one = tv; one.nu = 1; EXPECT(e, run(s, one), "");
}

// idto_hip_plant_track, and idto_hip_plant_tvlqr_track as the entry composes it: RefuseTrack without gains of its own, then RefuseLin
static void TrackEntries() {
  const PlantShape s = Shape(2, 2, 2), hold = Begun(s, IDTO_PLANT_HOLD);
  PlantShape kids = s; kids.children = true;
  PlantShape wide = s; wide.nv = 65;
  PlantShape heavy = s; heavy.blob_n = 30000;
  const int S = 3, R = 2;
  std::vector<double> xn(2 * (S + 1) * 4, 0.5), tn(2 * S * 2, 0.25), x0(2 * R * 4, 0.1), K(2 * S * 2 * 4, 1.0), Q(16, 1.0), Rm(4, 1.0);
  const int act[2] = {1, 0}, bad[2] = {0, 2};
  const TrackCall ok{S, 2, 1e-3, 0, 2, act, xn.data(), tn.data(), R, x0.data(), 0, nullptr, nullptr, nullptr, nullptr};
  const double eps_ok = 1e-6;
  for (bool own : {true, false}) {
    const char* e = own ? "plant_track" : "plant_tvlqr_track";
    const LinTv tv{2, act, Q.data(), Rm.data(), Q.data(), nullptr, nullptr, nullptr};
    auto run = [&](const PlantShape& sh, const TrackCall& a, double eps = 1e-6) {
      Refusal r = RefuseTrack(sh, e, a, own, own ? K.data() : nullptr);
      if (r.rc || own) return r;
      LinTv t = tv; t.nu = a.nu; t.actuated = a.actuated;
      return RefuseLin(sh, e, a.S, a.x_nom, a.tau_nom, a.h, a.substeps, eps, a.models, &t);   // (x_nom: the entry passes the first S states of each problem)
    };
    auto with = [&](auto edit) { TrackCall a = ok; edit(a); return a; };
    EXPECT(e, run(s, with([](auto& a) { a.S = 0; })), W(e, ": nsteps must be >= 1"));
    EXPECT(e, run(s, with([](auto& a) { a.R = 0; })), W(e, ": nrollouts must be >= 1"));
    const std::string req = W(e, ": x_nom[batch][nsteps + 1][nq + nv], tau_nom[batch][nsteps][nv], x0[batch][nrollouts][nq + nv], actuated[nu]") +
                            (own ? " and K[batch][nsteps][nu * n]" : "") + " are required";
    EXPECT(e, run(s, with([](auto& a) { a.x_nom = nullptr; })), req); EXPECT(e, run(s, with([](auto& a) { a.tau_nom = nullptr; })), req);
    EXPECT(e, run(s, with([](auto& a) { a.x0 = nullptr; })), req); EXPECT(e, run(s, with([](auto& a) { a.actuated = nullptr; })), req);
    if (own) EXPECT(e, RefuseTrack(s, e, ok, true, nullptr), req);
    EXPECT(e, run(s, with([](auto& a) { a.R = 32769; })), W(e, ": batch * nrollouts = 65538 rollouts, more than 65536 in one call"));
    for (int n : {0, 4097}) EXPECT(e, run(s, with([&](auto& a) { a.substeps = n; })), W(e, kSubsteps));
    for (int n : {1, 4097, -2}) EXPECT(e, run(s, with([&](auto& a) { a.max_launch_substeps = n; })), W(e, ": max_launch_substeps is 0 or in [substeps, 4096] (a launch holds whole control steps)"));
    for (double h : {0.0, kInf, kNan}) EXPECT(e, run(s, with([&](auto& a) { a.h = h; })), W(e, kH));
    EXPECT(e, run(s, with([](auto& a) { a.models = 2; })), W(e, kModels));
    EXPECT(e, run(s, with([](auto& a) { a.models = IDTO_SCENE_MODELS_PLANTS; })), W(e, kPlantsAsked));
    EXPECT(e, run(kids, ok), W(e, kChildren));
    EXPECT(e, run(wide, ok), W(e, kServes));
    for (int nu : {0, 3}) EXPECT(e, run(s, with([&](auto& a) { a.nu = nu; })), W(e, ": nu must be in [1, nv]"));
    EXPECT(e, run(s, with([&](auto& a) { a.actuated = bad; })), W(e, ": actuated[1] is not a velocity index in [0, nv)"));
    x0[5] = kNan; EXPECT(e, run(s, ok), W(e, ": x0 is not finite at index 5"));
    tn[11] = kInf; EXPECT(e, run(s, ok), W(e, ": tau_nom is not finite at index 11"));   // (both: tau_nom first)
    xn[31] = kNan; EXPECT(e, run(s, ok), W(e, ": x_nom is not finite at index 31"));     // (three: x_nom first - its last state, which only the rollouts read)
    EXPECT(e, run(heavy, ok), W(e, ": x_nom is not finite at index 31"));                // (four)
    x0[5] = 0.1; tn[11] = 0.25; xn[31] = 0.5;
    EXPECT(e, run(heavy, ok), W(e, ": the model, a substep's evaluations and the law's K_t do not fit the 160 KiB of LDS"));
    EXPECT(e, run(s, with([](auto& a) { a.S = 0; a.R = 0; a.substeps = 0; })), W(e, ": nsteps must be >= 1"));        // (three)
    EXPECT(e, run(s, with([](auto& a) { a.R = 0; a.x0 = nullptr; })), W(e, ": nrollouts must be >= 1"));              // (both)
    EXPECT(e, run(s, with([](auto& a) { a.substeps = 0; a.h = 0; a.max_launch_substeps = 5000; })), W(e, kSubsteps)); // (three)
    EXPECT(e, run(kids, with([](auto& a) { a.h = 0; a.nu = 0; })), W(e, kH));                                         // (three)
    if (!own) {   // the linearisation's refusals stand behind every one of the rollouts'
      EXPECT(e, run(s, ok, 0.0), W(e, ": eps must be > 0 and finite"));
      EXPECT(e, run(s, with([](auto& a) { a.R = 0; }), 0.0), W(e, ": nrollouts must be >= 1"));                        // (both)
      x0[0] = kNan; EXPECT(e, run(s, ok, kNan), W(e, ": x0 is not finite at index 0")); x0[0] = 0.1;                   // (both)
      Q[3] = kNan; EXPECT(e, run(s, ok), W(e, ": Q is not finite at index 3"));
      EXPECT(e, run(heavy, ok), W(e, ": the model, a substep's evaluations and the law's K_t do not fit the 160 KiB of LDS")); Q[3] = 1;   // (both)
      std::vector<double> lx(2 * 5043 * 4, 0.5), lt(2 * 5042 * 2, 0.25);   // (the rollouts' checks read all of them first)
      EXPECT(e, run(s, with([&](auto& a) { a.S = 5042; a.x_nom = lx.data(); a.tau_nom = lt.data(); })),
             W(e, ": nstates * (1 + 6 nv) = 65546 columns, more than 65536 in one call"));
    }
    EXPECT(e, run(s, ok, eps_ok), "");
    EXPECT(e, run(hold, with([](auto& a) { a.models = IDTO_SCENE_MODELS_PLANTS; a.max_launch_substeps = 2; a.nu = 1; })), "");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: plant_calls_check tests/golden/plant_call_layouts.txt\n"); return 2; }
  Layouts(argv[1]);
  BlockAndLds();
  PlantEntries();
  SceneEntry();
  LinEntries();
  TrackEntries();
  int cases = 0;
  for (const char* e : {"plant_begin", "plant_set_model", "plant_set_state", "plant_get_state", "plant_step", "mpc_batch_tick_plants", "forward_dynamics",
                        "scene_report", "plant_linearize", "plant_tvlqr", "plant_track", "plant_tvlqr_track"}) {
    CHECK(g_refused[e] > 0 && g_accepted[e] > 0, "%s: %d refusals and %d accepted calls were checked", e, g_refused[e], g_accepted[e]);
    cases += g_refused[e] + g_accepted[e];
  }
  CHECK(g_block_cases == 96, "block cases: %d", g_block_cases);
  if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
  std::printf("ok: 232 layouts, %d block and LDS cases, %d refusal cases\n", g_block_cases, cases);
  return 0;
}
