// fd_plan_check.cc — host/fd_plan.cc on the CPU: every finite-difference launch's block, evaluations per pass, fold, LDS,
// grid, shape and kernel.  A stand-alone program (tests/test_fd_plan.py builds it with the address and
// undefined-behaviour sanitizers):
//   fd_plan_check <golden file> <model file> ...      (--print in place of the golden file: the sweep's lines alone)
//   1. reproduces tests/golden/fd_plans.txt line by line - recorded from FdEvals, FdLds, FdBlock, FoldTerms, LaunchFd,
//      LaunchFused, create's geometry and fd_launch.hip's go<> as they stood before the plan became a unit,
//   2. checks the rules' properties on every plan of that sweep and of a synthetic sweep of sizes,
//   3. holds the closed LDS formula (fd_sizes.h fd_lds_doubles) to the kernel's carve-up (fd_carve) for every accepted plan.
// Prints "ok: ..." and returns 0, or says what failed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "fd_sizes.h"
#include "host/fd_plan.h"
#include "host/model_tables.h"
#include "idto/model_file.h"

namespace {

using namespace idto_dev;
using namespace idto_host;

int g_failed = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (++g_failed <= 40) {                                   \
        std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                               \
        std::printf("\n");                                      \
      }                                                         \
    }                                                           \
  } while (0)

const char* const kRefusal = "finite-difference evaluation set does not fit in LDS";
const char* const kFamilies[] = {"FD", "FD_DEDUP", "FD_MODELS", "FD_DEDUP_MODELS", "FD_ALONG", "FD_ALONG_BATCH", "FD_ALONG_MODELS"};

// The sizing rules at the commit that introduced the unit, as that commit's issue quotes them: they are in the fixture as
// they stand here, so that the fixture is seen to be the rules' record and not the unit's own output.
const char* const kQuoted[] = {
    "size | mini_cheetah | 1, diagonal | 256 | 57 | 57 | 1 | 102408 |",  "size | mini_cheetah | 3, diagonal | 256 | 229 | 192 | 1 | 154480 |",
    "size | allegro_hand | 3, dense | 256 | 277 | 128 | 0 | 145112 |",   "size | allegro_hand | 3, diagonal | 256 | 277 | 64 | 1 | 135456 |",
    "size | dual_jaco | 2, diagonal | 128 | 127 | 64 | 1 | 143672 |",    "size | dual_jaco | 3, diagonal | 128 | 253 | 64 | 0 | 146368 |",
    "size | punyo | 1, diagonal | 192 | 63 | 48 | 1 | 161232 |",         "size | punyo | 2, diagonal | 192 | 127 | 48 | 0 | 152520 |",
    "size | punyo | 3, diagonal | 128 | 253 | 32 | 1 | 159200 |",        "size | hopper | 1, diagonal | 64 | 16 | 16 | 1 | 6944 |",
};

struct Counters {
  long plans = 0, refused = 0, stem64 = 0, carved = 0;
  int slack_min = 1 << 30, slack_max = -1;
};

// ---- 2. and 3.: what holds for every plan
void CheckPlan(const FdShape& s, const FdRequest& r, int rc, const FdPlan& p, const std::string& err, Counters* n, const char* what) {
  ++n->plans;
  const bool fused = r.kind == FdRequest::FUSED, along = r.kind == FdRequest::CANDIDATES;
  if (rc == 0) CHECK(p.lds <= kMaxDynamicLds && err.empty(), "%s: accepted with %d bytes", what, p.lds);
  else { ++n->refused; CHECK(rc == -1 && err == kRefusal && p.lds > kMaxDynamicLds, "%s: rc %d '%s' lds %d", what, rc, err.c_str(), p.lds); }
  CHECK(p.mode == (r.mode >= 1 ? 1 + s.gradients_method : 0) && p.E == fd_evals(p.mode, s.nq, s.nv), "%s: mode %d E %d", what, p.mode, p.E);
  CHECK(p.block % 64 == 0 && p.block >= 64 && p.block <= 256 && (p.mode != 0 || p.block == 64), "%s: block %d", what, p.block);
  CHECK(p.groups == p.block / s.npaths && p.groups >= 1, "%s: groups %d", what, p.groups);
  CHECK(p.echunk == p.E || (p.echunk >= p.groups && p.echunk % p.groups == 0), "%s: echunk %d of %d, groups %d", what, p.echunk, p.E, p.groups);
  CHECK(!p.fold || (p.mode >= 1 && s.weights_diagonal && s.asm_fold && !fused), "%s: fold", what);
  CHECK(!p.dedup || (p.mode == 1 && r.kind == FdRequest::RESIDENT && p.block == kFdMainLanes + kFdHelperLanes && tree_shape_dedup(p.shape) &&
                     s.fd_dedup && s.fd_fast && s.lane_map),
        "%s: dedup", what);
  if (s.nstem > 1 && !fused && p.mode >= 1 && p.block == 64 && std::min(256, (fd_evals(1, s.nq, s.nv) * s.npaths + 63) / 64 * 64) > 64) ++n->stem64;
  if (!fused) {
    // the kernel, as fd_launch.hip's go<> chose it from the pointers of its argument
    const bool records = s.model_records, cstride = along, along_batch = along && s.batch > 1;
    FdFamily want = FD;
    if (records && cstride) want = FD_ALONG_MODELS;
    else if (p.dedup && !cstride) want = records ? FD_DEDUP_MODELS : FD_DEDUP;
    else if (records) want = FD_MODELS;
    else if (cstride && along_batch) want = FD_ALONG_BATCH;
    else if (cstride) want = FD_ALONG;
    CHECK(p.family == want, "%s: family %s, not %s", what, kFamilies[p.family], kFamilies[want]);
    CHECK(p.grid_x == r.ke - r.kb && p.grid_y == (along ? r.m : s.batch) && p.grid_z == (along_batch ? s.batch : 1), "%s: grid %d x %d x %d",
          what, p.grid_x, p.grid_y, p.grid_z);
    const int shape = s.nstem > 1 ? SHAPE_STEM : (s.nxb ? SHAPE_XCH : (s.fd_fast ? s.fast_shape : 0));
    CHECK(p.shape == shape && p.maxc == (shape ? tree_shape(shape).KC : FdChainBound(s.maxc)), "%s: shape %d maxc %d", what, p.shape, p.maxc);
  }
  if (rc != 0) return;
  // the kernel's walk, with what the kernel of this plan stages and exchanges, ends inside what the launch asks for
  const bool fast_kernel = !fused && p.shape != 0 && p.shape != SHAPE_XCH && p.shape != SHAPE_STEM;
  const FdCarve c = fd_carve(s.nq, s.nv, p.E, std::min(p.echunk, p.E), p.fold, fast_kernel ? s.fast_n : s.blob_n,
                             fd_xch_doubles(s.nxb, p.block, s.npaths, s.nstem), p.dedup ? fd_dedup_doubles() : 0);
  const int slack = p.lds / (int)sizeof(double) - c.end;
  CHECK(slack >= 0, "%s: the carve-up ends at %d doubles, the launch asks for %d", what, c.end, p.lds / (int)sizeof(double));
  CHECK(c.rec % 2 == 0 && c.xch >= c.rec && c.end >= c.lanes && c.lanes >= c.xch, "%s: the walk's alignment", what);
  ++n->carved;
  n->slack_min = std::min(n->slack_min, slack);
  n->slack_max = std::max(n->slack_max, slack);
}

std::string PlanLine(const std::string& head, const FdShape& s, const FdRequest& r, Counters* n) {
  FdPlan p;
  std::string err;
  const int rc = PlanFd(s, r, &p, &err);
  CheckPlan(s, r, rc, p, err, n, head.c_str());
  char b[512];
  std::snprintf(b, sizeof b, "%s | %d | %d | %d | %d | %d | groups %d grid %d x %d x %d shape %d maxc %d dedup %d %s%s", head.c_str(), p.block, p.E,
                p.echunk, p.fold ? 1 : 0, p.lds, p.groups, p.grid_x, p.grid_y, p.grid_z, p.shape, p.maxc, p.dedup ? 1 : 0, kFamilies[p.family],
                rc ? " REFUSED" : "");
  return b;
}

FdShape ShapeOf(const idto::ModelFile& f, const ModelTables& t) {
  FdShape s;
  s.nq = f.nq; s.nv = f.nv; s.npaths = f.npaths;
  s.blob_n = (int)t.blob.size(); s.fast_n = t.fast_n; s.fast_shape = t.fast_shape; s.maxc = t.maxc; s.nxb = t.nxb; s.nstem = t.nstem;
  s.lane_map = t.fd_dedup;
  return s;
}

bool OneOf(const std::string& name, std::initializer_list<const char*> names) {
  for (const char* x : names)
    if (name == x) return true;
  return false;
}

// ---- 1. the sweep of the model files.  Independent dimensions one at a time, the others at their defaults: mode 0 and
// gradients_method 0 .. 2 ("mode 0 .. 3") with diagonal and dense weights; three options switched off; the kernel family
// over batch, records, candidate points and a shard; the fused launch's evaluation; create's geometry.
void SweepModel(const std::string& path, std::vector<std::string>* out, Counters* n) {
  const idto::ModelFile f = idto::ModelFile::Load(path);
  const idto_model_t m = f.c_model();
  ModelTables t;
  std::string err;
  if (BuildModelTables(&m, &t, &err) != 0) { CHECK(false, "%s: %s", path.c_str(), err.c_str()); return; }
  const FdShape base = ShapeOf(f, t);
  const int N = 4;
  auto resident = [&](int mode, int kb, int ke) { FdRequest r; r.mode = mode >= 1 ? 1 : 0; r.kb = kb; r.ke = ke; return r; };
  auto with_mode = [&](FdShape s, int mode) { s.gradients_method = mode >= 1 ? mode - 1 : 0; return s; };
  for (int mode = 0; mode <= 3; ++mode)
    for (int dense = 0; dense <= 1; ++dense) {
      FdShape s = with_mode(base, mode);
      s.weights_diagonal = !dense;
      out->push_back(PlanLine("size | " + f.name + " | " + std::to_string(mode) + (dense ? ", dense" : ", diagonal"), s, resident(mode, 0, N), n));
    }
  if (OneOf(f.name, {"mini_cheetah", "punyo", "dual_jaco", "hopper"}))
    for (const char* opt : {"asm_fold", "fd_fast", "fd_dedup"})
      for (int mode = 0; mode <= 3; ++mode) {
        FdShape s = with_mode(base, mode);
        (opt[0] == 'a' ? s.asm_fold : (opt[3] == 'f' ? s.fd_fast : s.fd_dedup)) = false;
        out->push_back(PlanLine(std::string("option ") + opt + " 0 | " + f.name + " | " + std::to_string(mode) + ", diagonal", s, resident(mode, 0, N), n));
      }
  for (int batch : {1, 3})
    for (int records = 0; records <= 1; ++records)
      for (int what = 0; what < 3; ++what) {   // tau, forward differences, 5 candidate points
        FdShape s = base;
        s.batch = batch; s.model_records = records != 0;
        FdRequest r = resident(what == 1 ? 1 : 0, 0, N);
        if (what == 2) { r.kind = FdRequest::CANDIDATES; r.m = 5; }
        out->push_back(PlanLine("family batch " + std::to_string(batch) + (records ? " records " : " ") + (what == 2 ? "candidates" : "resident") + " | " +
                                    f.name + " | " + std::to_string(what == 1 ? 1 : 0) + ", diagonal",
                                s, r, n));
      }
  out->push_back(PlanLine("family shard [1, 3) | " + f.name + " | 1, diagonal", base, resident(1, 1, 3), n));
  if (OneOf(f.name, {"acrobot", "spinner", "hopper", "mini_cheetah", "allegro_hand"}))
    for (int mode = 1; mode <= 3; ++mode) {
      FdRequest r;
      r.kind = FdRequest::FUSED; r.mode = 1;
      out->push_back(PlanLine("fused | " + f.name + " | " + std::to_string(mode) + ", diagonal", with_mode(base, mode), r, n));
    }
  const FdCreate g = FdCreateGeometry(base);
  out->push_back("create | " + f.name + " | fd_threads " + std::to_string(g.fd_threads) + " fd_lds " + std::to_string(g.fd_lds));
}

// ---- the synthetic sweep: sizes no model file has, generic and stem shapes, and a shape with the lane map
void SweepSynthetic(Counters* n) {
  for (int nq = 1; nq <= 40; ++nq)
    for (int nv : {nq, nq - 1})
      for (int npaths : {1, 2, 4})
        for (int parity = 0; parity <= 1; ++parity)
          for (int nxb : {0, 4, 8})
            for (int nstem : {0, 2, 4})
              for (int lane_map = 0; lane_map <= (npaths == 4 && !nxb && !nstem ? 1 : 0); ++lane_map)
                for (int mode = 0; mode <= 3; ++mode)
                  for (int dense = 0; dense <= 1; ++dense) {
                    if (nv < 1) continue;
                    FdShape s;
                    s.nq = nq; s.nv = nv; s.npaths = npaths;
                    s.blob_n = 120 * nq + 64 + parity; s.maxc = 1 + (nq - 1) / npaths; s.nxb = nxb; s.nstem = nstem;
                    if (lane_map) { s.fast_shape = 3; s.fast_n = 60 * nq + 129 - parity; s.lane_map = true; }
                    s.gradients_method = mode >= 1 ? mode - 1 : 0;
                    s.weights_diagonal = !dense;
                    char what[160];
                    std::snprintf(what, sizeof what, "nq %d nv %d npaths %d blob_n %d nxb %d nstem %d lane_map %d mode %d dense %d", nq, nv, npaths,
                                  s.blob_n, nxb, nstem, lane_map, mode, dense);
                    for (int kind = 0; kind < (mode == 0 ? 2 : 1); ++kind) {   // (candidate points: tau only)
                      FdRequest r;
                      r.mode = mode >= 1 ? 1 : 0; r.ke = 4;
                      if (kind) { r.kind = FdRequest::CANDIDATES; r.m = 5; }
                      FdPlan p;
                      std::string err;
                      const int rc = PlanFd(s, r, &p, &err);
                      CheckPlan(s, r, rc, p, err, n, what);
                    }
                  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: fd_plan_check <golden file | --print> <model file> ...\n"); return 2; }
  const bool print = std::strcmp(argv[1], "--print") == 0;
  std::vector<std::string> lines;
  Counters models, synthetic;
  for (int i = 2; i < argc; ++i) {
    try {
      SweepModel(argv[i], &lines, &models);
    } catch (const std::exception& e) {
      std::printf("FAILED %s: %s\n", argv[i], e.what());
      ++g_failed;
    }
  }
  if (print) {
    for (const std::string& l : lines) std::printf("%s\n", l.c_str());
    return g_failed ? 1 : 0;
  }
  std::ifstream in(argv[1]);
  std::vector<std::string> golden;
  for (std::string l; std::getline(in, l);)
    if (!l.empty() && l[0] != '#') golden.push_back(l);
  CHECK(!golden.empty() && golden.size() == lines.size(), "%s has %zu lines, the sweep %zu", argv[1], golden.size(), lines.size());
  for (size_t i = 0; i < std::min(golden.size(), lines.size()); ++i)
    CHECK(golden[i] == lines[i], "line %zu\n  recorded: %s\n  the unit: %s", i + 1, golden[i].c_str(), lines[i].c_str());
  for (const char* q : kQuoted) {
    bool found = false;
    for (const std::string& l : golden) found = found || l.compare(0, std::strlen(q), q) == 0;
    CHECK(found, "the fixture has no line '%s ...'", q);
  }
  CHECK(models.refused == 0, "%ld plans of the tree's model files are refused", models.refused);
  SweepSynthetic(&synthetic);
  CHECK(synthetic.refused > 0, "no synthetic shape is refused");
  CHECK(synthetic.stem64 > 0, "no synthetic stem shape shrinks to 64 threads");
  if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
  std::printf("ok: %zu lines, %ld + %ld plans (%ld refused, %ld stem shapes at 64 threads); the carve-up ends %d .. %d doubles (models) and %d .. %d "
              "(synthetic) short of the launch's LDS\n",
              lines.size(), models.plans, synthetic.plans, synthetic.refused, synthetic.stem64, models.slack_min, models.slack_max,
              synthetic.slack_min, synthetic.slack_max);
  return 0;
}
