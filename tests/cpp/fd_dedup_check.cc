// fd_dedup_check.cc — host/model_tables.cc BuildFdDedup on the CPU: the paths each column touches and fd_kernel's lane
// map without the redundant path lanes (model_layout.h tree_shape_dedup, FDL_*, FDH_*).  A stand-alone program
// (tests/test_fd_support.py builds it with the address and undefined-behaviour sanitizers):
//   fd_dedup_check <model file> ...
// checks every model's tables, prints one line per model - "paths <name> <fd_dedup> q <nq masks> v <nv masks>" - then
// "ok: ..." and returns 0, or says what failed.  The first model must be one that takes the lane map (mini_cheetah).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/model_tables.h"
#include "idto/model_file.h"

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      ++g_failed;                                               \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                 \
      std::printf("\n");                                        \
    }                                                           \
  } while (0)

using namespace idto_dev;

// the lane words of a model that takes the map: every evaluation on exactly the paths it touches, the helpers' records
void CheckLanes(const idto::ModelFile& f, const idto_host::ModelTables& t) {
  const int K = f.npaths, nq = f.nq, nv = f.nv, E = 1 + 2 * nq + nv, all = (1 << K) - 1;
  const int* ints = reinterpret_cast<const int*>(t.blob.data());
  const size_t end = 2 * t.blob.size();
  CHECK(t.fd_lanes_at + kFdMainLanes + kFdHelperLanes <= end, "the words lie inside the blob");
  CHECK(t.fd_lanes_at == t.at.f_seg + (size_t)K * (t.maxc + 2), "the words follow f_seg's");
  CHECK((t.fd_lanes_at + kFdMainLanes + kFdHelperLanes + 1) / 2 <= (size_t)(t.fast_lo + t.fast_n),
        "the words lie in the part of the blob a shape's kernel stages");
  const int* main = ints + t.fd_lanes_at;
  const int* help = main + kFdMainLanes;
  std::vector<int> seen(E, 0);
  int body_own = 0, valid = 0;
  for (int l = 0; l < kFdMainLanes; ++l) {
    const int w = main[l], e = w & 255, p = (w >> 8) & 3;
    CHECK(p < K, "lane %d: path %d", l, p);
    if (!(w & FDL_VALID)) {
      CHECK(!(w & (FDL_FULL | FDL_WHOLE | FDL_BODY_OWN | FDL_BODY_BASE)) && e == 0, "lane %d: a lane without a task is the baseline, tau only", l);
      continue;
    }
    ++valid;
    CHECK(e < E, "lane %d: evaluation %d", l, e);
    if (e >= E) continue;
    const int want = e == 0 ? all : (e < 1 + 2 * nq ? t.fd_qpaths[(e - 1) % nq] : t.fd_vpaths[e - 1 - 2 * nq]);
    CHECK(want >> p & 1, "lane %d: evaluation %d does not touch path %d", l, e, p);
    CHECK(!(seen[e] >> p & 1), "lane %d: (evaluation %d, path %d) twice", l, e, p);
    seen[e] |= 1 << p;
    CHECK(((w & FDL_FULL) != 0) == (e < 1 + 2 * nq), "lane %d: full", l);
    CHECK(((w & FDL_WHOLE) != 0) == (want == all), "lane %d: whole", l);
    if (w & FDL_WHOLE) {   // four aligned lanes, path = lane % 4: the butterfly's partners
      CHECK(p == l % K && (main[l - p] & 255) == e && (main[l - p + K - 1] & 255) == e, "lane %d: the quad of evaluation %d", l, e);
    }
    CHECK(!((w & FDL_BODY_OWN) && (w & FDL_BODY_BASE)), "lane %d: both body flags", l);
    if (w & FDL_BODY_OWN) { ++body_own; CHECK((w & FDL_WHOLE) && (w & FDL_FULL), "lane %d: body_own", l); }
    if (w & FDL_BODY_BASE) CHECK(!(w & FDL_WHOLE) && (w & FDL_FULL), "lane %d: body_base", l);
    // the lane whose helper has the baseline's result for FDL_BODY_BASE is in quad 0
    if (w & FDL_BODY_BASE) {
      bool found = false;
      for (int b = 0; b < K; ++b) found = found || ((main[b] & FDL_BODY_OWN) && (main[b] & 255) == 0 && ((main[b] >> 8) & 3) == p);
      CHECK(found, "lane %d: no baseline lane of path %d adds the common body's pair", l, p);
    }
  }
  for (int e = 0; e < E; ++e) {
    const int want = e == 0 ? all : (e < 1 + 2 * nq ? t.fd_qpaths[(e - 1) % nq] : t.fd_vpaths[e - 1 - 2 * nq]);
    CHECK(seen[e] == want, "evaluation %d: lanes for paths %d, touches %d", e, seen[e], want);
  }
  for (int b = 0; b < K; ++b) CHECK((main[b] & 255) == 0 && (main[b] & FDL_VALID), "the baseline is lanes 0 .. K - 1");
  int foots = 0, bodies = 0;
  for (int h = 0; h < kFdHelperLanes; ++h) {
    const int w = help[h], m = (w >> 8) & 255, fr = (w >> 16) & 255, br = (w >> 24) & 255;
    CHECK(m == h, "helper %d serves lane %d", h, m);
    const bool full = (main[m] & FDL_VALID) && (main[m] & FDL_FULL);
    CHECK(((w & FDH_FOOT) != 0) == full, "helper %d: foot", h);
    CHECK(((w & FDH_BODY) != 0) == ((main[m] & FDL_BODY_OWN) != 0), "helper %d: body", h);
    foots += (w & FDH_FOOT) != 0; bodies += (w & FDH_BODY) != 0;
    CHECK(fr < K * t.f_maxpp && br < K * t.f_maxpp, "helper %d: pair records %d, %d", h, fr, br);
    if (fr >= K * t.f_maxpp || br >= K * t.f_maxpp) continue;
    if (w & FDH_FOOT) {   // a pair of the lane's own path whose other body is the world
      int info[4];
      std::memcpy(info, t.blob.data() + t.at.f_pairs + (size_t)fr * FP_STRIDE + FP_INFO, sizeof(info));
      CHECK(fr / t.f_maxpp == ((main[m] >> 8) & 3) && info[3] == 0, "helper %d: the chain pair's record", h);
    }
    if (w & FDH_BODY) {
      int info[4];
      std::memcpy(info, t.blob.data() + t.at.f_pairs + (size_t)br * FP_STRIDE + FP_INFO, sizeof(info));
      CHECK(br / t.f_maxpp == ((main[m] >> 8) & 3) && info[3] == 0, "helper %d: the common body's pair's record", h);
    }
  }
  CHECK(bodies == body_own, "body tasks %d, lanes that add them %d", bodies, body_own);
  std::printf("lanes %s main %d foot %d body %d\n", f.name.c_str(), valid, foots, bodies);
}

int CheckModel(const std::string& path, bool must_have) {
  using namespace idto_host;
  const idto::ModelFile f = idto::ModelFile::Load(path);
  const idto_model_t m = f.c_model();
  ModelTables t;
  std::string err;
  CHECK(BuildModelTables(&m, &t, &err) == 0, "%s: %s", path.c_str(), err.c_str());
  CHECK((int)t.fd_qpaths.size() == f.nq && (int)t.fd_vpaths.size() == f.nv, "%s: path sets", path.c_str());
  if (must_have) CHECK(t.fd_dedup, "%s: the lane map was refused", path.c_str());
  CHECK(!t.fd_dedup || tree_shape_dedup(t.fast_shape), "%s: lane map without the shape's trait", path.c_str());
  // no lane words where the map is refused: the next table begins where they would
  if (!t.fd_dedup) {
    bool empty = false;
#define X(name) if (t.at.name == t.fd_lanes_at) empty = true;
    IDTO_MODEL_INT_TABLES(X)
#undef X
    CHECK(empty, "%s: refused, but there are lane words", path.c_str());
  } else {
    CheckLanes(f, t);
  }
  std::printf("paths %s %d q", f.name.c_str(), t.fd_dedup ? 1 : 0);
  for (int v : t.fd_qpaths) std::printf(" %d", v);
  std::printf(" v");
  for (int v : t.fd_vpaths) std::printf(" %d", v);
  std::printf("\n");

  // ---- the refusal: the common body's pair with the world moved to the front of the pair list - it then comes before
  // the chains' pairs in the walking order, which the lane map's evaluation does not walk.  The model keeps its shape.
  if (t.fd_dedup) {
    idto::ModelFile v = f;
    const int np = (int)v.pair_a.size();
    int bw = -1;
    for (int i = 0; i < np; ++i)
      if (v.geom_body[v.pair_a[i]] == v.common_body && v.geom_body[v.pair_b[i]] < 0) bw = i;
    CHECK(bw > 0, "%s: no pair of the common body with the world behind another pair", path.c_str());
    if (bw > 0) {
      for (std::vector<int>* tb : {&v.pair_a, &v.pair_b, &v.pair_path}) {
        const int x = (*tb)[bw];
        tb->erase(tb->begin() + bw);
        tb->insert(tb->begin(), x);
      }
      const idto_model_t vm = v.c_model();
      ModelTables vt;
      CHECK(BuildModelTables(&vm, &vt, &err) == 0, "%s: reordered pairs: %s", path.c_str(), err.c_str());
      CHECK(vt.fast_shape == t.fast_shape, "%s: reordered pairs: shape %d", path.c_str(), vt.fast_shape);
      CHECK(!vt.fd_dedup, "%s: reordered pairs: the lane map was not refused", path.c_str());
      CHECK(vt.fd_qpaths == t.fd_qpaths && vt.fd_vpaths == t.fd_vpaths, "%s: reordered pairs: path sets", path.c_str());
      CHECK(vt.blob.size() + (kFdMainLanes + kFdHelperLanes) / 2 == t.blob.size(), "%s: reordered pairs: the table is not empty", path.c_str());
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: fd_dedup_check <model file> ...\n"); return 2; }
  for (int i = 1; i < argc; ++i) {
    try {
      CheckModel(argv[i], i == 1);
    } catch (const std::exception& e) {
      std::printf("FAILED %s: %s\n", argv[i], e.what());
      ++g_failed;
    }
  }
  if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
  std::printf("ok: %d models\n", argc - 1);
  return 0;
}
