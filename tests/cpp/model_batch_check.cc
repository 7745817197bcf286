// model_batch_check.cc — host/model_batch.cc on the CPU: what may differ between the models of a batch and what may not,
// and a problem's parameter record.  A stand-alone program (tests/test_model_batch.py builds it with the address and
// undefined-behaviour sanitizers): model_batch_check <model file> ...; prints "ok: ..." and returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host/model_batch.h"
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

// a few percent off every entry, from a seeded generator (zeros stay zeros: a rotation's and a box's)
struct Lcg {
  unsigned long long s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};
void Perturb(std::vector<double>* v, Lcg* g) {
  for (double& x : *v) x *= 1.0 + 0.03 * (g->next() - 0.5);
}

// the first double of the blob's int part: the smallest int table offset, halved
size_t DoublePart(const idto_host::ModelTables& t) {
  size_t first = t.at.parent;
#define X(name) if (t.at.name < first) first = t.at.name;
  IDTO_MODEL_INT_TABLES(X)
#undef X
  return first / 2;
}

int CheckModel(const std::string& path) {
  using namespace idto_host;
  const idto::ModelFile base = idto::ModelFile::Load(path);
  const idto_model_t bm = base.c_model();
  ModelTables bt;
  std::string err;
  CHECK(BuildModelTables(&bm, &bt, &err) == 0, "%s: %s", path.c_str(), err.c_str());
  const idto_contact_params_t contact{123.5, 0.11, 0.052, 0.93, 0.0123};
  const std::vector<double> brec = ModelRecord(&bm, bt, contact);
  const size_t n = bt.blob.size(), nd = DoublePart(bt);
  CHECK(brec.size() == idto_dev::model_record_doubles(n) && brec.size() % 8 == 0, "record size");

  // ---- the contact doubles are the expression idto_hip_create has always used
  {
    const double k = contact.contact_stiffness, sigma = contact.smoothing_factor;
    const double eps = std::sqrt(2.220446049250313e-16);
    const double threshold = -sigma * idto::detmath::log(idto::detmath::exp(eps / (sigma * k)) - 1.0);
    const double want[6] = {k, contact.dissipation_velocity, contact.stiction_velocity, contact.friction_coefficient, sigma, threshold};
    double got[6];
    ContactValues(contact, got);
    CHECK(std::memcmp(got, want, sizeof(want)) == 0, "ContactValues");
    CHECK(std::memcmp(brec.data() + idto_dev::model_record_contact_at(n), want, sizeof(want)) == 0, "the record's contact doubles");
    CHECK(std::memcmp(brec.data() + idto_dev::model_record_gravity_at(n), bm.gravity, 3 * sizeof(double)) == 0, "the record's gravity");
    CHECK(std::isfinite(threshold), "threshold");
  }

  // ---- every free table perturbed: accepted, and the blob differs inside the double tables only
  {
    idto::ModelFile v = base;
    Lcg g{12345};
    Perturb(&v.X_PF, &g); Perturb(&v.axis, &g); Perturb(&v.mass, &g); Perturb(&v.com, &g); Perturb(&v.inertia, &g);
    Perturb(&v.damping, &g); Perturb(&v.geom_X, &g); Perturb(&v.geom_size, &g);
    for (size_t gi = 0; gi < v.geom_body.size(); ++gi)   // (a world-fixed box keeps its identity rotation: the pair checks ask for it)
      if (v.geom_body[gi] < 0) std::copy(base.geom_X.begin() + 12 * gi, base.geom_X.begin() + 12 * gi + 9, v.geom_X.begin() + 12 * gi);
    v.gravity[0] = 0.3; v.gravity[2] *= 1.02;
    const idto_model_t vm = v.c_model();
    const idto_contact_params_t vc{150.0, 0.12, 0.05, 0.9, 0.02};
    std::vector<double> rec;
    ModelTables vt;
    const int rc = BuildModelVariant(&bm, bt, 1, &vm, vc, &rec, &err, &vt);
    CHECK(rc == 0, "%s: perturbed variant refused: %s", path.c_str(), err.c_str());
    if (rc == 0) {
      CHECK(rec.size() == brec.size() && vt.blob.size() == n, "sizes");
      CHECK(std::memcmp(rec.data(), vt.blob.data(), n * sizeof(double)) == 0, "the record begins with the blob");
      CHECK(std::memcmp(vt.blob.data() + nd, bt.blob.data() + nd, (n - nd) * sizeof(double)) == 0, "the blob's int part moved");
      size_t changed = 0;
      for (size_t i = 0; i < nd; ++i) changed += std::memcmp(&vt.blob[i], &bt.blob[i], sizeof(double)) != 0;
      CHECK(changed > 0, "the blob's double part did not move");
      CHECK(rec[idto_dev::model_record_gravity_at(n)] == 0.3, "gravity");
      CHECK(rec[idto_dev::model_record_contact_at(n)] == 150.0, "contact");
    }
    // the base model itself with other contact parameters
    CHECK(BuildModelVariant(&bm, bt, 0, &bm, vc, &rec, &err) == 0, "base as a variant: %s", err.c_str());
    CHECK(std::memcmp(rec.data(), brec.data(), n * sizeof(double)) == 0, "base blob");
  }

  // ---- refusals: each names the problem and the table
  auto refused = [&](const char* what, const std::function<void(idto::ModelFile*)>& change, bool own_text_ok = false) {
    idto::ModelFile v = base;
    change(&v);
    const idto_model_t vm = v.c_model();
    std::vector<double> rec(3, 1.0);
    std::string e;
    const int rc = BuildModelVariant(&bm, bt, 2, &vm, contact, &rec, &e);
    const std::string want = std::string("model of problem 2 differs from the batch's model in ") + what;
    // (own_text_ok: the changed model may be one BuildModelTables itself refuses, with its own text)
    const bool named = e == want || (own_text_ok && rc != 0 && !e.empty() && e.find("differs") == std::string::npos);
    CHECK(rc != 0 && named, "%s: changed %s: rc %d, \"%s\"", path.c_str(), what, rc, e.c_str());
    CHECK(rec.size() == 3, "a refusal left a record");
    return rc != 0 && e == want;
  };
  refused("actuated", [](idto::ModelFile* v) { v->actuated[0] ^= 1; });
  refused("gravity_enabled", [](idto::ModelFile* v) {
    if (v->gravity_enabled.empty()) v->gravity_enabled.assign(v->parent.size(), 1);
    v->gravity_enabled.back() ^= 1;
  });
  // the last one-dof joint: revolute <-> prismatic keeps nq and nv
  refused("jtype", [](idto::ModelFile* v) {
    for (size_t b = v->jtype.size(); b-- > 0;)
      if (v->jtype[b] == IDTO_JOINT_REVOLUTE || v->jtype[b] == IDTO_JOINT_PRISMATIC) {
        v->jtype[b] = (v->jtype[b] == IDTO_JOINT_REVOLUTE) ? IDTO_JOINT_PRISMATIC : IDTO_JOINT_REVOLUTE;
        return;
      }
  });
  // one body fewer: the last body, its geometries and their pairs are dropped
  refused("nbodies", [](idto::ModelFile* v) {
    const int b = (int)v->parent.size() - 1;
    const int dq = v->nq - v->qstart[b], dv = v->nv - v->vstart[b];
    for (std::vector<int>* t : {&v->parent, &v->jtype, &v->qstart, &v->vstart, &v->body_path}) t->pop_back();
    if (!v->gravity_enabled.empty()) v->gravity_enabled.pop_back();
    v->X_PF.resize(12 * b); v->axis.resize(3 * b); v->mass.resize(b); v->com.resize(3 * b); v->inertia.resize(6 * b);
    v->nq -= dq; v->nv -= dv; v->damping.resize(v->nv); v->actuated.resize(v->nv);
    std::vector<int> keep_g(v->geom_body.size(), -1), gb, gt, pa, pb, pp;
    std::vector<double> gx, gs;
    for (size_t g = 0; g < v->geom_body.size(); ++g)
      if (v->geom_body[g] != b) {
        keep_g[g] = (int)gb.size(); gb.push_back(v->geom_body[g]); gt.push_back(v->geom_type[g]);
        gx.insert(gx.end(), v->geom_X.begin() + 12 * g, v->geom_X.begin() + 12 * g + 12);
        gs.insert(gs.end(), v->geom_size.begin() + 3 * g, v->geom_size.begin() + 3 * g + 3);
      }
    for (size_t k = 0; k < v->pair_a.size(); ++k)
      if (keep_g[v->pair_a[k]] >= 0 && keep_g[v->pair_b[k]] >= 0) {
        pa.push_back(keep_g[v->pair_a[k]]); pb.push_back(keep_g[v->pair_b[k]]); pp.push_back(v->pair_path[k]);
      }
    v->geom_body = gb; v->geom_type = gt; v->geom_X = gx; v->geom_size = gs; v->pair_a = pa; v->pair_b = pb; v->pair_path = pp;
  }, true);
  // a sphere turned into a capsule (of its own radius: a valid capsule where a capsule is allowed)
  {
    int sphere = -1;
    for (size_t g = 0; g < base.geom_type.size() && sphere < 0; ++g)
      if (base.geom_type[g] == IDTO_GEOM_SPHERE) sphere = (int)g;
    if (sphere >= 0)
      refused("geom_type", [&](idto::ModelFile* v) { v->geom_type[sphere] = IDTO_GEOM_CAPSULE; v->geom_size[3 * sphere + 1] = 0.01; v->geom_size[3 * sphere + 2] = 0.0; }, true);
  }
  // parent and pair_path: a change the model's own checks pass exists for some models only (main() asks for one of each)
  int named = 0;
  for (size_t b = 1; b < base.parent.size(); ++b)
    for (int p = -1; p < (int)b; ++p) {
      if (p == base.parent[b] || (named & 1)) continue;
      idto::ModelFile v = base;
      v.parent[b] = p;
      const idto_model_t vm = v.c_model();
      ModelTables t;
      std::string e;
      if (BuildModelTables(&vm, &t, &e) == 0 && refused("parent", [&](idto::ModelFile* w) { w->parent[b] = p; })) named |= 1;
    }
  for (size_t k = 0; k < base.pair_path.size(); ++k)
    for (int p = 0; p < base.npaths; ++p) {
      if (p == base.pair_path[k] || (named & 2)) continue;
      idto::ModelFile v = base;
      v.pair_path[k] = p;
      const idto_model_t vm = v.c_model();
      ModelTables t;
      std::string e;
      if (BuildModelTables(&vm, &t, &e) == 0 && refused("pair_path", [&](idto::ModelFile* w) { w->pair_path[k] = p; })) named |= 2;
    }
  return named;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: model_batch_check <model file> ...\n"); return 2; }
  int named = 0;
  for (int i = 1; i < argc; ++i) {
    try {
      named |= CheckModel(argv[i]);
    } catch (const std::exception& e) {
      std::printf("FAILED %s: %s\n", argv[i], e.what());
      ++g_failed;
    }
  }
  // (a changed parent / pair_path that is still a valid model: at least one of the models must have offered one)
  if (!(named & 1)) { std::printf("FAILED: no model had a valid changed parent to refuse\n"); ++g_failed; }
  if (!(named & 2)) { std::printf("FAILED: no model had a valid changed pair_path to refuse\n"); ++g_failed; }
  if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
  std::printf("ok: %d models\n", argc - 1);
  return 0;
}
