// model_batch.cc — see model_batch.h.
#include "model_batch.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace idto_host {
namespace {

int Differs(std::string* err, int problem, const char* what) {
  *err = "model of problem " + std::to_string(problem) + " differs from the batch's model in " + what;
  return -1;
}

bool SameInts(const int* a, const int* b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(int)) == 0; }

// the derived int tables: (name, first int, ints) - a table ends where the next one in the blob begins
struct IntTable { const char* name; size_t at, n; };
std::vector<IntTable> IntTablesOf(const ModelTables& t) {
  std::vector<IntTable> v;
#define X(name) v.push_back(IntTable{#name, t.at.name, 0});
  IDTO_MODEL_INT_TABLES(X)
#undef X
  size_t first = v[0].at;
  for (const IntTable& e : v) first = std::min(first, e.at);
  const size_t end = 2 * t.blob.size();   // (the trailing pad is zeros in every model's blob)
  for (IntTable& e : v) {
    size_t next = end;
    for (const IntTable& o : v)
      if (o.at > e.at) next = std::min(next, o.at);
    e.n = next - e.at;
    e.at -= first;   // relative to the int part: the double part in front may not be compared here
  }
  return v;
}
size_t FirstInt(const ModelTables& t) {
  size_t first = t.at.parent;
#define X(name) first = std::min(first, t.at.name);
  IDTO_MODEL_INT_TABLES(X)
#undef X
  return first;
}

}  // namespace

std::vector<double> ModelRecord(const idto_model_t* m, const ModelTables& t, const idto_contact_params_t& contact) {
  const size_t n = t.blob.size();
  std::vector<double> r(idto_dev::model_record_doubles(n), 0.0);
  std::copy(t.blob.begin(), t.blob.end(), r.begin());
  ContactValues(contact, r.data() + idto_dev::model_record_contact_at(n));
  for (int i = 0; i < idto_dev::MREC_GRAVITY; ++i) r[idto_dev::model_record_gravity_at(n) + i] = m->gravity[i];
  return r;
}

int BuildModelVariant(const idto_model_t* base, const ModelTables& base_t, int problem, const idto_model_t* m,
                      const idto_contact_params_t& contact, std::vector<double>* record, std::string* err,
                      ModelTables* tables_out) {
  ModelTables own;
  ModelTables& t = tables_out ? *tables_out : own;
  if (int rc = BuildModelTables(m, &t, err)) return rc;   // (every check of a model, with its own text)
  // ---- the sizes
#define SIZE(name) if (m->name != base->name) return Differs(err, problem, #name);
  SIZE(nbodies) SIZE(nq) SIZE(nv) SIZE(ngeoms) SIZE(npairs) SIZE(npaths) SIZE(common_body)
#undef SIZE
  // ---- the model's own int tables, so that the refusal names what the caller changed
  const size_t nb = (size_t)m->nbodies, nv = (size_t)m->nv, ng = (size_t)m->ngeoms, np = (size_t)m->npairs;
#define TABLE(name, n) if (!SameInts(m->name, base->name, n)) return Differs(err, problem, #name);
  TABLE(parent, nb) TABLE(jtype, nb) TABLE(qstart, nb) TABLE(vstart, nb) TABLE(actuated, nv)
  TABLE(geom_body, ng) TABLE(geom_type, ng) TABLE(pair_a, np) TABLE(pair_b, np) TABLE(body_path, nb) TABLE(pair_path, np)
#undef TABLE
  for (size_t i = 0; i < nb; ++i)   // (NULL: gravity acts on every body)
    if ((m->gravity_enabled ? m->gravity_enabled[i] : 1) != (base->gravity_enabled ? base->gravity_enabled[i] : 1))
      return Differs(err, problem, "gravity_enabled");
  // ---- what BuildModelTables derived: the kernels' int tables ...
  {
    const std::vector<IntTable> a = IntTablesOf(base_t), b = IntTablesOf(t);
    const int* ai = reinterpret_cast<const int*>(base_t.blob.data()) + FirstInt(base_t);
    const int* bi = reinterpret_cast<const int*>(t.blob.data()) + FirstInt(t);
    for (size_t i = 0; i < a.size(); ++i)
      if (a[i].at != b[i].at || a[i].n != b[i].n || !SameInts(ai + a[i].at, bi + b[i].at, a[i].n)) return Differs(err, problem, a[i].name);
  }
  // ... where every table starts, and the scalars
#define X(name) if (t.at.name != base_t.at.name) return Differs(err, problem, #name);
  IDTO_MODEL_DOUBLE_TABLES(X) IDTO_MODEL_INT_TABLES(X)
#undef X
#define SCALAR(name) if (t.name != base_t.name) return Differs(err, problem, #name);
  SCALAR(maxpp) SCALAR(nfloat)
  for (int i = 0; i < 4; ++i) {
    if (t.float_qs[i] != base_t.float_qs[i]) return Differs(err, problem, "float_qs");
    if (t.float_vs[i] != base_t.float_vs[i]) return Differs(err, problem, "float_vs");
  }
  SCALAR(fast_shape) SCALAR(fast_lo) SCALAR(fast_n) SCALAR(f_maxpp) SCALAR(nxb) SCALAR(nstem) SCALAR(gcommon) SCALAR(gstem)
  SCALAR(gslots) SCALAR(maxc) SCALAR(capsules) SCALAR(cylinders)
#undef SCALAR
  if (t.blob.size() != base_t.blob.size()) return Differs(err, problem, "the blob's size");
  *record = ModelRecord(m, t, contact);
  return 0;
}

}  // namespace idto_host
