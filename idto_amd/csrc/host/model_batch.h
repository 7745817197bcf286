// model_batch.h — a batch whose problems have models of their own (idto_hip_set_model_batch): what may differ between
// the batch's model and problem b's, checked before any device is touched, and problem b's parameter record as the
// kernels read it (model_layout.h: blob | contact | gravity).  Plain C++ like model_tables.h: the unit builds, runs and is
// sanitized without HIP.
//
// Shared by every problem - the launch geometry, the LDS carve-up and the kernel instantiation are chosen once per
// context: the sizes, every int table of the model (the tree, the joints, the geometry types, the pairs and their paths,
// the actuated mask, the gravity switches), hence every int table and scalar that BuildModelTables derives from them.
// Free per problem: the double tables (X_PF, axis, mass, com, inertia, damping, geom_X, geom_size), gravity[3] and the
// contact parameters.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "idto/detmath.h"
#include "idto_model.h"
#include "model_tables.h"

namespace idto_host {

// DevContact's six doubles (id_eval.h: k, vd, vs, mu, sigma, threshold) of a set of contact parameters.  The ONE place
// that forms the threshold: reference TO.cc:266-269, evaluated with the same deterministic exp / log as the device code.
inline void ContactValues(const idto_contact_params_t& c, double v[6]) {
  v[0] = c.contact_stiffness; v[1] = c.dissipation_velocity; v[2] = c.stiction_velocity; v[3] = c.friction_coefficient;
  v[4] = c.smoothing_factor;
  const double eps = std::sqrt(2.220446049250313e-16);
  v[5] = -v[4] * idto::detmath::log(idto::detmath::exp(eps / (v[4] * v[0])) - 1.0);
}

// The parameter record (model_record_doubles(blob size) doubles) of a model whose tables are `t`
std::vector<double> ModelRecord(const idto_model_t* m, const ModelTables& t, const idto_contact_params_t& contact);

// Problem `problem`'s record for model `m` in a batch of `base` (tables `base_t`).  0, or -1 with the refusal in *err:
// BuildModelTables' own text for a model it refuses, else "model of problem <b> differs from the batch's model in
// <name>", <name> the first that differs of: the sizes, the model's int tables, the derived int tables
// (IDTO_MODEL_INT_TABLES), the derived scalars, the blob's size.  tables_out (optional): the variant's tables.
int BuildModelVariant(const idto_model_t* base, const ModelTables& base_t, int problem, const idto_model_t* m,
                      const idto_contact_params_t& contact, std::vector<double>* record, std::string* err,
                      ModelTables* tables_out = nullptr);

}  // namespace idto_host
