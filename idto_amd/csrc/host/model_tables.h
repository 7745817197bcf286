// model_tables.h — everything idto_hip_create derives from an idto_model_t before it touches a device: the checks of
// the model and the tables DevModel (id_eval.h) points at, packed as the one blob the kernels stage.  Plain C++: the
// unit builds, runs and is sanitized without HIP.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "idto_model.h"
#include "model_layout.h"   // IDTO_MODEL_DOUBLE_TABLES / IDTO_MODEL_INT_TABLES: DevModel's table pointers, by member name

namespace idto_host {

struct ModelTables {
  // the double tables, then the int tables (two per double slot) and a trailing pad
  std::vector<double> blob;
  // where each table starts: a double table as an index into blob, an int table as an index into the blob read as int[]
  struct Offsets {
#define X(name) size_t name = 0;
    IDTO_MODEL_DOUBLE_TABLES(X) IDTO_MODEL_INT_TABLES(X)
#undef X
  } at;
  // DevModel's scalars of the same names
  int maxpp = 1, nfloat = 0, float_qs[4] = {0, 0, 0, 0}, float_vs[4] = {0, 0, 0, 0};
  int fast_shape = 0, fast_lo = 0, fast_n = 0, f_maxpp = 1, nxb = 0, nstem = 0, gcommon = 1, gstem = 0;
  unsigned long long gslots = 0;
  // the context's: the longest chain, and whether the model has a capsule / a cylinder
  int maxc = 1;
  bool capsules = false, cylinders = false;
  // fd_kernel's forward-difference lane map without the redundant path lanes (model_layout.h tree_shape_dedup): whether the
  // model takes it (then the blob read as int[] holds kFdMainLanes + kFdHelperLanes lane words from fd_lanes_at on, right
  // behind f_seg's words and inside the part a shape's kernel stages; else none), and what it was
  // derived from - the paths (bit p) that column c of q / mass column j touches, all of them for a column of the common body
  bool fd_dedup = false;
  size_t fd_lanes_at = 0;
  std::vector<int> fd_qpaths, fd_vpaths;
};

// 0, or -1 with the refusal in *err.  The checks run in a fixed order - geometry, stem, then paths, joints, gravity
// switches, chains and pairs - and the first one that fails is reported.
int BuildModelTables(const idto_model_t* m, ModelTables* out, std::string* err);

}  // namespace idto_host
