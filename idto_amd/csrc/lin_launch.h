// lin_launch.h — how idto_hip.hip starts lin_perturb_kernel, lin_difference_kernel and tvlqr_kernel (plant_lin.h): their
// arguments and launches.  The kernels themselves live in csrc/lin_launch.hip, a translation unit of their own, so that
// fd_launch.hip, plant_launch.hip, scene_launch.hip and idto_hip.hip's kernels compile to what they compiled to without them.
#pragma once

#include <hip/hip_runtime.h>

#include "plant_sizes.h"
#include "plant_tangent.h"

namespace idto_dev {

using idto_plant::lin_columns;

struct LinArgs {
  int S, P, nb, nq, nv;
  const int* jtype; const int* qstart; const int* vstart;   // the model's tables (the topology: one per context)
  const double* x;       // [B][S][nq + nv]
  const double* tau;     // [B][S][nv]
  double eps, two_eps;
  double* pstate;        // [B][S * P][1 + nq + nv]: the columns' plants
  double* ptau;          // [B][S * P][nv]
  const int* pstatus;    // [B][S * P][2]: plant_kernel's status words
  double* x_next;        // [B][S][nq + nv]
  double* A;             // [B][S][n * n] column-major, n = 2 nv
  double* Bm;            // [B][S][n * nv]
  int* status;           // [B][S][2]
};

struct TvlqrArgs {
  int S, nv, nu;
  const int* actuated;   // [nu] velocity indices: the columns Bu of B
  const double* A;       // [B][S][n * n]
  const double* Bm;      // [B][S][n * nv]
  const double* Q; const double* R; const double* Qf;   // [n * n], [nu * nu], [n * n], column-major (symmetric)
  double* K;             // [B][S][nu * n]
  double* P;             // [B][S + 1][n * n]
  int* status;           // [B]
};

// (dynamic LDS of tvlqr_kernel: plant_sizes.h tvlqr_lds_doubles)

// each enqueues its kernel on `stream`; the caller checks hipGetLastError()
void lin_perturb_launch(const LinArgs& a, int batch, hipStream_t stream);      // grid (S, batch)
void lin_difference_launch(const LinArgs& a, int batch, hipStream_t stream);   // grid (S, batch)
void tvlqr_launch(const TvlqrArgs& a, int batch, int lds_bytes, hipStream_t stream);   // grid (batch)
// opt-in of tvlqr_kernel to `max_lds` bytes of dynamic LDS
hipError_t tvlqr_set_max_lds(int max_lds);

}  // namespace idto_dev
