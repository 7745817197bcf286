// fd_plan.h — every finite-difference launch (fd_launch.hip's kernels, and the evaluation that the fused launch embeds): its
// block, the evaluations per pass, whether the assembly products fold into it, the dynamic LDS, the grid, the evaluation's
// shape and which kernel runs - one decision, made here, as a pure function of (sizes, model tables, options, request).
// Host-only C++ (no HIP include): idto_hip.hip fills pointers and strides and launches what the plan names;
// tests/cpp/fd_plan_check.cc holds the unit to tests/golden/fd_plans.txt and the LDS formula to the kernel's carve-up on the CPU.
#pragma once

#include <string>

namespace idto_host {

// What the decision reads of a context, and nothing else (idto_hip.hip FdShapeOf fills it)
struct FdShape {
  int nq = 0, nv = 0, npaths = 1, batch = 1;
  // the model's tables (host/model_tables.h): the whole blob, the part a tree shape's kernel stages, the shape, the longest
  // chain, the bodies of shared pairs, the stem
  int blob_n = 0, fast_n = 0, fast_shape = 0, maxc = 1, nxb = 0, nstem = 0;
  bool lane_map = false;        // the model takes the lane map without the redundant path lanes (ModelTables::fd_dedup)
  bool model_records = false;   // a batch whose problems have parameter records of their own
  // the options of the same names
  bool fd_fast = true, fd_dedup = true, asm_fold = true, weights_diagonal = true;
  int gradients_method = 0;
};

struct FdRequest {
  enum Kind {
    RESIDENT,     // records [kb, ke) of the context's q, grid.y = problem
    CANDIDATES,   // tau of `m` candidate points of each problem (grid.y = candidate; a batch: grid.z = problem)
    FUSED,        // the evaluation inside gn_fused_kernel: generic, the whole blob, the context's widest block, no fold
  };
  Kind kind = RESIDENT;
  int mode = 0;   // 0: tau only; >= 1: with derivatives, by the context's gradients_method
  int kb = 0, ke = 0;
  int m = 0;
};

// which kernel of fd_launch.hip runs
enum FdFamily {
  FD,                // fd_kernel
  FD_DEDUP,          // fd_dedup_kernel: forward differences on the lane map without the redundant path lanes
  FD_MODELS,         // fd_models_kernel: a batch with per-problem parameter records
  FD_DEDUP_MODELS,   // fd_dedup_models_kernel
  FD_ALONG,          // fd_along_kernel: candidate points of one problem, tau only
  FD_ALONG_BATCH,    // fd_along_batch_kernel: ... of the problems of a batch
  FD_ALONG_MODELS,   // fd_along_models_kernel: ... with per-problem parameter records
};

struct FdPlan {
  int mode = 0;     // what the kernel gets: 0 tau only, 1 forward, 2 central, 3 central (4th order)
  int E = 1;        // evaluations of a record
  int block = 64;   // threads; groups = block / npaths evaluations run concurrently
  int groups = 64;
  int echunk = 1;   // evaluations whose inputs are built per pass: all E, or a multiple of groups
  bool fold = false;   // the launch also forms the single-record products of the assembly (the kernel's `terms`)
  int lds = 0;      // dynamic LDS, bytes
  int grid_x = 0, grid_y = 1, grid_z = 1;   // (FUSED: the launch's grid is its own)
  int shape = 0;    // the evaluation: a tree shape of model_layout.h, 0 generic, SHAPE_XCH, SHAPE_STEM
  int maxc = 8;     // the chain bound the kernel is instantiated with: the shape's KC, or the bucket 2 / 3 / 4 / 8 of the longest chain
  bool dedup = false;
  FdFamily family = FD;
};

// the chain bound the generic evaluation is instantiated with for a model whose longest chain has `maxc` bodies: 2, 3, 4 or 8
int FdChainBound(int maxc);

// 0, or -1 with *err: the evaluation set does not fit in LDS
int PlanFd(const FdShape& shape, const FdRequest& request, FdPlan* plan, std::string* err);

// What idto_hip_create checks: the widest block (one wavefront per 64 lanes of forward differences' E * npaths, up to 256)
// and the smallest carve-up of forward differences - the inputs of one round of concurrent evaluations per pass
struct FdCreate { int fd_threads, fd_lds; };
FdCreate FdCreateGeometry(const FdShape& shape);

}  // namespace idto_host
