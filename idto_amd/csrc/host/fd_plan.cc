// fd_plan.cc — see fd_plan.h.
#include "host/fd_plan.h"

#include <algorithm>

#include "fd_sizes.h"

namespace idto_host {
namespace {

using namespace idto_dev;

// the context's widest block: a wavefront per 64 lanes of forward differences' (evaluation, path) pairs, up to 256 - one wave
// per SIMD: the evaluation keeps its bodies in up to 512 VGPRs
int FdThreads(const FdShape& s) { return std::min(256, (fd_evals(1, s.nq, s.nv) * s.npaths + 63) / 64 * 64); }

// dynamic LDS of fd_kernel, bytes, when it builds the inputs of `ec` evaluations per pass in a block of `threads`
// (fast: fd_kernel<MAXC, SHAPE != 0>, which stages only the shape's records of the model; the fused launch runs the
// generic evaluation and stages the whole blob)
int LdsBytes(const FdShape& s, int mode, int ec, bool with_terms, bool fast, int threads) {
  const int blob_n = (fast && s.fd_fast && s.fast_shape) ? s.fast_n : s.blob_n;   // what fd_body stages of the model
  // the exchange of shared pairs and of a stem, per concurrent evaluation - or, in its place, what the main and helper
  // lanes of the lane map without the redundant path lanes hand each other
  const int xch = fd_xch_doubles(s.nxb, threads, s.npaths, s.nstem) + ((fast && s.lane_map && mode == 1) ? fd_dedup_doubles() : 0);
  return (int)sizeof(double) * fd_lds_doubles(s.nq, s.nv, fd_evals(mode, s.nq, s.nv), ec, with_terms, blob_n, xch);
}

// Threads of fd_kernel's block.  A stem model keeps a record per touched body and concurrent evaluation in LDS (punyo: 1.8 KB
// an evaluation): where the carve-up of one round does not fit beside them, the block shrinks by a wavefront at a time and
// the launch goes in rounds (punyo, forward differences: 48 concurrent evaluations - the 43 with contact and 5 mass-matrix
// columns in the first round, the other 15 columns, which have no contact, in the second).
int Block(const FdShape& s, int mode) {
  if (mode == 0) return 64;
  int t = FdThreads(s);
  while (s.nstem > 1 && t > 64 && LdsBytes(s, mode, t / s.npaths, false, true, t) > kMaxDynamicLds) t -= 64;
  return t;
}

// evaluations per pass: all of them if they fit in LDS, otherwise the largest multiple of the number of evaluations the
// block runs concurrently; -1: not even one round fits
int Chunk(const FdShape& s, FdPlan* p, bool fast, int threads, std::string* err) {
  int ec = p->E;
  while (ec > p->groups && LdsBytes(s, p->mode, ec, p->fold, fast, threads) > kMaxDynamicLds) ec = ((ec - 1) / p->groups) * p->groups;
  p->echunk = ec;
  p->lds = LdsBytes(s, p->mode, ec, p->fold, fast, threads);
  if (p->lds > kMaxDynamicLds) {
    if (err) *err = "finite-difference evaluation set does not fit in LDS";
    return -1;
  }
  return 0;
}

}  // namespace

int FdChainBound(int maxc) { return maxc <= 2 ? 2 : (maxc <= 3 ? 3 : (maxc <= 4 ? 4 : 8)); }

int PlanFd(const FdShape& s, const FdRequest& r, FdPlan* plan, std::string* err) {
  FdPlan p;
  p.mode = r.mode >= 1 ? 1 + s.gradients_method : 0;   // 1 forward, 2 central, 3 central (4th order)
  p.E = fd_evals(p.mode, s.nq, s.nv);
  if (r.kind == FdRequest::FUSED) {   // gn_fused_kernel's block is 256 threads; its exchange term is the widest block's (none: FusedVariant)
    p.block = 256; p.groups = 256 / s.npaths;
    p.maxc = FdChainBound(s.maxc);
    *plan = p;
    return Chunk(s, plan, false, p.mode >= 1 ? FdThreads(s) : 64, err);
  }
  const bool along = r.kind == FdRequest::CANDIDATES;
  p.block = Block(s, p.mode);
  p.groups = p.block / s.npaths;
  // fd_kernel also forms the single-record products of the Gauss-Newton assembly (diagonal weights, derivatives
  // requested): grad_hess then only combines them - where the record fits beside one round of evaluations
  p.fold = s.asm_fold && s.weights_diagonal && p.mode >= 1;
  if (p.fold && LdsBytes(s, p.mode, std::min(p.E, p.groups), true, true, p.block) > kMaxDynamicLds) p.fold = false;
  p.grid_x = r.ke - r.kb; p.grid_y = along ? r.m : s.batch;
  if (along && s.batch > 1) p.grid_z = s.batch;
  p.shape = s.fd_fast ? s.fast_shape : 0;    // id_fast.h: the straight-line evaluation of the model's tree shape
  if (s.nxb) p.shape = SHAPE_XCH;            // shared pairs: the generic evaluation with the exchange (whatever fd_fast says)
  if (s.nstem > 1) p.shape = SHAPE_STEM;     // a stem below the common body: ... and the walk along it
  p.maxc = p.shape ? tree_shape(p.shape).KC : FdChainBound(s.maxc);
  p.dedup = p.mode == 1 && !along && s.fd_dedup && s.fd_fast && s.lane_map && p.shape == s.fast_shape && tree_shape_dedup(p.shape) &&
            p.block == kFdMainLanes + kFdHelperLanes;
  if (s.model_records && along) p.family = FD_ALONG_MODELS;
  else if (p.dedup) p.family = s.model_records ? FD_DEDUP_MODELS : FD_DEDUP;
  else if (s.model_records) p.family = FD_MODELS;
  else if (along) p.family = s.batch > 1 ? FD_ALONG_BATCH : FD_ALONG;
  *plan = p;
  return Chunk(s, plan, true, p.block, err);
}

FdCreate FdCreateGeometry(const FdShape& s) {
  const int threads = Block(s, 1);   // (a stem model: fewer where the exchange records leave no room, PlanFd decides per mode)
  return FdCreate{FdThreads(s), LdsBytes(s, 1, threads / s.npaths, false, true, threads)};
}

}  // namespace idto_host
