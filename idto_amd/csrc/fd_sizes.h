// fd_sizes.h — how many evaluations a finite-difference launch runs and how much dynamic LDS fd_kernel takes, as pure
// functions of the sizes: what fd_kernel.h and id_fast.h carve by on the device and what the host plans a launch by
// (host/fd_plan.cc).  Plain C++ like plant_sizes.h, no HIP type and no HIP include: the host-only units include it as it
// is, hipcc compiles the same text for both sides.
#pragma once

#include "model_layout.h"
#include "plant_sizes.h"

namespace idto_dev {

// the most dynamic LDS a kernel of the library asks for, in bytes (every kernel that needs more than the default 64 KiB opts in to this)
constexpr int kMaxDynamicLds = 160 * 1024;

// evaluations of one record.  mode 0: tau only; 1: forward differences (+ nv mass-matrix columns for dtau_k/dq_{k-1});
// 2 / 3: central differences of 2nd / 4th order, every partial from evaluations at q + m dq, m in {+1,-1} / {+1,-1,+2,-2}
IDTO_PLANT_HD inline int fd_evals(int mode, int nq, int nv) {
  return (mode == 0) ? 1 : ((mode == 1) ? 1 + 2 * nq + nv : 1 + ((mode == 2) ? 2 : 4) * 3 * nq);
}

// the part of fd_body's LDS that id_eval<MAXC, true> exchanges the chain states through: a record per chain body that a
// pair touches, for each of the block's concurrent evaluations
IDTO_PLANT_HD inline int fd_xch_doubles(int nxb, int threads, int npaths, int nstem = 0) {
  return (threads / npaths) * xch_eval_doubles(nxb, nstem);
}

// ---- the forward-difference lane map without the redundant path lanes (model_layout.h tree_shape_dedup):
// what main and helper lanes hand each other through LDS.  Every value is stored and read back as it is - an exact copy.
enum { FDX_STATE = 19, FDX_RES = 9 };   // doubles per body state (18 used) and per pair result (fc, nc, hit); odd strides: no bank conflicts
constexpr int fd_dedup_doubles() {
  return kFdMainLanes * FDX_STATE + (kFdMainLanes / 4) * FDX_STATE + kFdMainLanes * FDX_RES + (kFdMainLanes / 4) * FDX_RES + 4 * 12;
}

// Dynamic LDS of fd_kernel in doubles when it builds the inputs of `ec` of its E evaluations per pass: what a launch asks
// for.  A closed formula with slack for the alignment steps of fd_body's carve-up, which fd_carve below walks exactly:
// each restates the other, and tests/cpp/fd_plan_check.cc holds fd_carve's end to this on the CPU.
//   with_terms: the record, its weighted copy, diag R', tau R' (+1: 16-byte alignment)
//   blob_n: what fd_body stages of the model; xch: the exchange area and the lane map's, together
IDTO_PLANT_HD inline int fd_lds_doubles(int nq, int nv, int E, int ec, bool with_terms, int blob_n, int xch) {
  const int nvp = (nv + 1) & ~1;
  const int rec = with_terms ? 6 * nvp * nq + 2 * nvp + 1 : 0;
  return 3 * nq + 2 * nv * nq + 3 * nv + 3 * E + E * nv + ec * (nq + 2 * nv) + nv + blob_n + 2 + nq / 2 + 2 + rec + xch;
}

// fd_body's carve-up (fd_kernel.h, the pointer walk from qm1 to xch) as offsets in doubles from the start of the dynamic
// LDS, in the kernel's order and with its alignment steps.  EC = min(echunk, E).  wr and tw are meant with_terms only (the
// exchange area then lies behind them, else at rec).  lanes: the lane map's area - the kernels that use it have an empty
// exchange area, so it begins where fd_body puts it, at xch.  end: behind the last region.
struct FdCarve {
  int qm1, q0, q1, N0, N1, v0, v1, a0, edq, edv, eda, etau, eq, ev, ea, edump, mblob, colinfo, rec, wr, tw, xch, lanes, end;
};
IDTO_PLANT_HD inline FdCarve fd_carve(int nq, int nv, int E, int EC, bool with_terms, int blob_n, int xch_doubles, int lane_doubles) {
  const int bsz = nv * nq, nvp = (nv + 1) & ~1, psz = nvp * nq;
  FdCarve c;
  c.qm1 = 0;
  c.q0 = c.qm1 + nq;
  c.q1 = c.q0 + nq;
  c.N0 = c.q1 + nq;
  c.N1 = c.N0 + bsz;
  c.v0 = c.N1 + bsz;
  c.v1 = c.v0 + nv;
  c.a0 = c.v1 + nv;
  c.edq = c.a0 + nv;
  c.edv = c.edq + E;
  c.eda = c.edv + E;
  c.etau = c.eda + E;
  c.eq = c.etau + E * nv;
  c.ev = c.eq + EC * nq;
  c.ea = c.ev + EC * nv;
  c.edump = c.ea + EC * nv;
  c.mblob = c.edump + nv;
  c.colinfo = c.mblob + blob_n + (blob_n & 1);        // [nq] ints
  c.rec = c.colinfo + (nq + (nq & 1)) / 2;
  c.rec += c.rec & 1;                                 // (16-byte aligned)
  c.wr = c.rec + 6 * psz;
  c.tw = c.wr + nvp;
  c.xch = c.rec + (with_terms ? 6 * psz + 2 * nvp : 0);
  c.lanes = c.xch + xch_doubles;
  c.end = c.lanes + lane_doubles;
  return c;
}

}  // namespace idto_dev
