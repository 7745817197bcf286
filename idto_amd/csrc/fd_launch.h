// fd_launch.h — how idto_hip.hip starts fd_kernel: its instantiations live in csrc/fd_launch.hip, a
// translation unit of their own (built in parallel with the solvers, with its own scheduling flags: build.sh).
#pragma once

#include <hip/hip_runtime.h>

#include "fd_kernel.h"

namespace idto_dev {

struct FdLaunch {
  dim3 grid, block;
  int lds;
  hipStream_t stream;
  DevModel M;
  DevContact cp;
  DevProblem P;
  const double* q;
  double* slab;
  int slab_stride;
  double *v, *a, *nplus;
  int k_begin, mode, stop_after, echunk;
  size_t pstride;
  double* terms;
  AltSel alt;
  const double* gate = nullptr;   // a device word: the launch returns at once when it is not 0.0
  size_t cstride = 0;   // != 0: grid.y counts candidate points of one problem, cstride bytes apart: fd_along_kernel, mode 0
  // along_batch: grid.z counts the problems of a batch as well (fd_along_batch_kernel): their arrays pstride bytes apart, their
  // candidates' arenas bstride bytes, their gate words gstride bytes
  bool along_batch = false; size_t bstride = 0, gstride = 0;
  // records != nullptr: a batch whose problems have parameter records of their own, mstride bytes apart (fd_models_kernel,
  // fd_along_models_kernel): the kernel reads the problem's DevModel and DevContact rec_model / rec_contact bytes into its
  // record (model_layout.h model_record_*), not this struct's M and cp
  const double* records = nullptr; size_t mstride = 0, rec_contact = 0, rec_model = 0;
  int shape;   // id_fast.h: the model's instantiated tree shape, 0: id_eval<MAXC>, SHAPE_XCH: id_eval<8, true> (shared pairs), SHAPE_STEM: id_eval<8, true, true>
  int maxc;
  // forward differences on the lane map without the redundant path lanes (fd_dedup_kernel / fd_dedup_models_kernel): a shape
  // with model_layout.h's tree_shape_dedup, mode 1, a block of kFdMainLanes + kFdHelperLanes threads, no candidates
  bool dedup = false;
};
// enqueues fd_kernel<MAXC, SHAPE>; the caller checks hipGetLastError()
void fd_launch(const FdLaunch& a);
// opt-in of every instantiation to `max_lds` bytes of dynamic LDS
void fd_set_max_lds(int max_lds);

}  // namespace idto_dev
