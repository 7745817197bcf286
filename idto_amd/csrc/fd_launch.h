// fd_launch.h — how idto_hip.hip starts fd_kernel: its instantiations live in csrc/fd_launch.hip, a
// translation unit of their own (built in parallel with the solvers, with its own scheduling flags: build.sh).
#pragma once

#include <hip/hip_runtime.h>

#include "fd_kernel.h"
#include "host/fd_plan.h"

namespace idto_dev {

struct FdLaunch {
  idto_host::FdPlan plan;   // the kernel, grid, block, LDS, mode, chunk and shape (host/fd_plan.h PlanFd)
  hipStream_t stream;
  DevModel M;
  DevContact cp;
  DevProblem P;
  const double* q;
  double* slab;
  int slab_stride;
  double *v, *a, *nplus;
  int k_begin, stop_after;
  size_t pstride;
  double* terms;   // (plan.fold: the context's products, else nullptr)
  AltSel alt;
  const double* gate = nullptr;   // a device word: the launch returns at once when it is not 0.0
  size_t cstride = 0;   // candidate points (grid.y), cstride bytes apart: fd_along_kernel, mode 0
  // ... of the problems of a batch (grid.z, fd_along_batch_kernel): their arrays pstride bytes apart, their candidates' arenas
  // bstride bytes, their gate words gstride bytes
  size_t bstride = 0, gstride = 0;
  // records != nullptr: a batch whose problems have parameter records of their own, mstride bytes apart (fd_models_kernel,
  // fd_along_models_kernel): the kernel reads the problem's DevModel and DevContact rec_model / rec_contact bytes into its
  // record (model_layout.h model_record_*), not this struct's M and cp
  const double* records = nullptr; size_t mstride = 0, rec_contact = 0, rec_model = 0;
};
// enqueues the plan's kernel <plan.maxc, plan.shape>; the caller checks hipGetLastError()
void fd_launch(const FdLaunch& a);
// opt-in of every instantiation to `max_lds` bytes of dynamic LDS
void fd_set_max_lds(int max_lds);

}  // namespace idto_dev
