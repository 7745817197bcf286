// fd_launch.hip — the instantiations of fd_kernel (fd_kernel.h) and their launch.
#include "fd_launch.h"

#include <utility>

namespace idto_dev {

// The instantiations: the generic evaluation for chains of up to 2, 3, 4 and 8 bodies, and one kernel per row of
// model_layout.h's shapes - the tree shapes, SHAPE_XCH, SHAPE_STEM - with the chain bound the table gives it.
template <int MC, int SH>
static void go(const FdLaunch& a) {
  using namespace idto_host;
  const FdPlan& p = a.plan;
  const dim3 grid(p.grid_x, p.grid_y, p.grid_z), block(p.block);
  switch (p.family) {
    case FD_ALONG_MODELS:   // candidate points of a batch with per-problem parameter records
      hipLaunchKernelGGL((fd_along_models_kernel<MC, SH>), grid, block, p.lds, a.stream, a.records, a.mstride, a.rec_contact,
                         a.rec_model, a.P, a.q, a.slab, a.slab_stride, a.v, a.a, a.nplus, a.k_begin, a.stop_after, p.echunk, a.cstride, a.gate, a.pstride,
                         a.bstride, a.gstride);
      return;
    case FD_DEDUP_MODELS:   // forward differences on the lane map without the redundant path lanes (mode 1, 256 threads)
    case FD_DEDUP:
      if constexpr (tree_shape_dedup(SH)) {
        if (p.family == FD_DEDUP_MODELS)
          hipLaunchKernelGGL((fd_dedup_models_kernel<MC, SH>), grid, block, p.lds, a.stream, a.records, a.mstride, a.rec_contact, a.rec_model,
                             a.P, a.q, a.slab, a.slab_stride, a.v, a.a, a.nplus, a.k_begin, a.stop_after, p.echunk, a.pstride, a.terms, a.alt);
        else
          hipLaunchKernelGGL((fd_dedup_kernel<MC, SH>), grid, block, p.lds, a.stream, a.M, a.cp, a.P, a.q, a.slab, a.slab_stride, a.v,
                             a.a, a.nplus, a.k_begin, a.stop_after, p.echunk, a.pstride, a.terms, a.alt);
      }
      return;
    case FD_MODELS:   // a batch with per-problem parameter records
      hipLaunchKernelGGL((fd_models_kernel<MC, SH>), grid, block, p.lds, a.stream, a.records, a.mstride, a.rec_contact, a.rec_model,
                         a.P, a.q, a.slab, a.slab_stride, a.v, a.a, a.nplus, a.k_begin, p.mode, a.stop_after, p.echunk, a.pstride, a.terms, a.alt);
      return;
    case FD_ALONG_BATCH:   // candidate points of the problems of a batch, tau only
      hipLaunchKernelGGL((fd_along_batch_kernel<MC, SH>), grid, block, p.lds, a.stream, a.M, a.cp, a.P, a.q, a.slab,
                         a.slab_stride, a.v, a.a, a.nplus, a.k_begin, a.stop_after, p.echunk, a.cstride, a.gate, a.pstride,
                         a.bstride, a.gstride);
      return;
    case FD_ALONG:   // candidate points of one problem, tau only
      hipLaunchKernelGGL((fd_along_kernel<MC, SH>), grid, block, p.lds, a.stream, a.M, a.cp, a.P, a.q, a.slab, a.slab_stride,
                         a.v, a.a, a.nplus, a.k_begin, a.stop_after, p.echunk, a.cstride, a.gate);
      return;
    case FD:
      hipLaunchKernelGGL((fd_kernel<MC, SH>), grid, block, p.lds, a.stream, a.M, a.cp, a.P, a.q, a.slab, a.slab_stride, a.v,
                         a.a, a.nplus, a.k_begin, p.mode, a.stop_after, p.echunk, a.pstride, a.terms, a.alt);
      return;
  }
}
template <int MC, int SH>
static void allow(int max_lds) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_along_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_along_batch_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_models_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_along_models_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  if constexpr (tree_shape_dedup(SH)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_dedup_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fd_dedup_models_kernel<MC, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
  }
}
using Shapes = std::make_integer_sequence<int, SHAPE_STEM>;   // (shape = 1 + the index)

template <int... I>
static void go_shape(const FdLaunch& a, std::integer_sequence<int, I...>) {
  ((a.plan.shape == I + 1 ? go<tree_shape(I + 1).KC, I + 1>(a) : void()), ...);
}
void fd_launch(const FdLaunch& a) {
  if (a.plan.shape) go_shape(a, Shapes{});
  else if (a.plan.maxc == 2) go<2, 0>(a);
  else if (a.plan.maxc == 3) go<3, 0>(a);
  else if (a.plan.maxc == 4) go<4, 0>(a);
  else go<8, 0>(a);
}

template <int... I>
static void allow_shapes(int max_lds, std::integer_sequence<int, I...>) {
  (allow<tree_shape(I + 1).KC, I + 1>(max_lds), ...);
}
void fd_set_max_lds(int max_lds) {
  allow<2, 0>(max_lds); allow<3, 0>(max_lds); allow<4, 0>(max_lds); allow<8, 0>(max_lds);
  allow_shapes(max_lds, Shapes{});
}

}  // namespace idto_dev
