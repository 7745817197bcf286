// lin_launch.hip — the kernels of plant_lin.h and their launches
#include "plant_lin.h"

namespace idto_dev {

void lin_perturb_launch(const LinArgs& a, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(lin_perturb_kernel, dim3(a.S, batch), dim3(256), 0, stream, a);
}

void lin_difference_launch(const LinArgs& a, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(lin_difference_kernel, dim3(a.S, batch), dim3(256), 0, stream, a);
}

void tvlqr_launch(const TvlqrArgs& a, int batch, int lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(tvlqr_kernel, dim3(batch), dim3(256), lds_bytes, stream, a);
}

hipError_t tvlqr_set_max_lds(int max_lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&tvlqr_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
}

}  // namespace idto_dev
