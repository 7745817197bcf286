// scene_launch.hip — the instantiations of scene_kernel (scene_report.h) and their launch
#include "scene_launch.h"

namespace idto_dev {

void scene_launch(const SceneLaunch& a) {
  const dim3 grid(a.nstates, a.batch), block(a.block);
  if (a.args.records) hipLaunchKernelGGL(scene_kernel<true>, grid, block, a.lds, a.stream, a.args);
  else hipLaunchKernelGGL(scene_kernel<false>, grid, block, a.lds, a.stream, a.args);
}

hipError_t scene_set_max_lds(int max_lds) {
  const hipError_t rc[] = {
      hipFuncSetAttribute(reinterpret_cast<const void*>(&scene_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds),
      hipFuncSetAttribute(reinterpret_cast<const void*>(&scene_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds)};
  for (hipError_t e : rc)
    if (e != hipSuccess) return e;
  return hipSuccess;
}

}  // namespace idto_dev
