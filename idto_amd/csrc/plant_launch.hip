// plant_launch.hip — the instantiations of plant_kernel (plant.h) and their launch; the dispatch mirrors fd_launch.hip's.
#include "plant_launch.h"

namespace idto_dev {

template <int MC, bool XCH, bool STEM = false>
static void go(const PlantLaunch& a) {
  hipLaunchKernelGGL((plant_kernel<MC, XCH, STEM>), dim3(a.plants), dim3(a.block), a.lds, a.stream, a.args);
}
// (a launch above 64 KiB of dynamic LDS fails without this opt-in: its result is the caller's to check, per instantiation)
template <int MC, bool XCH, bool STEM = false>
static hipError_t allow(int max_lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&plant_kernel<MC, XCH, STEM>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
}

void plant_launch(const PlantLaunch& a) {
  if (a.nstem > 1) go<8, true, true>(a);
  else if (a.nxb) go<8, true>(a);
  else if (a.maxc <= 2) go<2, false>(a);
  else if (a.maxc <= 3) go<3, false>(a);
  else if (a.maxc <= 4) go<4, false>(a);
  else go<8, false>(a);
}

hipError_t plant_set_max_lds(int max_lds) {
  const hipError_t rc[] = {allow<2, false>(max_lds), allow<3, false>(max_lds), allow<4, false>(max_lds), allow<8, false>(max_lds),
                           allow<8, true>(max_lds), allow<8, true, true>(max_lds)};
  for (hipError_t e : rc)
    if (e != hipSuccess) return e;
  return hipSuccess;
}

}  // namespace idto_dev
