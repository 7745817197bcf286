// plant_launch.hip — the instantiations of plant_kernel (plant.h) and their launch; the dispatch mirrors fd_launch.hip's.
#include "plant_launch.h"

namespace idto_dev {

template <int MC, bool XCH>
static void go(const PlantLaunch& a) {
  hipLaunchKernelGGL((plant_kernel<MC, XCH>), dim3(a.plants), dim3(a.block), a.lds, a.stream, a.args);
}
template <int MC, bool XCH>
static void allow(int max_lds) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&plant_kernel<MC, XCH>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
}

void plant_launch(const PlantLaunch& a) {
  if (a.nxb) go<8, true>(a);   // (a stem below the common body: refused by idto_hip_plant_begin, plant_abi.inc PlantServes)
  else if (a.maxc <= 2) go<2, false>(a);
  else if (a.maxc <= 3) go<3, false>(a);
  else if (a.maxc <= 4) go<4, false>(a);
  else go<8, false>(a);
}

void plant_set_max_lds(int max_lds) {
  allow<2, false>(max_lds); allow<3, false>(max_lds); allow<4, false>(max_lds); allow<8, false>(max_lds);
  allow<8, true>(max_lds);
}

}  // namespace idto_dev
