// track_launch.hip — the instantiations of track_kernel (plant.h) and their launch; the dispatch is plant_launch.hip's.
#include "track_launch.h"

namespace idto_dev {

template <int MC, bool XCH, bool STEM = false>
static void go(const PlantLaunch& a, const TrackArgs& t) {
  hipLaunchKernelGGL((track_kernel<MC, XCH, STEM>), dim3(a.plants), dim3(a.block), a.lds, a.stream, a.args, t);
}
// (a launch above 64 KiB of dynamic LDS fails without this opt-in: its result is the caller's to check, per instantiation)
template <int MC, bool XCH, bool STEM = false>
static hipError_t allow(int max_lds) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&track_kernel<MC, XCH, STEM>), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
}

void track_launch(const PlantLaunch& a, const TrackArgs& t) {
  if (a.nstem > 1) go<8, true, true>(a, t);
  else if (a.nxb) go<8, true>(a, t);
  else if (a.maxc <= 2) go<2, false>(a, t);
  else if (a.maxc <= 3) go<3, false>(a, t);
  else if (a.maxc <= 4) go<4, false>(a, t);
  else go<8, false>(a, t);
}

hipError_t track_set_max_lds(int max_lds) {
  const hipError_t rc[] = {allow<2, false>(max_lds), allow<3, false>(max_lds), allow<4, false>(max_lds), allow<8, false>(max_lds),
                           allow<8, true>(max_lds), allow<8, true, true>(max_lds)};
  for (hipError_t e : rc)
    if (e != hipSuccess) return e;
  return hipSuccess;
}

}  // namespace idto_dev
