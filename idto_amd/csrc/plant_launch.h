// plant_launch.h — how idto_hip.hip starts plant_kernel (plant.h): its instantiations live in csrc/plant_launch.hip, a
// translation unit of their own, so that fd_launch.hip and idto_hip.hip compile to what they compiled to without it.
#pragma once

#include <hip/hip_runtime.h>

#include "plant.h"

namespace idto_dev {

struct PlantLaunch {
  int plants, block, lds;
  hipStream_t stream;
  PlantArgs args;
  int maxc;      // the model's longest chain: the generic evaluation for chains of up to 2, 3, 4 and 8 bodies
  int nxb;       // DevModel's: shared pairs -> id_eval<8, true>
  int nstem;     // DevModel's: a stem below the common body -> id_eval<8, true, true>
};
// enqueues plant_kernel<MAXC, XCH, STEM>; the caller checks hipGetLastError()
void plant_launch(const PlantLaunch& a);
// opt-in of every instantiation to `max_lds` bytes of dynamic LDS: hipSuccess, or the first instantiation's error
hipError_t plant_set_max_lds(int max_lds);

}  // namespace idto_dev
