// scene_launch.h — how idto_hip.hip starts scene_kernel (scene_report.h): its instantiations live in csrc/scene_launch.hip, a
// translation unit of their own, so that fd_launch.hip, plant_launch.hip and idto_hip.hip compile to what they compiled to
// without it.
#pragma once

#include <hip/hip_runtime.h>

#include "scene_report.h"

namespace idto_dev {

struct SceneLaunch {
  int nstates, batch, block, lds;
  hipStream_t stream;
  SceneArgs args;
};
// enqueues scene_kernel<args.records != null> on the grid (nstates, batch); the caller checks hipGetLastError()
void scene_launch(const SceneLaunch& a);
// opt-in of both instantiations to `max_lds` bytes of dynamic LDS: hipSuccess, or the first instantiation's error
hipError_t scene_set_max_lds(int max_lds);

}  // namespace idto_dev
