// track_launch.h — how idto_hip.hip starts track_kernel (plant.h: plant_body with the time-varying LQR law): its
// instantiations live in csrc/track_launch.hip, a translation unit of their own, so that fd_launch.hip, plant_launch.hip,
// scene_launch.hip, lin_launch.hip and idto_hip.hip's kernels compile to what they compiled to without them.
#pragma once

#include <hip/hip_runtime.h>

#include "plant_launch.h"

namespace idto_dev {

// enqueues track_kernel<MAXC, XCH, STEM> on a.plants workgroups (a.args: PlantArgs with substeps = S * m, record_every = m);
// the caller checks hipGetLastError()
void track_launch(const PlantLaunch& a, const TrackArgs& t);
// opt-in of every instantiation to `max_lds` bytes of dynamic LDS: hipSuccess, or the first instantiation's error
hipError_t track_set_max_lds(int max_lds);

}  // namespace idto_dev
