#!/bin/bash
# Builds libidto_hip.so (gfx950 kernels + C-ABI; RCCL for the multi-GPU slab exchange is resolved at run time: dlopen).
# hipcc cross-compiles without a GPU.
# -ffp-contract=off: host/device bit-exactness of the finite-difference path.
# -amdgpu-mfma-vgpr-form: MFMA results land in VGPRs, not AGPRs (saves the v_accvgpr_read moves on
# the solver's products phase: -150 cycles per block row).
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Iinclude -Iidto_amd/csrc"
mkdir -p build
# six HIP translation units, compiled side by side: the finite-difference kernel, the plants' kernel, the scene report's, the
# linearisation's, the tracked rollouts' and everything else.
# -Rpass-analysis=kernel-resource-usage: the compiler's register / scratch / spill figures per kernel go to
# build/*.remarks, and tools/check_resources.py FAILS THE BUILD when a production kernel spills vector registers or
# exceeds its scratch / SGPR-spill limit (fd_kernel once computed wrong partials after an edit
# pushed its SGPR spills from 105 to 146 - that must not wait for a GPU to be noticed).
REM="-Rpass-analysis=kernel-resource-usage"
( $HIPCC $FLAGS $FD_FLAGS $REM -c idto_amd/csrc/fd_launch.hip -o build/fd_launch.o "$@" 2> build/fd_launch.remarks || { grep -v "remark:" build/fd_launch.remarks >&2; exit 1; } ) &
# the plants' kernel (csrc/plant.h): a unit of its own beside the two, so that those compile to what they compiled to without it
( $HIPCC $FLAGS $REM -c idto_amd/csrc/plant_launch.hip -o build/plant_launch.o "$@" 2> build/plant_launch.remarks || { grep -v "remark:" build/plant_launch.remarks >&2; exit 1; } ) &
# the scene report's kernel (csrc/scene_report.h): a unit of its own for the same reason
( $HIPCC $FLAGS $REM -c idto_amd/csrc/scene_launch.hip -o build/scene_launch.o "$@" 2> build/scene_launch.remarks || { grep -v "remark:" build/scene_launch.remarks >&2; exit 1; } ) &
# the linearisation's and the Riccati recursion's kernels (csrc/plant_lin.h): a unit of their own for the same reason
( $HIPCC $FLAGS $REM -c idto_amd/csrc/lin_launch.hip -o build/lin_launch.o "$@" 2> build/lin_launch.remarks || { grep -v "remark:" build/lin_launch.remarks >&2; exit 1; } ) &
# the plants under the time-varying LQR law (csrc/plant.h track_kernel): a unit of its own for the same reason
( $HIPCC $FLAGS $REM -c idto_amd/csrc/track_launch.hip -o build/track_launch.o "$@" 2> build/track_launch.remarks || { grep -v "remark:" build/track_launch.remarks >&2; exit 1; } ) &
# the model's checks and tables: host-only C++ (no HIP include), so that the unit also builds for the CPU under sanitizers.
# -ffp-contract=off, no fast-math: its gathered records use explicit std::fma and a deliberate 0.0 + x.
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/model_tables.cc -o build/model_tables.o ) &
# which solver kernel serves a system, and with which geometry: host-only as well (tests/cpp/solver_plan_check.cc sweeps it on the CPU)
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/solver_plan.cc -o build/solver_plan.o ) &
# what may differ between the models of a batch, and a problem's parameter record: host-only (tests/cpp/model_batch_check.cc)
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/model_batch.cc -o build/model_batch.o ) &
# where every per-problem array lies in a context's arena, and the launch sizes that are pure functions of the sizes: host-only
# (tests/cpp/context_layout_check.cc holds it to tests/golden/context_layout.txt on the CPU)
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/context_layout.cc -o build/context_layout.o ) &
# what the plant family's entries (csrc/*_abi.inc) refuse, the sizes of their launches and where a call's arrays lie: host-only
# (tests/cpp/plant_calls_check.cc holds it to tests/golden/plant_call_layouts.txt and to every message on the CPU)
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/plant_calls.cc -o build/plant_calls.o ) &
# every finite-difference launch - block, evaluations per pass, fold, LDS, grid, kernel: host-only (tests/cpp/fd_plan_check.cc
# holds it to tests/golden/fd_plans.txt and the LDS formula to the kernel's carve-up on the CPU)
( g++ -O2 -std=c++17 -fPIC -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc -c idto_amd/csrc/host/fd_plan.cc -o build/fd_plan.o ) &
$HIPCC $FLAGS -mllvm -amdgpu-mfma-vgpr-form=1 $MAIN_FLAGS $REM -c idto_amd/csrc/idto_hip.hip -o build/idto_hip.o "$@" 2> build/idto_hip.remarks || { grep -v "remark:" build/idto_hip.remarks >&2; exit 1; }
wait %1
wait %2
wait %3
wait %4
wait %5
wait %6
wait %7
wait %8
wait %9
wait %10
wait %11
grep -h -A3 "warning:" build/fd_launch.remarks build/idto_hip.remarks build/plant_launch.remarks build/scene_launch.remarks build/lin_launch.remarks build/track_launch.remarks >&2 || true
if [ -z "$IDTO_SKIP_RESOURCE_CHECK" ]; then python3 tools/check_resources.py build/fd_launch.remarks build/idto_hip.remarks build/plant_launch.remarks build/scene_launch.remarks build/lin_launch.remarks build/track_launch.remarks > build/resource_check.txt || { cat build/resource_check.txt >&2; exit 1; }; fi
$HIPCC --offload-arch=gfx950 -fPIC -shared build/fd_launch.o build/plant_launch.o build/scene_launch.o build/lin_launch.o build/track_launch.o build/idto_hip.o build/model_tables.o build/solver_plan.o build/model_batch.o build/context_layout.o build/plant_calls.o build/fd_plan.o -o idto_amd/libidto_hip.so -ldl
# libidto_opt.so: the host-side TrajectoryOptimizer (C++) + its C-ABI, on top of libidto_hip.so
g++ -O3 -std=c++17 -fPIC -shared -Wall -Iinclude -Iidto_amd/csrc idto_amd/csrc/host/trajectory_optimizer.cc \
  idto_amd/csrc/host/batch_rows.cc idto_amd/csrc/host/ls_rows.cc idto_amd/csrc/host/mpc_controller.cc idto_amd/csrc/host/idto_opt_c.cc -o idto_amd/libidto_opt.so -Lidto_amd -lidto_hip -Wl,-rpath,'$ORIGIN'

# a C++ consumer of the boundary with no Python in the process (tests/test_gpu_cpp_consumer.py runs it on the GPU box)
g++ -O2 -std=c++17 -Wall -Iinclude tests/cpp/solve_acrobot.cc -o build/solve_acrobot -Lidto_amd -lidto_opt -lidto_hip -Wl,-rpath,'$ORIGIN/../idto_amd'
# ... and one of TrajectoryOptimizer::Tvlqr (tests/test_gpu_tvlqr_cpp.py)
g++ -O2 -std=c++17 -Wall -Iinclude tests/cpp/tvlqr_acrobot.cc -o build/tvlqr_acrobot -Lidto_amd -lidto_opt -lidto_hip -Wl,-rpath,'$ORIGIN/../idto_amd'
# ... and one of TrajectoryOptimizer::Track (tests/test_gpu_plant_track.py)
g++ -O2 -std=c++17 -Wall -Iinclude tests/cpp/track_pendulum.cc -o build/track_pendulum -Lidto_amd -lidto_opt -lidto_hip -Wl,-rpath,'$ORIGIN/../idto_amd'

# csrc/plant_tangent.h and csrc/tvlqr_step.h compiled for the host, as a program the tests drive through files (tests/lin_cases.py)
g++ -O1 -std=c++17 -ffp-contract=off -Wall -Wextra -Iinclude -Iidto_amd/csrc tests/cpp/lin_host.cc -o build/lin_host
