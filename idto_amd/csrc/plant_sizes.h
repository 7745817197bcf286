// plant_sizes.h — how much dynamic LDS the plant family's kernels take and how wide the scene report's block is, as pure
// functions of the sizes: what plant.h, lin_launch.h, scene_report.h and id_eval.h carve by on the device and what the host
// sizes a launch by (host/plant_calls.cc).  Plain C++ like plant_tangent.h, no HIP type and no HIP include: the host-only
// units include it as it is, hipcc compiles the same text for both sides.
#pragma once

#include <cstddef>

#include "plant_step.h"

namespace idto_dev {

// A body's record in the exchange area of id_eval<MAXC, true>: R (row-major), p, w, v - the doubles contact_pair reads -,
// then the contact force and moment on the body (XEXT: summed there by the lane that owns the body)
constexpr int XREC = 24, XEXT = 18;
// id_eval<MAXC, true, true>: behind the M.nxb records of an evaluation, one block per stem body below the common one with what the
// backward pass needs of it: the joint axis hW, the inertial wrench (fin, nin) and the offset r of the NEXT stem body from it
constexpr int SAUX = 12, SA_HW = 0, SA_FIN = 3, SA_NIN = 6, SA_RC = 9;
IDTO_PLANT_HD inline int xch_eval_doubles(int nxb, int nstem) { return nxb * XREC + (nstem > 1 ? nstem - 1 : 0) * SAUX; }

// what PD+ adds to plant_kernel's LDS, in doubles: the plan, the breaks, the gains, the nominal [q, v, u], the actuated dofs
IDTO_PLANT_HD inline size_t plant_pd_doubles(int nq, int nv, int nu, int n, size_t plan_len) {
  return plan_len + (size_t)n + (size_t)nu * (nq + nv) + (size_t)(nq + nv + nu) + (size_t)(nu + 1) / 2;
}
// what the time-varying LQR law adds to the LDS, in doubles: K_t, x*_t, tau*_t, dx, the actuated dofs (u_t goes straight into tau_app)
IDTO_PLANT_HD inline size_t plant_law_doubles(int nq, int nv, int nu) {
  return (size_t)nu * 2 * nv + (size_t)(nq + nv) + (size_t)nv + (size_t)2 * nv + (size_t)(nu + 1) / 2;
}
// dynamic LDS of plant_kernel in doubles, for a block of `threads`
IDTO_PLANT_HD inline int plant_lds_doubles(int nq, int nv, int blob_n, int nxb, int nstem, int npaths, int threads) {
  return 3 * nq + 7 * nv + (2 * nv - 1) + (nv + 1) * nv + 2 + blob_n + (threads / npaths) * xch_eval_doubles(nxb, nstem);
}

// dynamic LDS of tvlqr_kernel in doubles: P, A, W, Acl, Q [n x n]; Bu, PBu [n x nu]; K, RK [nu x n]; G, R [nu x nu]; col [nu]
IDTO_PLANT_HD inline size_t tvlqr_lds_doubles(int n, int nu) {
  return 5 * (size_t)n * n + 4 * (size_t)n * nu + 2 * (size_t)nu * nu + (size_t)nu;
}

// a body's record in scene_kernel's LDS: put_state's 18 doubles, then hW (the axis of a revolute / prismatic joint in the world)
constexpr int SREC = 21, SR_HW = 18;
IDTO_PLANT_HD inline int scene_row_stride(int nv) { return nv | 1; }
// dynamic LDS of scene_kernel in doubles
IDTO_PLANT_HD inline size_t scene_lds_doubles(int nb, int nq, int nv, int npairs, int blob_n) {
  return (size_t)blob_n + nq + nv + (size_t)nb * SREC + (size_t)npairs * scene_row_stride(nv);
}
// threads of its block: a lane per body, pair (in rounds beyond 256) and DoF
IDTO_PLANT_HD inline int scene_block(int nb, int nv, int npairs) {
  const int want = nb > nv ? (nb > npairs ? nb : npairs) : (nv > npairs ? nv : npairs);
  const int t = (want + 63) / 64 * 64;
  return t < 64 ? 64 : (t > 256 ? 256 : t);
}

}  // namespace idto_dev
