// id_eval.h — one inverse-dynamics evaluation with compliant contact, spread over
// the `npaths` adjacent lanes of a wavefront that cooperate on it.
//
// Replaces, for the hot path, what the reference asks Drake for in
// CalcInverseDynamicsSingleTimeStep (reference optimizer/trajectory_optimizer.cc:228-245):
// force elements (:232), CalcContactForceContribution (:247-386, restated in
// contact_pair() below line by line) and plant.CalcInverseDynamics (:244).
//
// Formulation: world-frame recursive Newton-Euler about the body origins.  Each
// lane owns one *path* of the model's star decomposition (include/idto_model.h):
// it evaluates the optional common root body redundantly, then its own chain of
// up to MAXC bodies entirely in registers (all loops over chain slots are
// unrolled so the per-slot state never leaves VGPRs), evaluates the contact
// pairs assigned to its path, and meets the other lanes of the evaluation only
// in two butterfly sums (contact wrench on the common body, chain-root wrenches).
// The association order of every floating-point sum is the one documented in
// DESIGN.md §3.2, which is what makes the result bit-identical to the serial
// CPU oracle.
#pragma once

#include "dev_math.h"
#include "idto_model.h"
#include "model_layout.h"
#include "plant_sizes.h"

namespace idto_dev {

struct DevModel {
  int nb, nq, nv, npaths, common_body, ngeoms, npairs, maxpp;
  const int* parent;
  const int* jtype;
  const int* qstart;
  const int* vstart;
  const double* X_PF;     // 12 per body
  const double* axis;     // 3
  const double* mass;     // 1
  const double* com;      // 3
  const double* inertia;  // 6
  const double* damping;  // nv
  double gravity[3];
  const int* geom_type;
  const double* geom_X;     // 12
  const double* geom_size;  // 3
  // star decomposition tables
  const int* chain;        // [npaths*MAXCHAIN] body index (-1 = unused slot)
  const int* nchain;       // [npaths]
  const int* pkind;        // [npaths*MAXCHAIN] 0 world, 1 common, 2 previous slot
  const int* path_npairs;  // [npaths]
  const int* path_pairs;   // [npaths*maxpp] pair index, ascending
  const int* pair_ga;      // geometry A of the pair
  const int* pair_gb;
  const int* pair_sa;      // body slot of geometry A: -2 world, -1 common, >= 0 chain slot
  const int* pair_sb;
  // all tables above live in ONE device buffer (doubles first, then the int tables) so that a
  // kernel can stage the whole model into LDS with one coalesced copy and rebase the pointers
  const double* blob;
  int blob_n;              // size in doubles
  // fd_kernel's prologue: the floating joints (nfloat < 0: more than four, nplus_pair looks them up), the constant part
  // of N+ (nv x nq column-major: ones and zeros, NaN where a quaternion block goes; in the blob, read from global memory)
  // and where the non-zeros of each column / row of N+ are (first | count << 16)
  int nfloat;
  int float_qs[4], float_vs[4];
  const double* nplus_const;
  const int* colinfo;
  const int* rowinfo;
  // id_fast.h: the instantiated tree shape this model has (0: none, id_eval<MAXC> serves it) and
  // the gathered records of its bodies and contact pairs (inside the blob)
  int fast_shape;
  int fast_lo, fast_n;     // the part of the blob (doubles) a kernel of that shape needs: the records, jtype, qstart, vstart, f_seg
  int f_maxpp;
  const double* f_body;
  const double* f_cbody;
  const double* f_pairs;
  const int* f_seg;
  // per-body gravity switch (idto_model_t::gravity_enabled), resolved at create: bit path * IDTO_MAX_CHAIN + slot is set
  // when that chain body's weight is applied, gcommon when the common body's is (all set: every body, the default)
  unsigned long long gslots;
  int gcommon;
  // shared pairs (a pair between the chains of two paths, include/idto_model.h), evaluated by id_eval<MAXC, true> through
  // an exchange area per evaluation: one record (XREC doubles, id_eval.h) per chain body that some pair touches.  nxb: how many
  // records (0: the model has no shared pair and no stem, every table below is unused); xrec: the record of (path, slot), -1 = none;
  // pair_xa / pair_xb: the record of the pair's body A / B, -1 the common body, -2 the world
  int nxb;
  const int* xrec;      // [npaths*IDTO_MAX_CHAIN]
  const int* pair_xa;   // [npairs]
  const int* pair_xb;
  // the stem (include/idto_model.h): the common body and its ancestors, world side first, evaluated by id_eval<MAXC, true, true>.
  // nstem: its bodies (0 / 1: the common body, if any, is attached to the world - every table below is unused); stem: [2 *
  // IDTO_MAX_STEM] body k of the stem, then its state record in the exchange area (-1: no pair touches it; the common body: -1);
  // gstem: bit k set when the weight of stem body k < nstem - 1 is applied (the common body's: gcommon).  A pair's stem side has
  // the code -4 - k in pair_sa / pair_sb and its state record in pair_xa / pair_xb.
  int nstem;
  const int* stem;
  int gstem;
};

// The model with every table pointer rebased from the global blob to a copy at `dst`
// (LDS: the per-body tables sit on the dependent chain of id_eval; from L2 each access costs
// ~1-2 us of exposed latency, from LDS ~100 cycles).
IDTO_DEV DevModel rebase_model(const DevModel& M, const double* dst) {
  DevModel L = M;
  auto d = [&](const double* p) { return dst + (p - M.blob); };
  auto i = [&](const int* p) {
    return reinterpret_cast<const int*>(dst) + (p - reinterpret_cast<const int*>(M.blob));
  };
  L.parent = i(M.parent); L.jtype = i(M.jtype); L.qstart = i(M.qstart); L.vstart = i(M.vstart);
  L.X_PF = d(M.X_PF); L.axis = d(M.axis); L.mass = d(M.mass); L.com = d(M.com); L.inertia = d(M.inertia);
  L.damping = d(M.damping);
  L.geom_type = i(M.geom_type); L.geom_X = d(M.geom_X); L.geom_size = d(M.geom_size);
  L.chain = i(M.chain); L.nchain = i(M.nchain); L.pkind = i(M.pkind);
  L.path_npairs = i(M.path_npairs); L.path_pairs = i(M.path_pairs);
  L.pair_ga = i(M.pair_ga); L.pair_gb = i(M.pair_gb); L.pair_sa = i(M.pair_sa); L.pair_sb = i(M.pair_sb);
  L.f_body = d(M.f_body); L.f_cbody = d(M.f_cbody); L.f_pairs = d(M.f_pairs); L.f_seg = i(M.f_seg);
  L.xrec = i(M.xrec); L.pair_xa = i(M.pair_xa); L.pair_xb = i(M.pair_xb);
  L.stem = i(M.stem);
  L.blob = dst;
  return L;
}

struct DevContact {
  double k, vd, vs, mu, sigma, threshold;
};

static_assert(sizeof(DevContact) == MREC_CONTACT * sizeof(double), "model_layout.h: the record's contact doubles are a DevContact");
static_assert(sizeof(DevModel) <= MREC_DEVMODEL * sizeof(double), "model_layout.h: the record's room for a DevModel");

// M with every table pointer (model_layout.h's two lists) and the blob moved from its blob to a copy of it at `blob`:
// how the DevModel in a problem's parameter record is made from the context's (idto_hip_set_model_batch)
__host__ __device__ inline void shift_model(DevModel& M, const double* blob) {
  const ptrdiff_t shift = reinterpret_cast<const char*>(blob) - reinterpret_cast<const char*>(M.blob);
#define X(name) M.name = reinterpret_cast<decltype(M.name)>(reinterpret_cast<const char*>(M.name) + shift);
  IDTO_MODEL_DOUBLE_TABLES(X) IDTO_MODEL_INT_TABLES(X)
#undef X
  M.blob = blob;
}
// A problem's parameter record, read like a kernel's arguments are: through the constant address space - the record is
// written by the host before the launch and by nobody during it -, so that a uniform access is a scalar load whatever the
// kernel has stored in between, a member indexed at run time (float_qs) included.  (A DevModel shifted inside the kernel
// is a private copy that such an index keeps in scratch: 424 B a lane, and up to 107 spilled vector registers.)
typedef const char __attribute__((address_space(4))) * RecordPtr;
IDTO_DEV RecordPtr record_at(const double* records, size_t byte_off) {
  return (RecordPtr)(reinterpret_cast<const char*>(records) + byte_off);
}

struct BodyState {  // what later stages need of a body
  M3 R;
  V3 p, w, v;
};

// (a body's record in the exchange area of id_eval<MAXC, true> - XREC, XEXT -, a stem body's block behind the records - SAUX,
// SA_* - and xch_eval_doubles: plant_sizes.h, which the host-only units read as well)
IDTO_DEV void put_v3(double* x, V3 a) { x[0] = a.x; x[1] = a.y; x[2] = a.z; }
IDTO_DEV V3 get_v3(const double* x) { return mk(x[0], x[1], x[2]); }
IDTO_DEV void put_state(double* x, const BodyState& b) {
#pragma unroll
  for (int i = 0; i < 9; ++i) x[i] = b.R.m[i];
  x[9] = b.p.x; x[10] = b.p.y; x[11] = b.p.z;
  x[12] = b.w.x; x[13] = b.w.y; x[14] = b.w.z;
  x[15] = b.v.x; x[16] = b.v.y; x[17] = b.v.z;
}
IDTO_DEV BodyState get_state(const double* x) {
  BodyState b;
#pragma unroll
  for (int i = 0; i < 9; ++i) b.R.m[i] = x[i];
  b.p = mk(x[9], x[10], x[11]); b.w = mk(x[12], x[13], x[14]); b.v = mk(x[15], x[16], x[17]);
  return b;
}
// The lanes of one evaluation are adjacent lanes of ONE wavefront, whose LDS accesses are carried out in issue order:
// between the records' stores and the other lanes' loads only the compiler has to be held back (no instruction is
// emitted for a wavefront-scope fence).
IDTO_DEV void wave_exchange_point() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct JointOut {
  M3 R_FM;
  V3 d2, w_rel, v_rel, al_rel, a_rel, hW;
};

// Joint kinematics in the world frame given the joint frame R_WF (restates the
// switch of oracle/rigid_body.h Kinematics()).
IDTO_DEV JointOut joint_kin(int jtype, const M3& R_WF, V3 axis, const double* qi, const double* vi, const double* ai) {
  JointOut o;
  const V3 zero = mk(0, 0, 0);
  o.R_FM = ident3();
  o.d2 = zero; o.w_rel = zero; o.v_rel = zero; o.al_rel = zero; o.a_rel = zero; o.hW = zero;
  if (jtype == IDTO_JOINT_REVOLUTE) {
    double s, c;
    idto::detmath::sincos(qi[0], &s, &c);
    o.R_FM = axis_angle(axis, s, c);
    o.hW = R_WF * axis;
    o.w_rel = o.hW * vi[0];
    o.al_rel = o.hW * ai[0];
  } else if (jtype == IDTO_JOINT_PRISMATIC) {
    o.hW = R_WF * axis;
    o.d2 = o.hW * qi[0];
    o.v_rel = o.hW * vi[0];
    o.a_rel = o.hW * ai[0];
  } else if (jtype == IDTO_JOINT_PLANAR) {
    double s, c;
    idto::detmath::sincos(qi[2], &s, &c);
    o.R_FM.m[0] = c; o.R_FM.m[1] = -s; o.R_FM.m[3] = s; o.R_FM.m[4] = c;
    const V3 ex = col(R_WF, 0), ey = col(R_WF, 1), ez = col(R_WF, 2);
    o.d2 = ex * qi[0] + ey * qi[1];
    o.v_rel = ex * vi[0] + ey * vi[1];
    o.a_rel = ex * ai[0] + ey * ai[1];
    o.w_rel = ez * vi[2];
    o.al_rel = ez * ai[2];
  } else {  // floating
    o.R_FM = quat_to_rot(qi);
    o.d2 = R_WF * mk(qi[4], qi[5], qi[6]);
    o.w_rel = R_WF * mk(vi[0], vi[1], vi[2]);
    o.v_rel = R_WF * mk(vi[3], vi[4], vi[5]);
    o.al_rel = R_WF * mk(ai[0], ai[1], ai[2]);
    o.a_rel = R_WF * mk(ai[3], ai[4], ai[5]);
  }
  return o;
}

struct SdResult {
  bool valid;
  double phi;
  V3 n, Ca, Cb;
};

// ---- capsules (include/idto_model.h): a capsule side of a pair becomes a sphere of the capsule's radius at a
// substitute centre on its segment p + u s, s in [-h, h] (u: the geometry frame's z in the world), and the sphere-sphere /
// sphere-box expressions of signed_distance then run unchanged.  s == 0 selects p itself: with h = 0 every rule clamps s
// to +-0, so a zero-length capsule is its sphere bit for bit.
constexpr double CAPSULE_PARALLEL = 1e-10;   // 1 - dot(u1, u2)^2 at or below which two segments count as parallel
IDTO_DEV double clamp_h(double s, double h) { return __builtin_fmin(__builtin_fmax(s, -h), h); }
IDTO_DEV V3 seg_point(V3 p, V3 u, double s) { return (s == 0.0) ? p : p + u * s; }
// one capsule (p, u, h) against a sphere centred at x, or against a world-fixed box of identity rotation: its lower end
IDTO_DEV V3 capsule_single(V3 p, V3 u, double h, int other, V3 x) {
  double s;
  if (other == IDTO_GEOM_SPHERE) s = clamp_h(dot(x - p, u), h);
  else s = ((p + u * h).z < (p + u * (-h)).z) ? h : -h;   // (a tie: the -h end)
  return seg_point(p, u, s);
}
// The substitute centres of a pair with a capsule side: *pA / *pB replaced for the capsule side(s).  Two capsules: the
// closest points of the segments (Ericson 5.1.9 with unit directions, parameters in [-h, h]); parallel segments take the
// middle of the overlap of segment A with B's projection onto A's line.
IDTO_DEV void capsule_centres(int typeA, V3 uA, double hA, V3* pA, int typeB, V3 uB, double hB, V3* pB) {
  if (typeA == IDTO_GEOM_CAPSULE && typeB == IDTO_GEOM_CAPSULE) {
    const V3 r = *pA - *pB;
    const double b = dot(uA, uB), c = dot(uA, r), f = dot(uB, r);
    const double denom = 1.0 - b * b;
    double s = (denom > CAPSULE_PARALLEL) ? clamp_h((b * f - c) / denom, hA)
                                          : clamp_h(0.5 * (__builtin_fmax(-hA, -c - hB) + __builtin_fmin(hA, hB - c)), hA);
    double t = b * s + f;
    if (t < -hB || t > hB) {
      t = clamp_h(t, hB);
      s = clamp_h(b * t - c, hA);
    }
    *pA = seg_point(*pA, uA, s);
    *pB = seg_point(*pB, uB, t);
  } else if (typeA == IDTO_GEOM_CAPSULE) {
    *pA = capsule_single(*pA, uA, hA, typeB, *pB);
  } else {
    *pB = capsule_single(*pB, uB, hB, typeA, *pA);
  }
}

// ---- cylinders (include/idto_model.h): the cylinder side (R, H, axis z of RX, centre *p) of a sphere-cylinder pair
// becomes, by the region of the sphere's centre x, the primitive whose existing expression is the closed form there:
//  - the side (|c.z| <= H and r > R, or inside with R - r <= H - |c.z| and r > 0): a sphere of radius R on the axis at the
//    height of x;
//  - the rim (|c.z| > H and r > R): a sphere of radius 0 at the rim point;
//  - the cap (r <= R above or below it, inside nearer to a cap, and r == 0 inside): a box of half extents (R, R, H).
//    There |c.x|, |c.y| <= r, so the box's x and y faces are never nearer than the side; at r == 0 its x face is the side
//    in the direction (1, 0, 0) with the box branch's own tie rule (dx <= dz), which is the cylinder's rule.
// *type, *p and *s are replaced; RX stays (a sphere reads no rotation).
IDTO_DEV void cylinder_reduce(const M3& RX, V3 x, int* type, V3* p, V3* s) {
  const double R = s->x, H = s->y;
  const V3 c = tmul(RX, x - *p);
  const double r = __builtin_sqrt(c.x * c.x + c.y * c.y), az = __builtin_fabs(c.z);
  const bool above = az > H;
  if (above ? (r <= R) : (r <= R && !(R - r <= H - az && r > 0))) {
    *type = IDTO_GEOM_BOX;
    *s = mk(R, R, H);
    return;
  }
  *type = IDTO_GEOM_SPHERE;
  const double k = above ? R / r : 0.0;
  *p = *p + RX * mk(c.x * k, c.y * k, above ? ((c.z >= 0) ? H : -H) : c.z);
  *s = mk(above ? 0.0 : R, 0, 0);
}

// Signed distance between two primitives (restates oracle SignedDistance(); capsules: reduced to spheres first, a
// cylinder: to the sphere or box of its region).
IDTO_DEV SdResult signed_distance(int typeA, const M3& RA, V3 pA, V3 sA, int typeB, const M3& RB, V3 pB, V3 sB) {
  SdResult out;
  out.valid = false; out.phi = 0; out.n = mk(0, 0, 1); out.Ca = mk(0, 0, 0); out.Cb = mk(0, 0, 0);
  // (unlikely: the register allocation of the kernels that compile this text follows the paths of the models without
  // a cylinder)
  if (__builtin_expect(typeA == IDTO_GEOM_CYLINDER || typeB == IDTO_GEOM_CYLINDER, 0)) {
    if (typeA == IDTO_GEOM_CYLINDER) cylinder_reduce(RA, pB, &typeA, &pA, &sA);
    else cylinder_reduce(RB, pA, &typeB, &pB, &sB);
  }
  if (typeA == IDTO_GEOM_CAPSULE || typeB == IDTO_GEOM_CAPSULE) {   // (radius: size[0], as a sphere's)
    capsule_centres(typeA, col(RA, 2), sA.y, &pA, typeB, col(RB, 2), sB.y, &pB);
    typeA = (typeA == IDTO_GEOM_CAPSULE) ? IDTO_GEOM_SPHERE : typeA;
    typeB = (typeB == IDTO_GEOM_CAPSULE) ? IDTO_GEOM_SPHERE : typeB;
  }
  if (typeA == IDTO_GEOM_SPHERE && typeB == IDTO_GEOM_SPHERE) {
    const V3 d = pB - pA;
    const double dist = __builtin_sqrt(dot(d, d));
    out.phi = (dist - sA.x) - sB.x;
    out.n = d / dist;
    out.Ca = pA + out.n * sA.x;
    out.Cb = pB - out.n * sB.x;
    out.valid = true;
  } else if ((typeA == IDTO_GEOM_SPHERE && typeB == IDTO_GEOM_BOX) ||
             (typeA == IDTO_GEOM_BOX && typeB == IDTO_GEOM_SPHERE)) {  // sphere-box in either order
    const bool sphere_is_A = (typeA == IDTO_GEOM_SPHERE);
    const V3 pS = sphere_is_A ? pA : pB;
    const double rad = sphere_is_A ? sA.x : sB.x;
    const M3& RX = sphere_is_A ? RB : RA;
    const V3 pX = sphere_is_A ? pB : pA;
    const V3 h = sphere_is_A ? sB : sA;
    const V3 c = tmul(RX, pS - pX);
    V3 pc = c;
    bool outside = false;
    if (pc.x > h.x) { pc.x = h.x; outside = true; } else if (pc.x < -h.x) { pc.x = -h.x; outside = true; }
    if (pc.y > h.y) { pc.y = h.y; outside = true; } else if (pc.y < -h.y) { pc.y = -h.y; outside = true; }
    if (pc.z > h.z) { pc.z = h.z; outside = true; } else if (pc.z < -h.z) { pc.z = -h.z; outside = true; }
    V3 g;
    double phi;
    if (outside) {
      const V3 dv = c - pc;
      const double dist = __builtin_sqrt(dot(dv, dv));
      g = dv / dist;
      phi = dist - rad;
    } else {
      const double dx = h.x - __builtin_fabs(c.x), dy = h.y - __builtin_fabs(c.y), dz = h.z - __builtin_fabs(c.z);
      g = mk(0, 0, 0);
      double depth;
      if (dx <= dy && dx <= dz) { depth = dx; g.x = (c.x >= 0) ? 1.0 : -1.0; pc.x = g.x * h.x; }
      else if (dy <= dz) { depth = dy; g.y = (c.y >= 0) ? 1.0 : -1.0; pc.y = g.y * h.y; }
      else { depth = dz; g.z = (c.z >= 0) ? 1.0 : -1.0; pc.z = g.z * h.z; }
      phi = -depth - rad;
    }
    const V3 gW = RX * g;
    const V3 boxW = pX + RX * pc;
    const V3 sphW = pS - gW * rad;
    out.phi = phi;
    if (sphere_is_A) { out.n = -gW; out.Ca = sphW; out.Cb = boxW; }
    else { out.n = gW; out.Ca = boxW; out.Cb = sphW; }
    out.valid = true;
  } else {  // box (moving) vs world-fixed axis-aligned box: lowest vertex against the top face
    const double ztop = pB.z + sB.z;
    double zmin = 0;
    V3 best = mk(0, 0, 0);
    bool first = true;
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy)
        for (int iz = 0; iz < 2; ++iz) {
          const V3 cb = mk(ix ? sA.x : -sA.x, iy ? sA.y : -sA.y, iz ? sA.z : -sA.z);
          const V3 cw = pA + RA * cb;
          if (first || cw.z < zmin) { zmin = cw.z; best = cw; first = false; }
        }
    out.phi = zmin - ztop;
    out.n = mk(0, 0, -1);
    out.Ca = best;
    out.Cb = mk(best.x, best.y, ztop);
    out.valid = true;
  }
  return out;
}

struct PairForce {
  bool active;
  V3 fA, nA, fB, nB;  // wrenches on bodies A and B about their origins (world frame)
};

// reference TO.cc:281-385 for one signed-distance pair
IDTO_DEV PairForce contact_pair(const DevModel& M, const DevContact& cp, int ga, int gb, const BodyState& A,
                                const BodyState& B) {
  PairForce out;
  out.active = false;
  const M3 RgA = A.R * ldm3(M.geom_X + 12 * ga);
  const V3 pgA = A.p + A.R * ldv3(M.geom_X + 12 * ga + 9);
  const M3 RgB = B.R * ldm3(M.geom_X + 12 * gb);
  const V3 pgB = B.p + B.R * ldv3(M.geom_X + 12 * gb + 9);
  const SdResult sd = signed_distance(M.geom_type[ga], RgA, pgA, ldv3(M.geom_size + 3 * ga), M.geom_type[gb], RgB,
                                      pgB, ldv3(M.geom_size + 3 * gb));
  if (!sd.valid) return out;
  if (sd.phi > cp.threshold) return out;
  const V3 nhat = sd.n;
  const V3 pC = (sd.Ca + sd.Cb) * 0.5;
  const V3 pAC = pC - A.p, pBC = pC - B.p;
  const V3 vAc = A.v + cross(A.w, pAC);
  const V3 vBc = B.v + cross(B.w, pBC);
  const V3 vrel = vBc - vAc;
  const double vn = dot(nhat, vrel);
  const V3 vt = vrel - nhat * vn;
  double dissipation = 0.0;
  const double s = vn / cp.vd;
  if (s < 0) dissipation = 1 - s;
  else if (s < 2) dissipation = (s - 2) * (s - 2) / 4;
  double compliant_fn;
  const double exponent = -sd.phi / cp.sigma;
  if (exponent >= 37) compliant_fn = -cp.k * sd.phi;
  else compliant_fn = cp.sigma * cp.k * idto::detmath::log(1 + idto::detmath::exp(exponent));
  const double fn = compliant_fn * dissipation;
  const V3 that = (-vt) / __builtin_sqrt(cp.vs * cp.vs + dot(vt, vt));
  const V3 ft = (that * cp.mu) * fn;
  out.fB = nhat * fn + ft;
  out.fA = -out.fB;
  out.nB = cross(pBC, out.fB);
  out.nA = cross(pAC, out.fA);
  out.active = true;
  return out;
}

// The gravity a body's inertial wrench subtracts: g, or exact zeros for a body whose weight is switched off - then
// (acom - 0) * m is acom * m bit for bit, the oracle's expression with a zero gravity vector.
IDTO_DEV V3 body_gravity(bool on, V3 g) { return mk(on ? g.x : 0.0, on ? g.y : 0.0, on ? g.z : 0.0); }
IDTO_DEV bool slot_gravity(unsigned long long gslots, int path, int s) {
  return ((gslots >> (path * IDTO_MAX_CHAIN + s)) & 1ull) != 0;
}

// Inertial wrench of body b about its origin, world frame.
IDTO_DEV void inertial_wrench(const DevModel& M, int b, const M3& R, V3 w, V3 al, V3 a, V3 g, V3* f_in, V3* n_in) {
  const V3 cW = R * ldv3(M.com + 3 * b);
  const V3 t1 = cross(al, cW);
  const V3 t2 = cross(w, cross(w, cW));
  const V3 acom = (a + t1) + t2;
  *f_in = (acom - g) * M.mass[b];
  const V3 wB = tmul(R, w), alB = tmul(R, al);
  const double* I = M.inertia + 6 * b;
  const V3 Iw = mk(fma3(I[0], wB.x, I[3], wB.y, I[4], wB.z), fma3(I[3], wB.x, I[1], wB.y, I[5], wB.z),
                   fma3(I[4], wB.x, I[5], wB.y, I[2], wB.z));
  const V3 Ial = mk(fma3(I[0], alB.x, I[3], alB.y, I[4], alB.z), fma3(I[3], alB.x, I[1], alB.y, I[5], alB.z),
                    fma3(I[4], alB.x, I[5], alB.y, I[2], alB.z));
  const V3 nB = Ial + cross(wB, Iw);
  *n_in = R * nB + cross(cW, *f_in);
}

// Generalised forces of body b's joint from the total wrench (f, n) on the body.
IDTO_DEV void put_tau(int j, double t, bool full, const double* damping, const double* v, double* tau) {
  tau[j] = full ? t + damping[j] * v[j] : t;
}
// Planar and floating joints are attached to the world (checked when the model is built), so
// their joint frame R_WF = I * R_PF is re-formed here from the model table (the same expression
// the forward pass evaluates) instead of being kept in 9 registers per body across the contact
// phase: that was what pushed the kernel over 512 registers per lane.
IDTO_DEV void project_tau(int jtype, int vs, const double* xpf, V3 hW, V3 f, V3 n, bool full, const double* damping,
                          const double* v, double* tau) {
  if (jtype == IDTO_JOINT_REVOLUTE) {
    put_tau(vs, dot(hW, n), full, damping, v, tau);
  } else if (jtype == IDTO_JOINT_PRISMATIC) {
    put_tau(vs, dot(hW, f), full, damping, v, tau);
  } else if (jtype == IDTO_JOINT_PLANAR) {
    const M3 R_WF = ident3() * ldm3(xpf);
    put_tau(vs, dot(col(R_WF, 0), f), full, damping, v, tau);
    put_tau(vs + 1, dot(col(R_WF, 1), f), full, damping, v, tau);
    put_tau(vs + 2, dot(col(R_WF, 2), n), full, damping, v, tau);
  } else {
    const M3 R_WF = ident3() * ldm3(xpf);
    const V3 nF = tmul(R_WF, n), fF = tmul(R_WF, f);
    put_tau(vs, nF.x, full, damping, v, tau);
    put_tau(vs + 1, nF.y, full, damping, v, tau);
    put_tau(vs + 2, nF.z, full, damping, v, tau);
    put_tau(vs + 3, fF.x, full, damping, v, tau);
    put_tau(vs + 4, fF.y, full, damping, v, tau);
    put_tau(vs + 5, fF.z, full, damping, v, tau);
  }
}

// tau = ID(q, v, a) for the lane's path.  q, v, a and tau point to this
// evaluation's arrays in LDS (tau: written for the lane's own DoFs; path 0 also
// writes the common body's).  `full` selects gravity + damping + contact, otherwise
// the mass-matrix column mode.  Must be called by all `npaths` lanes of the
// evaluation together (it contains cross-lane butterfly sums).
// XCH (models with shared pairs, M.nxb > 0): `xs` is the evaluation's exchange area in LDS (M.nxb records).  Each lane
// stores the state of its chain bodies that a pair touches as the forward pass forms them, and the pair loop reads
// every chain body of a pair from there - its own ones and those of another lane of the evaluation - so that the chain
// states are not kept in registers across the loop.  Both lanes of a shared pair run contact_pair on the same doubles
// and get the same bits; each adds its own side, into the contact sum of its body's record, in the pair order of the
// path's list.  The sums live in the records rather than in registers for the same reason: with
// them in registers the MAXC = 8 kernel spills vector registers to scratch.
// STEM (models whose common body has a parent, M.nstem > 1; implies XCH): every lane walks the stem from the world to the
// common body, parent by parent, keeping only the running state (`cb` ends as the common body's); path 0 leaves what the
// later stages need of the bodies below the common one in the exchange area - the state record of a body that a pair
// touches, and the SAUX block.  All pairs on one such body are in ONE path's list (checked at create), so that lane forms
// the body's contact sum in the record, in index order from +0, as it does for its own chain bodies.  Behind the butterflies
// path 0 takes the common body's total up the stem: tot = (f_in - ext) + child, the oracle's order.
template <int MAXC, bool XCH = false, bool STEM = false>
IDTO_DEV void id_eval(const DevModel& M, const DevContact& cp, int path, bool full, const double* q, const double* v,
                      const double* a, double* tau, double* xs = nullptr) {
  const V3 zero = mk(0, 0, 0);
  const V3 g = full ? mk(M.gravity[0], M.gravity[1], M.gravity[2]) : zero;

  // ---- common root body (identical in every lane of the evaluation)
  BodyState cb;
  cb.R = ident3(); cb.p = zero; cb.w = zero; cb.v = zero;
  V3 cb_al = zero, cb_a = zero, cb_fin = zero, cb_nin = zero;
  V3 cb_hW = zero;
  const int cbody = M.common_body;
  static_assert(!STEM || XCH, "the stem lives in the exchange area");
  if constexpr (STEM) {
    double* aux = xs + XREC * M.nxb;
    wave_exchange_point();   // (the previous evaluation's loads of this area come first)
    for (int k = 0; k < M.nstem; ++k) {
      const int b = M.stem[k];
      const M3 R_WF = cb.R * ldm3(M.X_PF + 12 * b);   // (k == 0: I * R_PF, as a chain root off the world)
      const V3 d1 = cb.R * ldv3(M.X_PF + 12 * b + 9);
      const JointOut j = joint_kin(M.jtype[b], R_WF, ldv3(M.axis + 3 * b), q + M.qstart[b], v + M.vstart[b], a + M.vstart[b]);
      const V3 rk = d1 + j.d2;
      const V3 al = (cb_al + j.al_rel) + cross(cb.w, j.w_rel);
      const V3 acc = (((cb_a + cross(cb_al, rk)) + cross(cb.w, cross(cb.w, rk))) + cross(cb.w, j.v_rel) * 2.0) + j.a_rel;
      const V3 vk = (cb.v + cross(cb.w, rk)) + j.v_rel;
      cb.R = R_WF * j.R_FM;
      cb.p = cb.p + rk;
      cb.w = cb.w + j.w_rel;
      cb.v = vk;
      cb_al = al;
      cb_a = acc;
      cb_hW = j.hW;
      const bool last = k == M.nstem - 1;
      inertial_wrench(M, b, cb.R, cb.w, cb_al, cb_a, body_gravity(last ? M.gcommon != 0 : ((M.gstem >> k) & 1) != 0, g), &cb_fin,
                      &cb_nin);
      if (path == 0) {
        if (k > 0) put_v3(aux + SAUX * (k - 1) + SA_RC, rk);
        if (!last) {
          double* ak = aux + SAUX * k;
          put_v3(ak + SA_HW, cb_hW); put_v3(ak + SA_FIN, cb_fin); put_v3(ak + SA_NIN, cb_nin);
          const int x = M.stem[IDTO_MAX_STEM + k];
          if (full && x >= 0) {
            put_state(xs + XREC * x, cb);
#pragma unroll
            for (int i = 0; i < 6; ++i) xs[XREC * x + XEXT + i] = 0.0;
          }
        }
      }
    }
  } else if (cbody >= 0) {
    const M3 cb_RWF = ldm3(M.X_PF + 12 * cbody);  // parent is the world: I * R_PF
    const V3 d1 = ldv3(M.X_PF + 12 * cbody + 9);
    const JointOut j = joint_kin(M.jtype[cbody], cb_RWF, ldv3(M.axis + 3 * cbody), q + M.qstart[cbody],
                                 v + M.vstart[cbody], a + M.vstart[cbody]);
    cb.R = cb_RWF * j.R_FM;
    cb.p = d1 + j.d2;
    cb.w = j.w_rel;
    cb.v = j.v_rel;
    cb_al = j.al_rel;
    cb_a = j.a_rel;
    cb_hW = j.hW;
    inertial_wrench(M, cbody, cb.R, cb.w, cb_al, cb_a, body_gravity(M.gcommon != 0, g), &cb_fin, &cb_nin);
  }

  // ---- own chain: forward pass
  BodyState bs[MAXC];
  V3 r[MAXC], hW[MAXC], fin[MAXC], nin[MAXC], fext[MAXC], next[MAXC];
  const int nch = M.nchain[path];
  V3 al_prev = zero, a_prev = zero;
  if constexpr (XCH) wave_exchange_point();   // (the previous evaluation's loads of this area come first)
#pragma unroll
  for (int s = 0; s < MAXC; ++s) {
    bs[s].R = ident3(); bs[s].p = zero; bs[s].w = zero; bs[s].v = zero;
    r[s] = zero; hW[s] = zero; fin[s] = zero; nin[s] = zero; fext[s] = zero; next[s] = zero;
    if (s < nch) {
      const int b = M.chain[path * IDTO_MAX_CHAIN + s];
      const int kind = M.pkind[path * IDTO_MAX_CHAIN + s];
      M3 Rp = ident3();
      V3 pp = zero, wp = zero, vp = zero, alp = zero, ap = zero;
      if (kind == PK_COMMON) { Rp = cb.R; pp = cb.p; wp = cb.w; vp = cb.v; alp = cb_al; ap = cb_a; }
      if (s > 0 && kind == PK_PREV) {
        Rp = bs[s > 0 ? s - 1 : 0].R; pp = bs[s > 0 ? s - 1 : 0].p; wp = bs[s > 0 ? s - 1 : 0].w;
        vp = bs[s > 0 ? s - 1 : 0].v; alp = al_prev; ap = a_prev;
      }
      const M3 R_WF = Rp * ldm3(M.X_PF + 12 * b);
      const V3 d1 = Rp * ldv3(M.X_PF + 12 * b + 9);
      const JointOut j = joint_kin(M.jtype[b], R_WF, ldv3(M.axis + 3 * b), q + M.qstart[b], v + M.vstart[b],
                                   a + M.vstart[b]);
      hW[s] = j.hW;
      bs[s].R = R_WF * j.R_FM;
      r[s] = d1 + j.d2;
      bs[s].p = pp + r[s];
      bs[s].w = wp + j.w_rel;
      bs[s].v = (vp + cross(wp, r[s])) + j.v_rel;
      const V3 al = (alp + j.al_rel) + cross(wp, j.w_rel);
      const V3 acc = (((ap + cross(alp, r[s])) + cross(wp, cross(wp, r[s]))) + cross(wp, j.v_rel) * 2.0) + j.a_rel;
      inertial_wrench(M, b, bs[s].R, bs[s].w, al, acc, body_gravity(slot_gravity(M.gslots, path, s), g), &fin[s], &nin[s]);
      al_prev = al;
      a_prev = acc;
      if constexpr (XCH) {
        const int x = M.xrec[path * IDTO_MAX_CHAIN + s];
        if (full && x >= 0) {
          put_state(xs + XREC * x, bs[s]);
#pragma unroll
          for (int i = 0; i < 6; ++i) xs[XREC * x + XEXT + i] = 0.0;
        }
      }
    }
  }
  if constexpr (XCH) wave_exchange_point();

  // ---- contact pairs of this path (TO.cc:247-386)
  V3 cfe = zero, cne = zero;  // this path's partial contact wrench on the common body
  if (full) {
    const int np = M.path_npairs[path];
    for (int k = 0; k < np; ++k) {
      const int pi = M.path_pairs[path * M.maxpp + k];
      int sa = M.pair_sa[pi], sb = M.pair_sb[pi];
      BodyState A, B;
      A.R = ident3(); A.p = zero; A.w = zero; A.v = zero;
      B = A;
      if (sa == -1) A = cb;
      if (sb == -1) B = cb;
      if constexpr (XCH) {
        // chain bodies from the exchange area; a body of another path (a shared pair) gets no force from this lane
        const int xa = M.pair_xa[pi], xb = M.pair_xb[pi];
        // (a stem body, code <= -4: this lane is the one that evaluates its pairs, the sum in its record is this lane's)
        if (xa >= 0) {
          A = get_state(xs + XREC * xa);
          if (STEM && sa <= -4) sa = 0;
          else if (M.xrec[path * IDTO_MAX_CHAIN + sa] != xa) sa = -3;
        }
        if (xb >= 0) {
          B = get_state(xs + XREC * xb);
          if (STEM && sb <= -4) sb = 0;
          else if (M.xrec[path * IDTO_MAX_CHAIN + sb] != xb) sb = -3;
        }
      } else {
#pragma unroll
        for (int s = 0; s < MAXC; ++s) {
          if (sa == s) A = bs[s];
          if (sb == s) B = bs[s];
        }
      }
      const PairForce pf = contact_pair(M, cp, M.pair_ga[pi], M.pair_gb[pi], A, B);
      if (pf.active) {
        if (sa == -1) { cfe = cfe + pf.fA; cne = cne + pf.nA; }
        if (sb == -1) { cfe = cfe + pf.fB; cne = cne + pf.nB; }
        if constexpr (XCH) {   // (sa / sb >= 0: a body of this lane, its record is xa / xb)
          auto add = [&](int x, V3 f, V3 n) {
            double* e = xs + XREC * x + XEXT;
            const V3 fe = mk(e[0], e[1], e[2]) + f, ne = mk(e[3], e[4], e[5]) + n;
            e[0] = fe.x; e[1] = fe.y; e[2] = fe.z; e[3] = ne.x; e[4] = ne.y; e[5] = ne.z;
          };
          if (sa >= 0) add(M.pair_xa[pi], pf.fA, pf.nA);
          if (sb >= 0) add(M.pair_xb[pi], pf.fB, pf.nB);
        } else {
#pragma unroll
          for (int s = 0; s < MAXC; ++s) {
            if (sa == s) { fext[s] = fext[s] + pf.fA; next[s] = next[s] + pf.nA; }
            if (sb == s) { fext[s] = fext[s] + pf.fB; next[s] = next[s] + pf.nB; }
          }
        }
      }
    }
  }

  // ---- backward pass along the chain, joint torques
  V3 child_f = zero, child_n = zero;   // contribution of slot s+1 to slot s
  V3 root_f = zero, root_n = zero;     // contribution of the chain root to the common body
#pragma unroll
  for (int s = MAXC - 1; s >= 0; --s) {
    if (s < nch) {
      const int b = M.chain[path * IDTO_MAX_CHAIN + s];
      if constexpr (XCH) {
        const int x = M.xrec[path * IDTO_MAX_CHAIN + s];
        if (full && x >= 0) {
          const double* e = xs + XREC * x + XEXT;
          fext[s] = mk(e[0], e[1], e[2]);
          next[s] = mk(e[3], e[4], e[5]);
        }
      }
      V3 f = fin[s] - fext[s];
      V3 n = nin[s] - next[s];
      // slot s+1 hangs off slot s ?
      if (s + 1 < MAXC) {
        const bool has_child = (s + 1 < nch) && (M.pkind[path * IDTO_MAX_CHAIN + (s + 1 < MAXC ? s + 1 : s)] == PK_PREV);
        if (has_child) { f = f + child_f; n = n + child_n; }
      }
      project_tau(M.jtype[b], M.vstart[b], M.X_PF + 12 * b, hW[s], f, n, full, M.damping, v, tau);
      const int kind = M.pkind[path * IDTO_MAX_CHAIN + s];
      const V3 cf = f, cn = n + cross(r[s], f);
      if (kind == PK_PREV) { child_f = cf; child_n = cn; }
      else if (kind == PK_COMMON) { root_f = cf; root_n = cn; }
    }
  }

  // ---- common body: butterfly sums over the lanes of this evaluation
  if (cbody >= 0) {   // uniform over the launch
    const V3 ext_f = tree_sum(cfe, M.npaths);
    const V3 ext_n = tree_sum(cne, M.npaths);
    const V3 ch_f = tree_sum(root_f, M.npaths);
    const V3 ch_n = tree_sum(root_n, M.npaths);
    V3 f = (cb_fin - ext_f) + ch_f;
    V3 n = (cb_nin - ext_n) + ch_n;
    if (path == 0) project_tau(M.jtype[cbody], M.vstart[cbody], M.X_PF + 12 * cbody, cb_hW, f, n, full, M.damping, v, tau);
    if constexpr (STEM) {
      wave_exchange_point();   // (the contact sums of the stem's records are another lane's stores)
      if (path == 0) {
        const double* aux = xs + XREC * M.nxb;
        for (int k = M.nstem - 2; k >= 0; --k) {
          const double* ak = aux + SAUX * k;
          const int b = M.stem[k], x = M.stem[IDTO_MAX_STEM + k];
          V3 ef = zero, en = zero;
          if (full && x >= 0) { ef = get_v3(xs + XREC * x + XEXT); en = get_v3(xs + XREC * x + XEXT + 3); }
          const V3 child_f = f, child_n = n + cross(get_v3(ak + SA_RC), f);
          f = (get_v3(ak + SA_FIN) - ef) + child_f;
          n = (get_v3(ak + SA_NIN) - en) + child_n;
          project_tau(M.jtype[b], M.vstart[b], M.X_PF + 12 * b, get_v3(ak + SA_HW), f, n, full, M.damping, v, tau);
        }
      }
    }
  }
}

}  // namespace idto_dev
