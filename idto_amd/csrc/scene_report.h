// scene_report.h — the scene report (include/idto_hip.h idto_hip_scene_report): for every state [q, v] of a trajectory the
// pose and spatial velocity of every body, the signed distance, witness points, relative velocity and compliant force of
// every candidate contact pair, and the generalised force of contact, per pair and summed.  What the reference reads from
// the plant's context behind EvalPlantContext (optimizer/trajectory_optimizer.h) - body poses, spatial velocities,
// signed-distance pairs, contact results - in one launch.
//
// Grid (nstates, batch): one workgroup per state, blockIdx.y the problem.  No workgroup talks to another and there is no
// wait of any kind.  The workgroup stages the problem's model blob and the state's q, v into LDS, then:
//   bodies  a lane per body walks parent[] from the world down to its body (at most IDTO_MAX_STEM + IDTO_MAX_CHAIN joints,
//           the ancestors recomputed in registers: no lane waits for another) with the expressions of id_eval's forward
//           pass, the acceleration terms dropped, and leaves (R, p, w, v, hW) in LDS - put_state's 18 doubles, then the
//           joint axis in the world.  The walk is blind to the star decomposition.
//   pairs   (behind a barrier) a lane per candidate pair, in rounds of the block: scene_pair - contact_pair restated with its
//           intermediate values handed out - on the two bodies' records (the world: identity and zeros), the pair's record
//           to global memory, and for an active pair its row of generalised force into LDS: body B's ancestors take
//           project_tau of (f, cross(pC - p_body, f)), body A's the same of -f, added into a row that starts as +0.
//   dofs    (behind a barrier) a lane per DoF sums the rows in ascending pair index from +0.
// LDS strides: a body's record is SREC = 21 doubles and a row nv | 1, both odd, so that the lanes of a 32-lane group, each
// at the same offset of its own record, fall on 32 different bank pairs of the 64-bit LDS accesses.
#pragma once

#include <hip/hip_runtime.h>

#include "id_eval.h"
#include "idto_hip.h"

namespace idto_dev {

// (a body's record in LDS - SREC, SR_HW -, scene_row_stride, scene_lds_doubles and scene_block: plant_sizes.h)
constexpr int SCENE_BODY = IDTO_SCENE_BODY_DOUBLES, SCENE_PAIR = IDTO_SCENE_PAIR_DOUBLES;

struct SceneArgs {
  // where problem b's DevModel and DevContact come from: its parameter record (records != null: model_layout.h
  // model_record_*, mstride bytes apart, as plant_kernel reads them) or the context's one model below
  const double* records; size_t mstride, rec_contact, rec_model;
  DevModel M; DevContact cp;
  const int* geom_body;     // [ngeoms] the body of every geometry, -1 the world (DevModel names only decomposition slots)
  const double* x;          // [batch][nstates][nq + nv]
  int nstates;
  // each may be null
  double* bodies;           // [batch][nstates][nb][SCENE_BODY]
  double* pairs;            // [batch][nstates][npairs][SCENE_PAIR]
  double* tau_contact;      // [batch][nstates][nv]
  double* tau_pairs;        // [batch][nstates][npairs][nv]
};

struct ScenePair {
  bool active;
  double phi, vn, fn;
  V3 n, Ca, Cb, vt, f, pC;   // f: on body B at pC, world frame
};

// contact_pair (id_eval.h; reference TO.cc:281-385) with the same expressions in the same order, handing out what it
// keeps to itself.  A pair beyond the threshold keeps its geometry and velocities; its fn and f are zero.
IDTO_DEV ScenePair scene_pair(const DevModel& M, const DevContact& cp, int ga, int gb, const BodyState& A, const BodyState& B) {
  ScenePair out;
  const V3 zero = mk(0, 0, 0);
  const M3 RgA = A.R * ldm3(M.geom_X + 12 * ga);
  const V3 pgA = A.p + A.R * ldv3(M.geom_X + 12 * ga + 9);
  const M3 RgB = B.R * ldm3(M.geom_X + 12 * gb);
  const V3 pgB = B.p + B.R * ldv3(M.geom_X + 12 * gb + 9);
  const SdResult sd = signed_distance(M.geom_type[ga], RgA, pgA, ldv3(M.geom_size + 3 * ga), M.geom_type[gb], RgB,
                                      pgB, ldv3(M.geom_size + 3 * gb));
  out.active = sd.valid && !(sd.phi > cp.threshold);
  out.phi = sd.phi; out.n = sd.n; out.Ca = sd.Ca; out.Cb = sd.Cb;
  const V3 nhat = sd.n;
  const V3 pC = (sd.Ca + sd.Cb) * 0.5;
  const V3 pAC = pC - A.p, pBC = pC - B.p;
  const V3 vAc = A.v + cross(A.w, pAC);
  const V3 vBc = B.v + cross(B.w, pBC);
  const V3 vrel = vBc - vAc;
  const double vn = dot(nhat, vrel);
  const V3 vt = vrel - nhat * vn;
  out.pC = pC; out.vn = vn; out.vt = vt;
  out.fn = 0.0; out.f = zero;
  if (!out.active) return out;
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
  out.fn = fn;
  out.f = nhat * fn + ft;
  return out;
}

// The state of `body` and its joint's axis in the world: the joints from the world down to it, one after the other.  The
// k-th ancestor is found by walking parent[] k times (no list of ancestors is kept: an array indexed at run time would
// live in scratch).
IDTO_DEV BodyState scene_body_state(const DevModel& M, int body, const double* q, const double* v, V3* hW) {
  const V3 zero = mk(0, 0, 0);
  BodyState cur;
  cur.R = ident3(); cur.p = zero; cur.w = zero; cur.v = zero;
  *hW = zero;
  int depth = 0;
  for (int b = body; b >= 0 && depth < M.nb; b = M.parent[b]) ++depth;
  for (int k = depth - 1; k >= 0; --k) {
    int b = body;
    for (int i = 0; i < k; ++i) b = M.parent[b];
    const M3 R_WF = cur.R * ldm3(M.X_PF + 12 * b);
    const V3 d1 = cur.R * ldv3(M.X_PF + 12 * b + 9);
    // (the accelerations' slot: the velocities again - what joint_kin forms of them is not used)
    const JointOut j = joint_kin(M.jtype[b], R_WF, ldv3(M.axis + 3 * b), q + M.qstart[b], v + M.vstart[b], v + M.vstart[b]);
    const V3 r = d1 + j.d2;
    const V3 vk = (cur.v + cross(cur.w, r)) + j.v_rel;
    cur.R = R_WF * j.R_FM;
    cur.p = cur.p + r;
    cur.w = cur.w + j.w_rel;
    cur.v = vk;
    *hW = j.hW;
  }
  return cur;
}

// The force f at pC on `body`, projected on the joints from the body to the world and added into `row`
IDTO_DEV void scene_project(const DevModel& M, const double* recs, int body, V3 pC, V3 f, double* row) {
  int steps = 0;
  for (int b = body; b >= 0 && steps < M.nb; b = M.parent[b], ++steps) {
    const double* rec = recs + SREC * b;
    const V3 n = cross(pC - get_v3(rec + 9), f);
    const int jt = M.jtype[b], vs = M.vstart[b];
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    project_tau(jt, 0, M.X_PF + 12 * b, get_v3(rec + SR_HW), f, n, false, nullptr, nullptr, t);
    const int nvj = jt == IDTO_JOINT_FLOATING ? 6 : (jt == IDTO_JOINT_PLANAR ? 3 : 1);
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (i < nvj) row[vs + i] = row[vs + i] + t[i];
  }
}

// One state of one problem: state index s, problem b (the kernel passes blockIdx.x, blockIdx.y)
IDTO_DEV void scene_block_body(const DevModel& M, const DevContact& cp, const SceneArgs& A, const int s, const int b) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nb = M.nb, nq = M.nq, nv = M.nv, np = M.npairs, rs = scene_row_stride(nv);
  double* mblob = lds;              // [M.blob_n] the model tables
  double* q = mblob + M.blob_n;     // [nq]
  double* v = q + nq;               // [nv]
  double* recs = v + nv;            // [nb][SREC]
  double* rows = recs + nb * SREC;  // [np][rs]
  const size_t st = (size_t)b * A.nstates + s;
  const double* x = A.x + st * (nq + nv);
  for (int i = tid; i < M.blob_n; i += nt) mblob[i] = M.blob[i];
  for (int i = tid; i < nq + nv; i += nt) q[i] = x[i];
  __syncthreads();
  const DevModel Ml = rebase_model(M, mblob);

  // ---- bodies
  for (int body = tid; body < nb; body += nt) {
    V3 hW;
    const BodyState bs = scene_body_state(Ml, body, q, v, &hW);
    put_state(recs + SREC * body, bs);
    put_v3(recs + SREC * body + SR_HW, hW);
  }
  __syncthreads();
  if (A.bodies) {
    double* out = A.bodies + st * nb * SCENE_BODY;
    for (int i = tid; i < nb * SCENE_BODY; i += nt) out[i] = recs[SREC * (i / SCENE_BODY) + i % SCENE_BODY];
  }

  // ---- pairs
  const V3 zero = mk(0, 0, 0);
  for (int pi = tid; pi < np; pi += nt) {
    const int ga = Ml.pair_ga[pi], gb = Ml.pair_gb[pi];
    const int ba = A.geom_body[ga], bb = A.geom_body[gb];
    BodyState SA, SB;
    SA.R = ident3(); SA.p = zero; SA.w = zero; SA.v = zero;
    SB = SA;
    if (ba >= 0) SA = get_state(recs + SREC * ba);
    if (bb >= 0) SB = get_state(recs + SREC * bb);
    const ScenePair sp = scene_pair(Ml, cp, ga, gb, SA, SB);
    if (A.pairs) {
      double* o = A.pairs + (st * np + pi) * SCENE_PAIR;
      o[IDTO_SCENE_PAIR_ACTIVE] = sp.active ? 1.0 : 0.0;
      o[IDTO_SCENE_PAIR_PHI] = sp.phi;
      put_v3(o + IDTO_SCENE_PAIR_N, sp.n);
      put_v3(o + IDTO_SCENE_PAIR_CA, sp.Ca);
      put_v3(o + IDTO_SCENE_PAIR_CB, sp.Cb);
      o[IDTO_SCENE_PAIR_VN] = sp.vn;
      put_v3(o + IDTO_SCENE_PAIR_VT, sp.vt);
      o[IDTO_SCENE_PAIR_FN] = sp.fn;
      put_v3(o + IDTO_SCENE_PAIR_F, sp.f);
      o[IDTO_SCENE_PAIR_PAD] = 0.0;
    }
    double* row = rows + pi * rs;
    for (int j = 0; j < nv; ++j) row[j] = 0.0;
    if (sp.active) {
      scene_project(Ml, recs, bb, sp.pC, sp.f, row);
      scene_project(Ml, recs, ba, sp.pC, -sp.f, row);
    }
    if (A.tau_pairs) {
      double* o = A.tau_pairs + (st * np + pi) * nv;
      for (int j = 0; j < nv; ++j) o[j] = row[j];
    }
  }
  __syncthreads();

  // ---- the generalised contact force of the state
  if (A.tau_contact)
    for (int j = tid; j < nv; j += nt) {
      double sum = 0.0;
      for (int pi = 0; pi < np; ++pi) sum = sum + rows[pi * rs + j];
      A.tau_contact[st * nv + j] = sum;
    }
}

template <bool RECORDS>
__global__ void __launch_bounds__(256) scene_kernel(SceneArgs A) {
  if constexpr (RECORDS) {
    const RecordPtr rec = record_at(A.records, (size_t)blockIdx.y * A.mstride);
    scene_block_body(*(const DevModel*)(rec + A.rec_model), *(const DevContact*)(rec + A.rec_contact), A, (int)blockIdx.x, (int)blockIdx.y);
  } else {
    scene_block_body(A.M, A.cp, A, (int)blockIdx.x, (int)blockIdx.y);
  }
}

}  // namespace idto_dev
