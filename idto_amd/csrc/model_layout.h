// model_layout.h — what the host's table builder (host/model_tables.cc) and the kernels agree on: the codes in the model
// tables, the layout of id_fast.h's gathered records, and the instantiated tree shapes.  Constants only: no device code.
#pragma once

#include <cstddef>

#include "idto_model.h"

// DevModel's table pointers, by member name: what the host's packer places in the blob and what a kernel shifts when it
// moves the model to another copy of the blob (id_eval.h shift_model)
#define IDTO_MODEL_DOUBLE_TABLES(X) \
  X(X_PF) X(axis) X(mass) X(com) X(inertia) X(damping) X(geom_X) X(geom_size) X(nplus_const) X(f_body) X(f_cbody) X(f_pairs)
#define IDTO_MODEL_INT_TABLES(X)                                                                                      \
  X(parent) X(jtype) X(qstart) X(vstart) X(geom_type) X(chain) X(nchain) X(pkind) X(path_npairs) X(path_pairs) X(pair_ga) \
  X(pair_gb) X(pair_sa) X(pair_sb) X(colinfo) X(rowinfo) X(f_seg) X(xrec) X(pair_xa) X(pair_xb) X(stem)

namespace idto_dev {

// The parameter record of one problem of a batch with per-problem models (idto_hip_set_model_batch): the model's blob,
// then - on the next 64-byte boundary - DevContact's six doubles and the three of gravity (host/model_batch.cc forms the
// record up to here), then - 128 bytes on - the problem's DevModel as the kernels read it: the context's, its table
// pointers moved to THIS record's blob and its gravity the problem's (idto_hip.hip writes it: it knows the device
// address).  The record ends on a 64-byte boundary.  In doubles, for a blob of blob_n of them:
constexpr int MREC_CONTACT = 6, MREC_GRAVITY = 3, MREC_PARAMS = 16, MREC_DEVMODEL = 64;
constexpr size_t model_record_contact_at(size_t blob_n) { return (blob_n + 7) & ~(size_t)7; }
constexpr size_t model_record_gravity_at(size_t blob_n) { return model_record_contact_at(blob_n) + MREC_CONTACT; }
constexpr size_t model_record_devmodel_at(size_t blob_n) { return model_record_contact_at(blob_n) + MREC_PARAMS; }
constexpr size_t model_record_doubles(size_t blob_n) { return model_record_devmodel_at(blob_n) + MREC_DEVMODEL; }

// DevModel::pkind: what a chain slot's body hangs off
enum { PK_WORLD = 0, PK_COMMON = 1, PK_PREV = 2 };

// id_fast.h's record of one body (doubles); FB_IDX holds {qstart, vstart} as two ints
enum { FB_XPF = 0, FB_AXIS = 12, FB_MASS = 15, FB_COM = 16, FB_INERTIA = 19, FB_DAMP = 25, FB_IDX = 31, FB_STRIDE = 34 };
// record of one contact pair; FP_INFO holds {type on C, type on the other body, C is the pair's A, the other body is
// the common one} as four ints.
// XC, SC: geometry frame and size on C (the chain slot of the pair's group; the common body for a pair without a
// chain body); XO, SO: on the other body - for the world [I R | 0 + I p], formed on the host
enum { FP_INFO = 0, FP_XC = 2, FP_SC = 14, FP_XO = 17, FP_SO = 29, FP_STRIDE = 34 };

// The instantiated tree shapes of id_fast.h (DevModel::fast_shape = 1 + the row; 0 = any model: id_eval<MAXC>).  A model
// has a shape when every path has MAXC bodies, there are NP paths, the common body's joint is CJ (-1: no common body),
// slot 0 of every path has joint J0 and parent kind K0, and the later slots are revolute on the previous one - but for
// slot W2 (-1: none) of a single path, which hangs off the world again.  On top of the tuple:
//   - GS: bodies whose weight is switched off are allowed; a shape without it is chosen only when every body has gravity
//   - a capsule or a cylinder clears the shape (id_fast.h's pair code has neither reduction)
//   - shared pairs or a stem below the common body clear it (the pair records are per path; no shape has a stem)
// KC: the chain bound fd_kernel<KC, shape> is instantiated with (fd_launch.hip).
struct TreeShape { int MAXC, NP, CJ, J0, K0, W2, GS, KC; };
constexpr TreeShape kTreeShapes[] = {
    {2, 1, -1, IDTO_JOINT_REVOLUTE, PK_WORLD, -1, 0, 2},                     // 1 acrobot
    {3, 1, -1, IDTO_JOINT_PLANAR, PK_WORLD, -1, 0, 3},                       // 2 hopper
    {3, 4, IDTO_JOINT_FLOATING, IDTO_JOINT_REVOLUTE, PK_COMMON, -1, 0, 3},   // 3 mini_cheetah
    {4, 4, IDTO_JOINT_FLOATING, IDTO_JOINT_REVOLUTE, PK_WORLD, -1, 0, 4},    // 4 allegro_hand + ball
    {3, 1, -1, IDTO_JOINT_REVOLUTE, PK_WORLD, 2, 0, 3},                      // 5 spinner: two-link finger + the spinner, off the world
    {7, 1, IDTO_JOINT_FLOATING, IDTO_JOINT_REVOLUTE, PK_WORLD, -1, 1, 8},    // 6 a free object + an arm of seven revolute bodies off the world (jaco, jaco_ball)
};
constexpr int kNumTreeShapes = sizeof(kTreeShapes) / sizeof(kTreeShapes[0]);
// Not tree shapes: SHAPE_XCH selects the generic evaluation with the exchange area of shared pairs (id_eval<MAXC, true>,
// models with DevModel::nxb > 0; DevModel::fast_shape stays 0 for them)
constexpr int SHAPE_XCH = kNumTreeShapes + 1;
// ... and SHAPE_STEM the one that also walks a stem below the common body (id_eval<MAXC, true, true>, DevModel::nstem > 1): its
// exchange area has the stem's blocks behind the records (id_eval.h xch_eval_doubles)
constexpr int SHAPE_STEM = kNumTreeShapes + 2;
// (both serve any chain length: KC = 8)
constexpr TreeShape tree_shape(int shape) {
  return shape >= 1 && shape <= kNumTreeShapes ? kTreeShapes[shape - 1] : TreeShape{0, 1, -1, 0, 0, -1, 0, 8};
}
// fd_kernel's forward-difference lane map without the redundant path lanes (id_fast.h id_eval_fast<..., DD>):
// a column of q, or a mass column, that belongs to a joint of ONE chain leaves the common body and the other chains what
// they are in the baseline evaluation, so that evaluation runs on one lane - its own path's - and the lanes this frees
// evaluate contact pairs for the others.  The trait of the shapes whose kernel has that path (the host still refuses it
// per model, host/model_tables.cc BuildFdDedup), and the lane budget: main lanes in the block's first half, one helper
// lane behind each in the second.
constexpr bool tree_shape_dedup(int shape) { return shape == 3; }
constexpr int kFdMainLanes = 128, kFdHelperLanes = 128;
// The lane words, in the blob right behind DevModel::f_seg's NP * (MAXC + 2) segment words (nothing there where the host
// refused the map): [kFdMainLanes] main words, then [kFdHelperLanes] helper words
//   main word:   evaluation | path << 8 | flags
enum {
  FDL_WHOLE = 1 << 12,      // four lanes, one per path, meet in the butterfly sums as they always did
  FDL_FULL = 1 << 13,       // gravity, damping and contact (not a mass column)
  FDL_VALID = 1 << 14,      // (a lane without a task runs the baseline into the dump row)
  FDL_BODY_OWN = 1 << 15,   // the lane that adds the common body's own pair, evaluated by its helper
  FDL_BODY_BASE = 1 << 16   // a single-path lane that adds it from the baseline's helper (the common body is the baseline's)
};
//   helper word: FDH_* | main lane << 8 | the chain pair's record (path * f_maxpp + place) << 16 | the common body's pair's << 24
enum { FDH_FOOT = 1, FDH_BODY = 2 };

// Shapes 1 ... kNumSizedShapes - the five example configurations - have the constants compiled into fd_kernel's tail.  The Jaco
// shape (6) takes the g rows but keeps the run-time loops: no benchmark configuration has it, and the constants were never
// measured on it.
constexpr int kNumSizedShapes = 5;
// nq and nv of a model of a tree shape (0: not a tree shape): the common body's joint, then NP chains of slot 0's joint and
// MAXC - 1 revolute ones.  The host gives a model the shape only if its nq and nv are these (model_tables.cc), so the tail of
// fd_kernel<KC, shape> takes its sizes from here at compile time.
constexpr int joint_nq(int jt) { return jt == IDTO_JOINT_FLOATING ? 7 : (jt == IDTO_JOINT_PLANAR ? 3 : (jt < 0 ? 0 : 1)); }
constexpr int joint_nv(int jt) { return jt == IDTO_JOINT_FLOATING ? 6 : (jt == IDTO_JOINT_PLANAR ? 3 : (jt < 0 ? 0 : 1)); }
constexpr int tree_shape_nq(int shape) {
  return shape >= 1 && shape <= kNumTreeShapes
             ? joint_nq(kTreeShapes[shape - 1].CJ) + kTreeShapes[shape - 1].NP * (joint_nq(kTreeShapes[shape - 1].J0) + kTreeShapes[shape - 1].MAXC - 1)
             : 0;
}
constexpr int tree_shape_nv(int shape) {
  return shape >= 1 && shape <= kNumTreeShapes
             ? joint_nv(kTreeShapes[shape - 1].CJ) + kTreeShapes[shape - 1].NP * (joint_nv(kTreeShapes[shape - 1].J0) + kTreeShapes[shape - 1].MAXC - 1)
             : 0;
}
// (a wrong size here would not fail loudly: the host would refuse the shape and the generic kernel would run)
static_assert(tree_shape_nq(1) == 2 && tree_shape_nv(1) == 2, "acrobot");
static_assert(tree_shape_nq(2) == 5 && tree_shape_nv(2) == 5, "hopper");
static_assert(tree_shape_nq(3) == 19 && tree_shape_nv(3) == 18, "mini_cheetah");
static_assert(tree_shape_nq(4) == 23 && tree_shape_nv(4) == 22, "allegro_hand");
static_assert(tree_shape_nq(5) == 3 && tree_shape_nv(5) == 3, "spinner");
static_assert(tree_shape_nq(6) == 14 && tree_shape_nv(6) == 13, "jaco, jaco_ball");

}  // namespace idto_dev
