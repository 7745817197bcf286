// model_tables.cc — see model_tables.h.  One function per job, in the order BuildModelTables calls them; every refusal is
// made here, on host tables only, so a refused model fails the same way with or without a GPU.
// Build with -ffp-contract=off and without fast-math: the gathered records use explicit std::fma and a deliberate 0.0 + x.
#include "model_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "model_layout.h"

namespace idto_host {
namespace {
using namespace idto_dev;

int Refuse(std::string* err, const char* why) {
  *err = why;
  return -1;
}

bool IdentityRotation(const double* X) {
  bool ident = true;
  for (int e = 0; e < 9; ++e) ident &= (X[e] == ((e % 4 == 0) ? 1.0 : 0.0));
  return ident;
}

// ---- 1. the geometry types and the pairs a capsule or a cylinder may take part in (include/idto_model.h).  The one place that checks
// a pair's geometry indices: every later step reads geom_*[pair_a[i]] without asking.
int CheckGeometry(const idto_model_t* m, std::string* err) {
  for (int g = 0; g < m->ngeoms; ++g) {
    const int t = m->geom_type[g];
    if (t != IDTO_GEOM_SPHERE && t != IDTO_GEOM_BOX && t != IDTO_GEOM_CAPSULE && t != IDTO_GEOM_CYLINDER)
      return Refuse(err, "unknown geometry type (0 sphere, 1 box, 2 capsule, 4 cylinder)");
    const double* s = m->geom_size + (size_t)3 * g;
    if (t == IDTO_GEOM_CAPSULE &&
        !(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]) && s[0] > 0 && s[1] >= 0))
      return Refuse(err, "capsule size must be finite with radius > 0 and h >= 0");
    if (t == IDTO_GEOM_CYLINDER &&
        !(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]) && s[0] > 0 && s[1] > 0))
      return Refuse(err, "cylinder size must be finite with radius > 0 and H > 0");
  }
  for (int i = 0; i < m->npairs; ++i) {
    const int ga = m->pair_a[i], gb = m->pair_b[i];
    if (ga < 0 || ga >= m->ngeoms || gb < 0 || gb >= m->ngeoms) return Refuse(err, "pair geometry index out of range");
    const int ta = m->geom_type[ga], tb = m->geom_type[gb];
    if ((ta == IDTO_GEOM_CAPSULE && tb == IDTO_GEOM_BOX) || (ta == IDTO_GEOM_BOX && tb == IDTO_GEOM_CAPSULE)) {
      const int box = (ta == IDTO_GEOM_BOX) ? ga : gb;
      if (m->geom_body[box] >= 0 || !IdentityRotation(m->geom_X + (size_t)12 * box))
        return Refuse(err, "capsule-box contact pairs need a world-fixed box with identity rotation");
    }
    if ((ta == IDTO_GEOM_CYLINDER && tb != IDTO_GEOM_SPHERE) || (tb == IDTO_GEOM_CYLINDER && ta != IDTO_GEOM_SPHERE))
      return Refuse(err, "cylinder contact pairs need a sphere on the other side");
  }
  return 0;
}

// ---- 2. the stem (include/idto_model.h): the common body and its ancestors.  A body below the common one carries
// nothing but the next stem body and has no path of its own; all its pairs are in ONE path's list, so that one lane forms
// its contact sum in index order, and its partner in a pair is the world or a chain body.
struct Stem {
  std::vector<int> bodies;      // world side first, the common body last (empty: no common body)
  std::vector<int> idx;         // [nbodies] a body's place in `bodies`, -1 for every other body
  std::vector<int> pair_path;   // [n] the path that evaluates the pairs of stem body k < n - 1, -1: no pair touches it
  int n() const { return (int)bodies.size(); }
  bool has(int b) const { return b >= 0 && idx[b] >= 0; }
  bool below_common(int b) const { return has(b) && idx[b] < n() - 1; }
};
int FindStem(const idto_model_t* m, Stem* s, std::string* err) {
  const int nb = m->nbodies;
  if (m->common_body >= nb) return Refuse(err, "common body out of range");
  for (int b = m->common_body; b >= 0; b = m->parent[b]) {
    if (m->parent[b] >= b) return Refuse(err, "bodies must be numbered so that parent[i] < i");
    if (s->n() == IDTO_MAX_STEM)
      return Refuse(err, "the stem (the common body and its ancestors) is longer than IDTO_MAX_STEM bodies");
    s->bodies.push_back(b);
  }
  std::reverse(s->bodies.begin(), s->bodies.end());
  s->idx.assign(nb, -1);
  for (int k = 0; k < s->n(); ++k) s->idx[s->bodies[k]] = k;
  s->pair_path.assign(s->n(), -1);
  for (int k = s->n() - 2; k >= 0; --k) {   // (from the common body towards the world)
    int children = 0;
    for (int i = 0; i < nb; ++i) children += m->parent[i] == s->bodies[k];
    if (children != 1)
      return Refuse(err, "a stem body below the common body has a second child (chains hang off the common body or the world)");
    if (m->body_path[s->bodies[k]] != -1) return Refuse(err, "a stem body must have body_path -1");
  }
  for (int i = 0; i < m->npairs; ++i) {
    const int ba = m->geom_body[m->pair_a[i]], bb = m->geom_body[m->pair_b[i]];
    if (ba >= nb || bb >= nb) return Refuse(err, "geometry body out of range");
    if (s->n() > 1 && s->has(ba) && s->has(bb)) return Refuse(err, "contact pair between two stem bodies (the common body included)");
    for (int b : {ba, bb})
      if (s->below_common(b)) {
        int& path = s->pair_path[s->idx[b]];
        if (path >= 0 && path != m->pair_path[i]) return Refuse(err, "the pairs of one stem body name different paths (pair_path)");
        path = m->pair_path[i];
      }
  }
  return 0;
}

// ---- 3. star decomposition: the chain of every path, and the per-body gravity switch resolved onto its slots
struct Star {
  std::vector<int> chain, nchain, pkind;   // DevModel's tables
  std::vector<int> slot_of;                // [nbodies] chain slot; -1 the common body; -4 - k stem body k < n - 1 (id_eval.h)
  int maxc = 1;
  bool all_gravity = true;                 // gravity_enabled: 0 or 1 per body, NULL = every body
  unsigned long long gslots = 0;
  int gcommon = 1, gstem = 0;
  int at(int path, int slot) const { return path * IDTO_MAX_CHAIN + slot; }
};
int BuildStar(const idto_model_t* m, const Stem& stem, Star* s, std::string* err) {
  const int nb = m->nbodies, K = m->npaths;
  if (K < 1 || K > IDTO_MAX_PATHS || (K & (K - 1))) return Refuse(err, "npaths must be a power of two <= 8");
  for (int i = 0; i < nb; ++i)
    if ((m->jtype[i] == IDTO_JOINT_PLANAR || m->jtype[i] == IDTO_JOINT_FLOATING) && m->parent[i] >= 0)
      return Refuse(err, "planar and floating joints must be attached to the world");
  if (m->gravity_enabled)
    for (int i = 0; i < nb; ++i) {
      if (m->gravity_enabled[i] != 0 && m->gravity_enabled[i] != 1) return Refuse(err, "gravity_enabled entries must be 0 or 1");
      s->all_gravity = s->all_gravity && m->gravity_enabled[i] == 1;
    }
  s->chain.assign((size_t)K * IDTO_MAX_CHAIN, -1);
  s->nchain.assign(K, 0);
  s->pkind.assign((size_t)K * IDTO_MAX_CHAIN, 0);
  s->slot_of.assign(nb, -3);
  for (int i = 0; i < nb; ++i) {
    if (i == m->common_body) { s->slot_of[i] = -1; continue; }
    if (stem.has(i)) { s->slot_of[i] = -4 - stem.idx[i]; continue; }
    const int p = m->body_path[i];
    if (p < 0 || p >= K) return Refuse(err, "body without a valid path");
    const int slot = s->nchain[p]++;
    if (slot >= IDTO_MAX_CHAIN) return Refuse(err, "chain longer than IDTO_MAX_CHAIN");
    s->chain[s->at(p, slot)] = i;
    s->slot_of[i] = slot;
    const int par = m->parent[i];
    if (par < 0) s->pkind[s->at(p, slot)] = PK_WORLD;
    else if (par == m->common_body) s->pkind[s->at(p, slot)] = PK_COMMON;
    else if (slot > 0 && s->chain[s->at(p, slot - 1)] == par) s->pkind[s->at(p, slot)] = PK_PREV;
    else return Refuse(err, "model is not a star decomposition (body parent is neither world, common nor previous in path)");
  }
  for (int p = 0; p < K; ++p) s->maxc = std::max(s->maxc, s->nchain[p]);
  for (int i = 0; i < nb; ++i) {
    const bool on = !m->gravity_enabled || m->gravity_enabled[i] == 1;
    if (i == m->common_body) s->gcommon = on ? 1 : 0;
    else if (stem.has(i)) s->gstem |= (on ? 1 : 0) << stem.idx[i];
    else if (on) s->gslots |= 1ull << s->at(m->body_path[i], s->slot_of[i]);
  }
  return 0;
}

// ---- 4. per-path pair lists.  A pair stays inside one path (with the common body, a stem body or the world), or joins
// chain bodies of two paths: a shared pair, which both paths evaluate (pair_path must name one of the two) - it goes
// into both pair lists, in index order.
struct PairLists {
  std::vector<int> path_npairs, path_pairs, sa, sb;   // DevModel's tables (sa, sb: pair_sa, pair_sb)
  std::vector<int> other;                             // [npairs] the second path of a shared pair, -1 for every other pair
  int maxpp = 1;
  bool shared = false;
};
int BuildPairLists(const idto_model_t* m, const Stem& stem, const Star& star, PairLists* l, std::string* err) {
  const int K = m->npaths, np = m->npairs;
  auto body_a = [&](int i) { return m->geom_body[m->pair_a[i]]; };
  auto body_b = [&](int i) { return m->geom_body[m->pair_b[i]]; };
  auto on_chain = [&](int b) { return b >= 0 && !stem.has(b); };
  l->path_npairs.assign(K, 0);
  l->other.assign(np, -1);
  for (int i = 0; i < np; ++i) {
    const int p = m->pair_path[i], ba = body_a(i), bb = body_b(i);
    if (p < 0 || p >= K) return Refuse(err, "pair without a valid path");
    if (on_chain(ba) && on_chain(bb) && m->body_path[ba] != m->body_path[bb] && (m->body_path[ba] == p || m->body_path[bb] == p))
      l->other[i] = m->body_path[ba] == p ? m->body_path[bb] : m->body_path[ba];
    l->path_npairs[p]++;
    if (l->other[i] >= 0) { l->path_npairs[l->other[i]]++; l->shared = true; }
  }
  for (int p = 0; p < K; ++p) l->maxpp = std::max(l->maxpp, l->path_npairs[p]);
  l->path_pairs.assign((size_t)K * l->maxpp, 0);
  l->sa.resize(np);
  l->sb.resize(np);
  std::vector<int> fill(K, 0);
  for (int i = 0; i < np; ++i) {
    const int p = m->pair_path[i], ba = body_a(i), bb = body_b(i);
    l->path_pairs[(size_t)p * l->maxpp + fill[p]++] = i;
    if (l->other[i] >= 0) l->path_pairs[(size_t)l->other[i] * l->maxpp + fill[l->other[i]]++] = i;
    l->sa[i] = ba < 0 ? -2 : star.slot_of[ba];
    l->sb[i] = bb < 0 ? -2 : star.slot_of[bb];
    for (int b : {ba, bb})
      if (l->other[i] < 0 && on_chain(b) && m->body_path[b] != p) return Refuse(err, "pair touches a body outside its path");
    // box-box is implemented for ONE configuration only (id_eval.h signed_distance): A = a box on a
    // moving body, B = a world-fixed, axis-aligned box whose top face acts as the half-space
    // z <= top (the ground boxes of the reference's examples).  Anything else would silently get
    // wrong witness points, so it is refused here.
    if (m->geom_type[m->pair_a[i]] == IDTO_GEOM_BOX && m->geom_type[m->pair_b[i]] == IDTO_GEOM_BOX &&
        (ba < 0 || bb >= 0 || !IdentityRotation(m->geom_X + (size_t)12 * m->pair_b[i])))
      return Refuse(err, "box-box contact pairs must be (box on a moving body, world-fixed axis-aligned box), in this order");
  }
  return 0;
}

// ---- 5. the exchange records of id_eval<MAXC, true>, for a model with shared pairs or a stem: one per chain body that
// some pair touches, numbered path by path, slot by slot; behind them one for each stem body below the common one that a
// pair touches (stem_tab[IDTO_MAX_STEM + k]); and each pair's two records
struct Exchange {
  bool on = false;
  int nxb = 0;
  std::vector<int> xrec, pair_xa, pair_xb;   // DevModel's tables
  std::vector<int> stem_tab;                 // DevModel::stem
};
Exchange BuildExchange(const idto_model_t* m, const Stem& stem, const Star& star, const PairLists& l) {
  Exchange x;
  x.on = l.shared || stem.n() > 1;
  x.xrec.assign((size_t)m->npaths * IDTO_MAX_CHAIN, -1);
  x.pair_xa.assign(m->npairs, -1);
  x.pair_xb.assign(m->npairs, -1);
  x.stem_tab.assign(2 * IDTO_MAX_STEM, -1);
  for (int k = 0; k < stem.n(); ++k) x.stem_tab[k] = stem.bodies[k];
  if (!x.on) return x;
  for (int i = 0; i < m->npairs; ++i)
    for (int b : {m->geom_body[m->pair_a[i]], m->geom_body[m->pair_b[i]]})
      if (b >= 0 && !stem.has(b)) x.xrec[star.at(m->body_path[b], star.slot_of[b])] = 0;
  for (int& r : x.xrec)
    if (r == 0) r = x.nxb++;
  for (int k = 0; k + 1 < stem.n(); ++k)
    if (stem.pair_path[k] >= 0) x.stem_tab[IDTO_MAX_STEM + k] = x.nxb++;
  // a pair's side: a chain body's record, a stem body's (slot code -4 - k), or the code itself (-1 common, -2 world)
  auto record = [&](int body, int slot) {
    return slot >= 0 ? x.xrec[star.at(m->body_path[body], slot)] : (slot <= -4 ? x.stem_tab[IDTO_MAX_STEM - 4 - slot] : slot);
  };
  for (int i = 0; i < m->npairs; ++i) {
    x.pair_xa[i] = record(m->geom_body[m->pair_a[i]], l.sa[i]);
    x.pair_xb[i] = record(m->geom_body[m->pair_b[i]], l.sb[i]);
  }
  return x;
}

// ---- 6. N+ (TO.cc:1633-1647): its constant entries (NaN where a quaternion block goes), the non-zero range of every
// column and row (first | count << 16), and the floating joints (nfloat < 0: more than four)
struct NPlus {
  std::vector<double> constant;
  std::vector<int> colinfo, rowinfo;
  int nfloat = 0, float_qs[4] = {0, 0, 0, 0}, float_vs[4] = {0, 0, 0, 0};
};
NPlus BuildNPlus(const idto_model_t* m) {
  const int nq = m->nq, nv = m->nv;
  NPlus n;
  n.constant.assign((size_t)nv * nq, 0.0);
  n.colinfo.assign(nq, 0);
  n.rowinfo.assign(nv, 0);
  auto one = [&](int q, int v) { n.constant[(size_t)q * nv + v] = 1.0; n.colinfo[q] = v | 1 << 16; n.rowinfo[v] = q | 1 << 16; };
  for (int b = 0; b < m->nbodies; ++b) {
    const int qs = m->qstart[b], vs = m->vstart[b], jt = m->jtype[b];
    if (jt == IDTO_JOINT_REVOLUTE || jt == IDTO_JOINT_PRISMATIC) {
      one(qs, vs);
    } else if (jt == IDTO_JOINT_PLANAR) {
      for (int k = 0; k < 3; ++k) one(qs + k, vs + k);
    } else {
      for (int r = 0; r < 3; ++r)
        for (int cq = 0; cq < 4; ++cq) n.constant[(size_t)(qs + cq) * nv + vs + r] = std::numeric_limits<double>::quiet_NaN();
      for (int k = 0; k < 4; ++k) n.colinfo[qs + k] = vs | 3 << 16;
      for (int r = 0; r < 3; ++r) n.rowinfo[vs + r] = qs | 4 << 16;
      for (int k = 0; k < 3; ++k) one(qs + 4 + k, vs + 3 + k);
      if (n.nfloat >= 0 && n.nfloat < 4) { n.float_qs[n.nfloat] = qs; n.float_vs[n.nfloat] = vs; ++n.nfloat; }
      else n.nfloat = -1;
    }
  }
  return n;
}

// ---- 7. id_fast.h: does the model have one of the instantiated tree shapes (model_layout.h kTreeShapes)?
struct FastShapeOf {
  int shape = 0;
  int w2 = -1;   // a later slot of the (single) path that hangs off the world again (the spinner)
};
FastShapeOf RecogniseShape(const idto_model_t* m, const Stem& stem, const Star& star, bool shared, bool reduced_geoms) {
  const int K = m->npaths, cbody = m->common_body, cj = cbody >= 0 ? m->jtype[cbody] : -1;
  FastShapeOf f;
  bool ok = !(cbody >= 0 && cj != IDTO_JOINT_FLOATING) && !shared && stem.n() <= 1 && !reduced_geoms;
  for (int p = 0; p < K; ++p) ok = ok && star.nchain[p] == star.maxc;
  int j0 = -1, k0 = -1;
  for (int p = 0; p < K && ok; ++p)
    for (int s = 0; s < star.maxc; ++s) {
      const int jt = m->jtype[star.chain[star.at(p, s)]], kd = star.pkind[star.at(p, s)];
      if (s == 0) {
        if (p == 0) { j0 = jt; k0 = kd; }
        if (jt != j0 || kd != k0) ok = false;
      } else if (jt == IDTO_JOINT_REVOLUTE && kd == PK_WORLD && K == 1 && f.w2 < 0) {
        f.w2 = s;
      } else if (jt != IDTO_JOINT_REVOLUTE || kd != PK_PREV) {
        ok = false;
      }
    }
  for (int s = 1; s <= kNumTreeShapes && ok; ++s) {
    const TreeShape& t = kTreeShapes[s - 1];
    // (nq, nv: the shape's kernel has them as constants, model_layout.h tree_shape_nq / _nv)
    if (star.maxc == t.MAXC && K == t.NP && cj == t.CJ && j0 == t.J0 && k0 == t.K0 && f.w2 == t.W2 && (t.GS || star.all_gravity) &&
        m->nq == tree_shape_nq(s) && m->nv == tree_shape_nv(s))
      f.shape = s;
  }
  return f;
}

// ---- 8. the order id_eval_fast walks a path's pairs in: [pairs without a chain body that come first | slot 0 | ... |
// slot maxc-1 | the other pairs without a chain body].  The sums that have an order are those onto one chain body (its
// pairs stay in list order) and the path's partial sum onto the common body: its pairs must keep their list order too.
// A path whose pairs admit no such order clears the shape (the segments written for the paths before it stay).
struct FastOrder {
  std::vector<std::vector<int>> order;   // [npaths] pair indices
  std::vector<int> seg;                  // DevModel::f_seg: [npaths][maxc + 2] first | count << 16 of each group
};
FastOrder OrderFastPairs(const idto_model_t* m, const Star& star, const PairLists& l, FastShapeOf* f) {
  const int K = m->npaths, maxc = star.maxc, w2 = f->w2;
  const std::vector<int>&sa = l.sa, &sb = l.sb;
  FastOrder o;
  o.order.resize(K);
  o.seg.assign((size_t)K * (maxc + 2), 0);
  for (int p = 0; p < K && f->shape; ++p) {
    const int* first = l.path_pairs.data() + (size_t)p * l.maxpp;
    const std::vector<int> mine(first, first + l.path_npairs[p]);
    int lo_chain_common = 1 << 30, hi_chain_common = -1, last_slot = -1;
    for (int pi : mine) {
      const int nchainb = (sa[pi] >= 0) + (sb[pi] >= 0);
      if (nchainb > 1) {
        // two chain bodies: slots (w2 - 1, w2) of the spinner's shape only, and slot w2 - 1 has no other pair (the
        // force on it is taken out of its wrench in one subtraction, as the generic sum fin - (0 + f) is)
        bool fine = w2 >= 0 && std::min(sa[pi], sb[pi]) == w2 - 1 && std::max(sa[pi], sb[pi]) == w2;
        for (int pj : mine) fine = fine && (pj == pi || (sa[pj] != w2 - 1 && sb[pj] != w2 - 1));
        if (!fine) { f->shape = 0; break; }
        continue;
      }
      if (nchainb == 1 && (sa[pi] == -1 || sb[pi] == -1)) {
        const int sl = std::max(sa[pi], sb[pi]);
        if (sl < last_slot) { f->shape = 0; break; }   // (slot, index) order != index order on the common body's sum
        last_slot = sl;
        lo_chain_common = std::min(lo_chain_common, pi);
        hi_chain_common = std::max(hi_chain_common, pi);
      }
    }
    if (!f->shape) break;
    std::vector<std::vector<int>> groups(maxc + 2);
    for (int pi : mine) {
      const int sl = std::max(sa[pi], sb[pi]);
      if (sl >= 0) { groups[1 + sl].push_back(pi); continue; }
      const bool touches_common = sa[pi] == -1 || sb[pi] == -1;
      if (!touches_common || (sa[pi] == -1 && sb[pi] == -1)) { f->shape = 0; break; }   // (world, world) / (common, common)
      if (pi < lo_chain_common) groups[0].push_back(pi);
      else if (pi > hi_chain_common) groups[maxc + 1].push_back(pi);
      else { f->shape = 0; break; }
    }
    if (!f->shape) break;
    for (int gi = 0; gi < maxc + 2; ++gi) {
      o.seg[(size_t)p * (maxc + 2) + gi] = (int)o.order[p].size() | ((int)groups[gi].size() << 16);
      for (int pi : groups[gi]) o.order[p].push_back(pi);
    }
  }
  return o;
}

// ---- 8b. fd_kernel's forward-difference lane map without the redundant path lanes (model_layout.h tree_shape_dedup,
// DESIGN.md 3.1).  A column of q, or a mass column, of a chain joint touches that chain's path only: in such an
// evaluation the other paths' lanes repeat the baseline's path (exact zeros in a mass column).  Main lanes: four per
// evaluation of the baseline and of the common body's columns, one per single-path evaluation; helper lane h evaluates
// pairs for main lane h.  Refused - `on` false, the lane map of every evaluation on all its paths stays - when
//   - the shape's kernel has no such path, or a pair touches two chains,
//   - N+'s column for a chain joint is not a unit column (the perturbed v and a would reach other joints),
//   - the pairs are not laid out as that path walks them: per path nothing before the last slot, on the last slot one pair
//     with the common body then one with the world, behind it at most one pair of the common body with the world and
//     that on one path only,
//   - the tasks do not fit kFdMainLanes.
struct FdDedup {
  bool on = false;
  std::vector<int> qpaths, vpaths, lanes;
};
FdDedup BuildFdDedup(const idto_model_t* m, const Stem& stem, const Star& star, const PairLists& l, const NPlus& nplus,
                     const FastShapeOf& fast, const FastOrder& o, int f_maxpp) {
  const int K = m->npaths, maxc = star.maxc, nq = m->nq, nv = m->nv, all = (1 << K) - 1;
  FdDedup d;
  d.qpaths.assign(nq, all);
  d.vpaths.assign(nv, all);
  bool unit = true;
  for (int b = 0; b < m->nbodies; ++b) {
    if (b == m->common_body || stem.has(b)) continue;
    const int jn = m->jtype[b] == IDTO_JOINT_PLANAR ? 3 : 1;   // (a chain body's joint: revolute, prismatic or planar)
    for (int e = 0; e < jn; ++e) {
      const int c = m->qstart[b] + e, j = m->vstart[b] + e;
      d.qpaths[c] = 1 << m->body_path[b];
      d.vpaths[j] = 1 << m->body_path[b];
      unit = unit && nplus.colinfo[c] == (j | 1 << 16) && nplus.constant[(size_t)c * nv + j] == 1.0;
    }
  }
  if (!tree_shape_dedup(fast.shape) || l.shared || !unit || m->common_body < 0 || K != 4) return d;
  // ---- the pairs, as id_eval_fast<..., DD> walks them
  int body_path = -1, body_rec = 0;
  std::vector<int> foot_rec(K, 0);
  for (int p = 0; p < K; ++p) {
    const int* seg = o.seg.data() + (size_t)p * (maxc + 2);
    for (int gi = 0; gi < maxc; ++gi)
      if (seg[gi] >> 16) return d;
    const int s0 = seg[maxc] & 0xffff, tail = seg[maxc + 1] >> 16;
    if ((seg[maxc] >> 16) != 2 || tail > 1) return d;
    auto other = [&](int pi) { return l.sa[pi] >= 0 ? l.sb[pi] : l.sa[pi]; };
    if (other(o.order[p][s0]) != -1 || other(o.order[p][s0 + 1]) != -2) return d;
    foot_rec[p] = p * f_maxpp + s0 + 1;
    if (tail) {
      if (body_path >= 0) return d;
      const int pi = o.order[p][seg[maxc + 1] & 0xffff];
      if (std::max(l.sa[pi], l.sb[pi]) != -1 || std::min(l.sa[pi], l.sb[pi]) != -2) return d;
      body_path = p;
      body_rec = p * f_maxpp + (seg[maxc + 1] & 0xffff);
    }
  }
  if (K * f_maxpp > 255) return d;
  // ---- the main lanes: the evaluations on all paths first (their four lanes aligned), then the single-path ones, each
  // in the order of fd_body's evaluation index e = 0 | 1 + c (P) | 1 + nq + c (T) | 1 + 2 nq + j (M)
  const int E = 1 + 2 * nq + nv;
  auto paths_of = [&](int e) { return e == 0 ? all : (e < 1 + 2 * nq ? d.qpaths[(e - 1) % nq] : d.vpaths[e - 1 - 2 * nq]); };
  std::vector<int> main;
  for (int e = 0; e < E; ++e) {
    if (paths_of(e) != all) continue;
    const int full = e < 1 + 2 * nq ? FDL_FULL : 0;
    for (int p = 0; p < K; ++p)
      main.push_back(e | p << 8 | FDL_WHOLE | FDL_VALID | full | ((full && p == body_path) ? FDL_BODY_OWN : 0));
  }
  for (int e = 0; e < E; ++e) {
    const int ps = paths_of(e);
    if (ps == all) continue;
    if (ps & (ps - 1)) return d;
    int p = 0;
    while (!(ps >> p & 1)) ++p;
    const int full = e < 1 + 2 * nq ? FDL_FULL : 0;
    main.push_back(e | p << 8 | FDL_VALID | full | ((full && p == body_path) ? FDL_BODY_BASE : 0));
  }
  if ((int)main.size() > kFdMainLanes || E > 255) return d;
  // (the baseline's lanes are lanes 0 .. K - 1: FDL_BODY_BASE reads the result of lane body_path's helper)
  for (int p = (int)main.size(); p < kFdMainLanes; ++p) main.push_back(0 | (p % K) << 8);
  d.lanes = main;
  for (int h = 0; h < kFdHelperLanes; ++h) {
    const int w = main[h], p = w >> 8 & 3;
    const bool foot = (w & FDL_VALID) && (w & FDL_FULL), body = (w & FDL_BODY_OWN) != 0;
    d.lanes.push_back((foot ? FDH_FOOT : 0) | (body ? FDH_BODY : 0) | h << 8 | foot_rec[p] << 16 | body_rec << 24);
  }
  d.on = true;
  return d;
}

// ---- 9. id_fast.h's records: one of constants per (path, slot), one for the common body, one per contact pair in
// walking order
struct FastRecords {
  std::vector<double> body, cbody, pairs;
  int f_maxpp = 1;
};
void IdentityTimes(const double* X, double* out) {   // [I * R | I * p] with the fused forms of dev_math.h
  static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[3 * r + c] = std::fma(I[3 * r + 2], X[6 + c], std::fma(I[3 * r + 1], X[3 + c], I[3 * r] * X[c]));
    out[9 + r] = std::fma(I[3 * r + 2], X[11], std::fma(I[3 * r + 1], X[10], I[3 * r] * X[9]));
  }
}
void BodyRecord(const idto_model_t* m, int b, bool world, double* rec) {
  if (world) IdentityTimes(m->X_PF + (size_t)12 * b, rec + FB_XPF);
  else std::memcpy(rec + FB_XPF, m->X_PF + (size_t)12 * b, 12 * sizeof(double));
  std::memcpy(rec + FB_AXIS, m->axis + (size_t)3 * b, 3 * sizeof(double));
  rec[FB_MASS] = m->mass[b];
  std::memcpy(rec + FB_COM, m->com + (size_t)3 * b, 3 * sizeof(double));
  std::memcpy(rec + FB_INERTIA, m->inertia + (size_t)6 * b, 6 * sizeof(double));
  const int ndof = m->jtype[b] == IDTO_JOINT_FLOATING ? 6 : (m->jtype[b] == IDTO_JOINT_PLANAR ? 3 : 1);
  for (int d = 0; d < ndof; ++d) rec[FB_DAMP + d] = m->damping[m->vstart[b] + d];
  const int ix[2] = {m->qstart[b], m->vstart[b]};
  std::memcpy(rec + FB_IDX, ix, sizeof(ix));
}
FastRecords GatherFastRecords(const idto_model_t* m, const Star& star, const PairLists& l, const FastOrder& o) {
  const int K = m->npaths, maxc = star.maxc;
  FastRecords r;
  r.body.assign((size_t)K * maxc * FB_STRIDE, 0.0);
  r.cbody.assign(FB_STRIDE, 0.0);
  for (int p = 0; p < K; ++p)
    for (int s = 0; s < maxc; ++s)
      BodyRecord(m, star.chain[star.at(p, s)], star.pkind[star.at(p, s)] == PK_WORLD, r.body.data() + ((size_t)p * maxc + s) * FB_STRIDE);
  if (m->common_body >= 0) BodyRecord(m, m->common_body, true, r.cbody.data());
  for (int p = 0; p < K; ++p) r.f_maxpp = std::max(r.f_maxpp, (int)o.order[p].size());
  r.pairs.assign((size_t)K * r.f_maxpp * FP_STRIDE, 0.0);
  for (int p = 0; p < K; ++p)
    for (size_t j = 0; j < o.order[p].size(); ++j) {
      const int pi = o.order[p][j], ga = m->pair_a[pi], gb = m->pair_b[pi], sa = l.sa[pi], sb = l.sb[pi];
      double* rec = r.pairs.data() + ((size_t)p * r.f_maxpp + j) * FP_STRIDE;
      // C: the chain body of the pair's group, or the common body for a pair without one; the other body is
      // the common one or the world
      // (two chain bodies - the spinner's shape: C is the body of the later slot, the other one is handed to
      // pair_eval where the common body goes)
      const bool a_chain = sa >= 0, b_chain = sb >= 0;
      const bool cia = (a_chain && b_chain) ? sa > sb : (a_chain || (!b_chain && sa == -1));
      const int gc = cia ? ga : gb, go = cia ? gb : ga, so = cia ? sb : sa;
      const int info[4] = {m->geom_type[gc], m->geom_type[go], cia ? 1 : 0, (so == -1 || so >= 0) ? 1 : 0};
      std::memcpy(rec + FP_INFO, info, sizeof(info));
      std::memcpy(rec + FP_XC, m->geom_X + (size_t)12 * gc, 12 * sizeof(double));
      std::memcpy(rec + FP_SC, m->geom_size + (size_t)3 * gc, 3 * sizeof(double));
      if (so == -2) {   // world: [I R | 0 + I p], the expressions id_eval.h evaluates for a world-fixed geometry
        IdentityTimes(m->geom_X + (size_t)12 * go, rec + FP_XO);
        for (int e = 0; e < 3; ++e) rec[FP_XO + 9 + e] = 0.0 + rec[FP_XO + 9 + e];
      } else {
        std::memcpy(rec + FP_XO, m->geom_X + (size_t)12 * go, 12 * sizeof(double));
      }
      std::memcpy(rec + FP_SO, m->geom_size + (size_t)3 * go, 3 * sizeof(double));
    }
  return r;
}

// ---- 10. one blob: double tables, then int tables (two per double slot)
struct Packer {
  std::vector<double> dbl;
  std::vector<int> ints;
  size_t d(const double* src, size_t n) { const size_t o = dbl.size(); dbl.insert(dbl.end(), src, src + n); return o; }
  size_t d(const std::vector<double>& v) { return d(v.data(), v.size()); }
  size_t i(const int* src, size_t n) { const size_t o = ints.size(); ints.insert(ints.end(), src, src + n); return o; }
  size_t i(const std::vector<int>& v) { return i(v.data(), v.size()); }
};
}  // namespace

int BuildModelTables(const idto_model_t* m, ModelTables* out, std::string* err) {
  Stem stem;
  Star star;
  PairLists lists;
  if (int rc = CheckGeometry(m, err)) return rc;
  if (int rc = FindStem(m, &stem, err)) return rc;
  if (int rc = BuildStar(m, stem, &star, err)) return rc;
  if (int rc = BuildPairLists(m, stem, star, &lists, err)) return rc;
  const Exchange xch = BuildExchange(m, stem, star, lists);
  const NPlus nplus = BuildNPlus(m);
  bool capsules = false, cylinders = false;
  for (int g = 0; g < m->ngeoms; ++g) {
    capsules = capsules || m->geom_type[g] == IDTO_GEOM_CAPSULE;
    cylinders = cylinders || m->geom_type[g] == IDTO_GEOM_CYLINDER;
  }
  FastShapeOf fast = RecogniseShape(m, stem, star, lists.shared, capsules || cylinders);
  const FastOrder order = OrderFastPairs(m, star, lists, &fast);

  ModelTables& t = *out;
  t = ModelTables();
  const int nb = m->nbodies, ng = m->ngeoms, np = m->npairs;
  Packer k;
  t.at.X_PF = k.d(m->X_PF, (size_t)12 * nb); t.at.axis = k.d(m->axis, (size_t)3 * nb); t.at.mass = k.d(m->mass, nb);
  t.at.com = k.d(m->com, (size_t)3 * nb); t.at.inertia = k.d(m->inertia, (size_t)6 * nb); t.at.damping = k.d(m->damping, m->nv);
  t.at.geom_X = k.d(m->geom_X, (size_t)12 * ng); t.at.geom_size = k.d(m->geom_size, (size_t)3 * ng);
  t.at.nplus_const = k.d(nplus.constant);
  if (fast.shape) {
    const FastRecords rec = GatherFastRecords(m, star, lists, order);
    t.at.f_body = k.d(rec.body); t.at.f_cbody = k.d(rec.cbody); t.at.f_pairs = k.d(rec.pairs);
    t.f_maxpp = rec.f_maxpp;
  }
  const FdDedup dedup = BuildFdDedup(m, stem, star, lists, nplus, fast, order, t.f_maxpp);
  // the int tables, those fd_kernel needs beside the gathered records first: with a fast shape it stages only
  // [fast_lo, fast_lo + fast_n) of the blob in LDS
  t.at.jtype = k.i(m->jtype, nb); t.at.qstart = k.i(m->qstart, nb); t.at.vstart = k.i(m->vstart, nb);
  t.at.colinfo = k.i(nplus.colinfo); t.at.rowinfo = k.i(nplus.rowinfo); t.at.f_seg = k.i(order.seg);
  const size_t lanes_at = k.i(dedup.lanes);   // (no table of DevModel's: the kernel finds the words behind f_seg's)
  const size_t fast_end = k.ints.size();
  t.at.parent = k.i(m->parent, nb); t.at.geom_type = k.i(m->geom_type, ng); t.at.chain = k.i(star.chain);
  t.at.nchain = k.i(star.nchain); t.at.pkind = k.i(star.pkind); t.at.path_npairs = k.i(lists.path_npairs);
  t.at.path_pairs = k.i(lists.path_pairs); t.at.pair_ga = k.i(m->pair_a, np); t.at.pair_gb = k.i(m->pair_b, np);
  t.at.pair_sa = k.i(lists.sa); t.at.pair_sb = k.i(lists.sb);
  // (the exchange tables only where there are shared pairs or a stem: other models stage the blob they staged before)
  t.at.xrec = xch.on ? k.i(xch.xrec) : t.at.parent; t.at.pair_xa = xch.on ? k.i(xch.pair_xa) : t.at.parent;
  t.at.pair_xb = xch.on ? k.i(xch.pair_xb) : t.at.parent;
  t.at.stem = stem.n() > 1 ? k.i(xch.stem_tab) : t.at.parent;
  const size_t nd = k.dbl.size(), ni = k.ints.size();
  t.blob.assign(nd + (ni + 1) / 2 + 1, 0.0);
  std::memcpy(t.blob.data(), k.dbl.data(), nd * sizeof(double));
  std::memcpy(t.blob.data() + nd, k.ints.data(), ni * sizeof(int));
#define X(name) t.at.name += 2 * nd;
  IDTO_MODEL_INT_TABLES(X)
#undef X
  t.maxpp = lists.maxpp; t.nfloat = nplus.nfloat;
  for (int i = 0; i < 4; ++i) { t.float_qs[i] = nplus.float_qs[i]; t.float_vs[i] = nplus.float_vs[i]; }
  t.fast_shape = fast.shape;
  t.fast_lo = fast.shape ? (int)t.at.f_body : 0;
  t.fast_n = (int)(nd + (fast_end + 1) / 2) - t.fast_lo;
  t.nxb = xch.nxb; t.nstem = stem.n(); t.gslots = star.gslots; t.gcommon = star.gcommon; t.gstem = star.gstem;
  t.maxc = star.maxc; t.capsules = capsules; t.cylinders = cylinders;
  t.fd_dedup = dedup.on; t.fd_lanes_at = lanes_at + 2 * nd; t.fd_qpaths = dedup.qpaths; t.fd_vpaths = dedup.vpaths;
  return 0;
}

}  // namespace idto_host
