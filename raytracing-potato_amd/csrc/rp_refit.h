// rp_refit.h -- the refit of a finished 4-wide tree to moved geometry (include/rp.h rp_scene_refit_device, DESIGN.md
// 4.17), written once: the kernels (rp_refit.hip) and the CPU loops behind rph_refit_records (rp_host_refit.cpp)
// compile these functions, and both libraries make their plan and their refusals from here.
//
// A refit keeps the topology -- entries, node order, leaf order, pad records -- and rewrites what depends on where the
// geometry is: the primitive records, the per-primitive normals and the child boxes of every reachable node.  Both
// builders store a child's box as f32_child / quantize_child of the child's exact f64 box, a Q8 node's frame as qframe
// of the exact union of its children's boxes, and exact boxes are unions of hittable_box (rp_bvh.cpp Collapser::fill,
// rp_bvh_gpu.hip collapse_kernel; restated here because rp_bvh.cpp's machine code is part of rp_build_id).  Rounding
// outward is monotonic under min and max, so the stored words are a function of the records alone: a refit with
// unchanged geometry gives back the builder's bytes (tests/test_refit.py, tests/test_gpu_refit.py).
//
// NaN: min and max are fmin and fmax, as in hittable_box and the device builder -- a NaN coordinate is ignored beside a
// number and stays where all are NaN; such a box then takes f32_child's NaN words or quantize_child's whole frame.
// Nothing is clamped or repaired.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rp_layout.h"

// Loops over a node's four slots are unrolled for the device, so a record held in registers is never indexed by a variable.
#if defined(__clang__)
#define RPF_UNROLL _Pragma("unroll")
#else
#define RPF_UNROLL
#endif

namespace rpf {

constexpr uint32_t STATUS_OUT_OF_BOUND = 1u;  // = RP_REFIT_OUT_OF_BOUND (include/rp.h)

struct alignas(16) Box6 {
  double lo[3], hi[3];
};
static_assert(sizeof(Box6) == 48, "the scratch holds 48 B per primitive and per node");

// A primitive's record from its geometry; p.kind and p.material are kept.  A triangle: its vertices a, b, c, stored as
// {a, a - b, a - c} (rp_bvh.cpp pack_prim).  A sphere: a = {center.xyz, radius}, b and c unread.
RPL_HD inline void prim_record(rpl::Prim& p, const double* a, const double* b, const double* c) {
  if (p.kind == rpl::PRIM_TRIANGLE) {
    for (int k = 0; k < 3; k++) {
      p.g[k] = a[k];
      p.g[3 + k] = a[k] - b[k];
      p.g[6 + k] = a[k] - c[k];
    }
  } else {
    for (int k = 0; k < 4; k++) p.g[k] = a[k];
    for (int k = 4; k < 9; k++) p.g[k] = 0.0;
  }
}

// hittable_box (rp_bvh.cpp): a triangle's box from its three VERTICES (not from the record's differences, which are
// rounded), a sphere's center -+ radius.  Arguments as prim_record.
RPL_HD inline Box6 prim_box(uint32_t kind, const double* a, const double* b, const double* c) {
  Box6 x;
  for (int k = 0; k < 3; k++) {
    if (kind == rpl::PRIM_TRIANGLE) {
      x.lo[k] = fmin(fmin(a[k], b[k]), c[k]);
      x.hi[k] = fmax(fmax(a[k], b[k]), c[k]);
    } else {
      x.lo[k] = a[k] - a[3];
      x.hi[k] = a[k] + a[3];
    }
  }
  return x;
}

RPL_HD inline Box6 box_union(const Box6& a, const Box6& b) {
  Box6 u;
  for (int k = 0; k < 3; k++) {
    u.lo[k] = fmin(a.lo[k], b.lo[k]);
    u.hi[k] = fmax(a.hi[k], b.hi[k]);
  }
  return u;
}

// A finite coordinate of the box lies beyond the bound (NaN and infinities report nothing).
RPL_HD inline bool beyond(double v, double bound) { return fabs(v) < __builtin_huge_val() && fabs(v) > bound; }
RPL_HD inline bool over_bound(const Box6& x, double bound) {
  bool over = false;
  for (int k = 0; k < 3; k++) over = over || beyond(x.lo[k], bound) || beyond(x.hi[k], bound);
  return over;
}

// A leaf child's exact box: the union of its 1..8 primitives' boxes, the first one's to begin with.
RPL_HD inline Box6 leaf_box(uint32_t entry, const Box6* prim_boxes) {
  const uint32_t first = entry & rpl::LEAF_FIRST_MASK, cnt = ((entry >> rpl::LEAF_SHIFT) & 7u) + 1u;
  Box6 x = prim_boxes[first];
  for (uint32_t k = 1; k < cnt; k++) x = box_union(x, prim_boxes[first + k]);
  return x;
}
// A child's exact box by its entry (not ENTRY_EMPTY): a leaf's from the primitives' boxes, an inner child's its own
// box, written when its level was refit.
RPL_HD inline Box6 child_box(uint32_t entry, const Box6* prim_boxes, const Box6* node_boxes) {
  return (entry & rpl::ENTRY_LEAF) ? leaf_box(entry, prim_boxes) : node_boxes[entry];
}

// The box of an empty slot: (+inf, -inf), the unit of the union.  f32_child of it stores f32_empty's words (+inf, -inf)
// and quantize_child of it empty_child's (q_down(+inf) = 255, q_up(-inf) = 0), so the slots of a node are encoded
// without a branch on the entry; the identity tests hold the empty slots' words to the builders'.
RPL_HD inline Box6 empty_box() {
  Box6 x;
  for (int a = 0; a < 3; a++) {
    x.lo[a] = __builtin_huge_val();
    x.hi[a] = -__builtin_huge_val();
  }
  return x;
}

// The new box words of a node from its slots' exact boxes kb[c] (empty_box() where child[c] is ENTRY_EMPTY); the child[]
// entries are never written.  Returns the node's own exact box: the union of the four from (+inf, -inf), as the
// builders' `nb`.
RPL_HD inline Box6 node_union(const Box6 kb[4]) {
  Box6 nb = empty_box();
  RPF_UNROLL
  for (int c = 0; c < 4; c++) nb = box_union(nb, kb[c]);
  return nb;
}
RPL_HD inline Box6 node_refit(rpl::Node4& n, const Box6 kb[4]) {
  RPF_UNROLL
  for (int c = 0; c < 4; c++) rpl::f32_child(n, c, kb[c].lo, kb[c].hi);  // an empty slot: f32_empty's words
  return node_union(kb);
}
RPL_HD inline Box6 node_refit(rpl::Node4Q& n, const Box6 kb[4]) {
  const Box6 nb = node_union(kb);
  RPF_UNROLL
  for (int a = 0; a < 3; a++) {  // rp_bvh.cpp node_frame, rp_bvh_gpu.hip collapse_kernel: the guard included
    const bool ok = fabs(nb.lo[a]) < __builtin_huge_val() && fabs(nb.hi[a]) < __builtin_huge_val() && nb.lo[a] <= nb.hi[a];
    rpl::qframe(ok ? nb.lo[a] : 0.0, ok ? nb.hi[a] : 0.0, n.o[a], n.s[a]);
  }
  RPF_UNROLL
  for (int c = 0; c < 4; c++) rpl::quantize_child(n, c, kb[c].lo, kb[c].hi);  // an empty slot: empty_child's words
  return nb;
}

// Primitive k of an update of the geometry: its new record into p (kind and material kept) and its exact box.
// positions: 3 doubles per global vertex (PrimRef::v's numbering); spheres: 4 doubles per sphere, `rank` this one's.
RPL_HD inline Box6 prim_update(rpl::Prim& p, const rpl::PrimRef& r, uint32_t rank, const double* positions,
                               const double* spheres) {
  const bool tri = p.kind == rpl::PRIM_TRIANGLE;
  const double* a = tri ? positions + 3 * (size_t)r.v[0] : spheres + 4 * (size_t)rank;
  const double* b = tri ? positions + 3 * (size_t)r.v[1] : a;
  const double* c = tri ? positions + 3 * (size_t)r.v[2] : a;
  prim_record(p, a, b, c);
  return prim_box(p.kind, a, b, c);
}

// One node of a level: its children's boxes gathered, the record's box words rewritten in nd, its own box returned.
template <class Node>
RPL_HD inline Box6 node_update(Node& nd, const Box6* prim_boxes, const Box6* node_boxes) {
  Box6 kb[4];
  RPF_UNROLL
  for (int c = 0; c < 4; c++) {
    kb[c] = empty_box();
    if (nd.child[c] != rpl::ENTRY_EMPTY) kb[c] = child_box(nd.child[c], prim_boxes, node_boxes);
  }
  return node_refit(nd, kb);
}

// ---------------------------------------------------------------------------------------------------------------------
// The refusals, once for both libraries (NULL: accepted).

inline const char* check_format(uint32_t node_format) {
  if (node_format == rpl::NODES_W8)
    return "an 8-wide tree cannot be refit: a Node8Q slot encodes where its child lies relative to the node's centre "
           "(rebuild the scene)";
  if (node_format != rpl::NODES_F32 && node_format != rpl::NODES_Q8) return "node_format must be RP_NODES_F32 or RP_NODES_Q8";
  return nullptr;
}
inline const char* check_coord_max(double coord_max) {
  if (!(coord_max >= 0.0) || !(coord_max <= rpl::COORD_MAX)) return "coord_max must be finite, >= 0 and at most 2^54";
  return nullptr;
}
// An update's inputs against the scene's triangle and sphere counts.  Normals alone rewrite the per-primitive normals;
// an update of the geometry names all of it: positions when the scene has triangles, spheres when it has spheres.
inline const char* check_update(uint64_t n_tris, uint64_t n_spheres, const void* positions, const void* normals,
                                const void* spheres, const void* status) {
  if (!status) return "status must be non-NULL";
  if (!positions && !normals && !spheres) return "positions, normals and spheres are all NULL: nothing to update";
  if (positions || spheres) {
    if (n_tris && !positions) return "an update of the geometry of a scene with triangles needs positions";
    if (n_spheres && !spheres) return "an update of the geometry of a scene with spheres needs spheres";
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// The plan, made once per tree on the host from its records.

struct Plan {
  std::vector<uint32_t> level;    // per node record: its level, or NOT_REACHED (pad records, unused capacity)
  std::vector<uint32_t> order;    // the reachable nodes sorted by (level, index)
  std::vector<uint32_t> offsets;  // level l is order[offsets[l], offsets[l + 1]); n_levels + 1 entries
  std::vector<uint32_t> sphere_rank;  // per primitive (empty without spheres): a sphere's rank among the sphere hittables
  uint64_t n_tris = 0, n_spheres = 0;
  uint64_t min_vertices = 0;  // 1 + the largest vertex id a triangle names (0 without triangles)
  double amax = 0.0;          // >= every |coordinate| of the current primitives' boxes (NaN ignored)
  uint32_t n_levels() const { return (uint32_t)offsets.size() - 1u; }
};
constexpr uint32_t NOT_REACHED = 0xFFFFFFFFu;

// The nodes reachable from root, each one's level (0 without inner children, else 1 + its inner children's highest) and
// their order.  A walk with an explicit stack; every index is checked, so a plan's launches stay inside the buffers.
template <class Node>
inline const char* plan_nodes(const Node* nodes, uint64_t n_nodes, uint32_t root, uint64_t n_tree_prims, Plan& pl) {
  pl.level.assign(n_nodes, NOT_REACHED);
  pl.order.clear();
  if (root >= n_nodes) return "root out of range";
  struct Frame { uint32_t node, next; };
  std::vector<Frame> stack{{root, 0u}};
  std::vector<uint8_t> open(n_nodes, 0);
  open[root] = 1;
  while (!stack.empty()) {
    Frame& f = stack.back();
    if (f.next < 4u) {
      const uint32_t e = nodes[f.node].child[f.next++];
      if (e == rpl::ENTRY_EMPTY) continue;
      if (e & rpl::ENTRY_LEAF) {
        const uint64_t first = e & rpl::LEAF_FIRST_MASK, cnt = ((e >> rpl::LEAF_SHIFT) & 7u) + 1u;
        if (first + cnt > n_tree_prims) return "a leaf's primitives are out of range";
        continue;
      }
      if (e >= n_nodes) return "a child index is out of range";
      if (open[e]) return "a node is reached twice";
      open[e] = 1;
      stack.push_back({e, 0u});
      continue;
    }
    uint32_t lv = 0;
    for (int c = 0; c < 4; c++) {
      const uint32_t e = nodes[f.node].child[c];
      if (e != rpl::ENTRY_EMPTY && !(e & rpl::ENTRY_LEAF) && pl.level[e] + 1u > lv) lv = pl.level[e] + 1u;
    }
    pl.level[f.node] = lv;
    stack.pop_back();
  }
  uint32_t n_levels = pl.level[root] + 1u;
  std::vector<uint32_t> count(n_levels + 1u, 0u);
  for (uint64_t i = 0; i < n_nodes; i++)
    if (pl.level[i] != NOT_REACHED) count[pl.level[i] + 1u]++;
  for (uint32_t l = 0; l < n_levels; l++) count[l + 1u] += count[l];
  pl.offsets = count;
  pl.order.resize(count[n_levels]);
  std::vector<uint32_t> at(count.begin(), count.end() - 1);
  for (uint64_t i = 0; i < n_nodes; i++)  // increasing index within a level
    if (pl.level[i] != NOT_REACHED) pl.order[at[pl.level[i]]++] = (uint32_t)i;
  return nullptr;
}

// What the plan takes from the primitive table: the counts, the largest vertex id, the spheres' ranks by source
// hittable, and a bound on the current boxes (a triangle's vertices b and c are a - (a - b) up to one rounding: the
// bound takes an ulp-scale slack, as rp_bvh.cpp check).
inline const char* plan_prims(const rpl::Prim* prims, const rpl::PrimRef* refs, uint64_t n_prims, Plan& pl) {
  pl.n_tris = pl.n_spheres = pl.min_vertices = 0;
  pl.amax = 0.0;
  pl.sphere_rank.clear();
  std::vector<uint32_t> src;
  for (uint64_t k = 0; k < n_prims; k++) {
    const rpl::Prim& p = prims[k];
    if (p.kind == rpl::PRIM_TRIANGLE) {
      pl.n_tris++;
      for (int j = 0; j < 3; j++)
        if ((uint64_t)refs[k].v[j] + 1u > pl.min_vertices) pl.min_vertices = (uint64_t)refs[k].v[j] + 1u;
      for (int q = 0; q < 3; q++) {
        const double a = p.g[q], b = a - p.g[3 + q], c = a - p.g[6 + q];
        const double slack = 4.0 * 0x1p-52 * (fabs(a) + fabs(p.g[3 + q]) + fabs(p.g[6 + q]));
        pl.amax = fmax(pl.amax, fmax(fmax(fabs(a), fabs(b)), fabs(c)) + slack);
      }
    } else if (p.kind == rpl::PRIM_SPHERE) {
      pl.n_spheres++;
      src.push_back(refs[k].src);
      for (int q = 0; q < 3; q++) pl.amax = fmax(pl.amax, fmax(fabs(p.g[q] - p.g[3]), fabs(p.g[q] + p.g[3])));
    } else {
      return "a primitive of unknown kind";
    }
  }
  if (pl.n_spheres) {
    std::vector<uint32_t> sorted(src);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); i++)
      if (sorted[i] == sorted[i - 1]) return "two sphere primitives share a source hittable";
    pl.sphere_rank.assign(n_prims, 0u);
    for (uint64_t k = 0; k < n_prims; k++)
      if (prims[k].kind == rpl::PRIM_SPHERE)
        pl.sphere_rank[k] = (uint32_t)(std::lower_bound(sorted.begin(), sorted.end(), refs[k].src) - sorted.begin());
  }
  return nullptr;
}

}  // namespace rpf
