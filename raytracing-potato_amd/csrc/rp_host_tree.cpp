// rp_host_tree.cpp -- librp_host.so (include/rp_host.h): the CPU model of the traversal over the packed tree and the
// hooks on the tree and on what the kernel and the model share -- traversal stats, selfcheck, tree hash, the material
// head, the ray setup (rp_ray.h) and the exact primitive tests (rp_isect.h).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rp_bvh.h"
#include "rp_host_util.h"
#include "rp_isect.h"
#include "rp_ray.h"

using rph::fail;

namespace {

// The slab test's terms over one node, per axis: the plane slope and the near and far addends -- the ray's own
// {inv, nb, fb} (rp_ray.h) for f32 planes, a frame's {A, Bn, Bf} (rp_isect.h frame_axis) for 8-bit codes.
struct Slabs {
  float A[3], Bn[3], Bf[3];
};
template <class Node>
Slabs frame_slabs(const Node& nd, const Slabs& ray) {
  Slabs f;
  for (int k = 0; k < 3; k++) {
    const rpi::FrameAxis a = rpi::frame_axis(nd.o[k], nd.s[k], ray.A[k], ray.Bn[k], ray.Bf[k]);
    f.A[k] = a.A;
    f.Bn[k] = a.Bn;
    f.Bf[k] = a.Bf;
  }
  return f;
}
// The children of a node (Node4: f32 planes; Node4Q, Node8Q: codes) that pass the slab test, as a bit mask, and every
// child's tnear.  Both planes with each addend and min / max where the kernel picks the near and the far plane by the
// slope's sign: the same pair of values.
template <class Node>
uint32_t children_hit(const Node& nd, const Slabs& s, float tmin32, float best32, float* tn) {
  const decltype(&nd.lo_x[0]) lo[3] = {nd.lo_x, nd.lo_y, nd.lo_z}, hi[3] = {nd.hi_x, nd.hi_y, nd.hi_z};
  uint32_t hits = 0;
  for (int c = 0; c < (int)(sizeof nd.lo_x / sizeof nd.lo_x[0]); c++) {
    float tnear = tmin32, tfar = best32;
    for (int k = 0; k < 3; k++) {
      const float l = (float)lo[k][c], h = (float)hi[k][c];
      tnear = fmaxf(tnear, fminf(rpi::plane_t(l, s.A[k], s.Bn[k]), rpi::plane_t(h, s.A[k], s.Bn[k])));
      tfar = fminf(tfar, fmaxf(rpi::plane_t(l, s.A[k], s.Bf[k]), rpi::plane_t(h, s.A[k], s.Bf[k])));
    }
    tn[c] = tnear;
    if (rpi::slab_pass(tnear, tfar)) hits |= 1u << c;
  }
  return hits;
}

// One exact test of a primitive with geometry g (rpl::Prim::g); accepted: take(t, u, v) (a sphere: u = v = 0).
template <class Take>
void prim_test(uint32_t kind, const double* g, rpi::V3 o, rpi::V3 d, double tmin, double best, Take take) {
  const rpi::V3 g0 = {g[0], g[1], g[2]};
  if (kind == rpl::PRIM_TRIANGLE) rpi::tri_test(g0, {g[3], g[4], g[5]}, {g[6], g[7], g[8]}, o, d, tmin, best, take);
  else rpi::sphere_test(g0, g[3], o, d, tmin, best, [&](double t) { take(t, 0.0, 0.0); });
}

// What the rph_bvh_*_opt hooks open with: the scene validated and its tree built with the hook's options (rp_host.h's
// always_max and always_minor: always_max < 0 is the builder's default).
int build_tree(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, uint32_t threads, int32_t always_max,
               uint32_t always_minor, rpb::PackedScene& ps) {
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::BuildOptions bo;
  bo.node_format = node_format;
  bo.collapse = collapse == RP_COLLAPSE_GREEDY ? rpb::COLLAPSE_GREEDY : rpb::COLLAPSE_SAH;
  bo.threads = threads;
  if (always_max >= 0) bo.always_max = (uint32_t)always_max;
  bo.always_minor = always_minor != 0;
  rc = rpb::build(desc, bo, ps, err);
  return rc != RP_OK ? fail(err) : RP_OK;
}

}  // namespace

extern "C" {

int rph_bvh_traversal_stats(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                            uint64_t* per_ray) {
  return rph_bvh_traversal_stats_ex(desc, rays, n, node_format, RP_COLLAPSE_AUTO, per_ray);
}

int rph_bvh_traversal_stats_ex(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                               uint32_t collapse, uint64_t* per_ray) {
  return rph_bvh_traversal_stats_opt(desc, rays, n, node_format, collapse, -1, 0, per_ray);
}

int rph_bvh_traversal_stats_opt(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                                uint32_t collapse, int32_t always_max, uint32_t always_minor, uint64_t* per_ray) {
  // CPU model of rp_device.h's traversal over the same packed tree.  The arithmetic is the kernel's source: the ray
  // setup (rp_ray.h), the frame terms, plane t^ and pass test of the conservative f32 slab test and the exact f64
  // primitive tests (rp_isect.h) -- except the reciprocal, a correctly rounded 1/x for the device's v_rcp_f32.  The
  // model's own: the min/max slab form instead of the device's octant selection (the same values), one child at a
  // time, near-first order, leaf primitives tested when reached.  per_ray: n x 3 {wide nodes visited, primitive
  // tests, closest hittable id or 2^64-1}.  tests/test_bvh.py checks the closest hits against brute force.
  rpb::PackedScene ps;
  if (const int rc = build_tree(desc, node_format, collapse, 0, always_max, always_minor, ps)) return rc;
  const bool q8 = ps.node_format != rpl::NODES_F32;  // Node4Q or Node8Q: the frame term
  const bool w8 = ps.node_format == rpl::NODES_W8;
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    const rpi::V3 o = {q[0], q[1], q[2]}, d = {q[3], q[4], q[5]};
    const double tmin = q[6];
    Slabs ray;  // per axis: slope, near- and far-plane addends (rp_ray.h, as rp_device.h setup_ray32)
    for (int k = 0; k < 3; k++) {
      const rpr::Axis a =
          q8 ? rpr::axis_setup<true>(q[k], q[3 + k], ps.qbound) : rpr::axis_setup<false>(q[k], q[3 + k], 0.0);
      ray.A[k] = a.inv;
      ray.Bn[k] = a.nb;
      ray.Bf[k] = a.fb;
    }
    const float tmin32 = rpr::f32_below(tmin);
    double best = q[7];
    float best32 = rpr::best_above(best);
    int64_t bestp = -1;
    uint64_t visits = 0, tests = 0;
    auto test = [&](uint32_t k) {
      tests++;
      prim_test(ps.prims[k].kind, ps.prims[k].g, o, d, tmin, best, [&](double t, double, double) {
        best = t;
        bestp = ps.prim_refs[k].src;
        best32 = rpr::best_above(best);
      });
    };
    // the always-tested primitives first (rp_bvh.h BuildOptions::always_max), as the kernel does
    for (uint32_t k = ps.always_first; k < ps.always_first + ps.n_always; k++) test(k);
    if (w8) {
      // 8-wide: children in rank order slot ^ octant; a stack of groups {family index | imask, rank bits}; the
      // leaf children's primitives are tested when their node is visited (the kernel parks them, same hits)
      const uint32_t oct = (d.x < 0.0 ? 1u : 0u) | (d.y < 0.0 ? 2u : 0u) | (d.z < 0.0 ? 4u : 0u);
      std::vector<std::pair<uint32_t, uint32_t>> groups;  // {inner word, remaining rank bits}
      auto visit = [&](uint32_t node) {
        visits++;
        const rpl::Node8Q& nd = ps.wnodes[node];
        float tn[8];
        const uint32_t hits = children_hit(nd, frame_slabs(nd, ray), tmin32, best32, tn);
        uint32_t pm = 0;
        for (int c = 0; c < 8; c++)
          if (hits >> c & 1u) pm |= nd.pmask[c];
        for (; pm; pm &= pm - 1u) test(nd.prim + (uint32_t)__builtin_ctz(pm));
        const uint32_t ih = hits & (nd.inner >> 24);
        uint32_t ranks = 0;
        for (int c = 0; c < 8; c++)
          if (ih >> c & 1u) ranks |= 1u << (c ^ oct);
        if (ranks) groups.push_back({nd.inner, ranks});
      };
      visit(ps.root);
      while (!groups.empty()) {
        auto& g = groups.back();
        const uint32_t rk = (uint32_t)__builtin_ctz(g.second), slot = rk ^ oct, word = g.first;
        g.second &= g.second - 1u;
        if (!g.second) groups.pop_back();
        visit((word & rpl::W8_INDEX) + (uint32_t)__builtin_popcount((word >> 24) & ((1u << slot) - 1u)));
      }
    } else {
      std::vector<uint32_t> stack;
      uint32_t cur = ps.root;
      for (;;) {
        while (!(cur & rpl::ENTRY_LEAF)) {
          visits++;
          float tn[4];
          const uint32_t hits = q8 ? children_hit(ps.qnodes[cur], frame_slabs(ps.qnodes[cur], ray), tmin32, best32, tn)
                                   : children_hit(ps.nodes[cur], ray, tmin32, best32, tn);
          const uint32_t* child = q8 ? ps.qnodes[cur].child : ps.nodes[cur].child;
          uint32_t cc[4];
          for (int c = 0; c < 4; c++) {
            if (!(hits >> c & 1u) || child[c] == rpl::ENTRY_EMPTY) tn[c] = INFINITY;
            cc[c] = child[c];
          }
          for (int a = 0; a < 4; a++)  // stable sort by tn (matches the device network for distinct keys)
            for (int b = a + 1; b < 4; b++)
              if (tn[b] < tn[a]) { std::swap(tn[a], tn[b]); std::swap(cc[a], cc[b]); }
          for (int c = 3; c >= 1; c--)
            if (tn[c] != INFINITY) stack.push_back(cc[c]);
          if (tn[0] != INFINITY) cur = cc[0];
          else if (stack.empty()) cur = rpl::ENTRY_EMPTY;
          else { cur = stack.back(); stack.pop_back(); }
        }
        if (cur == rpl::ENTRY_EMPTY) break;
        const uint32_t first = cur & rpl::LEAF_FIRST_MASK, cnt = ((cur >> rpl::LEAF_SHIFT) & 7u) + 1u;
        for (uint32_t k = first; k < first + cnt; k++) test(k);
        if (stack.empty()) cur = rpl::ENTRY_EMPTY;
        else { cur = stack.back(); stack.pop_back(); }
      }
    }
    per_ray[3 * r] = visits;
    per_ray[3 * r + 1] = tests;
    per_ray[3 * r + 2] = bestp < 0 ? ~0ull : (uint64_t)bestp;
  }
  return RP_OK;
}

int rph_bvh_selfcheck(const rp_scene_desc* desc, uint32_t node_format, uint64_t* stats) {
  return rph_bvh_selfcheck_ex(desc, node_format, RP_COLLAPSE_AUTO, stats);
}

int rph_bvh_selfcheck_ex(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, uint64_t* stats) {
  uint64_t st[6];
  const int rc = rph_bvh_selfcheck_opt(desc, node_format, collapse, -1, 0, st);
  if (rc == RP_OK && stats) std::memcpy(stats, st, 4 * sizeof(uint64_t));
  return rc;
}

int rph_bvh_selfcheck_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, int32_t always_max,
                          uint32_t always_minor, uint64_t* stats) {
  rpb::PackedScene ps;
  int rc = build_tree(desc, node_format, collapse, 0, always_max, always_minor, ps);
  if (rc) return rc;
  std::string err;
  rc = rpb::check(ps, err);
  if (rc != RP_OK) return fail(rc, err);
  if (stats) {
    stats[0] = ps.n_nodes();
    stats[1] = ps.n_leaves;
    stats[2] = ps.max_depth;
    stats[3] = desc->n_hittables;
    stats[4] = ps.n_always;
    stats[5] = 0;  // non-triangle primitives inside the tree (the leaf-ordered records in front of the always tail)
    for (uint32_t k = 0; k < ps.always_first; k++) stats[5] += ps.prims[k].kind != rpl::PRIM_TRIANGLE;
  }
  return RP_OK;
}

int rph_bvh_tree_hash(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, uint64_t* hash) {
  return rph_bvh_tree_hash_opt(desc, node_format, threads, -1, 0, hash);
}

int rph_bvh_tree_hash_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, int32_t always_max,
                          uint32_t always_minor, uint64_t* hash) {
  rpb::PackedScene ps;
  if (const int rc = build_tree(desc, node_format, RP_COLLAPSE_AUTO, threads, always_max, always_minor, ps)) return rc;
  uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the packed records
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  };
  if (ps.node_format == rpl::NODES_W8) mix(ps.wnodes.data(), ps.wnodes.size() * sizeof(rpl::Node8Q));
  else if (ps.node_format == rpl::NODES_Q8) mix(ps.qnodes.data(), ps.qnodes.size() * sizeof(rpl::Node4Q));
  else mix(ps.nodes.data(), ps.nodes.size() * sizeof(rpl::Node4));
  mix(ps.prim_refs.data(), ps.prim_refs.size() * sizeof(rpl::PrimRef));
  *hash = h;
  return RP_OK;
}

int rph_tri_normals(const rp_scene_desc* desc, uint32_t node_format, int32_t always_max, uint32_t always_minor, uint64_t cap,
                    double* normals, uint32_t* refs, uint32_t* kinds, uint64_t* n_prims) {
  if (!desc || !n_prims) return fail("rph_tri_normals: non-NULL pointers");
  rpb::PackedScene ps;
  if (const int rc = build_tree(desc, node_format, RP_COLLAPSE_AUTO, 0, always_max, always_minor, ps)) return rc;
  static_assert(sizeof(rpl::TriNormals) == 9 * sizeof(double) && sizeof(rpl::PrimRef) == 4 * sizeof(uint32_t), "rows");
  const uint64_t n = desc->n_hittables;  // the packed tables hold one record more for a scene without primitives
  *n_prims = n;
  for (uint64_t k = 0; k < n && k < cap; k++) {
    if (normals) std::memcpy(normals + 9 * k, &ps.tri_nrm[k], sizeof(rpl::TriNormals));
    if (refs) std::memcpy(refs + 4 * k, &ps.prim_refs[k], sizeof(rpl::PrimRef));
    if (kinds) kinds[k] = ps.prims[k].kind;
  }
  return RP_OK;
}

int rph_material_head(const uint32_t fields[6], uint32_t packed[2], uint32_t unpacked[7]) {
  if (!fields || !packed || !unpacked) return fail("rph_material_head: non-NULL pointers");
  rpl::Material m{};
  m.scatter_kind = fields[0]; m.absorb_kind = fields[1]; m.emit_kind = fields[2]; m.needs_uv = fields[3];
  m.absorb_tex = fields[4]; m.emit_tex = fields[5];
  rpl::material_head_pack(m, packed[0], packed[1]);
  const rpl::MaterialHead h = rpl::material_head_unpack(packed[0], packed[1]);
  const uint32_t u[7] = {h.scatter_kind, h.absorb_kind, h.emit_kind, h.needs_uv, h.absorb_tex, h.emit_tex, h.wide ? 1u : 0u};
  for (int k = 0; k < 7; k++) unpacked[k] = u[k];
  return RP_OK;
}

int rph_scene_materials(const rp_scene_desc* desc, uint64_t cap, uint32_t* words, uint64_t* n_materials) {
  if (!desc || !n_materials || (cap && !words)) return fail("rph_scene_materials: non-NULL pointers");
  std::string err;
  int rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(err);
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.tables_only = true;
  bo.vertex_tables = false;
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(err);
  *n_materials = desc->n_materials;
  for (uint64_t i = 0; i < desc->n_materials && i < cap; i++) {
    const rpl::Material& m = ps.materials[i];
    const uint32_t w[8] = {m.scatter_kind, m.absorb_kind, m.emit_kind, m.absorb_tex, m.emit_tex, m.needs_uv, m.head, m.head_tex};
    for (int k = 0; k < 8; k++) words[8 * i + k] = w[k];
  }
  return RP_OK;
}

int rph_ray_setup(uint32_t node_format, double qbound, const double* rays, uint64_t n, float* out) {
  if ((node_format != RP_NODES_F32 && node_format != RP_NODES_Q8 && node_format != RP_NODES_W8) || !(qbound >= 0.0) ||
      (n && (!rays || !out)))
    return fail("rph_ray_setup: node_format f32, q8 or w8, qbound >= 0, non-NULL pointers");
  const bool frame = node_format != RP_NODES_F32;
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    float* o = out + 11 * r;
    for (int k = 0; k < 3; k++) {
      const rpr::Axis a = frame ? rpr::axis_setup<true>(q[k], q[3 + k], qbound) : rpr::axis_setup<false>(q[k], q[3 + k], qbound);
      o[k] = a.inv;
      o[3 + k] = a.nb;
      o[6 + k] = a.fb;
    }
    o[9] = rpr::f32_below(q[6]);
    o[10] = rpr::best_above(q[7]);
  }
  return RP_OK;
}

int rph_prim_test(uint32_t kind, const double g[9], const double* rays, uint64_t n, double* out) {
  if ((kind != rpl::PRIM_SPHERE && kind != rpl::PRIM_TRIANGLE) || !g || (n && (!rays || !out)))
    return fail("rph_prim_test: kind 0 (sphere) or 1 (triangle), non-NULL pointers");
  for (uint64_t r = 0; r < n; r++) {
    const double* q = rays + 8 * r;
    double* h = out + 4 * r;
    h[0] = h[1] = h[2] = h[3] = 0.0;
    prim_test(kind, g, {q[0], q[1], q[2]}, {q[3], q[4], q[5]}, q[6], q[7], [&](double t, double u, double v) {
      h[0] = 1.0; h[1] = t; h[2] = u; h[3] = v;
    });
  }
  return RP_OK;
}

}  // extern "C"
