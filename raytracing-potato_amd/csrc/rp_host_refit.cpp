// rp_host_refit.cpp -- librp_host.so (include/rp_host.h): the CPU model of the refit (rp_refit.hip).  The plan, the
// arithmetic and the refusals are rp_refit.h's, the ones the device compiles; here are the loops over records laid out
// as rp_scene_tree returns them, and the hook that refits the host builder's own tree and runs the builder's check().
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rp_bvh.h"
#include "rp_host_util.h"
#include "rp_refit.h"

using rph::fail;

namespace {

// One refit of the records in place: the primitive pass, then the plan's levels from the leaves' parents upward.
template <class Node>
int refit_records(Node* nodes, uint64_t n_nodes, uint32_t root, rpl::Prim* prims, const rpl::PrimRef* refs,
                  rpl::TriNormals* tri_nrm, uint64_t n_prims, const double* positions, const double* normals,
                  const double* spheres, uint64_t n_vertices, uint64_t n_spheres, double bound, uint32_t* status) {
  if (!nodes || !n_nodes || (n_prims && (!prims || !refs))) return fail("refit: nodes, prims and refs must be non-NULL");
  if (!(bound >= 0.0) || !(bound < INFINITY)) return fail("refit: the bound must be finite and >= 0");
  rpf::Plan pl;
  const char* why = rpf::plan_nodes(nodes, n_nodes, root, n_prims, pl);
  if (!why) why = rpf::plan_prims(prims, refs, n_prims, pl);
  if (!why) why = rpf::check_update(pl.n_tris, pl.n_spheres, positions, normals, spheres, status);
  if (why) return fail(std::string("refit: ") + why);
  if ((positions || normals) && pl.min_vertices > n_vertices)
    return fail("refit: " + std::to_string(n_vertices) + " vertices, the triangles name " + std::to_string(pl.min_vertices));
  if (spheres && n_spheres != pl.n_spheres)
    return fail("refit: " + std::to_string(n_spheres) + " spheres, the scene has " + std::to_string(pl.n_spheres));
  if (normals && pl.n_tris && !tri_nrm) return fail("refit: normals need the per-primitive normal records");
  *status = 0;
  const bool geom = positions || spheres;
  std::vector<rpf::Box6> prim_boxes(geom ? n_prims : 0), node_boxes(geom ? n_nodes : 0);
  for (uint64_t k = 0; k < n_prims; k++) {
    if (geom) {
      prim_boxes[k] = rpf::prim_update(prims[k], refs[k], pl.n_spheres ? pl.sphere_rank[k] : 0u, positions, spheres);
      if (rpf::over_bound(prim_boxes[k], bound)) *status |= rpf::STATUS_OUT_OF_BOUND;
    }
    if (normals && prims[k].kind == rpl::PRIM_TRIANGLE)
      rpl::tri_normals_fill(tri_nrm[k], normals, refs[k].v[0], refs[k].v[1], refs[k].v[2]);
  }
  if (geom)
    for (uint32_t i : pl.order) node_boxes[i] = rpf::node_update(nodes[i], prim_boxes.data(), node_boxes.data());
  return RP_OK;
}

uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}
uint64_t records_hash(const rpb::PackedScene& ps) {
  uint64_t h = 0xcbf29ce484222325ull;
  if (ps.node_format == rpl::NODES_Q8) h = fnv(h, ps.qnodes.data(), ps.qnodes.size() * sizeof(rpl::Node4Q));
  else h = fnv(h, ps.nodes.data(), ps.nodes.size() * sizeof(rpl::Node4));
  h = fnv(h, ps.prims.data(), ps.prims.size() * sizeof(rpl::Prim));
  h = fnv(h, ps.prim_refs.data(), ps.prim_refs.size() * sizeof(rpl::PrimRef));
  return fnv(h, ps.tri_nrm.data(), ps.tri_nrm.size() * sizeof(rpl::TriNormals));
}

}  // namespace

extern "C" {

int rph_refit_records(uint32_t node_format, void* nodes, uint64_t n_nodes, uint32_t root, void* prims, const void* refs,
                      void* tri_normals, uint64_t n_prims, const double* positions, const double* normals,
                      const double* spheres, uint64_t n_vertices, uint64_t n_spheres, double bound, uint32_t* status) {
  if (const char* why = rpf::check_format(node_format)) return fail(std::string("refit: ") + why);
  auto* p = static_cast<rpl::Prim*>(prims);
  auto* r = static_cast<const rpl::PrimRef*>(refs);
  auto* t = static_cast<rpl::TriNormals*>(tri_normals);
  return node_format == rpl::NODES_Q8
             ? refit_records(static_cast<rpl::Node4Q*>(nodes), n_nodes, root, p, r, t, n_prims, positions, normals, spheres,
                             n_vertices, n_spheres, bound, status)
             : refit_records(static_cast<rpl::Node4*>(nodes), n_nodes, root, p, r, t, n_prims, positions, normals, spheres,
                             n_vertices, n_spheres, bound, status);
}

int rph_refit_plan(uint32_t node_format, const void* nodes, uint64_t n_nodes, uint32_t root, uint32_t* levels_out,
                   uint32_t* order_out, uint32_t* n_levels) {
  if (const char* why = rpf::check_format(node_format)) return fail(std::string("refit: ") + why);
  if (!nodes || !n_nodes || !n_levels) return fail("rph_refit_plan: nodes and n_levels must be non-NULL");
  rpf::Plan pl;
  const char* why = node_format == rpl::NODES_Q8
                        ? rpf::plan_nodes(static_cast<const rpl::Node4Q*>(nodes), n_nodes, root, rpl::MAX_PRIMS, pl)
                        : rpf::plan_nodes(static_cast<const rpl::Node4*>(nodes), n_nodes, root, rpl::MAX_PRIMS, pl);
  if (why) return fail(std::string("rph_refit_plan: ") + why);
  if (levels_out) std::memcpy(levels_out, pl.level.data(), sizeof(uint32_t) * n_nodes);
  if (order_out) {
    std::memcpy(order_out, pl.order.data(), sizeof(uint32_t) * pl.order.size());
    for (uint64_t i = pl.order.size(); i < n_nodes; i++) order_out[i] = rpf::NOT_REACHED;
  }
  *n_levels = pl.n_levels();
  return RP_OK;
}

int rph_bvh_refit_check(const rp_scene_desc* before, const rp_scene_desc* after, uint32_t node_format, int32_t always_max,
                        uint32_t always_minor, uint64_t* hashes, uint32_t* status) {
  if (!before || !after || !status) return fail("rph_bvh_refit_check: non-NULL descriptions and status");
  if (const char* why = rpf::check_format(node_format)) return fail(std::string("refit: ") + why);
  std::string err;
  if (rpb::validate(before, err) != RP_OK || rpb::validate(after, err) != RP_OK) return fail(err);
  // the same topology and counts: hittables of the same kinds over the same meshes' triangles
  bool same = before->n_hittables == after->n_hittables && before->n_meshes == after->n_meshes;
  for (uint32_t i = 0; same && i < before->n_meshes; i++) {
    const rp_mesh &a = before->meshes[i], &b = after->meshes[i];
    same = a.n_vertices == b.n_vertices && a.n_indices == b.n_indices &&
           (!a.n_indices || !std::memcmp(a.indices, b.indices, sizeof(uint32_t) * a.n_indices));
  }
  for (uint32_t i = 0; same && i < before->n_hittables; i++) {
    const rp_hittable &a = before->hittables[i], &b = after->hittables[i];
    same = a.kind == b.kind && (a.kind == RP_HITTABLE_SPHERE || (a.mesh == b.mesh && a.triangle == b.triangle));
  }
  if (!same) return fail("rph_bvh_refit_check: the two descriptions differ in more than where the geometry is");
  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  bo.node_format = node_format;
  if (always_max >= 0) bo.always_max = (uint32_t)always_max;
  bo.always_minor = always_minor != 0;
  int rc = rpb::build(before, bo, ps, err);
  if (rc != RP_OK) return fail(rc, err);
  if (hashes) hashes[0] = records_hash(ps);
  // the after-geometry in the refit's numbering: the meshes' vertices concatenated, the spheres in hittable order
  std::vector<double> pos, nrm, sph;
  for (uint32_t i = 0; i < after->n_meshes; i++) {
    const rp_mesh& m = after->meshes[i];
    pos.insert(pos.end(), m.positions, m.positions + 3 * (size_t)m.n_vertices);
    nrm.insert(nrm.end(), m.normals, m.normals + 3 * (size_t)m.n_vertices);
  }
  for (uint32_t i = 0; i < after->n_hittables; i++) {
    const rp_hittable& h = after->hittables[i];
    if (h.kind == RP_HITTABLE_SPHERE) sph.insert(sph.end(), {h.center[0], h.center[1], h.center[2], h.radius});
  }
  // the bound: both geometries', so the frames of the refit tree stay inside the qbound check() holds them to
  rpb::PrimInput pin;
  if ((rc = rpb::prim_input(after, pin, err)) != RP_OK) return fail(rc, err);
  const double bound = std::fmax(pin.amax, (ps.qbound - 0x1p-50) / 4.0);
  pos.push_back(0.0), nrm.push_back(0.0), sph.push_back(0.0);  // data() of an empty vector may be NULL: "unchanged"
  const uint64_t n_vert = (pos.size() - 1) / 3, n_sph = (sph.size() - 1) / 4, n_prims = before->n_hittables;
  const bool has_tri = n_prims > n_sph;
  void* nodes = node_format == rpl::NODES_Q8 ? (void*)ps.qnodes.data() : (void*)ps.nodes.data();
  rc = rph_refit_records(node_format, nodes, ps.n_nodes(), ps.root, ps.prims.data(), ps.prim_refs.data(), ps.tri_nrm.data(),
                         n_prims, has_tri ? pos.data() : nullptr, has_tri ? nrm.data() : nullptr,
                         n_sph ? sph.data() : nullptr, n_vert, n_sph, bound, status);
  if (rc != RP_OK) return rc;
  if (hashes) hashes[1] = records_hash(ps);
  ps.qbound = std::fmax(ps.qbound, rpl::qbound(bound));
  rc = rpb::check(ps, err);
  return rc != RP_OK ? fail(rc, "refit tree: " + err) : RP_OK;
}

}  // extern "C"
