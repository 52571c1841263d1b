// rp_refit.hip -- moving geometry (include/rp.h rp_refit_create, rp_scene_refit_device, rp_scene_refit):
// the primitive records, the per-primitive normals and the child boxes of a scene's existing 4-wide tree rewritten on
// the device from new vertex positions, normals and sphere records.  The topology is kept.  The arithmetic, the plan and
// the refusals are rp_refit.h's, shared with the CPU loops behind rph_refit_records; this file is the handle, the
// kernels, their launches and the C-ABI.
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like the other passes, not part of the
// rp_build_id hash: it runs between renders and decides no ray of them.  All of its state lives in rp_refit; of the
// scene it writes the records a refit is about and ks.qbound (rp_refit_create), and adds no member.
//
// prim_kernel: one lane per primitive, the always-tested tail included.  A gather of the primitive's vertices (or its
// sphere) through PrimRef, the 80 B record and the 48 B exact box written as 16 B stores, the 72 B normals as four 16 B
// stores and one of 8 B.  level_kernel: one launch per level of the plan, leaves' parents first; one lane per node reads
// its record and its children's exact boxes (a leaf's: the union of its primitives' boxes; an inner child's: the box the
// previous launch wrote), rewrites the record's box words -- never the entries -- and writes the node's own box.  Blocks
// of 64 lanes, no LDS; stream order is the only ordering, and the one atomic is a wave's report of a box beyond the
// bound.  Memory bound: per primitive 24..72 B gathered and 128..200 B written.
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers the shared headers use

#include "rp_refit.h"

#pragma clang fp contract(off)

#pragma GCC visibility push(hidden)
struct rp_refit {
  int device = 0;
  rp_scene* scene = nullptr;
  uint64_t n_prims = 0, n_tris = 0, n_spheres = 0, n_vertices = 0;
  double bound = 0.0;
  std::vector<uint32_t> offsets;       // the plan's levels in d_order
  DevBuf<uint32_t> d_order;            // reachable nodes by (level, index)
  DevBuf<uint32_t> d_sphere_rank;      // per primitive, when the scene has spheres
  DevBuf<rpf::Box6> d_prim_boxes, d_node_boxes;  // the exact boxes: 48 B per primitive and per node record
};
#pragma GCC visibility pop

namespace rpf {

constexpr int BLOCK = 64;

typedef double double2a8 __attribute__((ext_vector_type(2), aligned(8)));

struct PrimArgs {
  uint32_t n;
  rpl::Prim* prims;
  const rpl::PrimRef* refs;
  rpl::TriNormals* tri_nrm;
  const uint32_t* sphere_rank;  // NULL without spheres
  const double* positions;      // with spheres: the geometry is updated (check_update: both where the scene has both)
  const double* spheres;
  const double* normals;        // NULL: the per-primitive normals stay
  Box6* prim_boxes;
  double bound;
  uint32_t* status;
};

// The status word starts at zero: a kernel ahead of the others on the stream, not a memset, so a captured graph replays
// it as it replays them.
__global__ void __launch_bounds__(BLOCK) zero_status_kernel(uint32_t* status) {
  if (threadIdx.x == 0) *status = 0u;
}

__global__ void __launch_bounds__(BLOCK) prim_kernel(const PrimArgs A) {
  const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
  bool over = false;  // no early return: every lane reaches the ballot
  if (k < A.n) {
    const rpl::PrimRef r = A.refs[k];
    rpl::Prim p;
    p.kind = A.prims[k].kind;
    p.material = A.prims[k].material;
    if (A.positions || A.spheres) {
      const Box6 b = prim_update(p, r, A.sphere_rank ? A.sphere_rank[k] : 0u, A.positions, A.spheres);
      A.prims[k] = p;
      A.prim_boxes[k] = b;
      over = over_bound(b, A.bound);
    }
    if (A.normals && p.kind == rpl::PRIM_TRIANGLE) {
      rpl::TriNormals t;
      rpl::tri_normals_fill(t, A.normals, r.v[0], r.v[1], r.v[2]);
      const double* w = &t.n[0][0];
      char* dst = reinterpret_cast<char*>(A.tri_nrm + k);  // 72 B records, 8-byte aligned
#pragma unroll
      for (int q = 0; q < 4; q++) *reinterpret_cast<double2a8*>(dst + 16 * q) = double2a8{w[2 * q], w[2 * q + 1]};
      *reinterpret_cast<double*>(dst + 64) = w[8];
    }
  }
  if (__ballot(over) != 0ull && threadIdx.x == 0) atomicOr(A.status, STATUS_OUT_OF_BOUND);
}

// A record's entries (one 16 B load) and the words a refit rewrites, the 16 B chunks in front of them (rp_layout.h).
static_assert(offsetof(rpl::Node4, child) == 96 && offsetof(rpl::Node4Q, child) == 48, "16 B chunks in front of child[]");
template <class Node>
__device__ __forceinline__ void load_entries(const Node* src, Node& nd) {
  const uint4 c = *reinterpret_cast<const uint4*>(src->child);
  nd.child[0] = c.x, nd.child[1] = c.y, nd.child[2] = c.z, nd.child[3] = c.w;
}
__device__ __forceinline__ void store_boxes(rpl::Node4* dst, const rpl::Node4& nd) {
  float4* d = reinterpret_cast<float4*>(dst);
  const float* const rows[6] = {nd.lo_x, nd.hi_x, nd.lo_y, nd.hi_y, nd.lo_z, nd.hi_z};
#pragma unroll
  for (int q = 0; q < 6; q++) d[q] = make_float4(rows[q][0], rows[q][1], rows[q][2], rows[q][3]);
}
__device__ __forceinline__ uint32_t pack4(const uint8_t* b) {
  return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}
__device__ __forceinline__ void store_boxes(rpl::Node4Q* dst, const rpl::Node4Q& nd) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  d[0] = make_uint4(__float_as_uint(nd.o[0]), __float_as_uint(nd.o[1]), __float_as_uint(nd.o[2]), __float_as_uint(nd.s[0]));
  d[1] = make_uint4(__float_as_uint(nd.s[1]), __float_as_uint(nd.s[2]), pack4(nd.lo_x), pack4(nd.hi_x));
  d[2] = make_uint4(pack4(nd.lo_y), pack4(nd.hi_y), pack4(nd.lo_z), pack4(nd.hi_z));
}

template <class Node>
__global__ void __launch_bounds__(BLOCK) level_kernel(Node* __restrict__ nodes, const uint32_t* __restrict__ order,
                                                      uint32_t n, const Box6* __restrict__ prim_boxes,
                                                      Box6* node_boxes) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = order[i];
  Node nd;
  load_entries(nodes + idx, nd);
  const Box6 nb = node_update(nd, prim_boxes, node_boxes);
  store_boxes(nodes + idx, nd);
  node_boxes[idx] = nb;
}

template <class Node>
int launch_levels(const rp_refit* h, hipStream_t st) {
  Node* nodes = reinterpret_cast<Node*>(h->scene->d_nodes.get());
  for (size_t l = 0; l + 1 < h->offsets.size(); l++) {
    const uint32_t n = h->offsets[l + 1] - h->offsets[l];
    if (!n) continue;
    hipLaunchKernelGGL(level_kernel<Node>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, nodes,
                       h->d_order.get() + h->offsets[l], n, h->d_prim_boxes.get(), h->d_node_boxes.get());
    RP_HIP(hipGetLastError());
  }
  return RP_OK;
}

}  // namespace rpf

namespace {

template <class Node>
const char* plan_of(const std::vector<uint8_t>& nodes, const rp_scene* s, rpf::Plan& pl) {
  return rpf::plan_nodes(reinterpret_cast<const Node*>(nodes.data()), s->n_nodes, s->ks.root, s->n_prims, pl);
}

}  // namespace

extern "C" {

int rp_refit_create(rp_scene* s, double coord_max, rp_refit** out) {
  static_assert(RP_REFIT_OUT_OF_BOUND == rpf::STATUS_OUT_OF_BOUND, "include/rp.h and rp_refit.h disagree");
  if (!out) return fail(RP_EINVAL, "out is NULL");
  *out = nullptr;
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  if (const char* why = rpf::check_format(s->ks.node_format)) return fail(RP_EINVAL, why);
  if (const char* why = rpf::check_coord_max(coord_max)) return fail(RP_EINVAL, why);
  const uint64_t node_bytes = s->ks.node_format == rpl::NODES_Q8 ? sizeof(rpl::Node4Q) : sizeof(rpl::Node4);
  if (node_bytes * s->n_nodes > s->d_nodes.capacity() || s->n_prims > s->d_prims.capacity() ||
      s->n_prims > s->d_prim_refs.capacity() || s->n_prims > s->d_tri_nrm.capacity() || s->n_prims > 0xFFFFFFFFull ||
      s->n_nodes > 0xFFFFFFFFull)
    return fail(RP_EINTERNAL, "rp_refit_create: the scene's counts exceed its buffers");
  DeviceGuard g(s->device);
  // the records as they lie in device memory (rp_tree_io.cpp)
  std::vector<uint8_t> nodes(node_bytes * s->n_nodes);
  std::vector<rpl::Prim> prims(s->n_prims);
  std::vector<rpl::PrimRef> refs(s->n_prims);
  if (!nodes.empty()) RP_HIP(hipMemcpy(nodes.data(), s->d_nodes.get(), nodes.size(), hipMemcpyDeviceToHost));
  if (s->n_prims) {
    RP_HIP(hipMemcpy(prims.data(), s->d_prims.get(), sizeof(rpl::Prim) * s->n_prims, hipMemcpyDeviceToHost));
    RP_HIP(hipMemcpy(refs.data(), s->d_prim_refs.get(), sizeof(rpl::PrimRef) * s->n_prims, hipMemcpyDeviceToHost));
  }
  rpf::Plan pl;
  const char* why = s->ks.node_format == rpl::NODES_Q8 ? plan_of<rpl::Node4Q>(nodes, s, pl) : plan_of<rpl::Node4>(nodes, s, pl);
  if (!why) why = rpf::plan_prims(prims.data(), refs.data(), s->n_prims, pl);
  if (why) return fail(RP_EINTERNAL, std::string("rp_refit_create: ") + why);
  // the meshes' concatenated vertices: the uv table holds 2 doubles per vertex and one spare pair (rp_scene.cpp)
  const uint64_t n_vertices = s->d_vuv.capacity() >= 2 ? (s->d_vuv.capacity() - 2) / 2 : 0;
  if (pl.min_vertices > n_vertices) return fail(RP_EINTERNAL, "rp_refit_create: a triangle names a vertex beyond the meshes'");

  Guarded<rp_refit> h(new rp_refit());
  h->device = s->device;
  h->scene = s;
  h->n_prims = s->n_prims, h->n_tris = pl.n_tris, h->n_spheres = pl.n_spheres, h->n_vertices = n_vertices;
  h->bound = std::fmax(coord_max, pl.amax);
  if (s->ks.node_format == rpl::NODES_Q8 && !(h->bound <= rpl::COORD_MAX))
    return fail(RP_EINVAL, "rp_refit_create: the scene's coordinates exceed the quantized frames' range");
  h->offsets = pl.offsets;
  if (!h->d_order.alloc(pl.order.size()) || !h->d_prim_boxes.alloc(s->n_prims) || !h->d_node_boxes.alloc(s->n_nodes) ||
      (pl.n_spheres && !h->d_sphere_rank.alloc(s->n_prims)))
    return fail(RP_ENOMEM, "hipMalloc refit plan and scratch");
  if (!pl.order.empty())
    RP_HIP(hipMemcpy(h->d_order.get(), pl.order.data(), sizeof(uint32_t) * pl.order.size(), hipMemcpyHostToDevice));
  if (pl.n_spheres)
    RP_HIP(hipMemcpy(h->d_sphere_rank.get(), pl.sphere_rank.data(), sizeof(uint32_t) * s->n_prims, hipMemcpyHostToDevice));
  // the slab slack of the quantized traversal covers every frame a refit within the bound can make; a wider slack only
  // widens a conservative test
  if (s->ks.node_format == rpl::NODES_Q8) s->ks.qbound = std::fmax(s->ks.qbound, rpl::qbound(h->bound));
  *out = h.release();
  return RP_OK;
}

void rp_refit_destroy(rp_refit* h) {
  if (h) Guarded<rp_refit> drop(h);
}

int rp_refit_info(const rp_refit* h, uint64_t* n_vertices, uint64_t* n_spheres, uint32_t* n_levels, double* bound) {
  if (!h) return fail(RP_EINVAL, "refit is NULL");
  if (n_vertices) *n_vertices = h->n_vertices;
  if (n_spheres) *n_spheres = h->n_spheres;
  if (n_levels) *n_levels = (uint32_t)h->offsets.size() - 1u;
  if (bound) *bound = h->bound;
  return RP_OK;
}

int rp_scene_refit_device(rp_refit* h, const double* d_positions, const double* d_normals, const double* d_spheres,
                          uint32_t* d_status, void* stream) {
  if (!h) return fail(RP_EINVAL, "refit is NULL");
  if (const char* why = rpf::check_update(h->n_tris, h->n_spheres, d_positions, d_normals, d_spheres, d_status))
    return fail(RP_EINVAL, why);
  DeviceGuard g(h->device);
  hipStream_t st = (hipStream_t)stream;
  rp_scene* s = h->scene;
  hipLaunchKernelGGL(rpf::zero_status_kernel, dim3(1), dim3(rpf::BLOCK), 0, st, d_status);
  RP_HIP(hipGetLastError());
  if (!h->n_prims) return RP_OK;
  const bool geom = d_positions || d_spheres;
  rpf::PrimArgs a;
  a.n = (uint32_t)h->n_prims;
  a.prims = s->d_prims.get(), a.refs = s->d_prim_refs.get(), a.tri_nrm = s->d_tri_nrm.get();
  a.sphere_rank = h->n_spheres ? h->d_sphere_rank.get() : nullptr;
  // a scene without triangles reads no position, one without spheres no sphere
  a.positions = geom && h->n_tris ? d_positions : nullptr;
  a.spheres = geom && h->n_spheres ? d_spheres : nullptr;
  a.normals = h->n_tris ? d_normals : nullptr;
  a.prim_boxes = h->d_prim_boxes.get();
  a.bound = h->bound;
  a.status = d_status;
  if (!a.positions && !a.spheres && !a.normals) return RP_OK;
  hipLaunchKernelGGL(rpf::prim_kernel, dim3((a.n + rpf::BLOCK - 1) / rpf::BLOCK), dim3(rpf::BLOCK), 0, st, a);
  RP_HIP(hipGetLastError());
  if (!geom) return RP_OK;  // normals alone: no box moves
  return s->ks.node_format == rpl::NODES_Q8 ? rpf::launch_levels<rpl::Node4Q>(h, st) : rpf::launch_levels<rpl::Node4>(h, st);
}

int rp_scene_refit(rp_refit* h, const double* positions, const double* normals, const double* spheres, uint32_t* status,
                   double* seconds) {
  if (!h) return fail(RP_EINVAL, "refit is NULL");
  if (const char* why = rpf::check_update(h->n_tris, h->n_spheres, positions, normals, spheres, status))
    return fail(RP_EINVAL, why);
  DeviceGuard g(h->device);
  DevBuf<double> d_pos, d_nrm, d_sph;
  DevBuf<uint32_t> d_st;
  if ((positions && !d_pos.alloc(3 * h->n_vertices)) || (normals && !d_nrm.alloc(3 * h->n_vertices)) ||
      (spheres && !d_sph.alloc(4 * h->n_spheres)) || !d_st.alloc(1))
    return fail(RP_ENOMEM, "hipMalloc refit inputs");
  if (positions && h->n_vertices) RP_HIP(hipMemcpy(d_pos.get(), positions, 24 * h->n_vertices, hipMemcpyHostToDevice));
  if (normals && h->n_vertices) RP_HIP(hipMemcpy(d_nrm.get(), normals, 24 * h->n_vertices, hipMemcpyHostToDevice));
  if (spheres && h->n_spheres) RP_HIP(hipMemcpy(d_sph.get(), spheres, 32 * h->n_spheres, hipMemcpyHostToDevice));
  double sec = 0.0;
  const int rc = rpp::sync_call(h->device, "refit", &sec, [&](void* st) {
    return rp_scene_refit_device(h, positions ? d_pos.get() : nullptr, normals ? d_nrm.get() : nullptr,
                                 spheres ? d_sph.get() : nullptr, d_st.get(), st);
  });
  if (rc) return rc;
  RP_HIP(hipMemcpy(status, d_st.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (seconds) *seconds = sec;
  return RP_OK;
}

}  // extern "C"
