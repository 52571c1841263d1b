// rp_scene.cpp -- the scene side of the C-ABI in include/rp.h (librp.so).
//
// Host side of the drop-in: validates the reference-shaped scene (rp_scene_desc mirrors hittable.rs,
// mesh.rs, material.rs, texture.rs), builds the acceleration structure (rp_bvh.cpp / rp_bvh_gpu.hip) and
// copies it to HBM once.  rp_render.cpp launches the persistent render kernel (rp_kernel.hip) per frame / shard, and
// rp_gather.cpp assembles multi-GPU frames with one RCCL all-gather over xGMI.  The library reads no
// environment variables: every knob is an argument (rp_scene_options, rp_render_params).
#include <chrono>
#include <cmath>

#include "rp_bvh.h"
#include "rp_state.h"

static_assert(rpk::CTR_N == RP_COUNTERS_LEN, "kernel counter block = the ABI's");
static_assert(rpk::CTR_RAYS == RP_CTR_RAYS && rpk::CTR_STATUS == RP_CTR_STATUS, "counter order");
static_assert(rpk::STATUS_STACK_OVERFLOW == RP_STATUS_STACK_OVERFLOW && rpk::STATUS_PLAN_MISMATCH == RP_STATUS_PLAN_MISMATCH,
              "status bits");
static_assert(sizeof(rp_render_params) == 48, "rp_render_params layout (bindings mirror it)");

__attribute__((visibility("hidden"))) thread_local std::string g_err;

namespace {

// v's records into a fresh buffer of U (U = T, or bytes).
template <class T, class U>
int upload(const std::vector<T>& v, DevBuf<U>& out) {
  hipError_t e;
  if (!out.alloc((v.empty() ? 1 : v.size()) * (sizeof(T) / sizeof(U)), &e))
    return fail(RP_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  if (!v.empty()) {
    e = hipMemcpy(out.get(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(RP_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  return RP_OK;
}

// Defaults of rp_scene_options (the measured best).
constexpr uint32_t DEF_MAX_LEAF = 4, DEF_TRAV_THRESHOLD = 24, DEF_ALWAYS_MAX = 4;
constexpr double DEF_COST_TRAVERSE = 0.7;

// to_srgb_u8's byte for one channel (utility.rs:212-216), in the host libm: the reference's arithmetic
// (Rust's f64::powf is the platform pow).  Same expression as rph_to_srgb_u8 (rp_host_assets.cpp).
uint32_t srgb_byte(double x) {
  if (x < 0.0) x = 0.0;
  if (x > 1.0) x = 1.0;
  const double y = 255.0 * std::pow(x, 1.0 / 2.2);
  return !(y > 0.0) ? 0u : (y >= 255.0 ? 255u : (uint32_t)y);
}

rp_scene_options default_options() {
  rp_scene_options o{};
  o.builder = RP_BUILDER_AUTO;
  o.max_leaf = DEF_MAX_LEAF;
  o.cost_traverse = DEF_COST_TRAVERSE;
  o.always_max = (int32_t)DEF_ALWAYS_MAX;
  o.lds_depth = 0;
  o.self_check = 0;
  o.trav_threshold = 0;  // auto (scene_create): DEF_TRAV_THRESHOLD, or 32 for scenes past the Infinity Cache
  o.tile_order = 0;
  o.probe_n = rpk::PROBE_LATTICE_N;
  o.debug_stack_depth = 0;
  return o;
}

// Zero fields -> defaults; range checks.
int resolve_options(const rp_scene_options* in, rp_scene_options& o) {
  const rp_scene_options d = default_options();
  o = in ? *in : d;
  if (o.builder > RP_BUILDER_PLOC) return fail(RP_EINVAL, "options.builder must be RP_BUILDER_*");
  if (o.max_leaf == 0) o.max_leaf = d.max_leaf;
  if (o.max_leaf > rpl::LEAF_MAX) return fail(RP_EINVAL, "options.max_leaf must be 1..8");
  if (o.cost_traverse == 0.0) o.cost_traverse = d.cost_traverse;
  if (!(o.cost_traverse > 0.0) || !std::isfinite(o.cost_traverse)) return fail(RP_EINVAL, "options.cost_traverse must be > 0");
  if (o.always_max < 0) o.always_max = d.always_max;
  if (o.lds_depth != 0 && o.lds_depth < 8) return fail(RP_EINVAL, "options.lds_depth must be 0 or >= 8");
  if (o.trav_threshold > 64) return fail(RP_EINVAL, "options.trav_threshold must be 1..64");
  if (o.tile_order > RP_TILES_PROBE) return fail(RP_EINVAL, "options.tile_order must be RP_TILES_*");
  if (o.probe_n == 0) o.probe_n = d.probe_n;
  if (o.node_format > RP_NODES_W8) return fail(RP_EINVAL, "options.node_format must be RP_NODES_*");
  if (o.leaf_break > 64) return fail(RP_EINVAL, "options.leaf_break must be 0..64");
  if (o.unit_queues > RP_QUEUES_XCD_REGIONS) return fail(RP_EINVAL, "options.unit_queues must be RP_QUEUES_*");
  if (o.queue_chunk > 4096) return fail(RP_EINVAL, "options.queue_chunk must be 0..4096");
  if (o.debug_stack_depth != 0 && (o.debug_stack_depth < 8 || o.debug_stack_depth > 4096))
    return fail(RP_EINVAL, "options.debug_stack_depth must be 0 or 8..4096");
  if (o.collapse > RP_COLLAPSE_SAH) return fail(RP_EINVAL, "options.collapse must be RP_COLLAPSE_*");
  if (o.node_layout > RP_LAYOUT_DFS_LINE) return fail(RP_EINVAL, "options.node_layout must be RP_LAYOUT_*");
  if (o.unit_order > RP_UNITS_LEARNED) return fail(RP_EINVAL, "options.unit_order must be RP_UNITS_*");
  return RP_OK;
}

size_t rp_node_bytes(uint32_t node_format) {
  return node_format == rpl::NODES_W8 ? sizeof(rpl::Node8Q) : node_format == rpl::NODES_Q8 ? sizeof(rpl::Node4Q) : sizeof(rpl::Node4);
}

}  // namespace

// thr[k] = the smallest double x in [0, 1] with srgb_byte(x) >= k (bisection over the bit patterns of
// non-negative doubles, which order like their values); computed once.
const rpk::SrgbTable& srgb_table() {
  static const rpk::SrgbTable tab = [] {
    rpk::SrgbTable t{};
    t.thr[0] = -HUGE_VAL;
    for (uint32_t k = 1; k < 256; k++) {
      uint64_t lo = 0, hi = 0x3FF0000000000000ull;  // srgb_byte(0) = 0 < k <= 255 = srgb_byte(1)
      while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double x;
        std::memcpy(&x, &mid, sizeof x);
        if (srgb_byte(x) >= k) hi = mid;
        else lo = mid;
      }
      std::memcpy(&t.thr[k], &hi, sizeof hi);
    }
    return t;
  }();
  return tab;
}

int scene_create(const rp_scene_desc* desc, int device, const rp_scene_options* opt_in, rp_scene** out) {
  if (!out) return fail(RP_EINVAL, "out is NULL");
  *out = nullptr;
  rp_scene_options opt;
  int rc = resolve_options(opt_in, opt);
  if (rc) return rc;
  std::string err;
  const auto t_start = std::chrono::steady_clock::now();
  auto lap = [t = t_start]() mutable {
    const auto now = std::chrono::steady_clock::now();
    const double d = std::chrono::duration<double>(now - t).count();
    t = now;
    return d;
  };
  double phase[RP_BUILD_PHASES] = {0};
  rc = rpb::validate(desc, err);
  if (rc != RP_OK) return fail(rc, err);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RP_ENODEV, "no HIP device");
  if (device < 0 || device >= ndev) return fail(RP_EINVAL, "device index out of range");
  hipDeviceProp_t prop;
  RP_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(RP_ENODEV, std::string("librp.so is built for gfx950, device is ") + prop.gcnArchName);

  rpb::PackedScene ps;
  rpb::BuildOptions bo;
  // AUTO = the device PLOC build for scenes of >= 2^21 hittables (C5, 10 M triangles: its tree renders within
  // 1.5 % of the host binned SAH's and builds in a fraction of the host's 2.7 s), the host binned
  // SAH below (small scenes build in milliseconds, and only the host keeps always-tested primitives out of the
  // tree) and for 8-wide nodes; the LBVH stays an option (fastest build, ~46 % slower tree on C5).
  if (opt.builder == RP_BUILDER_AUTO && desc->n_hittables >= rpb::Q8_MIN_PRIMS && opt.node_format != RP_NODES_W8)
    opt.builder = RP_BUILDER_PLOC;
  const bool gpu_build = opt.builder == RP_BUILDER_DEVICE || opt.builder == RP_BUILDER_PLOC;
  const bool use_gpu = gpu_build && desc->n_hittables >= 2;  // the LBVH needs two primitives
  if (gpu_build && opt.node_format == RP_NODES_W8)
    return fail(RP_EINVAL, "the device builder makes 4-wide trees (options.node_format RP_NODES_F32 or RP_NODES_Q8)");
  bo.tables_only = use_gpu;
  bo.vertex_tables = false;  // uploaded straight from the meshes below
  bo.max_leaf = opt.max_leaf;
  bo.cost_traverse = opt.cost_traverse;
  bo.always_max = (uint32_t)opt.always_max;
  bo.always_minor = true;  // a mesh scene's few spheres are tested once per ray, not in divergent leaves (rp_bvh.h)
  bo.collapse = opt.collapse == RP_COLLAPSE_GREEDY ? rpb::COLLAPSE_GREEDY : rpb::COLLAPSE_SAH;
  bo.node_format = opt.node_format;  // RP_NODES_AUTO (0) resolved by the builder
  phase[0] = lap();
  rc = rpb::build(desc, bo, ps, err);
  if (rc != RP_OK) return fail(rc, err);
  phase[1] = lap();

  DeviceGuard g(device);
  Guarded<rp_scene> s(new rp_scene());  // every return below releases what the scene holds by then
  s->device = device;
  s->opt = opt;
  s->num_cu = prop.multiProcessorCount;
  uint64_t n_tree_nodes = ps.n_nodes(), n_tree_prims = ps.prims.size();
  uint32_t node_format = ps.node_format;
  if (use_gpu) {
    rpb::PrimInput pin;
    if ((rc = rpb::prim_input(desc, pin, err))) return fail(rc, err);
    phase[2] = lap();
    // AUTO: f32 for the LBVH (rp_bvh.h); the PLOC tree has the SAH tree's node count, so the host trees' size rule
    node_format = opt.node_format ? opt.node_format
                  : opt.builder == RP_BUILDER_PLOC ? rpb::auto_node_format(desc->n_hittables, pin.amax)
                                                   : (uint32_t)rpl::NODES_F32;
    rpg::GpuTree gt;
    const uint32_t algo = opt.builder == RP_BUILDER_PLOC ? rpg::GPU_PLOC : rpg::GPU_LBVH;
    // node families on 128-B lines (RP_LAYOUT_DFS_LINE) for 64-B quantized nodes; f32 nodes are a line each
    const uint32_t align = opt.node_layout == RP_LAYOUT_DFS_LINE && node_format == rpl::NODES_Q8 ? 2u : 1u;
    if ((rc = rpg::build_gpu(pin, opt.max_leaf, node_format, algo, opt.cost_traverse, align, gt, err)))
      return fail(rc, err);
    n_tree_nodes = gt.n_nodes;
    n_tree_prims = pin.prims.size();
    s->d_nodes.adopt(static_cast<uint8_t*>(gt.d_nodes), rp_node_bytes(node_format) * n_tree_nodes);
    s->d_prims.adopt(gt.d_prims, n_tree_prims);
    s->d_prim_refs.adopt(gt.d_prim_refs, n_tree_prims);
    // the per-primitive normals: the meshes' normals go up mesh after mesh, one gather fills the table (leaf order is
    // known only now), and the vertex table is freed again -- no kernel reads it
    {
      DevBuf<double> d_vnrm;
      uint64_t n_vert = 0;
      for (uint32_t i = 0; i < desc->n_meshes; i++) n_vert += desc->meshes[i].n_vertices;
      if (!d_vnrm.alloc(3 * n_vert + 3)) return fail(RP_ENOMEM, "hipMalloc vertex normals");
      for (uint64_t i = 0, vb = 0; i < desc->n_meshes; vb += desc->meshes[i].n_vertices, i++) {
        const rp_mesh& m = desc->meshes[i];
        if (m.n_vertices) RP_HIP(hipMemcpy(d_vnrm.get() + 3 * vb, m.normals, sizeof(double) * 3 * m.n_vertices, hipMemcpyHostToDevice));
      }
      if ((rc = rpg::gather_tri_normals(gt, n_tree_prims, d_vnrm.get(), err))) return fail(rc, err);
      s->d_tri_nrm.adopt(gt.d_tri_nrm, n_tree_prims);
    }
    ps.root = 0;
    ps.max_depth = gt.max_depth;
    ps.n_leaves = gt.n_leaves;
    ps.qbound = gt.qbound;
    ps.node_format = node_format;
    if (opt.self_check) {
      // the structural self-check of the host builder on the device-built tree (tests)
      rpb::PackedScene chk;
      chk.node_format = node_format;
      void* host_nodes;
      if (node_format == rpl::NODES_Q8) {
        chk.qnodes.resize(n_tree_nodes);
        host_nodes = chk.qnodes.data();
      } else {
        chk.nodes.resize(n_tree_nodes);
        host_nodes = chk.nodes.data();
      }
      chk.prims.resize(n_tree_prims);
      chk.prim_refs.resize(n_tree_prims);
      RP_HIP(hipMemcpy(host_nodes, s->d_nodes.get(), rp_node_bytes(node_format) * n_tree_nodes, hipMemcpyDeviceToHost));
      RP_HIP(hipMemcpy(chk.prims.data(), s->d_prims.get(), sizeof(rpl::Prim) * n_tree_prims, hipMemcpyDeviceToHost));
      RP_HIP(hipMemcpy(chk.prim_refs.data(), s->d_prim_refs.get(), sizeof(rpl::PrimRef) * n_tree_prims, hipMemcpyDeviceToHost));
      chk.root = 0;
      chk.max_depth = gt.max_depth;
      chk.n_leaves = gt.n_leaves;
      chk.qbound = gt.qbound;
      if ((rc = rpb::check(chk, err))) return fail(rc, "device BVH self-check: " + err);
    }
  } else if ((rc = node_format == rpl::NODES_W8   ? upload(ps.wnodes, s->d_nodes)
                   : node_format == rpl::NODES_Q8 ? upload(ps.qnodes, s->d_nodes)
                                                  : upload(ps.nodes, s->d_nodes)) ||
             (rc = upload(ps.prims, s->d_prims)) || (rc = upload(ps.prim_refs, s->d_prim_refs)) ||
             (rc = upload(ps.tri_nrm, s->d_tri_nrm))) {
    return rc;
  }
  phase[3] = lap();  // the device build, or the host tree's upload
  // vertex uvs (read at a closest hit on a textured mesh), mesh after mesh from the caller's arrays: no host copy.  The
  // vertex normals are on the device per primitive only (d_tri_nrm, above).
  uint64_t n_vert = 0;
  for (uint32_t i = 0; i < desc->n_meshes; i++) n_vert += desc->meshes[i].n_vertices;
  if (!s->d_vuv.alloc(2 * n_vert + 2)) return fail(RP_ENOMEM, "hipMalloc vertex tables");
  for (uint64_t i = 0, vb = 0; i < desc->n_meshes; vb += desc->meshes[i].n_vertices, i++) {
    const rp_mesh& m = desc->meshes[i];
    if (!m.n_vertices) continue;
    if (hipMemcpy(s->d_vuv.get() + 2 * vb, m.uvs, sizeof(double) * 2 * m.n_vertices, hipMemcpyHostToDevice) != hipSuccess)
      return fail(RP_EHIP, "vertex table upload");
  }
  if ((rc = upload(ps.materials, s->d_mats)) || (rc = upload(ps.textures, s->d_texs)) || (rc = upload(ps.texels, s->d_texels)))
    return rc;
  if (!s->d_diag.alloc(rpk::DIAG_N) || hipMemset(s->d_diag.get(), 0, sizeof(uint64_t) * rpk::DIAG_N) != hipSuccess)
    return fail(RP_ENOMEM, "hipMalloc diagnostics");
  s->ks.diag = s->d_diag.get();
  s->ks.nodes = s->d_nodes.get(), s->ks.prims = s->d_prims.get(), s->ks.prim_refs = s->d_prim_refs.get();
  s->ks.tri_nrm = s->d_tri_nrm.get(), s->ks.vuv = s->d_vuv.get();
  s->ks.mats = s->d_mats.get(), s->ks.texs = s->d_texs.get(), s->ks.texels = s->d_texels.get();
  s->ks.background = ps.background;
  s->ks.root = ps.root;
  s->ks.always_first = ps.always_first;  // 0 / 0 for a device-built tree
  s->ks.n_always = ps.n_always;
  s->ks.qbound = ps.qbound;
  s->ks.node_format = node_format;
  // a wide node pushes at most 3 entries (its non-nearest hits) per level below the root; +3 spare
  // entries for the kernel's branchless push (rp_kernel.hip STACK_SLACK)
  s->ks.stack_depth = 3 * ps.max_depth + 4 + 3;
  // Node8Q: groups of two words, per level at most the rest of a node group and one primitive group
  if (node_format == rpl::NODES_W8) s->ks.stack_depth = 4 * (ps.max_depth + 1) + 3;
  // floor of 17 entries: the spill split below never keeps fewer in LDS (options.lds_depth tests force 17)
  if (s->ks.stack_depth < 17) s->ks.stack_depth = 17;
  // test-only: a stack too small for the tree (the kernels flag RP_STATUS_STACK_OVERFLOW, never write past it)
  const bool debug_stack = opt.debug_stack_depth != 0;
  if (debug_stack) s->ks.stack_depth = opt.debug_stack_depth;
  s->n_nodes = n_tree_nodes;
  s->n_leaves = ps.n_leaves;
  s->n_prims = desc->n_hittables;
  s->max_depth = ps.max_depth;
  s->device_bytes = rp_node_bytes(node_format) * n_tree_nodes + (sizeof(rpl::Prim) + sizeof(rpl::PrimRef) + sizeof(rpl::TriNormals)) * n_tree_prims +
                    sizeof(double) * 2 * n_vert + sizeof(rpl::Material) * ps.materials.size() +
                    sizeof(rpl::Texture) * ps.textures.size() + sizeof(uint32_t) * ps.texels.size();
  // Cost-ordered tiles for every scene: cache-resident scenes (C3: 11 MB) gain ~15 % from them (short frame tail);
  // past the 256 MB Infinity Cache (C5: 2.5 GB) the Z-order once won (one device-wide queue: cost order scattered the
  // tiles in flight, +7 %), but with per-XCD queues and costs learned from the previous frame the cost order is even
  // or better there too (round 4: C5 -0.8 % on one box, -7.5 % on another, where the Z-order ran 11 % slower than
  // usual).  MORTON stays an option, and with it the balanced plan's square tile blocks.
  s->tiles_auto = RP_TILES_COST;
  // the speculative-traversal exit: C3 246.3 ms at 8 (3: 248.2, 12: 248.5); C5 at 16 (per-XCD queues, ab34: 12 +0.4 %,
  // 20 +0.1 %, 24 +0.7 %)
  s->ks.leaf_break = opt.leaf_break ? opt.leaf_break : (s->device_bytes > (256ull << 20) ? 16u : 8u);
  // lanes still traversing before the finished ones shade: C3 24 (16: +0.2 %, 32: +0.7 %), C5 32 (-1.6 %)
  if (s->opt.trav_threshold == 0) s->opt.trav_threshold = s->device_bytes > (256ull << 20) ? 32u : DEF_TRAV_THRESHOLD;
  // LDS holds the whole stack unless that costs resident blocks: then the deepest entries spill to a
  // per-lane global run (rp_kernel.hip stk_put/stk_get) and LDS keeps the largest depth that still fits
  // the occupancy of a shallow stack (C5's 43-entry stack: 3 -> 4 blocks per CU).  options.lds_depth
  // forces a depth (>= 17) for tests and tuning.
  s->ks.lds_depth = s->ks.stack_depth;
  int bpc = 0;
  if (rpk::render_blocks_per_cu(s->ks.stack_depth, false, node_format, &bpc) != 0 || bpc < 1) bpc = 1;
  int bpc_spill = 0;
  if (!debug_stack && rpk::render_blocks_per_cu(17, true, node_format, &bpc_spill) == 0 && bpc_spill > bpc) {
    uint32_t L = s->ks.stack_depth - 1;
    int b = 0;
    while (L > 17 && (rpk::render_blocks_per_cu(L, true, node_format, &b) != 0 || b < bpc_spill)) L--;
    s->ks.lds_depth = L;
    bpc = bpc_spill;
  }
  if (!debug_stack && opt.lds_depth && opt.lds_depth < s->ks.stack_depth) {
    s->ks.lds_depth = opt.lds_depth;
    if (rpk::render_blocks_per_cu(opt.lds_depth, true, node_format, &bpc) != 0 || bpc < 1) bpc = 1;
  }
  s->blocks_per_cu = bpc;
  phase[4] = lap();
  if ((rc = ws_alloc(s.get(), &s->ws0))) return rc;
  phase[5] = lap();
  std::memcpy(s->build_s, phase, sizeof phase);
  *out = s.release();
  return RP_OK;
}

extern "C" {

int rp_abi_version(void) { return RP_ABI_VERSION; }

const char* rp_last_error(void) { return g_err.c_str(); }

int rp_srgb_thresholds(double* out) {
  if (!out) return fail(RP_EINVAL, "out is NULL");
  std::memcpy(out, srgb_table().thr, sizeof(double) * 256);
  return RP_OK;
}

int rp_device_count(int* count) {
  if (!count) return fail(RP_EINVAL, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(RP_ENODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return RP_OK;
}

void rp_scene_destroy(rp_scene* s) { Guarded<rp_scene>{s}; }

int rp_scene_options_init(rp_scene_options* opt) {
  if (!opt) return fail(RP_EINVAL, "opt is NULL");
  *opt = default_options();
  return RP_OK;
}

int rp_scene_create_ex(const rp_scene_desc* desc, int device, const rp_scene_options* opt, rp_scene** out) {
  return scene_create(desc, device, opt, out);
}

int rp_scene_create(const rp_scene_desc* desc, int device, rp_scene** out) {
  return scene_create(desc, device, nullptr, out);
}

int rp_scene_build_times(const rp_scene* s, double* seconds, uint32_t n) {
  if (!s || (!seconds && n)) return fail(RP_EINVAL, "NULL argument");
  for (uint32_t i = 0; i < n; i++) seconds[i] = i < (uint32_t)RP_BUILD_PHASES ? s->build_s[i] : 0.0;
  return RP_OK;
}

int rp_scene_info(const rp_scene* s, uint64_t* n_nodes, uint64_t* n_leaves, uint32_t* max_depth, uint64_t* n_prims,
                  uint64_t* device_bytes) {
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  if (n_nodes) *n_nodes = s->n_nodes;
  if (n_leaves) *n_leaves = s->n_leaves;
  if (max_depth) *max_depth = s->max_depth;
  if (n_prims) *n_prims = s->n_prims;
  if (device_bytes) *device_bytes = s->device_bytes;
  return RP_OK;
}

int rp_diagnostics(rp_scene* s, uint64_t* out, uint32_t n, int reset) {
  if (!s || (!out && n)) return fail(RP_EINVAL, "NULL argument");
  DeviceGuard g(s->device);
  uint64_t buf[rpk::DIAG_N];
  RP_HIP(hipDeviceSynchronize());
  RP_HIP(hipMemcpy(buf, s->d_diag.get(), sizeof buf, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) out[i] = i < (uint32_t)rpk::DIAG_N ? buf[i] : 0;
  if (reset) RP_HIP(hipMemset(s->d_diag.get(), 0, sizeof buf));
  return RP_OK;
}

int rp_intersect(rp_scene* s, const double* rays, uint64_t n, double* out_hit, uint32_t* out_material) {
  if (!s || (n && (!rays || !out_hit || !out_material))) return fail(RP_EINVAL, "NULL argument");
  if (n == 0) return RP_OK;
  DeviceGuard g(s->device);
  DevBuf<double> d_rays, d_hit;
  DevBuf<uint32_t> d_mat;
  DevBuf<uint64_t> d_ctr;
  uint64_t ctr[rpk::CTR_N] = {0};
  if (!d_rays.alloc(8 * n) || !d_hit.alloc(9 * n) || !d_mat.alloc(n) || !d_ctr.alloc(rpk::CTR_N))
    return fail(RP_ENOMEM, "hipMalloc");
  if (hipMemcpy(d_rays.get(), rays, sizeof(double) * 8 * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_ctr.get(), 0, sizeof(uint64_t) * rpk::CTR_N) != hipSuccess)
    return fail(RP_EHIP, "hipMemcpy");
  RP_LAUNCH("intersect", rpk::launch_intersect(s->ks, d_rays.get(), n, d_hit.get(), d_mat.get(), d_ctr.get(), nullptr));
  hipError_t he = hipDeviceSynchronize();
  if (he != hipSuccess) return fail(RP_EHIP, std::string("intersect: ") + hipGetErrorString(he));
  if (hipMemcpy(out_hit, d_hit.get(), sizeof(double) * 9 * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(out_material, d_mat.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ctr, d_ctr.get(), sizeof ctr, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RP_EHIP, "copy back");
  if (ctr[rpk::CTR_STATUS] & rpk::STATUS_STACK_OVERFLOW) return fail(RP_EINTERNAL, "traversal stack overflow");
  return RP_OK;
}

}  // extern "C"
