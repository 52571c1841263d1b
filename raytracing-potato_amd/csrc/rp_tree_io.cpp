// rp_tree_io.cpp -- rp_scene_tree (include/rp.h): a scene's packed acceleration structure copied back to the host, so
// the tests can compare the device builders' trees with a written-out reference (tests/bvh_ref.py) record by record.
//
// A test hook: three copies and their size checks.  A translation unit of its own, linked into both libraries and not an
// argument of build_id.sh -- it reads a finished tree and decides no ray, so the id and the profile records that carry
// it stay.
#include "rp_state.h"

namespace {

uint64_t node_record_bytes(uint32_t node_format) {
  return node_format == rpl::NODES_W8 ? sizeof(rpl::Node8Q) : node_format == rpl::NODES_Q8 ? sizeof(rpl::Node4Q) : sizeof(rpl::Node4);
}

// `need` bytes of `what` from src into dst (NULL: not asked for), which holds `have`
int copy_out(const char* what, void* dst, uint64_t have, const void* src, uint64_t need) {
  if (!dst) return RP_OK;
  if (have < need)
    return fail(RP_EINVAL, std::string("rp_scene_tree: ") + what + " buffer of " + std::to_string(have) + " bytes, the tree's take " +
                               std::to_string(need));
  if (need) RP_HIP(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return RP_OK;
}

}  // namespace

extern "C" int rp_scene_tree(const rp_scene* s, void* nodes, uint64_t node_bytes, void* prims, uint64_t prim_bytes,
                             void* prim_refs, uint64_t ref_bytes, uint32_t* node_format, uint32_t* root) {
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  if (node_format) *node_format = s->ks.node_format;
  if (root) *root = s->ks.root;
  // every size is checked before anything is copied: a refused call writes nothing
  const uint64_t need[3] = {node_record_bytes(s->ks.node_format) * s->n_nodes, sizeof(rpl::Prim) * s->n_prims,
                            sizeof(rpl::PrimRef) * s->n_prims};
  if (need[0] > s->d_nodes.capacity() || s->n_prims > s->d_prims.capacity() || s->n_prims > s->d_prim_refs.capacity())
    return fail(RP_EINTERNAL, "rp_scene_tree: the scene's counts exceed its buffers");
  const uint64_t have[3] = {node_bytes, prim_bytes, ref_bytes};
  void* const dst[3] = {nodes, prims, prim_refs};
  const void* const src[3] = {s->d_nodes.get(), s->d_prims.get(), s->d_prim_refs.get()};
  static const char* const what[3] = {"node", "primitive", "primitive reference"};
  for (int k = 0; k < 3; k++)
    if (dst[k] && have[k] < need[k]) return copy_out(what[k], dst[k], have[k], src[k], need[k]);
  DeviceGuard g(s->device);
  for (int k = 0; k < 3; k++)
    if (const int rc = copy_out(what[k], dst[k], have[k], src[k], need[k])) return rc;
  return RP_OK;
}
