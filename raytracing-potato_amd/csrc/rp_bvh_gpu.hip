// rp_bvh_gpu.hip -- acceleration-structure build on the device, for scenes whose
// host binned-SAH build (rp_bvh.cpp) would dominate setup (config C5: 10 M triangles).
//
// Replaces Bvh::new / make_bvh / split (bvh.rs:36-91) like the host builder does: the tree shape is not
// part of the contract, only the packed layout of rp_layout.h, which is identical, so
// the render and intersect kernels run unchanged.  Two builders make a binary tree over the primitives in Morton
// order, and one kernel collapses either tree into 4-wide nodes:
//   build_gpu   the prologue: the upload, a Morton code of each box centroid, a device radix sort (hipCUB);
//   build_lbvh  Karras 2012: 30-bit codes, key = code << 32 | primitive (unique keys); one thread per inner node finds
//               its key range and split (the binary radix tree); bottom-up f64 boxes: each leaf walks to the root, the
//               second arrival at a node unions its children's boxes (AABB::union's exact min/max, utility.rs:130-135);
//   build_ploc  Meister & Bittner 2018: 63-bit codes; mutual nearest neighbours under the SAH distance merge, round by
//               round, and every merge decides by the SAH whether its subtree becomes one leaf;
//   collapse    collapse_kernel<NF, Src>, one launch per level: a wide node takes its binary node's children and opens
//               the inner child of largest surface area until it has four (the host collapser's rule); child boxes
//               rounded outward to f32 or quantized in the node's frame.  Src is the binary tree: RadixSrc or PlocSrc;
//   last        the primitive records permuted into leaf order; the PLOC tree's nodes renumbered depth-first.
// Every device buffer is a DevBuf, freed on every path; build_gpu releases the three outputs to the caller on success.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <hipcub/hipcub.hpp>

#include <string>
#include <vector>

#include "rp_bvh.h"
#include "rp_hip_util.h"

namespace rpg {

namespace {

constexpr uint32_t BIN_LEAF = 0x80000000u;  // binary child reference: leaf (sorted position) vs inner node

struct Box6 {
  double lo[3], hi[3];
};

template <uint32_t NF>
using NodeOf = typename std::conditional<NF == rpl::NODES_Q8, rpl::Node4Q, rpl::Node4>::type;

// f(integral_constant<NF>) for the node format: the one place a format picks a kernel instantiation
template <class F>
void with_format(uint32_t node_format, F&& f) {
  if (node_format == rpl::NODES_Q8) f(std::integral_constant<uint32_t, rpl::NODES_Q8>{});
  else f(std::integral_constant<uint32_t, rpl::NODES_F32>{});
}

int failed(std::string& err, int code, const std::string& msg) {
  err = msg;
  return code;
}

// The file's one check: a failed HIP call (e) or launch ends the build with "<what>: <HIP's message>" in `err`.
#define RPG_CHECK(what)                                                                                          \
  do {                                                                                                           \
    if (e == hipSuccess) e = hipGetLastError();                                                                  \
    if (e != hipSuccess) return failed(err, RP_EHIP, std::string(what) + ": " + hipGetErrorString(e));           \
  } while (0)

// n elements for `buf` unless an earlier allocation of the chain failed already (e keeps the first failure)
template <class T>
void alloc(hipError_t& e, DevBuf<T>& buf, uint64_t n) {
  if (e == hipSuccess) buf.alloc(n, &e);
}

int alloc_failed(const char* build, hipError_t e, std::string& err) {
  return failed(err, RP_ENOMEM, std::string("hipMalloc (") + build + "): " + hipGetErrorString(e));
}

__device__ __forceinline__ uint32_t expand_bits10(uint32_t v) {  // 10 bits -> every third bit of 30
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

__global__ void morton_kernel(uint32_t n, const Box6* __restrict__ boxes, double3 cmin, double3 scale,
                              uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Box6 b = boxes[i];
  const double c[3] = {0.5 * (b.lo[0] + b.hi[0]), 0.5 * (b.lo[1] + b.hi[1]), 0.5 * (b.lo[2] + b.hi[2])};
  const double m[3] = {cmin.x, cmin.y, cmin.z}, s[3] = {scale.x, scale.y, scale.z};
  uint32_t code = 0;
  for (int k = 0; k < 3; k++) {
    double q = (c[k] - m[k]) * s[k];
    q = !(q >= 0.0) ? 0.0 : (q > 1023.0 ? 1023.0 : q);  // a NaN centroid (NaN geometry) sorts as 0
    code |= expand_bits10((uint32_t)q) << (2 - k);
  }
  keys[i] = ((uint64_t)code << 32) | i;
}

__device__ __forceinline__ uint64_t expand_bits21(uint64_t v) {  // 21 bits -> every third bit of 63
  v &= 0x1FFFFFull;
  v = (v | v << 32) & 0x1F00000000FFFFull;
  v = (v | v << 16) & 0x1F0000FF0000FFull;
  v = (v | v << 8) & 0x100F00F00F00F00Full;
  v = (v | v << 4) & 0x10C30C30C30C30C3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

// PLOC's order: 63-bit Morton codes (21 bits per axis; 10 M triangles share 30-bit codes ~10 to a cell), sorted
// with the primitive index as the value
__global__ void morton63_kernel(uint32_t n, const Box6* __restrict__ boxes, double3 cmin, double3 scale,
                                uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Box6 b = boxes[i];
  const double c[3] = {0.5 * (b.lo[0] + b.hi[0]), 0.5 * (b.lo[1] + b.hi[1]), 0.5 * (b.lo[2] + b.hi[2])};
  const double m[3] = {cmin.x, cmin.y, cmin.z}, s[3] = {scale.x, scale.y, scale.z};
  uint64_t code = 0;
  for (int k = 0; k < 3; k++) {
    double q = (c[k] - m[k]) * s[k] * 2048.0;  // scale maps the centroid range to [0, 1024]
    q = !(q >= 0.0) ? 0.0 : (q > 2097151.0 ? 2097151.0 : q);  // NaN centroid -> 0
    code |= expand_bits21((uint64_t)q) << (2 - k);
  }
  keys[i] = code;
  idx[i] = i;
}

__device__ __forceinline__ int delta(const uint64_t* keys, uint32_t n, int i, int j) {
  if (j < 0 || j >= (int)n) return -1;
  return __clzll(keys[i] ^ keys[j]);  // keys are unique: < 64
}

// Karras 2012, Fig. 4: inner node i of n - 1.  Children are inner nodes or leaves (sorted positions).
__global__ void radix_tree_kernel(uint32_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ left,
                                  uint32_t* __restrict__ right, uint32_t* __restrict__ parent_inner,
                                  uint32_t* __restrict__ parent_leaf, uint32_t* __restrict__ first,
                                  uint32_t* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int)n - 1) return;
  const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0;
  for (int div = 2;; div *= 2) {
    const int t = (l + div - 1) / div;
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int g = i + s * d + (d < 0 ? -1 : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  first[i] = (uint32_t)lo;
  last[i] = (uint32_t)hi;
  if (lo == g) {
    left[i] = BIN_LEAF | (uint32_t)g;
    parent_leaf[g] = (uint32_t)i;
  } else {
    left[i] = (uint32_t)g;
    parent_inner[g] = (uint32_t)i;
  }
  if (hi == g + 1) {
    right[i] = BIN_LEAF | (uint32_t)(g + 1);
    parent_leaf[g + 1] = (uint32_t)i;
  } else {
    right[i] = (uint32_t)(g + 1);
    parent_inner[g + 1] = (uint32_t)i;
  }
}

__device__ __forceinline__ double load_coherent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ Box6 child_box(uint32_t c, const Box6* leaf_boxes, const uint32_t* order,
                                         const Box6* node_boxes) {
  Box6 b;
  if (c & BIN_LEAF) {
    b = leaf_boxes[order[c & ~BIN_LEAF]];  // written before the build: plain loads
  } else {
    const double* p = node_boxes[c].lo;  // written by another thread of this launch
    for (int k = 0; k < 3; k++) {
      b.lo[k] = load_coherent(p + k);
      b.hi[k] = load_coherent(p + 3 + k);
    }
  }
  return b;
}

// Bottom-up boxes: the second thread to reach an inner node computes it (the first stops there).
__global__ void boxes_kernel(uint32_t n, const Box6* __restrict__ leaf_boxes, const uint32_t* __restrict__ order,
                             const uint32_t* __restrict__ left, const uint32_t* __restrict__ right,
                             const uint32_t* __restrict__ parent_inner, const uint32_t* __restrict__ parent_leaf,
                             Box6* node_boxes, uint32_t* visits) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  uint32_t p = parent_leaf[k];
  for (;;) {
    __threadfence();
    if (atomicAdd(&visits[p], 1u) == 0u) return;
    __threadfence();
    const Box6 a = child_box(left[p], leaf_boxes, order, node_boxes);
    const Box6 b = child_box(right[p], leaf_boxes, order, node_boxes);
    Box6 u;
    for (int c = 0; c < 3; c++) {
      u.lo[c] = fmin(a.lo[c], b.lo[c]);
      u.hi[c] = fmax(a.hi[c], b.hi[c]);
    }
    double* q = node_boxes[p].lo;
    for (int c = 0; c < 3; c++) {
      __hip_atomic_store(q + c, u.lo[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(q + 3 + c, u.hi[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (p == 0) return;
    p = parent_inner[p];
  }
}

__device__ __forceinline__ double area(const Box6& b) {  // rp_bvh.cpp Box::area
  const double dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  if (!(dx >= 0) || !(dy >= 0) || !(dz >= 0)) return 0.0;
  return 2.0 * (dx * dy + dy * dz + dz * dx);
}

__device__ __forceinline__ Box6 box_union(const Box6& a, const Box6& b) {
  Box6 u;
  for (int c = 0; c < 3; c++) {
    u.lo[c] = fmin(a.lo[c], b.lo[c]);
    u.hi[c] = fmax(a.hi[c], b.hi[c]);
  }
  return u;
}

// ---------------------------------------------------------------------------------------------------------------
// The wide collapse, for either binary tree.  A child reference c is BIN_LEAF | x (one primitive) or a binary inner
// node's id.  The tree is a Src (RadixSrc here, PlocSrc below), passed to the kernel by value.  It answers for a c:
// left(c) and right(c), an inner node's children; is_leaf(c), whether c becomes one leaf of the wide tree (never
// opened); count(c) and box(c), its primitives and their box; place_leaf(c, off), which puts a leaf child's primitives
// into the leaf order and returns the leaf entry's first index (off: the first primitive slot of c's subtree).
struct Frontier {
  uint32_t bin, wide, poff;  // binary inner node, its wide node, the first primitive slot of its subtree (PlocSrc)
};

// The LBVH's radix tree: arrays over the inner nodes, leaves are sorted positions.  A subtree of <= max_leaf primitives
// is a contiguous run of the sorted order, which is the leaf order already.
struct RadixSrc {
  static constexpr const char* stage = "collapse";
  static constexpr const char* build = "device BVH build";
  const uint32_t *__restrict__ lefts, *__restrict__ rights, *__restrict__ first, *__restrict__ last;
  const uint32_t* __restrict__ order;
  const Box6 *__restrict__ leaf_boxes, *__restrict__ node_boxes;
  uint32_t max_leaf;
  __device__ uint32_t left(uint32_t c) const { return lefts[c]; }
  __device__ uint32_t right(uint32_t c) const { return rights[c]; }
  __device__ uint32_t count(uint32_t c) const { return (c & BIN_LEAF) ? 1u : last[c] - first[c] + 1u; }
  __device__ bool is_leaf(uint32_t c) const { return count(c) <= max_leaf; }
  __device__ Box6 box(uint32_t c) const { return (c & BIN_LEAF) ? leaf_boxes[order[c & ~BIN_LEAF]] : node_boxes[c]; }
  __device__ uint32_t place_leaf(uint32_t c, uint32_t) const { return (c & BIN_LEAF) ? (c & ~BIN_LEAF) : first[c]; }
};

// One level of the collapse: every frontier entry fills its wide node and appends its inner wide children to the next
// frontier.
template <uint32_t NF, class Src>
__global__ void collapse_kernel(const Src src, const Frontier* __restrict__ cur, uint32_t n_cur,
                                Frontier* __restrict__ next,
                                uint32_t* __restrict__ counters /* [0] wide nodes, [1] next frontier, [2] leaves */,
                                void* __restrict__ nodes) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_cur) return;
  const Frontier f = cur[t];
  uint32_t kids[4] = {src.left(f.bin), src.right(f.bin), 0u, 0u};
  uint32_t nk = 2;
  while (nk < 4) {
    int best = -1;
    double best_area = -1.0;
    for (uint32_t k = 0; k < nk; k++) {
      const uint32_t c = kids[k];
      if (src.is_leaf(c)) continue;  // leaves are not opened
      const double a = area(src.box(c));
      if (a > best_area) {
        best_area = a;
        best = (int)k;
      }
    }
    if (best < 0) break;
    const uint32_t open = kids[best];
    kids[best] = src.left(open);
    kids[nk++] = src.right(open);
  }
  Box6 kb[4];
  Box6 nb;
  for (int a = 0; a < 3; a++) {
    nb.lo[a] = __builtin_huge_val();
    nb.hi[a] = -__builtin_huge_val();
  }
  for (uint32_t k = 0; k < nk; k++) {
    kb[k] = src.box(kids[k]);
    nb = box_union(nb, kb[k]);
  }
  // child boxes in the node format: f32 rounded outward, or quantized in the node's frame (rp_layout.h
  // qframe; rp_bvh.cpp node_frame / Collapser)
  NodeOf<NF> nd;
  if constexpr (NF == rpl::NODES_Q8) {
    for (int a = 0; a < 3; a++) {
      const bool ok = isfinite(nb.lo[a]) && isfinite(nb.hi[a]) && nb.lo[a] <= nb.hi[a];
      rpl::qframe(ok ? nb.lo[a] : 0.0, ok ? nb.hi[a] : 0.0, nd.o[a], nd.s[a]);
    }
  } else {
    for (int k = 0; k < 4; k++) nd.pad[k] = 0;
  }
  // the inner children's wide nodes are allocated as one consecutive family (rp_bvh.cpp Collapser)
  uint32_t n_inner = 0;
  for (uint32_t k = 0; k < nk; k++) n_inner += !src.is_leaf(kids[k]);
  uint32_t fam = n_inner ? atomicAdd(&counters[0], n_inner) : 0u;
  uint32_t off = f.poff;
  for (uint32_t k = 0; k < 4; k++) {
    if (k >= nk) {
      if constexpr (NF == rpl::NODES_Q8) rpl::empty_child(nd, (int)k);
      else rpl::f32_empty(nd, (int)k);
      nd.child[k] = rpl::ENTRY_EMPTY;
      continue;
    }
    const uint32_t c = kids[k];
    if constexpr (NF == rpl::NODES_Q8) rpl::quantize_child(nd, (int)k, kb[k].lo, kb[k].hi);
    else rpl::f32_child(nd, (int)k, kb[k].lo, kb[k].hi);
    const uint32_t cnt = src.count(c);
    if (src.is_leaf(c)) {
      nd.child[k] = rpl::ENTRY_LEAF | ((cnt - 1u) << rpl::LEAF_SHIFT) | src.place_leaf(c, off);
      atomicAdd(&counters[2], 1u);
    } else {
      const uint32_t w = fam++;
      nd.child[k] = w;
      next[atomicAdd(&counters[1], 1u)] = Frontier{c, w, off};
    }
    off += cnt;
  }
  reinterpret_cast<NodeOf<NF>*>(nodes)[f.wide] = nd;
}

__global__ void permute_kernel(uint32_t n, const uint32_t* __restrict__ order, const rpl::Prim* __restrict__ prims_in,
                               const rpl::PrimRef* __restrict__ refs_in, rpl::Prim* __restrict__ prims,
                               rpl::PrimRef* __restrict__ refs) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = order[k];
  prims[k] = prims_in[i];
  refs[k] = refs_in[i];
}

// The per-primitive normals of a finished tree (rp_layout.h TriNormals): primitive k's three vertex normals from the
// concatenated vertex table at its PrimRef's ids, zeros for a sphere -- the host builder's pack_tri_normals.
__global__ void tri_normals_kernel(uint32_t n, const rpl::Prim* __restrict__ prims, const rpl::PrimRef* __restrict__ refs,
                                   const double* __restrict__ vnrm, rpl::TriNormals* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  rpl::TriNormals t{};
  if (prims[k].kind == rpl::PRIM_TRIANGLE) {
    const rpl::PrimRef r = refs[k];
    rpl::tri_normals_fill(t, vnrm, r.v[0], r.v[1], r.v[2]);
  }
  out[k] = t;
}

__global__ void order_kernel(uint32_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ order) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) order[k] = (uint32_t)keys[k];
}

// kernel k over n threads, in blocks of B on the null stream
template <unsigned B = 256, class K, class... A>
void launch(K k, uint64_t n, A... a) {
  hipLaunchKernelGGL(k, dim3((unsigned)((n + B - 1) / B)), dim3(B), 0, nullptr, a...);
}

// ---------------------------------------------------------------------------------------------------------------
// Depth-first layout of a collapsed wide tree.  The level-by-level collapse numbers wide nodes by atomic family
// allocation, one level after another in no particular order, so a node and its children sit far apart; the host
// builder numbers them depth-first (a node's inner children as one consecutive family, each child's own subtree --
// its family first -- right behind the family, in child order), so a descent walks forward through memory.  The
// relayout: per level (the collapse's frontiers, recorded), bottom-up the number of wide nodes below each node, then
// top-down each node's new index and the start of its family, then every record copied to its new index with its
// inner child indices renamed.  Leaf entries and the primitive order are unchanged.  `align` (nodes): every family
// starts at a multiple of it -- 2 puts a 64-B quantized node's family on 128-B cache lines (RP_LAYOUT_DFS_LINE; the
// pad slots are zero and never referenced), 1 packs the families.
template <uint32_t NF>
__device__ __forceinline__ const uint32_t* node_children(const void* nodes, uint32_t i) {
  return reinterpret_cast<const NodeOf<NF>*>(nodes)[i].child;
}

__global__ void record_level_kernel(const uint32_t* __restrict__ wide_of, uint32_t stride_words, uint32_t n,
                                    uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ids[i] = wide_of[(uint64_t)i * stride_words];
}

template <uint32_t NF>
__global__ void subtree_count_kernel(const uint32_t* __restrict__ ids, uint32_t n, const void* __restrict__ nodes,
                                     uint32_t align, uint32_t* __restrict__ below) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = ids[i];
  const uint32_t* ch = node_children<NF>(nodes, u);
  uint32_t f = 0, m = 0;
  for (int k = 0; k < 4; k++)
    if (!(ch[k] & rpl::ENTRY_LEAF)) {
      m++;
      f += below[ch[k]];
    }
  below[u] = f + (m + align - 1) / align * align;  // the family (padded) and the children's own subtrees
}

template <uint32_t NF>
__global__ void dfs_index_kernel(const uint32_t* __restrict__ ids, uint32_t n, const void* __restrict__ nodes,
                                 const uint32_t* __restrict__ below, uint32_t align, uint32_t* __restrict__ newid,
                                 uint32_t* __restrict__ fam) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = ids[i];
  const uint32_t* ch = node_children<NF>(nodes, u);
  uint32_t m = 0;
  for (int k = 0; k < 4; k++) m += !(ch[k] & rpl::ENTRY_LEAF);
  uint32_t slot = fam[u], next = fam[u] + (m + align - 1) / align * align;
  for (int k = 0; k < 4; k++) {
    const uint32_t c = ch[k];
    if (c & rpl::ENTRY_LEAF) continue;
    newid[c] = slot++;
    fam[c] = next;
    next += below[c];
  }
}

template <uint32_t NF>
__global__ void relayout_kernel(uint32_t n, const void* __restrict__ nodes, const uint32_t* __restrict__ newid,
                                void* __restrict__ out) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  NodeOf<NF> nd = reinterpret_cast<const NodeOf<NF>*>(nodes)[u];
  for (int k = 0; k < 4; k++)
    if (!(nd.child[k] & rpl::ENTRY_LEAF)) nd.child[k] = newid[nd.child[k]];
  reinterpret_cast<NodeOf<NF>*>(out)[newid[u]] = nd;
}

// Every collapse level's wide node ids: level k at ids[off[k] .. off[k + 1]).
struct Levels {
  DevBuf<uint32_t> ids;
  std::vector<uint32_t> off{0};
};

// Renumber the n_nodes wide nodes of `nodes` depth-first (see above).  Replaces `nodes` and n_nodes.
int dfs_relayout(DevBuf<uint8_t>& nodes, uint32_t node_format, uint64_t& n_nodes, const Levels& lv, uint32_t align,
                 std::string& err) {
  const size_t nb = node_format == rpl::NODES_Q8 ? sizeof(rpl::Node4Q) : sizeof(rpl::Node4);
  const uint32_t L = (uint32_t)lv.off.size() - 1;
  const uint32_t* ids = lv.ids.get();
  DevBuf<uint32_t> below, newid, fam;
  DevBuf<uint8_t> out;
  hipError_t e = hipSuccess;
  alloc(e, below, n_nodes);
  alloc(e, newid, n_nodes);
  alloc(e, fam, n_nodes);
  RPG_CHECK("depth-first relayout");
  for (uint32_t k = L; k-- > 0;) {
    const uint32_t n = lv.off[k + 1] - lv.off[k];
    with_format(node_format, [&](auto nf) {
      launch(subtree_count_kernel<decltype(nf)::value>, n, ids + lv.off[k], n, nodes.get(), align, below.get());
    });
    RPG_CHECK("depth-first relayout");
  }
  const uint32_t root_new = 0, root_fam = align;  // the root, padded to the alignment, then its family
  uint32_t root = 0, below_root = 0;
  e = hipMemcpy(&root, ids, sizeof root, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&below_root, below.get() + root, sizeof below_root, hipMemcpyDeviceToHost);
  const uint64_t total = (uint64_t)root_fam + below_root;  // == n_nodes when align == 1
  alloc(e, out, nb * total);
  if (e == hipSuccess && total != n_nodes) e = hipMemset(out.get(), 0, nb * total);
  if (e == hipSuccess) e = hipMemcpy(newid.get() + root, &root_new, sizeof root_new, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(fam.get() + root, &root_fam, sizeof root_fam, hipMemcpyHostToDevice);
  RPG_CHECK("depth-first relayout");
  for (uint32_t k = 0; k < L; k++) {
    const uint32_t n = lv.off[k + 1] - lv.off[k];
    with_format(node_format, [&](auto nf) {
      launch(dfs_index_kernel<decltype(nf)::value>, n, ids + lv.off[k], n, nodes.get(), below.get(), align, newid.get(),
             fam.get());
    });
    RPG_CHECK("depth-first relayout");
  }
  with_format(node_format, [&](auto nf) {
    launch(relayout_kernel<decltype(nf)::value>, n_nodes, (uint32_t)n_nodes, nodes.get(), newid.get(), out.get());
  });
  RPG_CHECK("depth-first relayout");
  e = hipDeviceSynchronize();
  RPG_CHECK("depth-first relayout");
  nodes = std::move(out);  // the old buffer goes with `out`
  n_nodes = total;
  return RP_OK;
}

// The collapse of either binary tree, level by level from its root (-> wide node 0, primitives from slot 0) into
// `nodes`; fills out.n_nodes / n_leaves / max_depth.  `rec`: every level's wide node ids, for the depth-first relayout.
template <class Src>
int collapse_levels(const Src& src, uint32_t root, uint32_t n, uint32_t node_format, void* nodes, GpuTree& out, Levels* rec,
                    std::string& err) {
  DevBuf<Frontier> fa, fb;
  DevBuf<uint32_t> ctr;
  hipError_t e = hipSuccess;
  alloc(e, fa, n);
  alloc(e, fb, n);
  alloc(e, ctr, 4);
  if (rec) alloc(e, rec->ids, n);
  if (e != hipSuccess) return alloc_failed(Src::build, e, err);
  const Frontier first{root, 0u, 0u};
  const uint32_t ctr0[4] = {1u, 0u, 0u, 0u};  // wide node 0 taken
  e = hipMemcpy(fa.get(), &first, sizeof first, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ctr.get(), ctr0, sizeof ctr0, hipMemcpyHostToDevice);
  RPG_CHECK(std::string(Src::stage) + " setup");
  uint32_t n_cur = 1, depth = 0;
  for (;;) {
    e = hipMemset(ctr.get() + 1, 0, sizeof(uint32_t));
    RPG_CHECK(Src::stage);
    if (rec) {
      launch(record_level_kernel, n_cur, &fa.get()->wide, (uint32_t)(sizeof(Frontier) / 4), n_cur,
             rec->ids.get() + rec->off.back());
      rec->off.push_back(rec->off.back() + n_cur);
    }
    with_format(node_format, [&](auto nf) {
      launch(collapse_kernel<decltype(nf)::value, Src>, n_cur, src, fa.get(), n_cur, fb.get(), ctr.get(), nodes);
    });
    RPG_CHECK(Src::stage);
    uint32_t c[4];
    e = hipMemcpy(c, ctr.get(), sizeof c, hipMemcpyDeviceToHost);
    RPG_CHECK(Src::stage);
    if (c[0] > n) return failed(err, RP_EINTERNAL, std::string(Src::build) + ": wide node overflow");
    if (c[1] == 0) {
      out.n_nodes = c[0];
      out.n_leaves = c[2];
      out.max_depth = depth;
      return RP_OK;
    }
    depth++;
    n_cur = c[1];
    std::swap(fa, fb);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// PLOC (Meister & Bittner 2018, "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction"):
// the primitives in Morton order are the initial clusters; every round, each cluster finds its nearest neighbour
// within PLOC_R positions of the (Morton-ordered) cluster array under the SAH distance -- the surface area of the
// union of the two boxes -- and mutual nearest neighbours merge into a new binary node (at the lower position;
// the higher one is removed and the array compacted, order kept).  Agglomerative like a sweep-SAH build, so the
// tree is of SAH quality where the LBVH above splits by Morton bits.  Deterministic: distances tie-break on the
// pair's positions, merges take node ids from a prefix sum.
// Search radius: measured on C5's 10 M random triangles (32-spp frame over the q8 tree; host SAH tree 229.5 ms):
// r = 1: 234.1, 2: 233.2, 3: 232.8, 4: 235.4, 6: 240.9, 8: 258.7, 16: 255.3, 32: 300.8, 64: 312.1 ms.  (The paper's
// r = 16 merges more distant Morton neighbours early, which here makes deeper, costlier trees.)
constexpr int PLOC_R = 3;
constexpr int PLOC_B = 256;

struct PNode {
  uint32_t left, right, size, leaf;  // children (BIN_LEAF | primitive, or a node id); primitives below; 1 = the
                                     // subtree becomes one leaf of the wide tree (the SAH decision, ploc_apply)
};

__global__ void ploc_init_kernel(uint32_t n, const uint32_t* __restrict__ order, const Box6* __restrict__ boxes,
                                 uint32_t* __restrict__ ref, Box6* __restrict__ cbox, uint32_t* __restrict__ csize,
                                 double* __restrict__ ccost) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = order[i];
  ref[i] = BIN_LEAF | p;
  cbox[i] = boxes[p];
  csize[i] = 1u;
  ccost[i] = 1.0;  // one primitive test
}

// nearest neighbour of every cluster within PLOC_R positions: the boxes of the block's window in LDS
__global__ void __launch_bounds__(PLOC_B) ploc_nn_kernel(uint32_t m, const Box6* __restrict__ cbox, uint32_t* __restrict__ nn) {
  __shared__ Box6 win[PLOC_B + 2 * PLOC_R];
  const int base = (int)(blockIdx.x * PLOC_B) - PLOC_R;
  for (int t = threadIdx.x; t < PLOC_B + 2 * PLOC_R; t += PLOC_B) {
    const int g = base + t;
    if (g >= 0 && g < (int)m) win[t] = cbox[g];
  }
  __syncthreads();
  const int i = (int)(blockIdx.x * PLOC_B + threadIdx.x);
  if (i >= (int)m) return;
  const Box6 a = win[threadIdx.x + PLOC_R];
  double best = __builtin_huge_val();
  int bj = -1;
  const int lo = max(0, i - PLOC_R), hi = min((int)m - 1, i + PLOC_R);
  for (int j = lo; j <= hi; j++) {
    if (j == i) continue;
    double d = area(box_union(a, win[j - base]));
    if (d != d) d = __builtin_huge_val();
    // strict order on (distance, lower position, higher position): the global minimum pair is mutual, so every
    // round merges at least one pair; candidates are scanned in increasing j, so `<` keeps the smaller j on ties.
    // A NaN distance (NaN geometry: fmin/fmax keep a NaN when both operands are NaN) ranks as +inf, and a cluster
    // with no finite candidate takes its first one (if no pair is finite, clusters 0 and 1 pair up, so the round
    // still merges) -- never the -1 that ploc_flags_kernel would index with.
    if (d < best || bj < 0) {
      best = d;
      bj = j;
    }
  }
  nn[i] = (uint32_t)bj;
}

// flags: keep[i] (the cluster survives at its position: not merged, or the lower of a mutual pair) and merge[i]
__global__ void ploc_flags_kernel(uint32_t m, const uint32_t* __restrict__ nn, uint32_t* __restrict__ keep,
                                  uint32_t* __restrict__ merge) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t j = nn[i];
  const bool mutual = j < m && nn[j] == i;
  keep[i] = (!mutual || i < j) ? 1u : 0u;
  merge[i] = (mutual && i < j) ? 1u : 0u;
}

__global__ void ploc_apply_kernel(uint32_t m, const uint32_t* __restrict__ nn, const uint32_t* __restrict__ keep,
                                  const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ merge,
                                  const uint32_t* __restrict__ mrank, uint32_t node_base, const uint32_t* __restrict__ ref,
                                  const Box6* __restrict__ cbox, const uint32_t* __restrict__ csize,
                                  const double* __restrict__ ccost, uint32_t* __restrict__ ref2, Box6* __restrict__ cbox2,
                                  uint32_t* __restrict__ csize2, double* __restrict__ ccost2, PNode* __restrict__ nodes,
                                  Box6* __restrict__ nbox, uint32_t max_leaf, double cost_traverse) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || !keep[i]) return;
  const uint32_t o = kpos[i];
  if (merge[i]) {
    const uint32_t j = nn[i], id = node_base + mrank[i];
    const Box6 u = box_union(cbox[i], cbox[j]);
    const uint32_t sz = csize[i] + csize[j];
    // SAH, bottom-up (the expected primitive-test cost of a ray entering the box, node visits at cost_traverse):
    // a subtree of <= max_leaf primitives becomes one leaf when testing them all is cheaper than splitting
    const double au = area(u);
    const double split = cost_traverse + (au > 0.0 ? (area(cbox[i]) * ccost[i] + area(cbox[j]) * ccost[j]) / au
                                                    : 0.5 * (ccost[i] + ccost[j]));
    const bool leaf = sz <= max_leaf && (double)sz <= split;
    PNode nd;
    nd.left = ref[i];
    nd.right = ref[j];
    nd.size = sz;
    nd.leaf = leaf ? 1u : 0u;
    nodes[id] = nd;
    nbox[id] = u;
    ref2[o] = id;
    cbox2[o] = u;
    csize2[o] = sz;
    ccost2[o] = leaf ? (double)sz : split;
  } else {
    ref2[o] = ref[i];
    cbox2[o] = cbox[i];
    csize2[o] = csize[i];
    ccost2[o] = ccost[i];
  }
}

// The PLOC tree as collapse_kernel's source: a leaf is where the SAH said so, and the primitives are laid out
// depth-first as the frontier descends -- each child subtree takes the next run of primitive slots, and a leaf child
// writes its primitives' ids into perm there.
struct PlocSrc {
  static constexpr const char* stage = "PLOC collapse";
  static constexpr const char* build = "PLOC build";
  const PNode* __restrict__ nodes;
  const Box6 *__restrict__ prim_boxes, *__restrict__ nbox;
  uint32_t* __restrict__ perm;
  __device__ uint32_t left(uint32_t c) const { return nodes[c].left; }
  __device__ uint32_t right(uint32_t c) const { return nodes[c].right; }
  __device__ uint32_t count(uint32_t c) const { return (c & BIN_LEAF) ? 1u : nodes[c].size; }
  __device__ bool is_leaf(uint32_t c) const { return (c & BIN_LEAF) || nodes[c].leaf; }
  __device__ Box6 box(uint32_t c) const { return (c & BIN_LEAF) ? prim_boxes[c & ~BIN_LEAF] : nbox[c]; }
  // the subtree's primitives (<= max_leaf <= 8: a binary subtree of <= 7 inner nodes) into perm[off ...]
  __device__ uint32_t place_leaf(uint32_t c, uint32_t off) const {
    uint32_t stk[8], sp = 0, w = off;
    stk[sp++] = c;
    while (sp) {
      const uint32_t x = stk[--sp];
      if (x & BIN_LEAF) {
        perm[w++] = x & ~BIN_LEAF;
      } else {
        stk[sp++] = nodes[x].right;
        stk[sp++] = nodes[x].left;
      }
    }
    return off;
  }
};


// What the common prologue leaves on the device: the input in hittable order and its Morton order.
struct Sorted {
  uint32_t n = 0;
  DevBuf<Box6> boxes;
  DevBuf<rpl::Prim> prims;
  DevBuf<rpl::PrimRef> refs;
  DevBuf<uint64_t> keys;   // sorted (the LBVH's radix tree reads them)
  DevBuf<uint32_t> order;  // order[k]: the primitive at sorted position k
};

// The three outputs, owned here until the build has succeeded.
struct Outputs {
  DevBuf<uint8_t> nodes;  // at most n - 1 wide nodes (each inner wide node has >= 2 children)
  DevBuf<rpl::Prim> prims;
  DevBuf<rpl::PrimRef> refs;
};

// The builds' last step: the primitive records into leaf order, and the wait for everything queued.
int permute(const Sorted& s, const uint32_t* order, Outputs& o, const char* what, const char* build, std::string& err) {
  hipError_t e = hipSuccess;
  launch(permute_kernel, s.n, s.n, order, s.prims.get(), s.refs.get(), o.prims.get(), o.refs.get());
  RPG_CHECK(what);
  e = hipDeviceSynchronize();
  RPG_CHECK(build);
  return RP_OK;
}

// LBVH: the radix tree over the sorted keys, its boxes bottom-up, the collapse; the sorted order is the leaf order.
int build_lbvh(const Sorted& s, uint32_t max_leaf, uint32_t node_format, Outputs& o, GpuTree& out, std::string& err) {
  const uint32_t n = s.n;
  DevBuf<uint32_t> left, right, pin, pleaf, first, last, visits;
  DevBuf<Box6> nboxes;
  hipError_t e = hipSuccess;
  for (DevBuf<uint32_t>* b : {&left, &right, &pin, &pleaf, &first, &last, &visits}) alloc(e, *b, n);
  alloc(e, nboxes, n);
  if (e != hipSuccess) return alloc_failed(RadixSrc::build, e, err);
  e = hipMemset(visits.get(), 0, sizeof(uint32_t) * n);
  RPG_CHECK("upload (device BVH build)");
  launch(radix_tree_kernel, n - 1, n, s.keys.get(), left.get(), right.get(), pin.get(), pleaf.get(), first.get(),
         last.get());
  RPG_CHECK("radix tree");
  launch(boxes_kernel, n, n, s.boxes.get(), s.order.get(), left.get(), right.get(), pin.get(), pleaf.get(),
         nboxes.get(), visits.get());
  RPG_CHECK("boxes");
  const RadixSrc src{left.get(), right.get(), first.get(), last.get(), s.order.get(), s.boxes.get(), nboxes.get(), max_leaf};
  if (const int rc = collapse_levels(src, 0u, n, node_format, o.nodes.get(), out, nullptr, err)) return rc;
  return permute(s, s.order.get(), o, "permute", RadixSrc::build, err);
}

// PLOC (see the kernels above) over the Morton order, the collapse with the primitives laid out depth-first (perm), and
// the depth-first relayout of the nodes.
int build_ploc(const Sorted& s, uint32_t max_leaf, double cost_traverse, uint32_t node_format, uint32_t align, Outputs& o,
               GpuTree& out, std::string& err) {
  const uint32_t n = s.n;
  DevBuf<uint32_t> ref[2], csz[2], nn, keep, kpos, merge, mrank, perm;
  DevBuf<Box6> cbox[2], nbox;
  DevBuf<double> ccost[2];
  DevBuf<PNode> bn;
  DevBuf<uint8_t> scan;
  hipError_t e = hipSuccess;
  for (int b = 0; b < 2; b++) {
    alloc(e, ref[b], n);
    alloc(e, csz[b], n);
    alloc(e, cbox[b], n);
    alloc(e, ccost[b], n);
  }
  for (DevBuf<uint32_t>* b : {&nn, &keep, &kpos, &merge, &mrank, &perm}) alloc(e, *b, n);
  alloc(e, bn, n);
  alloc(e, nbox, n);
  size_t scan_bytes = 0;
  if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keep.get(), kpos.get(), (int)n);
  alloc(e, scan, scan_bytes);
  if (e != hipSuccess) return alloc_failed(PlocSrc::build, e, err);
  launch(ploc_init_kernel, n, n, s.order.get(), s.boxes.get(), ref[0].get(), cbox[0].get(), csz[0].get(),
         ccost[0].get());
  RPG_CHECK("PLOC init");
  uint32_t m = n, node_base = 0;
  int cb = 0;
  while (m > 1) {
    launch<PLOC_B>(ploc_nn_kernel, m, m, cbox[cb].get(), nn.get());
    launch(ploc_flags_kernel, m, m, nn.get(), keep.get(), merge.get());
    RPG_CHECK("PLOC neighbours");
    e = hipcub::DeviceScan::ExclusiveSum(scan.get(), scan_bytes, keep.get(), kpos.get(), (int)m);
    if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(scan.get(), scan_bytes, merge.get(), mrank.get(), (int)m);
    uint32_t last[4];
    if (e == hipSuccess) e = hipMemcpy(&last[0], kpos.get() + (m - 1), 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&last[1], keep.get() + (m - 1), 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&last[2], mrank.get() + (m - 1), 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&last[3], merge.get() + (m - 1), 4, hipMemcpyDeviceToHost);
    RPG_CHECK("PLOC scan");
    const uint32_t m2 = last[0] + last[1], merges = last[2] + last[3];
    if (merges == 0 || m2 != m - merges) return failed(err, RP_EINTERNAL, "PLOC build: no progress");
    launch(ploc_apply_kernel, m, m, nn.get(), keep.get(), kpos.get(), merge.get(), mrank.get(), node_base,
           ref[cb].get(), cbox[cb].get(), csz[cb].get(), ccost[cb].get(), ref[1 - cb].get(), cbox[1 - cb].get(),
           csz[1 - cb].get(), ccost[1 - cb].get(), bn.get(), nbox.get(), max_leaf, cost_traverse);
    RPG_CHECK("PLOC merge");
    node_base += merges;
    m = m2;
    cb = 1 - cb;
  }
  if (node_base != n - 1) return failed(err, RP_EINTERNAL, "PLOC build: node count");
  Levels levels;
  const PlocSrc src{bn.get(), s.boxes.get(), nbox.get(), perm.get()};
  // the root is the last node made
  if (const int rc = collapse_levels(src, n - 2, n, node_format, o.nodes.get(), out, &levels, err)) return rc;
  if (const int rc = dfs_relayout(o.nodes, node_format, out.n_nodes, levels, align, err)) return rc;
  return permute(s, perm.get(), o, "PLOC permute", PlocSrc::build, err);
}

}  // namespace

// On success the caller owns out.d_nodes / d_prims / d_prim_refs; on failure `out` is empty.
int build_gpu(const rpb::PrimInput& in, uint32_t max_leaf, uint32_t node_format, uint32_t algo, double cost_traverse,
              uint32_t align, GpuTree& out, std::string& err) {
  out = GpuTree{};
  const uint32_t n = (uint32_t)in.prims.size();
  if (n < 2) return failed(err, RP_EINVAL, "device BVH build needs at least 2 primitives");
  if (node_format != rpl::NODES_F32 && node_format != rpl::NODES_Q8) return failed(err, RP_EINVAL, "unknown node format");
  if (node_format == rpl::NODES_Q8 && !(in.amax <= rpl::COORD_MAX))
    return failed(err, RP_EINVAL, "primitive coordinates beyond +-2^54 (or infinite) are not supported by the quantized nodes");
  if (max_leaf < 1 || max_leaf > rpl::LEAF_MAX) return failed(err, RP_EINVAL, "max_leaf out of range");
  // the prologue: the upload, the Morton keys and their sort (the unsorted keys and the sort's scratch end with it)
  const bool ploc = algo == GPU_PLOC;
  Sorted s;
  Outputs o;
  s.n = n;
  {
    DevBuf<uint64_t> keys;
    DevBuf<uint32_t> idx;  // PLOC sorts (key, primitive) pairs
    DevBuf<uint8_t> sort_tmp;
    hipError_t e = hipSuccess;
    alloc(e, s.boxes, n);
    alloc(e, s.prims, n);
    alloc(e, s.refs, n);
    alloc(e, keys, n);
    alloc(e, s.keys, n);
    alloc(e, s.order, n);
    if (ploc) alloc(e, idx, n);
    alloc(e, o.nodes, (node_format == rpl::NODES_Q8 ? sizeof(rpl::Node4Q) : sizeof(rpl::Node4)) * n);
    alloc(e, o.prims, n);
    alloc(e, o.refs, n);
    if (e != hipSuccess) return alloc_failed(RadixSrc::build, e, err);
    e = hipMemcpy(s.boxes.get(), in.boxes.data(), sizeof(Box6) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s.prims.get(), in.prims.data(), sizeof(rpl::Prim) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s.refs.get(), in.refs.data(), sizeof(rpl::PrimRef) * n, hipMemcpyHostToDevice);
    RPG_CHECK("upload (device BVH build)");
    const double3 cmin = make_double3(in.cmin[0], in.cmin[1], in.cmin[2]);
    double sc[3];
    for (int k = 0; k < 3; k++) {
      const double ext = in.cmax[k] - in.cmin[k];
      sc[k] = ext > 0.0 ? 1024.0 / ext : 0.0;
    }
    const double3 scale = make_double3(sc[0], sc[1], sc[2]);
    if (ploc)
      launch(morton63_kernel, n, n, s.boxes.get(), cmin, scale, keys.get(), idx.get());
    else
      launch(morton_kernel, n, n, s.boxes.get(), cmin, scale, keys.get());
    RPG_CHECK("morton");
    size_t sort_bytes = 0;
    auto sort = [&](void* tmp) {  // tmp == nullptr: the scratch size only
      return ploc ? hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, keys.get(), s.keys.get(), idx.get(), s.order.get(),
                                                       (int)n, 0, 63)
                  : hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, keys.get(), s.keys.get(), (int)n, 0, 62);
    };
    e = sort(nullptr);
    if (e == hipSuccess) sort_tmp.alloc(sort_bytes, &e);
    if (e == hipSuccess) e = sort(sort_tmp.get());
    RPG_CHECK("radix sort");
    if (!ploc) {
      launch(order_kernel, n, n, s.keys.get(), s.order.get());
      RPG_CHECK("order");
    }
  }
  const int rc = ploc ? build_ploc(s, max_leaf, cost_traverse, node_format, std::max(1u, align), o, out, err)
                      : build_lbvh(s, max_leaf, node_format, o, out, err);
  if (rc != RP_OK) {
    out = GpuTree{};
    return rc;
  }
  out.node_format = node_format;
  out.qbound = rpl::qbound(in.amax);
  out.d_nodes = o.nodes.release();
  out.d_prims = o.prims.release();
  out.d_prim_refs = o.refs.release();
  return RP_OK;
}

int gather_tri_normals(GpuTree& out, uint64_t n, const double* d_vnrm, std::string& err) {
  out.d_tri_nrm = nullptr;
  if (!out.d_prims || !out.d_prim_refs || !d_vnrm || n == 0 || n > 0xFFFFFFFFull)
    return failed(err, RP_EINVAL, "triangle normals: a built tree and the vertex normals are needed");
  DevBuf<rpl::TriNormals> t;
  hipError_t e = hipSuccess;
  alloc(e, t, n);
  if (e != hipSuccess) return alloc_failed("triangle normals", e, err);
  launch(tri_normals_kernel, n, (uint32_t)n, out.d_prims, out.d_prim_refs, d_vnrm, t.get());
  RPG_CHECK("triangle normals");
  e = hipDeviceSynchronize();
  RPG_CHECK("triangle normals");
  out.d_tri_nrm = t.release();
  return RP_OK;
}

}  // namespace rpg
