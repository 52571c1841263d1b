// rp_state.h -- the objects behind include/rp.h's opaque handles and the calls the C-ABI's translation units make
// across each other: rp_scene.cpp (options, scene build and upload), rp_render.cpp (workspace, render scheduling),
// rp_gather.cpp (multi-GPU frame assembly).  Internal to librp.so.
#pragma once
#include <cstring>
#include <vector>

#include "rp_hip_util.h"
#include "rp_kernel.h"
#include "rp_schedule.h"

using rps::FrameShape;
using rps::Tiling;

#pragma GCC visibility push(hidden)

// Per-frame device state of a render (include/rp.h rp_workspace): frames with different workspaces may
// run concurrently on different streams.
struct rp_workspace {
  rp_scene* scene = nullptr;
  int device = 0;                     // the scene's
  DevBuf<uint64_t> d_ctr;             // counters when the caller passes none (CTR_N x u64)
  DevBuf<uint64_t> d_probe_ctr;       // counters of the probe launch
  DevBuf<uint32_t> d_queue;           // unit queues, one 128 B line each: the frame's groups, then the probe
  DevBuf<uint32_t> d_tile_cost;       // cost probe output, 2 x rpk::TILE_SORT_MAX entries
  DevBuf<uint32_t> d_tile_order;      // cost-ordered shard tiles, rpk::TILE_SORT_MAX entries
  DevBuf<uint8_t> d_slab;             // keystream cache, one slab per resident render lane
  DevBuf<uint32_t> d_spill;           // traversal-stack overflow entries of every resident lane (deep trees)
  DevBuf<uint32_t> d_t0;              // start time of each resident lane's measured unit (tile costs)
  // reserved by rp_workspace_reserve:
  DevBuf<double> d_partial;           // per-batch sample sums of multi-batch frames, 3 per unit
  DevBuf<uint32_t> d_partial_hits;    //   one per unit
  // the learned per-unit order (rp_sched.hip): each unit's duration in the last render, the sort keys (two buffers),
  // the radix sort's scratch and the order; ucost_shape = the frame shape the durations belong to
  DevBuf<uint32_t> d_ucost, d_uorder;
  DevBuf<uint64_t> d_ukey, d_ukey2;
  DevBuf<uint8_t> d_usort;
  bool ucost_valid = false;
  FrameShape ucost_shape;
  DevBuf<double> d_gs_rgb;            // gather staging: this rank's shard, padded to the stride (3 f64 / slot)
  DevBuf<double> d_gather_rgb;        //   all ranks' shards (nranks x stride x 3 f64)
  // a frame gather's one collective (rpk::launch_gather_pack): this rank's packed block -- counters, measured tile
  // costs, to_srgb_u8 bytes -- and every rank's, in words
  DevBuf<uint32_t> d_pack_send, d_pack_recv;
  // the balanced tile plan (RP_SHARD_BALANCED) of the last frame rendered with this workspace: the deal order,
  // its inverse and its hash (rpk::launch_tile_plan), and the frame shape it was made for
  DevBuf<uint32_t> d_plan;
  bool plan_on = false;
  FrameShape plan_shape;
  // Measured tile costs (rp_kernel.h tile_meas / launch_learn_costs): the last render's per-shard-tile unit
  // durations, every rank's of them after a frame gather, and the learned per-frame-tile table the next frame of
  // the same shape schedules with instead of a cost probe.
  DevBuf<uint32_t> d_meas;   // 2 x TILE_SORT_MAX: [k] summed, [TILE_SORT_MAX + k] longest unit of shard tile k
  DevBuf<uint32_t> d_fcost;  // learned table: 2 x TILE_SORT_MAX, by frame tile
  DevBuf<uint64_t> d_sort;   // the tile sorts' keys (rpk::SORT_SCRATCH words: global memory, not LDS)
  bool meas_on = false;      // the last render measured (megakernel)
  bool fcost_valid = false;
  FrameShape fcost_shape;    // the learned table's frame and tiles
  uint32_t fcost_ranks = 0;  // ranks whose gather made it (1: a whole-frame render on one device)
  // A frame gather reads this workspace's measured costs (d_meas) and writes its learned table (d_fcost) on the gather
  // stream; the next render on the workspace reads the table and clears d_meas on ITS stream.  The gather records
  // this event at its end and render_shard waits on it, so a caller with separate render and gather streams cannot
  // race the two; on one stream the wait is already satisfied.
  Event ev_gathered;
  bool gathered_pending = false;
  uint32_t frame_flags = 0;  // RP_FRAME_* of the last render (rp_workspace_frame_info)

  // The learned cost table describes frames of params' shape.
  bool fcost_matches(const rp_render_params* p, const Tiling& t) const {
    return fcost_valid && fcost_shape == rps::tile_shape(p, t);
  }
  void set_fcost(const rp_render_params* p, const Tiling& t, uint32_t ranks) {
    fcost_valid = true;
    fcost_shape = rps::tile_shape(p, t);
    fcost_ranks = ranks;
  }
  // The plan applies to frames of params' shape (the render of this frame's shard made it).
  bool plan_matches(const rp_render_params* p, const Tiling& t) const {
    return plan_on && plan_shape == rps::plan_shape(p, t);
  }
};

struct rp_scene {
  int device = 0;
  rpk::KScene ks{};
  rp_scene_options opt{};
  DevBuf<uint8_t> d_nodes;  // rpl::Node4, Node4Q or Node8Q records (ks.node_format), in bytes
  DevBuf<rpl::Prim> d_prims;
  DevBuf<rpl::PrimRef> d_prim_refs;
  DevBuf<rpl::TriNormals> d_tri_nrm;  // per primitive: a triangle's vertex normals (the vertex normals' only copy)
  DevBuf<double> d_vuv;
  DevBuf<rpl::Material> d_mats;
  DevBuf<rpl::Texture> d_texs;
  DevBuf<uint32_t> d_texels;
  DevBuf<uint64_t> d_diag;  // diagnostic counters (rpk::DIAG_N)
  rp_workspace ws0;         // the scene's own workspace (rp_render, rp_render_device)
  int n_workspaces = 0;     // live workspaces from rp_workspace_create
  uint64_t n_nodes = 0, n_leaves = 0, n_prims = 0, device_bytes = 0;
  double build_s[RP_BUILD_PHASES] = {0};  // rp_scene_build_times
  uint32_t tiles_auto = RP_TILES_COST;    // the tile order of RP_TILES_AUTO (scene_create)
  uint32_t max_depth = 0;
  int num_cu = 0;
  int blocks_per_cu = 0;
  uint64_t resident() const { return (uint64_t)num_cu * (uint64_t)blocks_per_cu; }  // render blocks at once
  uint64_t lanes() const { return resident() * rpk::RENDER_BLOCK; }
};

inline int frame_tiling(const rp_render_params* p, Tiling& t) {
  const rps::Refusal r = rps::make_tiling(p, t);
  return r.code ? fail(r.code, r.msg) : RP_OK;
}

// The workspace a call works on: w, or the scene's own when w is NULL (S, W: const or not).
template <class S, class W>
int use_ws(S* s, W*& w) {
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  if (!w) w = &s->ws0;
  if (w->scene != s) return fail(RP_EINVAL, "workspace belongs to another scene");
  return RP_OK;
}

// rp_scene.cpp
int scene_create(const rp_scene_desc* desc, int device, const rp_scene_options* opt_in, rp_scene** out);
const rpk::SrgbTable& srgb_table();
// rp_render.cpp
int ws_alloc(rp_scene* s, rp_workspace* w);
int ws_reserve(rp_scene* s, rp_workspace* w, const rp_render_params* p, bool gather, uint32_t n_frames = 1);
int render_shard(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p, double* d_rgb,
                 float* d_fg, uint64_t* d_counters, void* stream, uint32_t n_frames = 1,
                 uint32_t frame_order = RP_FRAME_ORDER_AUTO);

#pragma GCC visibility pop
