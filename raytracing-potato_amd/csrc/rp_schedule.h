// rp_schedule.h -- the arithmetic of a render before anything is launched: the shard's tiling, the gather block sizes,
// and everything render_shard (rp_render.cpp) decides from its arguments alone.  No HIP, no allocation, no error slot:
// a refusal comes back as a code and a message and the caller reports it.  librp_host.so compiles the same header
// behind the test hook rph_plan_launch (include/rp_host.h), so tests/test_schedule.py checks this code, not a copy.
#pragma once
#include <algorithm>

#include "../../include/rp.h"
#include "rp_kernel.h"

namespace rps {

struct Refusal {
  int code = RP_OK;
  const char* msg = "";
};

struct Tiling {
  uint32_t tw, th, shards, shard, tiles_x, tiles_y, n_tiles, n_shard_tiles;
  uint64_t n_slots;
  uint32_t sps, nbatch;  // RNG contract: samples per stream, batches per pixel
  bool balanced;         // RP_SHARD_BALANCED in effect: the tiles are dealt by a plan (frames of <= TILE_SORT_MAX tiles)
};

inline Refusal make_tiling(const rp_render_params* p, Tiling& t) {
  if (!p) return {RP_EINVAL, "params is NULL"};
  if (p->width == 0 || p->height == 0) return {RP_EINVAL, "width and height must be >= 1"};
  if (p->width > 65535 || p->height > 65535) return {RP_EINVAL, "width and height must be <= 65535"};
  t.tw = p->tile_w ? p->tile_w : 32;
  t.th = p->tile_h ? p->tile_h : 32;
  if (t.tw > 65535 || t.th > 65535) return {RP_EINVAL, "tile_w and tile_h must be <= 65535"};
  t.shards = p->num_shards ? p->num_shards : 1;
  t.shard = p->shard;
  if (t.shard >= t.shards) return {RP_EINVAL, "shard must be < num_shards"};
  t.tiles_x = (p->width + t.tw - 1) / t.tw;
  t.tiles_y = (p->height + t.th - 1) / t.th;
  t.n_tiles = t.tiles_x * t.tiles_y;
  t.n_shard_tiles = t.n_tiles > t.shard ? (t.n_tiles - t.shard + t.shards - 1) / t.shards : 0;
  t.n_slots = (uint64_t)t.n_shard_tiles * t.tw * t.th;
  if (t.n_slots >= 0xffffffffull) return {RP_EINVAL, "shard too large (>= 2^32 pixel slots)"};
  t.sps = p->samples_per_stream ? p->samples_per_stream : RP_SAMPLES_PER_STREAM;
  t.nbatch = p->spp ? (uint32_t)(((uint64_t)p->spp + t.sps - 1) / t.sps) : 0;
  if (p->shard_map > RP_SHARD_BALANCED) return {RP_EINVAL, "shard_map must be RP_SHARD_INTERLEAVE or RP_SHARD_BALANCED"};
  t.balanced = p->shard_map == RP_SHARD_BALANCED && t.n_tiles <= (uint32_t)rpk::TILE_SORT_MAX;
  return {};
}

// The frame shape a piece of workspace state was made for.  The learned tile-cost table depends on the frame and its
// tiles; the balanced plan also on the shard count; the per-unit durations on every field.  A state leaves the fields
// it does not depend on at zero.
struct FrameShape {
  uint32_t width = 0, height = 0, tile_w = 0, tile_h = 0, shards = 0, shard = 0, spp = 0, sps = 0;
  bool operator==(const FrameShape& o) const {
    return width == o.width && height == o.height && tile_w == o.tile_w && tile_h == o.tile_h && shards == o.shards &&
           shard == o.shard && spp == o.spp && sps == o.sps;
  }
};
inline FrameShape tile_shape(const rp_render_params* p, const Tiling& t) { return {p->width, p->height, t.tw, t.th}; }
inline FrameShape plan_shape(const rp_render_params* p, const Tiling& t) {
  return {p->width, p->height, t.tw, t.th, t.shards};
}
inline FrameShape unit_shape(const rp_render_params* p, const Tiling& t) {
  return {p->width, p->height, t.tw, t.th, t.shards, t.shard, p->spp, t.sps};
}

// Balanced plans under tile_order = RP_TILES_MORTON deal square blocks of tiles (rpk::launch_tile_plan): 4 x 4, or 2 x 2,
// as long as every rank still gets >= PLAN_UNITS_MIN of them (balance needs many units per rank), else single tiles.
// (AUTO is the cost order for every scene since v49, which deals tile by tile; the block deal runs only when a caller
// asks for Z-order tiles.)  The deal hands out U = block^2 consecutive positions of the block-sorted order: on a grid
// whose tiles_x or tiles_y is not a multiple of block, the edge blocks hold fewer than U tiles, so a unit after the
// first partial block straddles two blocks -- counts and balance are unchanged, only the squares are no longer whole
// (tests/test_dist.py test_block_deal_ragged_grid).
constexpr uint32_t PLAN_UNITS_MIN = 32;
inline uint32_t plan_block(uint32_t n_tiles, uint32_t nranks) {
  for (uint32_t b : {4u, 2u})
    if (n_tiles >= PLAN_UNITS_MIN * nranks * b * b) return b;
  return 1u;
}

// Slots per rank buffer of a gathered frame: shard 0 holds the most tiles (one rank: the whole frame).
inline uint64_t stage_slots(const Tiling& t) {
  const uint32_t n0 = t.n_tiles ? (t.n_tiles + t.shards - 1) / t.shards : 0;
  return (uint64_t)n0 * t.tw * t.th;
}

// Words of a rank's packed gather block (rpk::launch_gather_pack): the counter block and 2 x tiles per rank of measured
// costs (rounded up to even), then, when the frame gathers BGRA8, the shard's bytes (rounded up to even: every block
// starts 8-byte aligned for the u64 counters).
inline uint64_t pack_head(const Tiling& t) {
  const uint64_t st = (t.n_tiles + t.shards - 1) / t.shards;
  return 2ull * rpk::GATHER_CTR + ((2 * st + 1) & ~1ull);
}
inline uint64_t bgra_words(const Tiling& t) { return (stage_slots(t) + 1) & ~1ull; }
// (a gather of n frames' shards -- rp_frames_gather -- packs their BGRA8 bytes one after the other behind one head)
inline uint64_t pack_words(const Tiling& t, bool bgra, uint32_t n_frames = 1) {
  return pack_head(t) + (bgra ? n_frames * bgra_words(t) : 0ull);
}

constexpr uint32_t DEF_UNIT_QUEUES = RP_QUEUES_XCD_TILES;
constexpr uint32_t QUEUE_CHUNK_AUTO = 8;  // rp_scene_options.queue_chunk = 0: tiles per queue chunk (plan_launch)
// The queue mode in effect (rp.h RP_QUEUES_*): AUTO resolved.
inline uint32_t queue_mode(const rp_scene_options& opt) {
  return opt.unit_queues == RP_QUEUES_AUTO ? DEF_UNIT_QUEUES : opt.unit_queues;
}

// What a render of n_frames frames of params' shard is launched with: the scalar fields of its kernel parameters (the
// camera and every device pointer are the caller's to fill) and the scheduling stages it takes.
struct LaunchPlan {
  Tiling t;
  rpk::KParams kp;
  // both tile sorts key the tiles by their Z-order code (frame grids up to 256 x 256 tiles; larger ones keep shard
  // order)
  bool sortable;
  // the megakernel measures its tiles' costs (the measured table holds TILE_SORT_MAX tiles: a shard of more tiles --
  // 8 x 8 tiles at 1080p, say -- is not measured, and its frame keeps the probe / interleave)
  bool measure;
};

// Blocks of a launch over `units` queue entries with `resident` blocks fitting the device at once.
inline int grid_for(uint64_t units, uint64_t resident) {
  const uint64_t want = (units + rpk::RENDER_BLOCK - 1) / rpk::RENDER_BLOCK;
  return (int)std::max<uint64_t>(1, std::min(want, resident));
}

// A launch is planned in two steps.  The first: the checks, the tiling and every field that depends on the frame, its
// tiles' size and the launch's frame count alone.  opt: the scene's resolved options (unit_queues, queue_chunk,
// trav_threshold).
inline Refusal plan_frame(const rp_render_params* p, uint32_t n_frames, uint32_t frame_order, const rp_scene_options& opt,
                          LaunchPlan& out) {
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return {RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES"};
  if (frame_order > RP_FRAME_ORDER_PIXEL) return {RP_EINVAL, "frame_order must be an RP_FRAME_ORDER_* value"};
  Tiling& t = out.t;
  const Refusal r = make_tiling(p, t);
  if (r.code) return r;
  if (p->max_bounce < 1) return {RP_EINVAL, "max_bounce must be >= 1 (render.rs:97 assert!(depth >= 1))"};
  rpk::KParams& kp = out.kp;
  kp = rpk::KParams{};
  kp.seed = p->seed;
  kp.W = p->width, kp.H = p->height, kp.spp = p->spp, kp.max_bounce = p->max_bounce;
  kp.tw = t.tw, kp.th = t.th, kp.shard = t.shard, kp.nshards = t.shards;
  kp.tiles_x = t.tiles_x;
  kp.trav_threshold = opt.trav_threshold;
  kp.spp_batch = t.sps;  // the RNG contract's samples per stream (rp_render_params.samples_per_stream)
  kp.nbatch = t.nbatch;
  kp.n_frames = n_frames;
  kp.dv_frames = rpk::make_div32(n_frames);
  // Per-XCD queues (rp.h RP_QUEUES_*): groups of blocks blockIdx mod 8 share an XCD (MI355X_MICROARCH.md,
  // observed round-robin dispatch; speed only -- any placement gives the same image).
  kp.queue_groups = queue_mode(opt) == RP_QUEUES_SINGLE ? 1u : (uint32_t)rpk::QUEUE_GROUPS;
  kp.dv_units = rpk::make_div32(std::max(1u, t.tw * t.th * kp.nbatch));
  kp.dv_nbatch = rpk::make_div32(kp.nbatch ? kp.nbatch : 1u);
  kp.dv_tiles_x = rpk::make_div32(t.tiles_x);
  kp.dv_tw = rpk::make_div32(t.tw);
  return {};
}

// The second: the launch runs n_shard_tiles tiles -- the shard's, or a caller's list -- and everything that depends on
// their count: the slots, the queue entries, the frames' stride, the queue chunk and the frame order that depends on it.
inline void plan_tiles(uint32_t n_shard_tiles, uint32_t n_frames, uint32_t frame_order, const rp_scene_options& opt,
                       LaunchPlan& out) {
  Tiling& t = out.t;
  rpk::KParams& kp = out.kp;
  t.n_shard_tiles = n_shard_tiles;
  t.n_slots = (uint64_t)n_shard_tiles * t.tw * t.th;
  kp.n_shard_tiles = n_shard_tiles, kp.n_slots = t.n_slots;
  kp.n_queue = t.n_slots * kp.nbatch * n_frames;  // every frame's units
  kp.dv_tiles = rpk::make_div32(std::max(1u, n_shard_tiles));
  kp.frames_inter = n_frames > 1 && frame_order != RP_FRAME_ORDER_SEQUENTIAL ? 1u : 0u;
  kp.out_stride = 3 * t.n_slots;
  // Default chunk: up to 8 consecutive (virtual) tiles of the order per queue at a time, while every queue still gets >= 16
  // chunks -- the tiles one XCD runs together are then neighbours in cost and, inside a cost bucket, in Z-order (a whole C3
  // frame, 2,040 tiles: chunks of 8, -1.0 % against chunks of one; an 8-way shard, 255 tiles: chunks of one, 8 cost
  // +3.8 % at one frame per launch); with interleaved frames a whole number of tiles of every frame (n_frames >= 8: one
  // tile of every frame, so one XCD renders a tile for all the launch's frames and its L2 serves the same pixels' rays
  // n_frames times: C3 -1.3 %, 8-way shards -1.9 %)
  const uint64_t vtiles = (uint64_t)n_shard_tiles * n_frames;
  uint32_t chunk_auto = 1;
  while (chunk_auto < QUEUE_CHUNK_AUTO && 2ull * chunk_auto * 8 * 16 <= vtiles) chunk_auto *= 2;
  if (kp.frames_inter) chunk_auto = n_frames * ((chunk_auto + n_frames - 1) / n_frames);
  kp.queue_chunk = queue_mode(opt) == RP_QUEUES_XCD_REGIONS ? (n_shard_tiles + kp.queue_groups - 1) / kp.queue_groups
                  : kp.queue_groups > 1 ? (opt.queue_chunk ? opt.queue_chunk : chunk_auto) : 1u;
  if (kp.queue_chunk == 0) kp.queue_chunk = 1;
  // RP_FRAME_ORDER_PIXEL needs a queue's runs of n_frames virtual tiles to be one tile of every frame: single queue, or
  // chunks of whole multiples of n_frames (the default chunk is); otherwise it is INTERLEAVED
  if (kp.frames_inter && frame_order == RP_FRAME_ORDER_PIXEL && (kp.queue_groups == 1 || kp.queue_chunk % n_frames == 0))
    kp.frames_inter = 2;
  kp.dv_chunk = rpk::make_div32(kp.queue_chunk);
}

// A render of n_frames frames of params' shard (render_shard).
inline Refusal plan_launch(const rp_render_params* p, uint32_t n_frames, uint32_t frame_order,
                           const rp_scene_options& opt, LaunchPlan& out) {
  const Refusal r = plan_frame(p, n_frames, frame_order, opt, out);
  if (r.code) return r;
  const Tiling& t = out.t;
  plan_tiles(t.n_shard_tiles, n_frames, frame_order, opt, out);
  out.sortable = t.n_shard_tiles > 1 && t.n_shard_tiles <= rpk::TILE_SORT_MAX && t.tiles_x <= 256 && t.tiles_y <= 256;
  out.measure = t.n_shard_tiles <= (uint32_t)rpk::TILE_SORT_MAX;
  return {};
}

// A render over a caller-given list of n_listed frame tiles (include/rp.h rp_render_tiles_device_ws): the
// launch of a "shard" whose tiles are the list -- shard 0 of 1 of the whole frame's params, and the list as tile_map
// (rp_units.h: shard tile k is frame tile tile_map[0 + k * 1]).  No stage of render_shard's scheduling runs: the tiles go
// out in list order and nothing is measured.
inline Refusal plan_tiles_launch(const rp_render_params* p, uint32_t n_listed, uint32_t n_frames, uint32_t frame_order,
                                 const rp_scene_options& opt, LaunchPlan& out) {
  if (!p) return {RP_EINVAL, "params is NULL"};
  if (p->num_shards > 1 || p->shard != 0 || p->shard_map != RP_SHARD_INTERLEAVE)
    return {RP_EINVAL, "a tile-list launch takes the whole frame's params: num_shards 0 or 1, shard 0, interleave"};
  const Refusal r = plan_frame(p, n_frames, frame_order, opt, out);
  if (r.code) return r;
  if (p->spp == 0) return {RP_EINVAL, "a tile-list launch needs spp >= 1"};
  if (out.t.nbatch != 1)
    return {RP_EINVAL, "a tile-list launch renders one stream per pixel: samples_per_stream must be >= spp"};
  if (n_listed > out.t.n_tiles) return {RP_EINVAL, "n_listed is above the frame's tile count"};
  plan_tiles(n_listed, n_frames, frame_order, opt, out);  // (its slots: <= the frame's, which make_tiling admitted)
  out.sortable = false;
  out.measure = false;
  return {};
}

// The launch's units fit its queue words and its unit decode; lanes: the render lanes the scene keeps resident.
// (render_shard asks once it has cleared the launch's counters and answered empty and spp = 0 frames.)
inline Refusal launch_limits(const LaunchPlan& lp, uint64_t lanes) {
  const rpk::KParams& kp = lp.kp;
  // a 32-bit queue word takes its units, plus one failed fetch per resident lane after the last unit (single
  // queue) or one per fetch that passes a drained queue on the way to another (per-XCD queues)
  if ((kp.queue_groups > 1 ? 2 * kp.n_queue : kp.n_queue) + lanes >= 0xffffffffull)
    return {RP_EINVAL, "shard too large (>= 2^32 pixel-batch units with the resident lanes)"};
  // the unit decode divides by launch constants with 31-bit numerators (rpk::make_div32)
  if (kp.n_queue >= (1ull << 31)) return {RP_EINVAL, "shard too large (>= 2^31 pixel-batch units)"};
  return {};
}

}  // namespace rps
