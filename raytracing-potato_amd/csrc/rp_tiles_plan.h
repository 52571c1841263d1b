// rp_tiles_plan.h -- the launch arithmetic of a render over a caller-given list of frame tiles (include/rp.h
// rp_render_tiles_device_ws), beside rps::plan_launch (rp_schedule.h) and in a header of its own: the
// objects rp_build_id hashes include rp_schedule.h, and an inline function added there may move their code.  librp.so's
// rp_tiles.hip and librp_host.so (the test hooks rph_plan_tiles_launch and rph_tiles_unit_walk) compile this one text.
//
// A tile-list launch is the launch of a "shard" whose tiles are the list: n_shard_tiles = n_listed, shard 0 of 1, and
// the list as tile_map (rp_units.h: shard tile k is frame tile tile_map[0 + k * 1]).  plan_launch plans the whole frame
// -- every check of the params, the frame order, the queues, every constant that does not depend on the shard's tile
// count -- and the fields that do are set again here from n_listed: n_shard_tiles, n_slots, n_queue, out_stride,
// dv_tiles and the queue chunk.  The chunk rule is plan_launch's, restated (that function cannot be split without
// touching hashed code); tests/test_accum_tiles.py holds the two together: over the full list every field of this plan
// equals plan_launch's.
#pragma once
#include "rp_schedule.h"

namespace rps {

inline Refusal plan_tiles_launch(const rp_render_params* p, uint32_t n_listed, uint32_t n_frames, uint32_t frame_order,
                                 const rp_scene_options& opt, LaunchPlan& out) {
  if (!p) return {RP_EINVAL, "params is NULL"};
  if (p->num_shards > 1 || p->shard != 0 || p->shard_map != RP_SHARD_INTERLEAVE)
    return {RP_EINVAL, "a tile-list launch takes the whole frame's params: num_shards 0 or 1, shard 0, interleave"};
  const Refusal r = plan_launch(p, n_frames, frame_order, opt, out);
  if (r.code) return r;
  Tiling& t = out.t;
  rpk::KParams& kp = out.kp;
  if (p->spp == 0) return {RP_EINVAL, "a tile-list launch needs spp >= 1"};
  if (t.nbatch != 1)
    return {RP_EINVAL, "a tile-list launch renders one stream per pixel: samples_per_stream must be >= spp"};
  if (n_listed > t.n_tiles) return {RP_EINVAL, "n_listed is above the frame's tile count"};
  // the list as the shard
  t.n_shard_tiles = n_listed;
  t.n_slots = (uint64_t)n_listed * t.tw * t.th;  // <= the frame's, which make_tiling admitted
  kp.n_shard_tiles = n_listed;
  kp.n_slots = t.n_slots;
  kp.n_queue = t.n_slots * kp.nbatch * n_frames;
  kp.dv_tiles = rpk::make_div32(std::max(1u, n_listed));
  kp.out_stride = 3 * t.n_slots;
  // the queue chunk, and the frame order that depends on it (plan_launch's rule over vtiles = n_listed * n_frames)
  const uint32_t qmode = opt.unit_queues == RP_QUEUES_AUTO ? DEF_UNIT_QUEUES : opt.unit_queues;
  const uint64_t vtiles = (uint64_t)n_listed * n_frames;
  uint32_t chunk_auto = 1;
  while (chunk_auto < QUEUE_CHUNK_AUTO && 2ull * chunk_auto * 8 * 16 <= vtiles) chunk_auto *= 2;
  kp.frames_inter = n_frames > 1 && frame_order != RP_FRAME_ORDER_SEQUENTIAL ? 1u : 0u;
  if (kp.frames_inter) chunk_auto = n_frames * ((chunk_auto + n_frames - 1) / n_frames);
  kp.queue_chunk = qmode == RP_QUEUES_XCD_REGIONS ? (n_listed + kp.queue_groups - 1) / kp.queue_groups
                  : kp.queue_groups > 1 ? (opt.queue_chunk ? opt.queue_chunk : chunk_auto) : 1u;
  if (kp.queue_chunk == 0) kp.queue_chunk = 1;
  if (kp.frames_inter && frame_order == RP_FRAME_ORDER_PIXEL && (kp.queue_groups == 1 || kp.queue_chunk % n_frames == 0))
    kp.frames_inter = 2;
  kp.dv_chunk = rpk::make_div32(kp.queue_chunk);
  // no stage of render_shard's scheduling runs: the tiles go out in list order, nothing is measured
  out.sortable = false;
  out.measure = false;
  return {};
}

}  // namespace rps
