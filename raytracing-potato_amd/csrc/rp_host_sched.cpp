// rp_host_sched.cpp -- librp_host.so (include/rp_host.h): the hooks on the launch arithmetic (rp_schedule.h) and the
// unit fetch (rp_units.h) -- the launch plans, and the kernel's unit walk run on the CPU through HostEnv.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rp_host_util.h"
#include "rp_kernel.h"
#include "rp_schedule.h"
#include "rp_units.h"

using rph::fail;

namespace {

// ---- the unit fetch on the CPU (rp_units.h; rph_unit_walk) ------------------------------------------

// One simulated launch: its arguments, its queue words, and what the environment saw.
struct UnitWalk {
  rpk::KArgs a{};
  uint32_t words[rpk::QUEUE_WORDS] = {};
  uint32_t entries[rpk::QUEUE_WORDS] = {};  // per word: fetches that got an entry (the vote's lane was not drained)
  bool probe = false;
  uint32_t block = 0;       // the fetching block
  uint32_t last_word = 0, last_q = 0;  // the fetch the next vote is about
  // the forced vote (rp_host.h rph_unit_walk any_every): queue_entries[w] = the entries of word w's queue
  uint32_t any_every = 0;
  const uint32_t* queue_entries = nullptr;
  uint64_t votes = 0, forced = 0;
  const char* err = nullptr;
};

// What fetch_pixel needs from the place it runs in (rp_device.h DevEnv is the GPU's): a wave of one lane.
struct HostEnv {
  static thread_local UnitWalk* w;
  static const rpk::KArgs* args() { return &w->a; }
  // a fetch may touch the word of a queue below queue_groups, a probe only the one word it was given
  static uint32_t fetch_add(unsigned int* p) {
    const ptrdiff_t i = p - w->words;
    const uint32_t G = std::max(w->a.P.queue_groups, 1u);
    const bool ok = i >= 0 && i < (ptrdiff_t)rpk::QUEUE_WORDS &&
                    (w->probe ? i == rpk::QUEUE_PROBE : i % rpk::QUEUE_STRIDE == 0 && i / rpk::QUEUE_STRIDE < (ptrdiff_t)G);
    if (!ok) {
      w->err = "unit walk: a fetch touched a queue word outside the launch's queues";
      w->last_word = 0;
      return w->last_q = 0xffffffffu;  // drained, whatever the queue: the walk ends without touching memory
    }
    w->last_word = (uint32_t)i;
    return w->last_q = w->words[i]++;
  }
  static bool any(bool drained) {
    w->votes++;
    if (drained) return true;
    w->entries[w->last_word]++;
    if (w->any_every && w->votes % w->any_every == 0 && w->last_q + 1 == w->queue_entries[w->last_word]) {
      w->forced++;
      return true;
    }
    return false;
  }
  static uint32_t uniform(uint32_t x) { return x; }
  static uint32_t block() { return w->block; }
  static uint32_t numerator(uint32_t n) {
    if (n >= (1u << 31)) w->err = "unit walk: a launch-constant division's numerator is 2^31 or more";
    return n;
  }
};
thread_local UnitWalk* HostEnv::w = nullptr;

// n_blocks one-lane blocks fetch in rounds until each has retired on a failed fetch; units (may be NULL): the fetched
// units, RPH_UNIT_WORDS each, up to cap.  Returns the units fetched.
template <bool PROBE>
uint64_t walk_units(UnitWalk& W, uint32_t n_blocks, uint32_t* units, uint64_t cap) {
  HostEnv::w = &W;
  std::vector<uint8_t> retired(n_blocks, 0);
  uint64_t n = 0;
  for (uint32_t live = n_blocks; live && !W.err;) {
    for (uint32_t b = 0; b < n_blocks && !W.err; b++) {
      if (retired[b]) continue;
      W.block = b;
      uint32_t slot = 0, pi = 0, pj = 0, batch = 0;
      if (!rpk::fetch_pixel<PROBE, HostEnv>(slot, pi, pj, batch)) {
        retired[b] = 1;
        live--;
        continue;
      }
      if (PROBE) W.entries[rpk::QUEUE_PROBE]++;  // (the probe's fetch takes no vote)
      if (units && n < cap) {
        const rpk::KArgs* A = &W.a;
        const uint32_t u[RPH_UNIT_WORDS] = {slot, pi, pj, batch, b, W.last_word / rpk::QUEUE_STRIDE,
                                           rpk::unit_frame(A, batch), rpk::unit_spp(A, batch)};
        std::memcpy(units + RPH_UNIT_WORDS * n, u, sizeof u);
      }
      n++;
    }
  }
  HostEnv::w = nullptr;
  return n;
}

}  // namespace

// (the hooks below take an rp_render_params field by field)
static rp_render_params scalar_params(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                                      uint32_t tile_h, uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream,
                                      uint32_t shard_map) {
  rp_render_params p{};
  p.width = width, p.height = height, p.spp = spp, p.max_bounce = max_bounce, p.tile_w = tile_w, p.tile_h = tile_h;
  p.shard = shard, p.num_shards = num_shards, p.samples_per_stream = samples_per_stream, p.shard_map = shard_map;
  return p;
}

// An rph_launch_plan's fields of a planned launch: the tiles, slots and batches it runs, and its queues, grid and
// launch-constant divisions at `lanes` resident lanes.  (plan_block, gather_stride and block_words are the caller's.)
static void fill_plan(const rps::LaunchPlan& lp, uint64_t lanes, rph_launch_plan* out) {
  const rpk::KParams& kp = lp.kp;
  out->n_shard_tiles = lp.t.n_shard_tiles;
  out->nbatch = lp.t.nbatch;
  out->n_slots = lp.t.n_slots;
  out->queue_groups = kp.queue_groups;
  out->queue_chunk = kp.queue_chunk;
  out->frames_inter = kp.frames_inter;
  out->sortable = lp.sortable;
  out->measure = lp.measure;
  out->grid = (uint32_t)rps::grid_for(kp.n_queue, lanes / rpk::RENDER_BLOCK);
  out->n_queue = kp.n_queue;
  out->out_stride = kp.out_stride;
  const rpk::Div32 dv[3] = {kp.dv_units, kp.dv_tiles_x, kp.dv_chunk};
  uint32_t* const dst[3] = {out->dv_units, out->dv_tiles_x, out->dv_chunk};
  for (int i = 0; i < 3; i++) dst[i][0] = dv[i].m, dst[i][1] = dv[i].s;
}

static int refuse(const rps::Refusal& r) { return r.code ? fail(r.code, r.msg) : RP_OK; }

// The plan of a tile-list launch (rp_schedule.h rps::plan_tiles_launch, what rp_render_tiles_device_ws launches with).
static rps::Refusal tiles_plan(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                               uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_listed, uint32_t n_frames,
                               uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, rps::LaunchPlan& lp) {
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, 0, 1, samples_per_stream,
                                           RP_SHARD_INTERLEAVE);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  return rps::plan_tiles_launch(&p, n_listed, n_frames, frame_order, opt, lp);
}

extern "C" {

int rph_make_div32(uint32_t d, uint32_t* m, uint32_t* s) {
  if (d == 0 || !m || !s) return fail("rph_make_div32: d must be >= 1 and m, s non-NULL");
  const rpk::Div32 v = rpk::make_div32(d);
  *m = v.m;
  *s = v.s;
  return RP_OK;
}

int rph_plan_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                    uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                    uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes, rph_launch_plan* out) {
  if (!out) return fail("rph_plan_launch: out is NULL");
  *out = rph_launch_plan{};
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, shard, num_shards,
                                           samples_per_stream, shard_map);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  rps::LaunchPlan lp{};
  if (!rps::make_tiling(&p, lp.t).code) {
    out->n_shard_tiles = lp.t.n_shard_tiles;
    out->nbatch = lp.t.nbatch;
    out->plan_block = rps::plan_block(lp.t.n_tiles, lp.t.shards);
    out->n_slots = lp.t.n_slots;
    out->gather_stride = rps::stage_slots(lp.t);
    out->block_words = rps::pack_words(lp.t, true, n_frames);
  }
  rps::Refusal r = rps::plan_launch(&p, n_frames, frame_order, opt, lp);
  if (r.code) return refuse(r);  // nothing planned
  fill_plan(lp, lanes, out);
  return refuse(rps::launch_limits(lp, lanes));
}

int rph_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                  uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                  uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tile_order,
                  const uint32_t* tile_map, const uint32_t* unit_order, uint32_t probe_lattice, uint32_t queue_groups,
                  uint32_t n_blocks, uint32_t any_every, uint32_t* units, uint64_t units_cap, uint64_t* n_units,
                  uint32_t* queue_words, uint32_t* entries, uint64_t* forced) {
  static_assert((int)RPH_QUEUE_WORDS == (int)rpk::QUEUE_WORDS, "rp_host.h states rp_kernel.h's queue words");
  if (!n_units || !queue_words || !entries || !forced || (units_cap && !units) || n_blocks == 0 ||
      queue_groups > (uint32_t)rpk::QUEUE_GROUPS)
    return fail("rph_unit_walk: NULL output, no blocks or more queues than QUEUE_GROUPS");
  const rp_render_params p = scalar_params(width, height, spp, max_bounce, tile_w, tile_h, shard, num_shards,
                                           samples_per_stream, shard_map);
  rp_scene_options opt{};
  opt.unit_queues = unit_queues;
  opt.queue_chunk = queue_chunk;
  rps::LaunchPlan lp{};
  rps::Refusal r = rps::plan_launch(&p, n_frames, frame_order, opt, lp);
  if (!r.code) r = rps::launch_limits(lp, n_blocks);
  if (r.code) return refuse(r);
  const rps::Tiling& t = lp.t;
  auto below = [](const uint32_t* v, uint64_t n, uint64_t bound) {
    for (uint64_t i = 0; v && i < n; i++)
      if (v[i] >= bound) return false;
    return true;
  };
  const uint64_t shard_units = t.n_slots * t.nbatch;
  if (!below(tile_order, t.n_shard_tiles, t.n_shard_tiles) || !below(tile_map, t.n_tiles, t.n_tiles) ||
      !below(unit_order, shard_units, shard_units))
    return fail("rph_unit_walk: an order or map entry is out of range");
  UnitWalk W;
  rpk::KParams& kp = W.a.P;
  kp = lp.kp;
  if (queue_groups) kp.queue_groups = queue_groups;
  kp.tile_map = tile_map;      // rp_render.cpp balanced_plan
  kp.tile_order = tile_order;  // rp_render.cpp tile_order
  W.a.queue = W.words;         // rp_render.cpp launch_units: the workspace's queue words
  if (probe_lattice) {         // rp_render.cpp launch_probe, over the shard's tiles
    kp.probe = 1, kp.spp = 1, kp.nbatch = 1, kp.spp_batch = 1, kp.n_frames = 1;
    kp.probe_n = std::min(probe_lattice, std::min(t.tw, t.th));
    kp.probe_px = kp.probe_n * kp.probe_n;
    kp.n_queue = kp.n_slots = (uint64_t)t.n_shard_tiles * kp.probe_px;
    kp.queue_groups = 1, kp.queue_chunk = 1;
    kp.tile_order = nullptr, kp.tile_map = nullptr;
    W.a.queue = W.words + rpk::QUEUE_PROBE;
    W.probe = true;
  } else if (unit_order) {     // rp_render.cpp unit_order
    kp.unit_order = unit_order;
    kp.order_chunk = rpk::UNIT_ORDER_CHUNK;
    kp.dv_ochunk = rpk::make_div32(kp.order_chunk);
    kp.dv_tile_px = rpk::make_div32(t.tw * t.th);
  }
  auto run = [&](uint32_t* out, uint64_t cap) {
    return W.probe ? walk_units<true>(W, n_blocks, out, cap) : walk_units<false>(W, n_blocks, out, cap);
  };
  uint32_t queue_entries[rpk::QUEUE_WORDS];
  if (any_every && !W.probe) {
    // a first walk, no vote forced, counts every queue's entries: where a forced vote's wave-mate can stand
    run(nullptr, 0);
    std::memcpy(queue_entries, W.entries, sizeof queue_entries);
    const rpk::KArgs a = W.a;
    W = UnitWalk{};
    W.a = a;
    W.a.queue = W.words;
    W.any_every = any_every;
    W.queue_entries = queue_entries;
  }
  *n_units = run(units, units_cap);
  std::memcpy(queue_words, W.words, sizeof W.words);
  std::memcpy(entries, W.entries, sizeof W.entries);
  *forced = W.forced;
  if (W.err) return fail(W.err);
  if (*n_units > units_cap) return fail("rph_unit_walk: more units than units_cap");
  return RP_OK;
}

int rph_plan_tiles_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                          uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_listed, uint32_t n_frames,
                          uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes,
                          rph_launch_plan* out) {
  if (!out) return fail("rph_plan_tiles_launch: out is NULL");
  *out = rph_launch_plan{};
  rps::LaunchPlan lp{};
  const rps::Refusal r = tiles_plan(width, height, spp, max_bounce, tile_w, tile_h, samples_per_stream, n_listed, n_frames,
                                    frame_order, unit_queues, queue_chunk, lp);
  if (r.code) return refuse(r);  // nothing planned
  fill_plan(lp, lanes, out);
  out->plan_block = 1;
  return refuse(rps::launch_limits(lp, lanes));
}

int rph_tiles_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                        uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_frames, uint32_t frame_order,
                        uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tiles, uint32_t n_listed,
                        uint32_t n_blocks, uint32_t* units, uint64_t units_cap, uint64_t* n_units, uint32_t* queue_words,
                        uint32_t* entries) {
  if (!n_units || !queue_words || !entries || (units_cap && !units) || n_blocks == 0 || (n_listed && !tiles))
    return fail("rph_tiles_unit_walk: NULL list or output, or no blocks");
  rps::LaunchPlan lp{};
  rps::Refusal r = tiles_plan(width, height, spp, max_bounce, tile_w, tile_h, samples_per_stream, n_listed, n_frames,
                              frame_order, unit_queues, queue_chunk, lp);
  if (!r.code) r = rps::launch_limits(lp, n_blocks);
  if (r.code) return refuse(r);
  UnitWalk W;
  W.a.P = lp.kp;
  W.a.P.tile_map = tiles;  // rp_tiles.hip: the list is the one-shard launch's tile map
  W.a.queue = W.words;
  *n_units = n_listed ? walk_units<false>(W, n_blocks, units, units_cap) : 0;
  std::memcpy(queue_words, W.words, sizeof W.words);
  std::memcpy(entries, W.entries, sizeof W.entries);
  if (W.err) return fail(W.err);
  if (*n_units > units_cap) return fail("rph_tiles_unit_walk: more units than units_cap");
  return RP_OK;
}

}  // extern "C"
