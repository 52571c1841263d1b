// rp_render.cpp -- the render side of the C-ABI in include/rp.h (librp.so): the workspace, the stages of a shard's
// render (render_shard: plan, tile costs, balanced deal, tile and unit order, the persistent kernel's launch, batch
// reduce, learned costs) and the calls that read a workspace's scheduling state back.
#include "rp_pass.h"

// Allocate a workspace for scene s (current device = the scene's): counters, queues, probe/sort buffers
// and a keystream slab for every lane the render grid can hold resident.
int ws_alloc(rp_scene* s, rp_workspace* w) {
  *w = rp_workspace{};
  w->scene = s;
  w->device = s->device;
  const uint64_t lanes = s->lanes();
  if (!w->d_ctr.alloc(rpk::CTR_N) || !w->d_probe_ctr.alloc(rpk::CTR_N) || !w->d_queue.alloc(rpk::QUEUE_WORDS) ||
      !w->d_tile_cost.alloc(2 * rpk::TILE_SORT_MAX) || !w->d_tile_order.alloc(rpk::TILE_SORT_MAX) ||
      !w->d_plan.alloc(2 * rpk::TILE_SORT_MAX + 2) || !w->d_meas.alloc(2 * rpk::TILE_SORT_MAX) ||
      !w->d_fcost.alloc(2 * rpk::TILE_SORT_MAX) || !w->d_sort.alloc(rpk::SORT_SCRATCH) ||
      !w->d_slab.alloc(lanes * rpk::rng_slab_bytes_per_lane(s->ks.node_format)) ||
      !w->d_spill.alloc(lanes * std::max<uint64_t>(1, s->ks.stack_depth - s->ks.lds_depth)) || !w->d_t0.alloc(lanes) ||
      hipEventCreateWithFlags(w->ev_gathered.put(), hipEventDisableTiming) != hipSuccess)
    return fail(RP_ENOMEM, "hipMalloc render workspace");  // (the workspace's owner frees what was allocated)
  return RP_OK;
}

namespace {

// The learned per-unit order (rp.h RP_UNITS_*) for frames of nbatch sample streams per pixel: LEARNED always, AUTO
// for one stream per pixel (nbatch 1).  Measured with round 6's bucket fix (profiles/r6/c3_unit_order_fix_ab.json,
// lone C3 frames): one stream per pixel 220.1 ms against 260.8 ms in tile order -- the longest pixels (glass-bunny
// paths of ~2,000 rays) start first instead of ending the frame -- while 32-sample streams lose 4.4 % (213.8 vs 204.8:
// a wave's units become pixels scattered over the frame, and their 8 short streams leave no long tail to fix).
bool units_on(const rp_scene* s, uint32_t nbatch) {
  return s->opt.unit_order == RP_UNITS_LEARNED || (s->opt.unit_order == RP_UNITS_AUTO && nbatch == 1);
}

}  // namespace

// Grow the workspace's reservation for renders of params' shape (synchronous): the multi-batch sums and,
// with `gather`, the staging and receive buffers of rp_frame_gather.
int ws_reserve(rp_scene* s, rp_workspace* w, const rp_render_params* p, bool gather, uint32_t n_frames) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return fail(RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES");
  DeviceGuard g(s->device);
  const uint64_t units = t.nbatch > 1 ? t.n_slots * t.nbatch * n_frames : 0;
  if (units > w->d_partial_hits.capacity()) {  // both or neither: a failed reservation leaves no batch workspace
    w->d_partial.reset();
    w->d_partial_hits.reset();
    if (!w->d_partial.alloc(3 * units) || !w->d_partial_hits.alloc(units))
      return fail(RP_ENOMEM, "hipMalloc sample-batch workspace");
  }
  // the learned per-unit order: 4 + 8 + 8 + 4 bytes per unit and the sort's scratch (C3 one stream: 2.1 M units, 50 MB)
  const uint64_t n_units = t.n_slots * t.nbatch;
  if (units_on(s, t.nbatch) && n_units > w->d_ucost.capacity() && n_units < (1ull << 31)) {
    w->ucost_valid = false;
    w->d_ucost.reset();  // its capacity is the reservation's: allocated last, once the other four are there
    const size_t sort_bytes = rpk::unit_order_scratch_bytes(n_units);
    if (!sort_bytes || !w->d_ukey.alloc(n_units) || !w->d_ukey2.alloc(n_units) || !w->d_uorder.alloc(n_units) ||
        !w->d_usort.alloc(sort_bytes) || !w->d_ucost.alloc(n_units))
      return fail(RP_ENOMEM, "hipMalloc per-unit order");
    RP_HIP(hipMemset(w->d_ucost.get(), 0, sizeof(uint32_t) * n_units));
  }
  if (gather) {
    const uint64_t stride = rps::stage_slots(t);
    const uint64_t pw = rps::pack_words(t, true, n_frames);  // rp_frames_gather: all of a launch's frames in one block
    if (!w->d_gs_rgb.reserve(stride * 3)) return fail(RP_ENOMEM, "hipMalloc gather staging");
    if (!w->d_gather_rgb.reserve(stride * t.shards * 3)) return fail(RP_ENOMEM, "hipMalloc gather buffers");
    if (!w->d_pack_send.reserve(pw)) return fail(RP_ENOMEM, "hipMalloc gather block");
    if (!w->d_pack_recv.reserve(pw * t.shards)) return fail(RP_ENOMEM, "hipMalloc gathered blocks");
  }
  return RP_OK;
}

namespace {

// One render_shard call: what its stages share.  Every stage enqueues on `stream`, in the order render_shard calls them.
struct Launch {
  rp_scene* s;
  rp_workspace* w;
  const rp_render_params* p;
  double* d_rgb;
  float* d_fg;
  uint64_t* ctr;
  void* stream;
  rps::LaunchPlan lp;  // the tiling, the kernel parameters (their pointers filled stage by stage), sortable, measure
  rpk::KScene ks;
  uint32_t order_mode = 0;               // RP_TILES_PLAIN, COST or MORTON
  bool learned = false;                  // the workspace's learned cost table is of this frame's shape
  const uint32_t* frame_cost = nullptr;  // per-frame-tile costs (sum, max) the plan and the shard order use
  uint32_t probe_px = 0;                 // samples behind each cost
  rpk::TileGeom tg{};
  bool ufit = false, uorder = false;     // the units' durations are stored / the units run in their learned order
  hipStream_t st() const { return (hipStream_t)stream; }
  int grid_for(uint64_t units) const { return rps::grid_for(units, s->resident()); }
};

// The cost probe: sample 0 of an n x n lattice of pixels per tile traced by the probe instantiation of the
// render kernel, which adds up per tile the traversal work and shaded rays (summed and costliest sample) --
// over the shard's tiles, or over the whole frame for a balanced plan (same stream, no host sync).
int launch_probe(Launch& L, uint32_t shard, uint32_t nshards, uint32_t n_tiles, uint32_t lattice) {
  rp_workspace* w = L.w;
  rpk::KParams pk = L.lp.kp;
  pk.probe = 1, pk.spp = 1, pk.nbatch = 1, pk.spp_batch = 1, pk.n_frames = 1;
  pk.shard = shard, pk.nshards = nshards, pk.n_shard_tiles = n_tiles;
  pk.probe_n = std::min(lattice, std::min(L.lp.t.tw, L.lp.t.th));
  pk.probe_px = pk.probe_n * pk.probe_n;
  pk.n_queue = pk.n_slots = (uint64_t)n_tiles * pk.probe_px;
  pk.queue_groups = 1, pk.queue_chunk = 1;
  pk.tile_cost = w->d_tile_cost.get();
  pk.tile_order = nullptr, pk.tile_map = nullptr;
  L.probe_px = pk.probe_px;
  RP_HIP(hipMemsetAsync(w->d_probe_ctr.get(), 0, sizeof(uint64_t) * rpk::CTR_N, L.st()));
  w->frame_flags |= RP_FRAME_PROBED;
  RP_HIP(hipMemsetAsync(w->d_tile_cost.get(), 0, sizeof(uint32_t) * 2 * rpk::TILE_SORT_MAX, L.st()));
  RP_LAUNCH("probe", rpk::launch_render(L.ks, pk, L.d_rgb, nullptr, w->d_probe_ctr.get(), w->d_queue.get() + rpk::QUEUE_PROBE,
                                        L.grid_for(pk.n_slots), L.stream));
  return RP_OK;
}

// Scheduling costs.  The megakernel measures every unit's duration into its tile's cost (kp.tile_meas); once a
// frame of this geometry has been rendered whole on one device, or gathered from all ranks, the workspace holds a
// learned per-tile table and the next frame schedules from it -- no probe launch.  For a balanced plan over
// N > 1 ranks the table must come from a gather over the same N ranks: every rank then holds the same bytes and
// deals the same plan.  Otherwise a probe (the first frame) supplies the costs.
int tile_costs(Launch& L) {
  rp_scene* s = L.s;
  rp_workspace* w = L.w;
  const Tiling& t = L.lp.t;
  L.order_mode = s->opt.tile_order == RP_TILES_AUTO ? s->tiles_auto : s->opt.tile_order;
  const bool probe_order = L.order_mode == RP_TILES_PROBE;
  if (probe_order) L.order_mode = RP_TILES_COST;
  w->plan_on = false;
  L.learned = L.lp.measure && !probe_order && w->fcost_matches(L.p, t);
  if (L.learned) w->frame_flags |= RP_FRAME_LEARNED_ORDER;
  // the shard order alone needs no agreement between ranks
  if (L.learned && (!t.balanced || t.shards == 1 || w->fcost_ranks == t.shards)) {
    L.frame_cost = w->d_fcost.get();
    L.probe_px = t.tw * t.th * std::max(1u, t.nbatch);  // units per tile: sum / units = mean unit
    return RP_OK;
  }
  if (t.balanced) {
    // RP_SHARD_BALANCED without a learned table: probe the whole frame (deterministic costs, rp_device.h trav_step
    // COUNT); scenes past the Infinity Cache (Z-order tiles, no cost order inside the shard) probe a sparser 4 x 4
    // lattice.
    const uint32_t lattice = L.order_mode == RP_TILES_COST ? s->opt.probe_n : std::min(s->opt.probe_n, 4u);
    L.frame_cost = w->d_tile_cost.get();
    return launch_probe(L, 0, 1, t.n_tiles, lattice);
  }
  // the shard's tiles by cost, without a table: a probe of the shard (its costs are indexed by shard tile)
  if (L.order_mode == RP_TILES_COST && L.lp.sortable) return launch_probe(L, t.shard, t.shards, t.n_shard_tiles, s->opt.probe_n);
  return RP_OK;
}

// RP_SHARD_BALANCED: deal the frame's tiles to the ranks by cost (rpk::launch_tile_plan).
int balanced_plan(Launch& L) {
  rp_workspace* w = L.w;
  const Tiling& t = L.lp.t;
  L.tg = rpk::TileGeom{t.tiles_x, t.shard, t.shards, nullptr, 0, 0};
  if (!t.balanced) return RP_OK;
  // Z-order tiles (tile_order = MORTON, on request only) deal square blocks of tiles: a rank's tiles stay in compact
  // squares of the frame, so its working set does too (C5 8-way shards: DESIGN.md 6); the cost order (AUTO, every
  // scene) deals tile by tile
  const uint32_t block = L.order_mode == RP_TILES_MORTON ? rps::plan_block(t.n_tiles, t.shards) : 1u;
  RP_LAUNCH("tile plan", rpk::launch_tile_plan(L.frame_cost, t.n_tiles, t.shards, t.tiles_x, block, w->d_plan.get(),
                                               w->d_sort.get(), L.stream));
  L.lp.kp.tile_map = w->d_plan.get();
  L.tg.map = w->d_plan.get();
  L.tg.map_tiles = t.n_tiles;
  w->plan_on = true;
  w->plan_shape = rps::plan_shape(L.p, t);
  return RP_OK;
}

// The shard's tiles in Z-order, or by cost: the learned table or the balanced plan's frame probe, else the shard's probe.
int tile_order(Launch& L) {
  rp_workspace* w = L.w;
  const uint32_t n = L.lp.t.n_shard_tiles;
  if (!L.lp.sortable || (L.order_mode != RP_TILES_MORTON && L.order_mode != RP_TILES_COST)) return RP_OK;
  if (L.order_mode == RP_TILES_MORTON) {
    RP_LAUNCH("tile sort", rpk::launch_tile_sort(nullptr, n, 1, L.tg, w->d_tile_order.get(), w->d_sort.get(), L.stream));
  } else {
    L.tg.cost_by_tile = L.frame_cost ? 1u : 0u;
    RP_LAUNCH("tile sort", rpk::launch_tile_sort(L.frame_cost ? L.frame_cost : w->d_tile_cost.get(), n, L.probe_px, L.tg,
                                                 w->d_tile_order.get(), w->d_sort.get(), L.stream));
  }
  L.lp.kp.tile_order = w->d_tile_order.get();
  return RP_OK;
}

// The learned per-unit order (rp.h RP_UNITS_*, units_on): units longest first by the last render's durations on this
// workspace -- same frame shape and shard, one frame per launch (or any launch under LEARNED: a unit's n_frames frames
// are then handed out together), and not a balanced plan over several ranks (its tiles may move) -- and such renders
// store their units' durations for the next one.
int unit_order(Launch& L) {
  rp_scene* s = L.s;
  rp_workspace* w = L.w;
  const Tiling& t = L.lp.t;
  rpk::KParams& kp = L.lp.kp;
  const uint64_t n_units = t.n_slots * t.nbatch;
  // (launches of several frames: LEARNED only -- AUTO keeps their interleaved tile order)
  L.ufit = (kp.n_frames == 1 || s->opt.unit_order == RP_UNITS_LEARNED) && units_on(s, t.nbatch) && w->d_ucost.get() &&
           n_units <= w->d_ucost.capacity() && (!t.balanced || t.shards == 1);
  if (L.ufit && w->ucost_valid && w->ucost_shape == rps::unit_shape(L.p, t)) {
    RP_LAUNCH("unit order", rpk::launch_unit_order(w->d_ucost.get(), n_units, w->d_ukey.get(), w->d_ukey2.get(), w->d_usort.get(),
                                                   w->d_usort.capacity(), w->d_uorder.get(), L.stream));
    kp.unit_order = w->d_uorder.get();
    kp.order_chunk = rpk::UNIT_ORDER_CHUNK;
    kp.dv_ochunk = rpk::make_div32(kp.order_chunk);
    kp.dv_tile_px = rpk::make_div32(t.tw * t.th);
    L.uorder = true;
  }
  if (L.ufit) kp.unit_cost = w->d_ucost.get();
  return RP_OK;
}

// The persistent kernel over every unit of the launch.  The workspace's durations and order are committed only once
// the launch is enqueued.
int launch_units(Launch& L) {
  rp_workspace* w = L.w;
  rpk::KParams& kp = L.lp.kp;
  RP_HIP(hipMemsetAsync(w->d_meas.get(), 0, sizeof(uint32_t) * 2 * rpk::TILE_SORT_MAX, L.st()));
  kp.tile_meas = L.lp.measure ? w->d_meas.get() : nullptr;
  w->meas_on = L.lp.measure;
  int e = rpk::launch_render(L.ks, kp, L.d_rgb, L.d_fg, L.ctr, w->d_queue.get(), L.grid_for(kp.n_queue), L.stream);
  if (e != 0) {
    w->ucost_valid = false;  // the durations may be partly overwritten
    return fail(RP_EHIP, std::string("render launch: ") + hipGetErrorString((hipError_t)e));
  }
  if (L.uorder) w->frame_flags |= RP_FRAME_UNIT_ORDER;
  w->ucost_valid = L.ufit;
  if (L.ufit) w->ucost_shape = rps::unit_shape(L.p, L.lp.t);
  return RP_OK;
}

// Multi-batch frames: each frame's batch sums, added in batch order.
int reduce_batches(Launch& L) {
  const rpk::KParams& kp = L.lp.kp;
  const uint64_t n_slots = L.lp.t.n_slots;
  for (uint32_t f = 0; kp.nbatch > 1 && f < kp.n_frames; f++) {
    rpk::KParams kf = kp;
    kf.partial = kp.partial + 3 * (uint64_t)f * n_slots * kp.nbatch;
    kf.partial_hits = kp.partial_hits + (uint64_t)f * n_slots * kp.nbatch;
    RP_LAUNCH("reduce", rpk::launch_reduce_batches(kf, L.d_rgb + (uint64_t)f * kp.out_stride,
                                                   L.d_fg ? L.d_fg + (uint64_t)f * n_slots : nullptr, L.stream));
  }
  return RP_OK;
}

// A whole frame on one device: its measured costs are the next frame's table (several ranks: the frame gather's).
int learn_costs(Launch& L) {
  rp_workspace* w = L.w;
  const Tiling& t = L.lp.t;
  if (!L.lp.measure || t.shards != 1 || t.n_tiles > (uint32_t)rpk::TILE_SORT_MAX) return RP_OK;
  RP_LAUNCH("cost table", rpk::launch_learn_costs(w->d_meas.get(), w->d_meas.get() + rpk::TILE_SORT_MAX, 0, 1, t.n_tiles,
                                                  L.lp.kp.tile_map, w->d_fcost.get(), L.stream));
  w->set_fcost(L.p, t, 1);
  return RP_OK;
}

}  // namespace

// The render of one shard on `stream` (rp_render_device_ws's body).
int render_shard(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p, double* d_rgb,
                 float* d_fg, uint64_t* d_counters, void* stream, uint32_t n_frames, uint32_t frame_order) {
  if (!s || !cam || !d_rgb) return fail(RP_EINVAL, "scene, camera and output must be non-NULL");
  if (!w || w->scene != s) return fail(RP_EINVAL, "workspace is NULL or belongs to another scene");
  w->frame_flags = 0;  //  before any return: an spp = 0 or refused render reports no scheduling
  Launch L{s, w, p, d_rgb, d_fg, d_counters ? d_counters : w->d_ctr.get(), stream};
  rps::Refusal refused = rps::plan_launch(p, n_frames, frame_order, s->opt, L.lp);
  if (refused.code) return fail(refused.code, refused.msg);
  const Tiling& t = L.lp.t;
  rpk::KParams& kp = L.lp.kp;
  DeviceGuard g(s->device);
  int rc = rpp::launch_begin(w, L.ctr, L.st());
  if (rc) return rc;
  if (t.n_slots == 0) return RP_OK;
  if (p->spp == 0) {
    // main.rs:86-87 with num_samples = 0: (0,0,0) / 0 and 0 / 0 are NaN; all-ones bits are a NaN.
    RP_HIP(hipMemsetAsync(d_rgb, 0xff, sizeof(double) * 3 * t.n_slots * n_frames, L.st()));
    if (d_fg) RP_HIP(hipMemsetAsync(d_fg, 0xff, sizeof(float) * t.n_slots * n_frames, L.st()));
    return RP_OK;
  }
  refused = rps::launch_limits(L.lp, s->lanes());
  if (refused.code) return fail(refused.code, refused.msg);
  rpp::set_camera(kp, cam);
  if (kp.nbatch > 1) {
    if (kp.n_queue > w->d_partial_hits.capacity() || 3 * kp.n_queue > w->d_partial.capacity())
      return fail(RP_EINVAL, n_frames > 1 ? "workspace not reserved for these frames' sample batches: call "
                                            "rp_workspace_reserve_frames"
                                          : "workspace not reserved for this frame's sample batches: call rp_workspace_reserve");
    kp.partial = w->d_partial.get();
    kp.partial_hits = w->d_partial_hits.get();
  }
  if ((rc = rpp::launch_bind(s, w, L.ks, L.st())) || (rc = tile_costs(L)) || (rc = balanced_plan(L)) ||
      (rc = tile_order(L)) || (rc = unit_order(L)) || (rc = launch_units(L)) || (rc = reduce_batches(L)) ||
      (rc = learn_costs(L)))
    return rc;
  return RP_OK;
}

extern "C" {

int rp_shard_to_bgra8(rp_scene* s, const rp_render_params* p, const double* d_shard_rgb, uint8_t* d_shard_bgra,
                      void* stream) {
  if (!s || !d_shard_rgb || !d_shard_bgra) return fail(RP_EINVAL, "scene and buffers must be non-NULL");
  if (reinterpret_cast<uintptr_t>(d_shard_bgra) % 4 != 0) return fail(RP_EINVAL, "d_shard_bgra must be 4-byte aligned");
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  DeviceGuard g(s->device);
  RP_LAUNCH("output stage", rpk::launch_srgb_bgra(srgb_table(), d_shard_rgb, t.n_slots, d_shard_bgra, stream));
  return RP_OK;
}

int rp_shard_pixel_count(const rp_render_params* p, uint64_t* count) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (!count) return fail(RP_EINVAL, "count is NULL");
  *count = t.n_slots;
  return RP_OK;
}

int rp_shard_unpack(const rp_render_params* p, const double* shard_buf, uint32_t channels, double* frame) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (!shard_buf || !frame || channels == 0) return fail(RP_EINVAL, "NULL buffer or zero channels");
  if (t.balanced) return fail(RP_EINVAL, "balanced frame: unpack with rp_shard_unpack_map and rp_workspace_tile_map");
  rpp::unpack_host(p, t, nullptr, shard_buf, sizeof(double), channels, frame);
  return RP_OK;
}

int rp_shard_unpack_map(const rp_render_params* p, const uint32_t* tile_map, const double* shard_buf, uint32_t channels,
                        double* frame) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (!shard_buf || !frame || channels == 0) return fail(RP_EINVAL, "NULL buffer or zero channels");
  if (tile_map) {
    std::vector<uint8_t> seen(t.n_tiles, 0);
    for (uint32_t i = 0; i < t.n_tiles; i++) {
      if (tile_map[i] >= t.n_tiles || seen[tile_map[i]]) return fail(RP_EINVAL, "tile_map is not a permutation of the frame's tiles");
      seen[tile_map[i]] = 1;
    }
  }
  rpp::unpack_host(p, t, tile_map, shard_buf, sizeof(double), channels, frame);
  return RP_OK;
}

int rp_workspace_tile_map(rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t* tile_map, uint32_t n) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!tile_map) return fail(RP_EINVAL, "scene and tile_map must be non-NULL");
  Tiling t;
  if ((rc = frame_tiling(p, t))) return rc;
  if (n < t.n_tiles) return fail(RP_EINVAL, "tile_map holds fewer entries than the frame has tiles");
  if (!t.balanced) {
    for (uint32_t i = 0; i < t.n_tiles; i++) tile_map[i] = i;
    return RP_OK;
  }
  if (!w->plan_matches(p, t)) return fail(RP_EINVAL, "no balanced plan for this frame in the workspace: render it first");
  DeviceGuard g(s->device);
  RP_HIP(hipDeviceSynchronize());
  RP_HIP(hipMemcpy(tile_map, w->d_plan.get(), sizeof(uint32_t) * t.n_tiles, hipMemcpyDeviceToHost));
  return RP_OK;
}

int rp_workspace_frame_info(const rp_scene* s, const rp_workspace* w, uint32_t* flags) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!flags) return fail(RP_EINVAL, "scene and flags must be non-NULL");
  *flags = w->frame_flags;
  return RP_OK;
}

int rp_workspace_unit_order(rp_scene* s, rp_workspace* w, uint32_t* durations, uint32_t* order, uint64_t n) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (n > w->d_ucost.capacity()) return fail(RP_EINVAL, "n exceeds the workspace's per-unit reservation");
  if (n == 0) return RP_OK;
  DeviceGuard g(s->device);
  RP_HIP(hipDeviceSynchronize());
  if (durations) RP_HIP(hipMemcpy(durations, w->d_ucost.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  if (order) RP_HIP(hipMemcpy(order, w->d_uorder.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  return RP_OK;
}

int rp_workspace_tile_costs(rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t* costs, uint32_t n) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!costs) return fail(RP_EINVAL, "scene and costs must be non-NULL");
  Tiling t;
  if ((rc = frame_tiling(p, t))) return rc;
  if (n < 2 * t.n_shard_tiles) return fail(RP_EINVAL, "costs holds fewer than 2 x the shard's tiles");
  if (!w->meas_on) return fail(RP_EINVAL, "the workspace's last render did not measure tile costs");
  if (t.n_shard_tiles > (uint32_t)rpk::TILE_SORT_MAX) return fail(RP_EINVAL, "more than 16384 shard tiles");
  DeviceGuard g(s->device);
  RP_HIP(hipDeviceSynchronize());
  RP_HIP(hipMemcpy(costs, w->d_meas.get(), sizeof(uint32_t) * t.n_shard_tiles, hipMemcpyDeviceToHost));
  RP_HIP(hipMemcpy(costs + t.n_shard_tiles, w->d_meas.get() + rpk::TILE_SORT_MAX, sizeof(uint32_t) * t.n_shard_tiles,
                   hipMemcpyDeviceToHost));
  return RP_OK;
}

int rp_workspace_set_tile_costs(rp_scene* s, rp_workspace* w, const rp_render_params* p, const uint32_t* costs,
                                uint32_t ranks) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!costs || ranks == 0) return fail(RP_EINVAL, "scene and costs must be non-NULL, ranks >= 1");
  Tiling t;
  if ((rc = frame_tiling(p, t))) return rc;
  if (t.n_tiles > (uint32_t)rpk::TILE_SORT_MAX) return fail(RP_EINVAL, "more than 16384 frame tiles");
  DeviceGuard g(s->device);
  RP_HIP(hipDeviceSynchronize());
  RP_HIP(hipMemcpy(w->d_fcost.get(), costs, sizeof(uint32_t) * t.n_tiles, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(w->d_fcost.get() + rpk::TILE_SORT_MAX, costs + t.n_tiles, sizeof(uint32_t) * t.n_tiles,
                   hipMemcpyHostToDevice));
  w->set_fcost(p, t, ranks);
  return RP_OK;
}

int rp_workspace_create(rp_scene* s, rp_workspace** out) {
  if (!out) return fail(RP_EINVAL, "out is NULL");
  *out = nullptr;
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  DeviceGuard g(s->device);
  Guarded<rp_workspace> w(new rp_workspace());
  int rc = ws_alloc(s, w.get());
  if (rc) return rc;
  s->n_workspaces++;
  *out = w.release();
  return RP_OK;
}

void rp_workspace_destroy(rp_workspace* w) {
  if (!w || !w->scene) return;
  w->scene->n_workspaces--;
  Guarded<rp_workspace>{w};
}

int rp_workspace_reserve(rp_scene* s, rp_workspace* w, const rp_render_params* p) {
  int rc = use_ws(s, w);
  return rc ? rc : ws_reserve(s, w, p, true);
}

int rp_workspace_reserve_frames(rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t n_frames) {
  int rc = use_ws(s, w);
  return rc ? rc : ws_reserve(s, w, p, true, n_frames);
}

int rp_render_device(rp_scene* s, const rp_camera* cam, const rp_render_params* p, double* d_rgb, float* d_fg,
                     uint64_t* d_counters, void* stream) {
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  return render_shard(s, &s->ws0, cam, p, d_rgb, d_fg, d_counters, stream);
}

// (a NULL workspace is refused here: render_shard's check)
int rp_render_device_ws(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p, double* d_rgb,
                        float* d_fg, uint64_t* d_counters, void* stream) {
  return render_shard(s, w, cam, p, d_rgb, d_fg, d_counters, stream);
}

int rp_render_frames_device_ws(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p,
                               uint32_t n_frames, uint32_t frame_order, double* d_rgb, float* d_fg, uint64_t* d_counters,
                               void* stream) {
  if (!s) return fail(RP_EINVAL, "scene is NULL");
  return render_shard(s, w ? w : &s->ws0, cam, p, d_rgb, d_fg, d_counters, stream, n_frames, frame_order);
}

int rp_render(rp_scene* s, const rp_camera* cam, const rp_render_params* p, double* out_rgb, float* out_fg,
              rp_stats* stats) {
  if (!s || !cam || !out_rgb) return fail(RP_EINVAL, "scene, camera and output must be non-NULL");
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if ((rc = ws_reserve(s, &s->ws0, p, false))) return rc;
  DeviceGuard g(s->device);
  std::vector<double> shard(3 * (t.n_slots ? t.n_slots : 1));
  std::vector<float> shard_fg(out_fg ? (t.n_slots ? t.n_slots : 1) : 0);
  uint64_t ctr[rpk::CTR_N] = {0};
  double seconds = 0.0;
  DevBuf<double> d_rgb;
  DevBuf<float> d_fg;
  DevBuf<uint64_t> d_ctr;
  if (!d_rgb.alloc(shard.size()) || !d_ctr.alloc(rpk::CTR_N) || (out_fg && !d_fg.alloc(shard_fg.size())))
    return fail(RP_ENOMEM, "hipMalloc output");
  if ((rc = rpp::sync_call(s->device, "render", &seconds, [&](void* st) {
         return render_shard(s, &s->ws0, cam, p, d_rgb.get(), d_fg.get(), d_ctr.get(), st);
       })))
    return rc;
  if (hipMemcpy(shard.data(), d_rgb.get(), sizeof(double) * shard.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ctr, d_ctr.get(), sizeof ctr, hipMemcpyDeviceToHost) != hipSuccess ||
      (out_fg && hipMemcpy(shard_fg.data(), d_fg.get(), sizeof(float) * shard_fg.size(), hipMemcpyDeviceToHost) != hipSuccess))
    return fail(RP_EHIP, "copy back");
  if ((rc = rpp::check_status(ctr, nullptr))) return rc;
  if (t.n_slots) {
    std::vector<uint32_t> map;
    if (t.balanced) {
      map.resize(t.n_tiles);
      if ((rc = rp_workspace_tile_map(s, &s->ws0, p, map.data(), t.n_tiles))) return rc;
    }
    rpp::unpack_host(p, t, t.balanced ? map.data() : nullptr, shard.data(), sizeof(double), 3, out_rgb);
    if (out_fg) rpp::unpack_host(p, t, t.balanced ? map.data() : nullptr, shard_fg.data(), sizeof(float), 1, out_fg);
  }
  rpp::fill_stats(ctr, seconds, stats);
  return RP_OK;
}

}  // extern "C"
