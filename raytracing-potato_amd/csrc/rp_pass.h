// rp_pass.h -- what the passes around the render kernel share, each written once: the feature pass (rp_aov.hip), the
// denoisers (rp_denoise.hip), the batch variance (rp_variance.hip), progressive accumulation (rp_accum.hip) and the
// tile-list launch and selection (rp_tiles.hip).  A new pass includes this header and copies none of it (DESIGN.md
// 4.15); the render itself (rp_render.cpp) takes its camera fill, launch prelude, host unpack and synchronous call from
// here as well.  Internal to librp.so, as rp_state.h.
#pragma once
#include <cmath>
#include <cstring>

#include "rp_overlap.h"
#include "rp_state.h"

#pragma GCC visibility push(hidden)

namespace rpp {

using rpo::overlaps;  // (rp_overlap.h: the host library's checks use the same one)

// The fields rpk::slot_pixel (rp_units.h) reads to decode a shard slot, under KParams' names, and the slot count: what
// a kernel with one lane per shard slot takes beside its own arguments.
struct ShardView {
  uint32_t W, H, tw, th, shard, nshards, tiles_x;
  uint64_t n_slots;
  const uint32_t* tile_map;  // the balanced plan's deal order (NULL = interleave)
};

// The shard of params as a pass after the render sees it: its tiling, and its view in v (a ShardView, or the KParams of
// a pass that launches with one).  A balanced shard holds the tiles of the beauty shard rendered before it, so the plan
// that render left in the workspace must be this frame's.
template <class KP>
int shard_view(const rp_workspace* w, const rp_render_params* p, Tiling& t, KP& v) {
  const int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (t.balanced && !w->plan_matches(p, t))
    return fail(RP_EINVAL, "no balanced plan for this frame in the workspace: render it first");
  v.W = p->width, v.H = p->height, v.tw = t.tw, v.th = t.th, v.shard = t.shard, v.nshards = t.shards;
  v.tiles_x = t.tiles_x;
  v.n_slots = t.n_slots;
  v.tile_map = t.balanced ? w->d_plan.get() : nullptr;
  return RP_OK;
}

// The camera's fields of a launch.
inline void set_camera(rpk::KParams& kp, const rp_camera* cam) {
  std::memcpy(kp.orient, cam->orientation, sizeof kp.orient);
  std::memcpy(kp.pos, cam->position, sizeof kp.pos);
  kp.aspect = cam->aspect_ratio;
  kp.tan_fov = std::tan(0.5 * cam->fov);  // render.rs:33, hoisted: a per-camera constant
  kp.focal = cam->focal_dist;
  kp.lens = cam->lens_radius;
}

// A render launch's prelude on the workspace, in two steps with the launch's early returns (an empty shard, spp = 0,
// the launch limits) between them.
// First: the last frame gather on this workspace (another stream, perhaps) has read d_meas and written d_fcost --
// whichever launch follows a gather waits for it -- and the launch's counters start at zero.
inline int launch_begin(rp_workspace* w, uint64_t* d_counters, hipStream_t st) {
  if (w->gathered_pending) {
    RP_HIP(hipStreamWaitEvent(st, w->ev_gathered.get(), 0));
    w->gathered_pending = false;
  }
  RP_HIP(hipMemsetAsync(d_counters, 0, sizeof(uint64_t) * rpk::CTR_N, st));
  return RP_OK;
}
// Then: the scene as the render kernel sees it with this workspace's keystream slab, spill and unit start times, and
// the queue words cleared.
inline int launch_bind(const rp_scene* s, rp_workspace* w, rpk::KScene& ks, hipStream_t st) {
  ks = s->ks;
  ks.rng_slab = reinterpret_cast<uint32_t*>(w->d_slab.get());
  ks.spill = w->d_spill.get();
  ks.unit_t0 = w->d_t0.get();
  RP_HIP(hipMemsetAsync(w->d_queue.get(), 0, sizeof(uint32_t) * rpk::QUEUE_WORDS, st));
  return RP_OK;
}

// Scatter a compact shard buffer into a frame on the host (rp_shard_unpack), tiles dealt by `map` (the deal order of a
// balanced plan) or the interleave (map NULL).
inline void unpack_host(const rp_render_params* p, const Tiling& t, const uint32_t* map, const void* shard_buf,
                        size_t elem, uint32_t channels, void* frame) {
  const uint64_t tile_px = (uint64_t)t.tw * t.th;
  const char* src = static_cast<const char*>(shard_buf);
  char* dst = static_cast<char*>(frame);
  for (uint32_t k = 0; k < t.n_shard_tiles; k++) {
    const uint32_t dk = t.shard + k * t.shards, tile = map ? map[dk] : dk;
    const uint32_t ox = (tile % t.tiles_x) * t.tw, oy = (tile / t.tiles_x) * t.th;
    for (uint32_t lj = 0; lj < t.th && oy + lj < p->height; lj++)
      for (uint32_t li = 0; li < t.tw && ox + li < p->width; li++)
        std::memcpy(dst + ((uint64_t)(oy + lj) * p->width + ox + li) * channels * elem,
                    src + (k * tile_px + (uint64_t)lj * t.tw + li) * channels * elem, channels * elem);
  }
}

// A synchronous call around a device-side one: `enqueue(stream)` runs on a non-blocking stream of its own between two
// events, the call returns once the stream has drained, and *seconds is the time between the events.  Allocation and
// copies stay with the caller, before and after.  what: the pass's name in a failed synchronisation's message.
template <class Enqueue>
int sync_call(int device, const char* what, double* seconds, Enqueue enqueue) {
  DeviceGuard g(device);
  Stream st;
  Event e0, e1;
  if (hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking) != hipSuccess) return fail(RP_EHIP, "stream");
  if (hipEventCreate(e0.put()) != hipSuccess || hipEventCreate(e1.put()) != hipSuccess) return fail(RP_EHIP, "event");
  (void)hipEventRecord(e0.get(), st.get());
  const int rc = enqueue(static_cast<void*>(st.get()));
  if (rc) return rc;
  (void)hipEventRecord(e1.get(), st.get());
  const hipError_t e = hipStreamSynchronize(st.get());
  if (e != hipSuccess) return fail(RP_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0.get(), e1.get());
  *seconds = ms * 1e-3;
  return RP_OK;
}

// A counter block (rpk::CTR_*) read back: its status bits as refusals -- pass: what to call a pass that has no other
// status bit than the overflow (NULL: only the overflow is looked at, as rp_render does) -- and its counts as rp_stats.
inline int check_status(const uint64_t* ctr, const char* pass) {
  if (ctr[rpk::CTR_STATUS] & rpk::STATUS_STACK_OVERFLOW) return fail(RP_EINTERNAL, "traversal stack overflow");
  if (pass && ctr[rpk::CTR_STATUS]) return fail(RP_EINTERNAL, std::string("the ") + pass + " reported a status bit");
  return RP_OK;
}
inline void fill_stats(const uint64_t* ctr, double seconds, rp_stats* stats) {
  if (!stats) return;
  stats->rays = ctr[rpk::CTR_RAYS];
  stats->samples = ctr[rpk::CTR_SAMPLES];
  stats->pixels = ctr[rpk::CTR_PIXELS];
  stats->seconds = seconds;
}

}  // namespace rpp

#pragma GCC visibility pop
