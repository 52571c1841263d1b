// rp_tiles.hip -- tile-adaptive progressive rendering (include/rp.h rp_render_tiles_device_ws and
// rp_accum_tiles_select_device): a render launch over a caller-given list of frame tiles, and the pass
// that picks the tiles still over the error tolerance.  (The third piece, the fold of such a launch into whole-frame
// state, shares accum_kernel's per-lane body and lives in rp_accum.hip.)
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like rp_accum.hip, not part of the
// rp_build_id hash.  The render launch is host code only: the unchanged render kernel (rpk::launch_render) already
// resolves a shard tile through tile_map and n_shard_tiles, so the list is handed to it as the tile map of a one-shard
// launch of n_listed tiles (rp_schedule.h plan_tiles_launch: the arithmetic).  No stage of render_shard's scheduling runs
// and nothing is measured: the workspace's learned state (tile costs, unit durations, plan, cost table) is neither read
// nor written.
//
// tile_over_kernel: one block per listed tile.  A lane reads its pixel's 48 bytes (3 doubles of mean, 3 of variance) as
// error_kernel does; the wave counts its pixels over by ballot and popcount, the block adds its four waves' counts
// through LDS, and one lane stores the tile's count and its active flag with plain stores -- no atomics, so nothing to
// clear.  compact_kernel: one block of 1024 lanes, 16 consecutive entries per lane (16384 = rpk::TILE_SORT_MAX): every
// lane reads its entries' flags and tile indices, then an exclusive scan of the lanes' counts (shuffles in the wave, the
// 16 wave totals through LDS) gives each lane where its active tiles go -- a stable compaction.  The flags live in the
// output list itself: position k of the output is never beyond entry k, and every flag is read before the barrier that
// precedes the first write.  Both passes move a few megabytes next to a render launch of hundreds of milliseconds; they
// are kept this simple on purpose (no vector loads, no second tile per block).
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers the shared headers use

#include "rp_accum.h"

#pragma clang fp contract(off)

namespace rpt {

constexpr int OVER_BLOCK = 256;
constexpr int OVER_WAVES = OVER_BLOCK / 64;
constexpr int SCAN_BLOCK = 1024;
constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
constexpr int SCAN_ITEMS = rpk::TILE_SORT_MAX / SCAN_BLOCK;  // entries per lane
static_assert(SCAN_ITEMS * SCAN_BLOCK == rpk::TILE_SORT_MAX && SCAN_ITEMS <= 32, "a lane's entries fit a 32-bit mask");

struct SelArgs {
  uint32_t W, H, tw, th, tiles_x, n_tiles, n_in;
  const uint32_t* tiles_in;  // NULL: the identity list
  const double* mean;        // 3 per slot, frame tile t at slot t * tw * th
  const double* var;
  double tol2, eps, tile_share;
  uint32_t* over;   // NULL: not wanted
  uint32_t* flags;  // the output list's buffer: entry k's active flag until compact_kernel replaces it
  uint32_t* count;
};

__global__ void __launch_bounds__(OVER_BLOCK) tile_over_kernel(const SelArgs A) {
  __shared__ uint32_t part[OVER_WAVES];
  const uint32_t k = blockIdx.x;
  const uint32_t t = A.tiles_in ? A.tiles_in[k] : k;
  const bool in_frame = t < A.n_tiles;  // the same for the whole block
  uint32_t n_over = 0;                  // the wave's count, the same in all its lanes
  if (in_frame) {
    const uint32_t tile_px = A.tw * A.th;
    const uint32_t ox = (t % A.tiles_x) * A.tw, oy = (t / A.tiles_x) * A.th;
    // (the same trip count for every lane of the block: the ballot is reached by all)
    for (uint32_t base = 0; base < tile_px; base += OVER_BLOCK) {
      const uint32_t local = base + threadIdx.x;
      bool over = false;
      if (local < tile_px && ox + local % A.tw < A.W && oy + local / A.tw < A.H) {
        const uint64_t slot = (uint64_t)t * tile_px + local;
        over = rpa::pixel_over(A.mean + 3 * slot, A.var + 3 * slot, A.eps, A.tol2);
      }
      n_over += (uint32_t)__popcll(__ballot(over));
    }
  }
  if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = n_over;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t v = part[0];
#pragma unroll
    for (int i = 1; i < OVER_WAVES; i++) v += part[i];
    if (A.over) A.over[k] = v;
    A.flags[k] = in_frame && rpa::tile_active(v, rpa::tile_pixels(t, A.W, A.H, A.tw, A.th, A.tiles_x), A.tile_share);
  }
}

__global__ void __launch_bounds__(SCAN_BLOCK) compact_kernel(const SelArgs A) {
  __shared__ uint32_t wave_total[SCAN_WAVES];
  const uint32_t first = threadIdx.x * SCAN_ITEMS, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  uint32_t ids[SCAN_ITEMS];
  uint32_t mask = 0, cnt = 0;
#pragma unroll
  for (int u = 0; u < SCAN_ITEMS; u++) {
    const uint32_t j = first + u;
    ids[u] = 0;
    if (j < A.n_in) {
      ids[u] = A.tiles_in ? A.tiles_in[j] : j;
      if (A.flags[j]) mask |= 1u << u, cnt++;
    }
  }
  __syncthreads();  // every flag is read: the list may now be written over them
  uint32_t inc = cnt;  // inclusive scan of the wave's counts
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < SCAN_WAVES; i++) {
    const uint32_t v = wave_total[i];
    before += (uint32_t)i < wave ? v : 0u;
    total += v;
  }
  uint32_t pos = before + inc - cnt;
#pragma unroll
  for (int u = 0; u < SCAN_ITEMS; u++)
    if (mask >> u & 1u) A.flags[pos++] = ids[u];
  if (threadIdx.x == 0) A.count[0] = total;
}

}  // namespace rpt

extern "C" {

int rp_render_tiles_device_ws(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p,
                              const uint32_t* d_tiles, uint32_t n_listed, uint32_t n_frames, uint32_t frame_order,
                              double* d_rgb, float* d_fg, uint64_t* d_counters, void* stream) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  w->frame_flags = 0;  // before any return, as render_shard: a tile-list launch reports no scheduling
  if (!cam || !p || !d_rgb || !d_counters || (n_listed && !d_tiles))
    return fail(RP_EINVAL, "camera, params, d_tiles, d_rgb and d_counters must be non-NULL");
  rps::LaunchPlan lp;
  rps::Refusal refused = rps::plan_tiles_launch(p, n_listed, n_frames, frame_order, s->opt, lp);
  if (refused.code) return fail(refused.code, refused.msg);
  rpk::KParams& kp = lp.kp;
  const hipStream_t st = (hipStream_t)stream;
  DeviceGuard g(s->device);
  // render_shard's prelude: this launch touches none of what a frame gather reads or writes, but whichever launch
  // follows a gather orders the workspace's streams the same way
  if ((rc = rpp::launch_begin(w, d_counters, st))) return rc;
  if (n_listed == 0) return RP_OK;
  refused = rps::launch_limits(lp, s->lanes());
  if (refused.code) return fail(refused.code, refused.msg);
  rpp::set_camera(kp, cam);
  kp.tile_map = d_tiles;  // shard tile k of the one-shard launch is frame tile d_tiles[k]
  rpk::KScene ks;         // (its unit_t0 is unread: nothing is measured)
  if ((rc = rpp::launch_bind(s, w, ks, st))) return rc;
  RP_LAUNCH("tile-list render", rpk::launch_render(ks, kp, d_rgb, d_fg, d_counters, w->d_queue.get(),
                                                   rps::grid_for(kp.n_queue, s->resident()), stream));
  return RP_OK;
}

int rp_accum_tiles_select_device(const rp_render_params* p, const rp_error_params* e, double tile_share,
                                 const double* d_mean, const double* d_var, const uint32_t* d_tiles_in, uint32_t n_in,
                                 uint32_t* d_over, uint32_t* d_tiles_out, uint32_t* d_count, void* stream) {
  if (!d_mean || !d_var || !d_tiles_out || !d_count)
    return fail(RP_EINVAL, "d_mean, d_var, d_tiles_out and d_count must be non-NULL");
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  double tol, eps;
  if (const char* why = rpa::check_select(t.shards, p->shard_map, e, tile_share, n_in, tol, eps)) return fail(RP_EINVAL, why);
  const uint64_t list_bytes = 4ull * n_in;
  if (rpp::overlaps(d_tiles_out, list_bytes, d_tiles_in, list_bytes) || rpp::overlaps(d_tiles_out, list_bytes, d_over, list_bytes) ||
      rpp::overlaps(d_count, 4, d_tiles_out, list_bytes) || rpp::overlaps(d_count, 4, d_over, list_bytes))
    return fail(RP_EINVAL, "d_tiles_out must not alias d_tiles_in or d_over, nor d_count either output");
  rpt::SelArgs a;
  a.W = p->width, a.H = p->height, a.tw = t.tw, a.th = t.th, a.tiles_x = t.tiles_x, a.n_tiles = t.n_tiles, a.n_in = n_in;
  a.tiles_in = d_tiles_in;
  a.mean = d_mean, a.var = d_var;
  a.tol2 = tol * tol, a.eps = eps, a.tile_share = tile_share;
  a.over = d_over, a.flags = d_tiles_out, a.count = d_count;
  if (n_in) {
    hipLaunchKernelGGL(rpt::tile_over_kernel, dim3(n_in), dim3(rpt::OVER_BLOCK), 0, (hipStream_t)stream, a);
    RP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rpt::compact_kernel, dim3(1), dim3(rpt::SCAN_BLOCK), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

}  // extern "C"
