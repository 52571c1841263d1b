// rp_units.h -- the unit fetch of the render kernel, for host and device: which (pixel, sample batch) unit a lane takes
// next from the unit queues, and what a unit's batch number says about its frame, its samples and its RNG stream.
//
// The render kernel (rp_kernel.hip, through rp_device.h's DevEnv) and the host library's test hook (rp_host.h
// rph_unit_walk, through rp_host_sched.cpp's HostEnv) compile this one text, so tests/test_unit_queues.py walks the kernel's
// own queues on the CPU: every unit of every frame exactly once, at the right pixel.
//
// ---- queue order
//
// A launch hands out n_queue units.  Their order: the shard's tiles (in cost or Z-order when tile_order is set), inside
// a tile the pixels row-major, each pixel's batches consecutive; slots of edge tiles outside the frame are skipped.
// With several frames per launch (KParams::n_frames) the tiles are n_frames x n_shard_tiles virtual tiles -- frame by
// frame, or rank by rank (frames_inter 1), or rank by rank with a unit's frames consecutive (frames_inter 2) -- and a
// unit carries its global batch f * nbatch + b.  With a learned unit_order the queues hand out its positions instead of
// tiles.  A probe launch (PROBE, probe_n > 0) has one queue word and takes an n x n lattice of pixels per tile.
//
// ---- the walk over the queues, and what it relies on
//
// There are G = queue_groups queues (1, or one per XCD); queue g's word is queue[g * QUEUE_STRIDE], and it serves the
// chunks g, g + G, ... of C consecutive tiles (or positions) of the order.  A block's home queue is block mod G.
//  * A fetch touches only the words of the queues g < G (a probe: word 0 of the queue pointer it was given), one
//    increment per loop trip, and starts at its home queue every time: a drained queue costs one failed increment.
//  * `tries` moves for the whole wave: once any lane of the wave finds queue home + tries drained, every lane goes on
//    to the next queue, whether its own increment still got an entry (it keeps that entry) or not.  The queue a wave
//    increments is therefore wave-uniform, and the compiler folds the lanes' atomicAdd into one wave atomic (ballot +
//    mbcnt); a per-lane atomic on one word cost C3 +35 %.
//  * g = home + tries stays below 2 G before its one conditional subtraction, so queue g is below G.  `tries` grows
//    only when a lane of the wave found queue home + tries drained, and a queue word never decreases, so a drained
//    queue stays drained: when tries reaches G every queue has been seen drained, the fetch at tries = G (the home
//    queue again) is drained for the lane itself, and the lane returns false.  A lane that is itself drained returns
//    as soon as tries >= G.  So tries <= G at every loop entry, and home < G.
//  * Every numerator of RPK_UDIV is below 2^31 (make_div32's range): all are queue entries, positions or slots of a
//    launch that rps::launch_limits admitted (n_queue < 2^31).
#pragma once
#include <stdint.h>

#include "rp_kernel.h"

#if defined(__HIPCC__)
#define RPU_FN __host__ __device__ __forceinline__
#else
#include <algorithm>
#define RPU_FN inline
#endif

namespace rpk {

#if !defined(__HIPCC__)
using std::max;
using std::min;
#endif

// All launch arguments in one kernarg struct.  The persistent loop re-reads the fields it needs through
// a laundered pointer to the kernarg segment (scalar loads, served by the constant cache) instead of
// keeping ~70 uniform values live in SGPRs for the whole kernel: that SGPR pressure otherwise spills
// into VGPR lanes and halves the wave occupancy of this register-bound kernel.
struct KArgs {
  KScene S;
  KParams P;
  double* out;
  float* out_fg;
  unsigned long long* ctr;
  unsigned int* queue;       // the unit queue's next index (workspace-owned, zeroed before the launch)
  unsigned long long* diag;  // RPK_DIAG builds only (DIAG_N counters)
};
#if defined(__HIPCC__)
typedef const __attribute__((address_space(4))) KArgs* KArgsPtr;
#endif

RPU_FN uint32_t udiv(uint32_t n, uint32_t m, uint32_t s) { return (uint32_t)(((uint64_t)n * m) >> s); }  // rp_kernel.h make_div32
#define RPK_UDIV(n, dv) udiv((n), A->P.dv.m, A->P.dv.s)

// Pull the next unit (pixel, sample batch) of the shard from the unit queues (the order and the walk: see the top of
// this file).  Returns false when every queue is drained.  E is the environment the fetch runs in (rp_device.h DevEnv
// on the GPU): args() the launch's KArgs, fetch_add(p) an atomic increment returning the old value, any(x) whether x
// holds for any lane of the wave, uniform(x) a wave-uniform x as a scalar, block() the block's index, numerator(n) the
// n of an RPK_UDIV (the host environment checks its range).
#define RPU_EDIV(n, dv) RPK_UDIV(E::numerator(n), dv)
template <bool PROBE, class E>
RPU_FN bool fetch_pixel(uint32_t& slot, uint32_t& pi, uint32_t& pj, uint32_t& batch) {
  auto A = E::args();
  unsigned int* queue = A->queue;
  const uint32_t tw = A->P.tw, th = A->P.th;
  if (PROBE && A->P.probe_n) {  // cost probe: an n x n lattice per tile (cell centres), clamped into the frame
    slot = E::fetch_add(queue);
    if ((uint64_t)slot >= A->P.n_queue) return false;
    batch = 0;
    const uint32_t n = A->P.probe_n;
    const uint32_t k = slot / A->P.probe_px, sub = slot % A->P.probe_px;
    const uint32_t dk = A->P.shard + k * A->P.nshards, t = A->P.tile_map ? A->P.tile_map[dk] : dk;
    const uint32_t tx = t % A->P.tiles_x, ty = t / A->P.tiles_x;
    pi = min(tx * tw + min((sub % n) * tw / n + tw / (2u * n), tw - 1u), A->P.W - 1u);
    pj = min(ty * th + min((sub / n) * th / n + th / (2u * n), th - 1u), A->P.H - 1u);
    return true;
  }
  const uint32_t tile_px = tw * th, tile_units = tile_px * A->P.nbatch;
  if (!PROBE && A->P.unit_order) {
    // the learned per-unit order (rp_sched.hip): queue g serves the chunks g, g + G, ... of C consecutive positions,
    // position p holds unit unit_order[p] = slot * nbatch + batch -- with several frames per launch, position p is frame
    // p mod n_frames of unit unit_order[p / n_frames] (a unit's frames consecutive); the same drained-queue walk as the
    // tile queues below
    const uint32_t G = max(A->P.queue_groups, 1u), C = A->P.order_chunk, GC = G * C;
    const uint32_t home = G > 1 ? E::block() % G : 0u;
    const uint32_t Q = (uint32_t)A->P.n_queue;
    for (uint32_t tries = 0;;) {
      uint32_t g = home + tries;
      if (g >= G) g -= G;
      g = E::uniform(g);
      const uint32_t rest = Q % GC, nq = (Q / GC) * C + min(rest - min(rest, g * C), C);
      const uint32_t q = E::fetch_add(A->queue + g * QUEUE_STRIDE);
      const bool drained = q >= nq;
      if (E::any(drained)) {
        ++tries;
        if (drained) {
          if (tries >= G) return false;
          continue;
        }
      }
      const uint32_t i = RPU_EDIV(q, dv_ochunk);
      uint32_t pos = i * GC + g * C + (q - i * C), f = 0;
      if (A->P.n_frames > 1) {
        const uint32_t r = RPU_EDIV(pos, dv_frames);
        f = pos - r * A->P.n_frames;
        pos = r;
      }
      const uint32_t u = A->P.unit_order[pos];
      const uint32_t sl = RPU_EDIV(u, dv_nbatch);
      batch = u - sl * A->P.nbatch + f * A->P.nbatch;  // (the unit carries its global batch)
      slot = sl;
      const uint32_t k = RPU_EDIV(sl, dv_tile_px), local = sl - k * tile_px;
      const uint32_t dk = A->P.shard + k * A->P.nshards, t = A->P.tile_map ? A->P.tile_map[dk] : dk;
      const uint32_t ty = RPU_EDIV(t, dv_tiles_x), tx = t - ty * A->P.tiles_x;
      const uint32_t lj = RPU_EDIV(local, dv_tw), li = local - lj * tw;
      pi = tx * tw + li;
      pj = ty * th + lj;
      if (pi < A->P.W && pj < A->P.H) return true;
    }
  }
  // Per-XCD queues (rp.h RP_QUEUES_*): blocks blockIdx mod G share an XCD; their queue g serves the tiles
  // k = g, g + G, ... of the order (or the g-th run of it), and once it is drained they take units from the
  // next queues in turn.
  // several frames per launch: n_frames x n_shard_tiles virtual tiles (rp_kernel.h KParams::n_frames)
  const uint32_t G = max(A->P.queue_groups, 1u), K = A->P.n_shard_tiles * (PROBE ? 1u : A->P.n_frames);
  const uint32_t home = G > 1 ? E::block() % G : 0u;
  for (uint32_t tries = 0;;) {
    uint32_t g = home + tries;
    if (g >= G) g -= G;
    g = E::uniform(g);
    // queue g serves the chunks g, g + G, ... of C consecutive tiles of the order: tile k of its i-th unit
    // run is (i / C) * G * C + g * C + i % C
    const uint32_t C = A->P.queue_chunk, GC = G * C;
    const uint32_t rest = K % GC, nk = (K / GC) * C + min(rest - min(rest, g * C), C);
    const uint32_t q = E::fetch_add(queue + g * QUEUE_STRIDE);
    const bool drained = (uint64_t)q >= (uint64_t)nk * tile_units;
    if (E::any(drained)) {
      ++tries;
      if (drained) {
        if (tries >= G) return false;  // every queue drained
        continue;
      }
    }
    // (PROBE launches decode with plain divisions: one small launch)
    uint32_t i = PROBE ? q / tile_units : RPU_EDIV(q, dv_units);
    uint32_t rem = q - i * tile_units;
    if (!PROBE && A->P.frames_inter == 2u) {
      // RP_FRAME_ORDER_PIXEL: the n_frames consecutive virtual tiles of a queue's sequence (one shard tile of every
      // frame) as one run of units with a unit's frames consecutive -- a wave holds ~64 / n_frames pixels x their frames
      const uint32_t grp = RPU_EDIV(i, dv_frames);
      const uint32_t o = (i - grp * A->P.n_frames) * tile_units + rem;
      const uint32_t u = RPU_EDIV(o, dv_frames);
      i = grp * A->P.n_frames + (o - u * A->P.n_frames);
      rem = u;
    }
    const uint32_t ic = PROBE ? i / C : RPU_EDIV(i, dv_chunk);
    uint32_t k = ic * GC + g * C + (i - ic * C);
    // a tile's units pixel-major, a pixel's batches consecutive: a wave fetches 64 / nbatch pixels with all
    // their batches, whose camera rays traverse nearly the same nodes (C3 -0.9 %, C5 -0.9 % against
    // batch-major, ab32)
    const uint32_t local = PROBE ? rem / A->P.nbatch : RPU_EDIV(rem, dv_nbatch);
    batch = rem - local * A->P.nbatch;
    if (!PROBE && A->P.n_frames > 1) {  // virtual tile -> frame f, its tile k; the unit carries its global batch
      uint32_t f;
      if (A->P.frames_inter) {
        const uint32_t r = RPU_EDIV(k, dv_frames);
        f = k - r * A->P.n_frames;
        k = r;
      } else {
        f = RPU_EDIV(k, dv_tiles);
        k -= f * A->P.n_shard_tiles;
      }
      batch += f * A->P.nbatch;
    }
    if (!PROBE && A->P.tile_order) k = A->P.tile_order[k];  // the queue hands out shard tiles in cost order
    slot = k * tile_px + local;                     // output slot: shard tile order (rp_shard_unpack)
    const uint32_t dk = A->P.shard + k * A->P.nshards, t = A->P.tile_map ? A->P.tile_map[dk] : dk;
    const uint32_t ty = PROBE ? t / A->P.tiles_x : RPU_EDIV(t, dv_tiles_x), tx = t - ty * A->P.tiles_x;
    const uint32_t lj = PROBE ? local / tw : RPU_EDIV(local, dv_tw), li = local - lj * tw;
    pi = tx * tw + li;
    pj = ty * th + lj;
    if (pi < A->P.W && pj < A->P.H) return true;
  }
}
#undef RPU_EDIV

// A shard slot's pixel (rp_shard_unpack's order): slot = k * tw * th + the row-major offset inside shard tile k, which
// is position shard + k * nshards of the frame's deal order (the tile index itself, or tile_map's entry).  Returns
// whether the pixel lies in the frame: slots of edge tiles outside it hold nothing.  P: the launch's KParams.
template <class KP, class Slot>
RPU_FN bool slot_pixel(const KP& P, Slot slot, uint32_t& pi, uint32_t& pj) {
  const uint32_t tile_px = P.tw * P.th, k = (uint32_t)(slot / tile_px), local = (uint32_t)(slot % tile_px);
  const uint32_t dk = P.shard + k * P.nshards, t = P.tile_map ? P.tile_map[dk] : dk;
  pi = (t % P.tiles_x) * P.tw + local % P.tw;
  pj = (t / P.tiles_x) * P.th + local / P.tw;
  return pi < P.W && pj < P.H;
}

// RNG contract (include/rp.h): batch b of pixel (i, j) is its own StdRng stream,
// seed_from_u64(seed + b * W * H + j * W + i); batch 0 is the per-pixel stream of the original contract.
// (A: a pointer to the launch's KArgs -- the kernels' KArgsPtr, a plain const KArgs* on the host.)
template <class AP>
RPU_FN uint64_t unit_seed(AP A, uint32_t pi, uint32_t pj, uint32_t batch) {
  return A->P.seed + (uint64_t)batch * A->P.W * A->P.H + (uint64_t)pj * A->P.W + pi;
}
// The frame of a unit's (global) batch and its batch within the frame (several frames per launch: KParams::n_frames).
template <class AP>
RPU_FN uint32_t unit_frame(AP A, uint32_t batch) { return A->P.n_frames > 1 ? RPK_UDIV(batch, dv_nbatch) : 0u; }
// Samples in this unit's batch.
template <class AP>
RPU_FN uint32_t unit_spp(AP A, uint32_t batch) {
  const uint32_t b = batch - unit_frame(A, batch) * A->P.nbatch;
  return min(A->P.spp_batch, A->P.spp - b * A->P.spp_batch);
}

}  // namespace rpk
