// rp_accum.h -- the arithmetic of progressive accumulation (include/rp.h rp_accum_frames_device and
// rp_accum_error_device_ws), for host and device: the Welford update of a running mean, the variance of
// that mean, and a pixel's squared relative standard error.
//
// Every value is IEEE binary64, every expression is written in the operation order include/rp.h gives and compiled
// without contraction (-ffp-contract=off), only + - * / and comparisons, so the kernels (rp_accum.hip), the CPU loops
// behind rph_accum_frames and rph_accum_error (rp_host_passes.cpp) and the numpy model of the tests (tests/accum_ref.py,
// written from the definition and not from this file) agree to the last bit.
//
// Below the arithmetic: what the folds and the tile selection refuse about their arguments, for both libraries -- plain
// host functions that return the reason (NULL: fine), which the device entry points hand to fail() and the host ones
// prefix with their name.
#pragma once
#include <stdint.h>

#include "../../include/rp.h"
#include "rp_kernel.h"
#include "rp_overlap.h"

#if defined(__HIPCC__)
#define RPA_FN __host__ __device__ __forceinline__
#else
#define RPA_FN inline
#endif

namespace rpa {

// 1 / k for frame number k >= 1 (counted over all frames ever folded in): one division per frame, not one per word
RPA_FN double frame_weight(uint32_t k) { return 1.0 / (double)k; }

// One word, one frame: x is frame k's value, r = frame_weight(k).
//   d = x - mean; mean = mean + d * r; m2 = m2 + d * (x - mean)      -- the new mean
// From mean = 0.0, m2 = 0.0 at k = 1: d = x, mean = 0.0 + x * 1.0 = x bit for bit, m2 = 0.0 + x * (x - x) = 0.
RPA_FN void welford(double x, double r, double& mean, double& m2) {
  const double d = x - mean;
  mean = mean + d * r;
  m2 = m2 + d * (x - mean);
}

// The variance of the mean after n >= 2 frames: m2 / (n (n - 1)), the divisor nn = mean_divisor(n) once per call.
RPA_FN double mean_divisor(uint32_t n) { return (double)n * (double)(n - 1u); }
RPA_FN double mean_variance(double m2, double nn) { return m2 / nn; }

// One pixel: e2 = s / q, s = (v.r + v.g) + v.b, q = ((m.r m.r + m.g m.g) + m.b m.b) + eps -- the squared relative
// standard error, an absolute one (in units of sqrt(eps)) for dark pixels.
RPA_FN double error2(const double* m, const double* v, double eps) {
  const double s = (v[0] + v[1]) + v[2];
  const double q = ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + eps;
  return s / q;
}

// Neither NaN nor an infinity, by comparisons alone.
RPA_FN bool finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// rp_error_params with the zeros replaced by the defaults; false: out of range (tol > 0; eps > 0 and finite).
template <class P>
RPA_FN bool resolve(const P* in, double& tol, double& eps) {
  tol = in && in->tol != 0.0 ? in->tol : 0.05;
  eps = in && in->eps != 0.0 ? in->eps : 1e-4;
  return tol > 0.0 && eps > 0.0 && finite(eps);
}

// Tile selection (include/rp.h rp_accum_tiles_select_device).  A pixel is over when e2 > tol^2: a NaN
// compares false and is never over, +inf is.  Frame tile t of a W x H frame in tw x th tiles, tiles_x per row, holds
// tile_pixels in-frame pixels (t below the frame's tile count), and stays active when more than tile_share of them are
// over -- both sides as doubles, so over == tile_share * px exactly is not active.
RPA_FN bool pixel_over(const double* m, const double* v, double eps, double tol2) { return error2(m, v, eps) > tol2; }
RPA_FN uint32_t tile_pixels(uint32_t t, uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t tiles_x) {
  const uint32_t ox = (t % tiles_x) * tw, oy = (t / tiles_x) * th;
  const uint32_t nx = W - ox < tw ? W - ox : tw, ny = H - oy < th ? H - oy : th;
  return nx * ny;
}
RPA_FN bool tile_active(uint32_t over, uint32_t px, double tile_share) {
  return (double)over > tile_share * (double)px;
}

// The four statistics of an error pass (RP_ERROR_STATS_LEN): all order-free -- integer sums and an integer maximum of
// the bit patterns of positive doubles, which order as the doubles do.
enum { STAT_PIXELS = 0, STAT_OVER = 1, STAT_MAX_BITS = 2, STAT_NONFINITE = 3, STATS_LEN = 4 };

// ---- the entry points' refusals (host side of both libraries)

constexpr uint64_t MAX_WORDS = (1ull << 40) - 512;  // of a fold's state: its lanes fit 2^31 - 1 blocks of 256

// frames, then mean, m2 and var (NULL: not wanted) of state_bytes each: no output aliases the frames, nor another.
inline const char* check_state_alias(const double* frames, uint64_t in_bytes, const double* mean, const double* m2,
                                     const double* var, uint64_t state_bytes) {
  using rpo::overlaps;
  if (overlaps(mean, state_bytes, frames, in_bytes) || overlaps(m2, state_bytes, frames, in_bytes) ||
      overlaps(var, state_bytes, frames, in_bytes))
    return "mean, m2 and var must not alias the frames";
  if (overlaps(mean, state_bytes, m2, state_bytes) || overlaps(var, state_bytes, mean, state_bytes) ||
      overlaps(var, state_bytes, m2, state_bytes))
    return "mean, m2 and var must not alias one another";
  return nullptr;
}

// The plain and the tile fold.  A frame of the call holds n_in blocks of block_words words and the state (mean, m2, var)
// n_state such blocks.  The plain fold (listed = false) is one block of n_words in both, without a list; the tile fold
// n_listed and n_state_tiles blocks of tile_words, tiles naming the state block of each listed one.  n_in = 0 (an empty
// list) is fine: nothing is read, so nothing can alias.
inline const char* check_fold(bool listed, uint64_t block_words, uint32_t n_in, uint32_t n_state, const uint32_t* tiles,
                              uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride,
                              const double* mean, const double* m2, const double* var) {
  if (!frames || !mean || !m2) return "frames, mean and m2 must be non-NULL";
  if (block_words == 0) return listed ? "tile_words is zero" : "n_words is zero";
  if (n_in > n_state) return "n_listed is above n_state_tiles";
  if (listed && n_in && !tiles) return "tiles must be non-NULL";
  if (block_words > MAX_WORDS / (n_state ? n_state : 1u))
    return "the state is above 2^40 - 512 words (n_words, or n_state_tiles * tile_words)";
  if (n_frames == 0) return "n_frames is zero: nothing to fold in";
  const uint64_t in_words = n_in * block_words;
  if (frame_stride < in_words)
    return "frame_stride is below a frame's words (n_words, or n_listed * tile_words): the frames would overlap";
  const uint64_t n = (uint64_t)n_prior + n_frames;
  if (n > 0x7fffffffu) return "more than 2^31 - 1 frames (n_prior + n_frames)";
  if (var && n < 2) return "the variance needs at least two frames (n_prior + n_frames >= 2)";
  if (n_in == 0) return nullptr;
  // byte counts: the words are below 2^40 here; a stride that wraps 64 bits is the caller's address space running out
  const uint64_t in_bytes = 8 * ((uint64_t)(n_frames - 1) * frame_stride + in_words);
  const uint64_t state_bytes = 8 * ((uint64_t)n_state * block_words), list_bytes = 4ull * n_in;
  if (rpo::overlaps(mean, state_bytes, tiles, list_bytes) || rpo::overlaps(m2, state_bytes, tiles, list_bytes) ||
      rpo::overlaps(var, state_bytes, tiles, list_bytes))
    return "mean, m2 and var must not alias the list";
  return check_state_alias(frames, in_bytes, mean, m2, var, state_bytes);
}

// The fold with the frame number taken per pixel.
inline const char* check_fold_counts(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* frames,
                                     uint64_t frame_stride, const uint32_t* count, const double* mean, const double* m2,
                                     const double* var, double var_one) {
  using rpo::overlaps;
  if (!frames || !mean || !m2 || !count) return "frames, count, mean and m2 must be non-NULL";
  if (n_pixels == 0 || words_per_pixel == 0) return "n_pixels or words_per_pixel is zero";
  if (n_frames == 0) return "n_frames is zero: nothing to fold in";
  if (n_frames > 0x7fffffffu) return "more than 2^31 - 1 frames";
  if (n_pixels > MAX_WORDS / words_per_pixel) return "n_pixels * words_per_pixel is above 2^40 - 512";
  const uint64_t n_words = n_pixels * words_per_pixel;
  if (frame_stride < n_words) return "frame_stride is below n_pixels * words_per_pixel: the frames would overlap";
  if (!(var_one >= 0.0 && finite(var_one))) return "var_one must be finite and >= 0";
  const uint64_t in_bytes = 8 * ((uint64_t)(n_frames - 1) * frame_stride + n_words), state_bytes = 8 * n_words;
  const uint64_t count_bytes = 4 * n_pixels;
  if (const char* why = check_state_alias(frames, in_bytes, mean, m2, var, state_bytes)) return why;
  if (overlaps(count, count_bytes, frames, in_bytes) || overlaps(count, count_bytes, mean, state_bytes) ||
      overlaps(count, count_bytes, m2, state_bytes) || overlaps(count, count_bytes, var, state_bytes))
    return "count must not alias the frames or the state";
  return nullptr;
}

// Tile selection, after the frame's tiling is made: the state is a whole frame's (shards, shard_map: the tiling's and
// the params'), the error params resolve into tol and eps, tile_share is in [0, 1) and the list fits the compaction.
template <class P>
inline const char* check_select(uint32_t shards, uint32_t shard_map, const P* error, double tile_share, uint32_t n_in,
                                double& tol, double& eps) {
  if (shards != 1 || shard_map != RP_SHARD_INTERLEAVE)
    return "the state is a whole frame's: num_shards 0 or 1, shard 0, interleave";
  if (!resolve(error, tol, eps)) return "error params out of range (tol > 0; eps > 0 and finite)";
  if (!(tile_share >= 0.0 && tile_share < 1.0)) return "tile_share must be in [0, 1)";
  if (n_in > (uint32_t)rpk::TILE_SORT_MAX) return "n_in is above 16384 (rpk::TILE_SORT_MAX)";
  return nullptr;
}

}  // namespace rpa
