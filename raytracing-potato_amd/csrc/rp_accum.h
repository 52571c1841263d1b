// rp_accum.h -- the arithmetic of progressive accumulation (include/rp.h rp_accum_frames_device and
// rp_accum_error_device_ws), for host and device: the Welford update of a running mean, the variance of
// that mean, and a pixel's squared relative standard error.
//
// Every value is IEEE binary64, every expression is written in the operation order include/rp.h gives and compiled
// without contraction (-ffp-contract=off), only + - * / and comparisons, so the kernels (rp_accum.hip), the CPU loops
// behind rph_accum_frames and rph_accum_error (rp_host.cpp) and the numpy model of the tests (tests/accum_ref.py, written
// from the definition and not from this file) agree to the last bit.
#pragma once
#include <stdint.h>

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

}  // namespace rpa
