// rp_variance.h -- the arithmetic of the per-pixel variance pass (include/rp.h rp_render_variance_device_ws, DESIGN.md
// 4.12), for host and device: the variance of a pixel's mean from the sample sums of its batches.
//
// Every value is IEEE binary64, every expression is written in the operation order include/rp.h gives and compiled
// without contraction (-ffp-contract=off), so the kernel (rp_variance.hip), the CPU loop behind rph_batch_variance
// (rp_host_passes.cpp) and the numpy model of the tests (tests/denoise_var_ref.py, written from the definition and not
// from this file) agree to the last bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RPV_FN __host__ __device__ __forceinline__
#else
#define RPV_FN inline
#endif

namespace rpv {

// B = ceil(spp / sps), the batches of a pixel (sps >= 1)
RPV_FN uint32_t batches(uint32_t spp, uint32_t sps) { return (uint32_t)(((uint64_t)spp + sps - 1) / sps); }

// One channel of one pixel: S[b * stride] is batch b's sample sum, b = 0 .. B - 1 with B = batches(spp, sps) >= 2.
//   x = (((0.0 + S_0) + S_1) + ...) / spp                the render's pixel, bit for bit
//   e_b = S_b / spp - x * (n_b / spp), n_b = min(sps, spp - b sps)
//   var = (sum of e_b e_b from 0.0 in b order) * (B / (B - 1))
RPV_FN double batch_variance(const double* S, uint32_t stride, uint32_t B, uint32_t spp, uint32_t sps) {
  const double n = (double)spp;
  double x = 0.0;
  for (uint32_t b = 0; b < B; b++) x = x + S[(uint64_t)b * stride];
  x = x / n;
  double acc = 0.0;
  for (uint32_t b = 0; b < B; b++) {
    const uint64_t left = (uint64_t)spp - (uint64_t)b * sps;
    const uint32_t nb = left < sps ? (uint32_t)left : sps;
    const double e = S[(uint64_t)b * stride] / n - x * ((double)nb / n);
    acc = acc + e * e;
  }
  return acc * ((double)B / (double)(B - 1u));
}

}  // namespace rpv
