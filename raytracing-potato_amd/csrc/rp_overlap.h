// rp_overlap.h -- the one overlap test of the passes' alias refusals, for both libraries: no HIP, no project header.
// The checks that use it (rp_accum.h, rp_denoise.h, rp_reproject.h) are compiled into librp.so and librp_host.so alike;
// rp_pass.h keeps the name rpp::overlaps for the device-only ones.
#pragma once
#include <stdint.h>

namespace rpo {

// Byte ranges [a, a + na) and [b, b + nb) share a byte (a NULL pointer is no range).
inline bool overlaps(const void* a, uint64_t na, const void* b, uint64_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace rpo
