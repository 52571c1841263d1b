// rp_host_rng.cpp -- librp_host.so (include/rp_host.h): the reference's StdRng keystream (ChaCha12) and the hooks on
// what the kernel's draw sites share with the host (rp_draw.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "rp_draw.h"
#include "rp_host_util.h"

using rph::fail;

namespace {
inline uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
// ChaCha12 block `ctr` of `key` (randomness.rs:5 StdRng = rand_chacha 0.3 ChaCha12Rng).
void chacha12_block(const uint32_t key[8], uint64_t ctr, uint32_t out[16]) {
  uint32_t x[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                    key[4],      key[5],      key[6],      key[7],      (uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
  uint32_t s[16];
  std::memcpy(s, x, sizeof s);
  auto qr = [&](int a, int b, int c, int d) {
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 16);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 12);
    x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl32(x[d], 8);
    x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl32(x[b], 7);
  };
  for (int r = 0; r < 6; r++) {
    qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
    qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
  }
  for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
}  // namespace

extern "C" {

int rph_stdrng_u64(const uint8_t seed[32], uint64_t first, uint64_t n, uint64_t* out) {
  if (!seed || (n && !out)) return fail("NULL argument");
  uint32_t key[8];
  for (int i = 0; i < 8; i++)
    key[i] = (uint32_t)seed[4 * i] | (uint32_t)seed[4 * i + 1] << 8 | (uint32_t)seed[4 * i + 2] << 16 |
             (uint32_t)seed[4 * i + 3] << 24;
  // draw k = words 2k, 2k+1 of the keystream = block k / 8, u64 k % 8 of it
  auto work = [&](uint64_t a, uint64_t b) {
    uint32_t w[16];
    uint64_t blk = ~0ull;
    for (uint64_t k = a; k < b; k++) {
      const uint64_t d = first + k;
      if (d / 8 != blk) {
        blk = d / 8;
        chacha12_block(key, blk, w);
      }
      const uint32_t q = (uint32_t)(d % 8);
      out[k] = (uint64_t)w[2 * q] | (uint64_t)w[2 * q + 1] << 32;
    }
  };
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const unsigned nt = n < (1u << 20) ? 1u : hw;
  std::vector<std::thread> th;
  const uint64_t per = (n + nt - 1) / nt;
  for (unsigned t = 1; t < nt; t++) {
    const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
    if (a < b) th.emplace_back(work, a, b);
  }
  work(0, std::min<uint64_t>(n, per));
  for (auto& t : th) t.join();
  return RP_OK;
}

int rph_draw_round(uint32_t kind, uint32_t ring_blocks, const uint32_t* ring_image, uint32_t pos, double out[3],
                   uint32_t* new_pos, uint32_t* accepted) {
  if (kind < rpd::DRAW_SPHERE || kind > rpd::DRAW_DISK || (ring_blocks != 4 && ring_blocks != 8) || (pos & 1u) ||
      !ring_image || !out || !new_pos || !accepted)
    return fail("rph_draw_round: kind 1-4, ring_blocks 4 or 8, even pos, non-NULL pointers");
  out[0] = out[1] = out[2] = 0.0;
  // the raw image as the kernel's slab holds it: every u64 decoded where its block is made (rp_device.h ring_values)
  double held[(16u * 8u + rpd::TAIL_WORDS) / 2u];
  for (uint32_t i = 0; i < rpd::ring_image_words(ring_blocks) / 2u; i++)
    held[i] = rpd::value_store(ring_image[2 * i], ring_image[2 * i + 1]);
  if (kind == rpd::DRAW_UNIFORM) {  // the kernel's gen_f64: from the stored value at the window address
    out[0] = rpd::unit_of(held[rpd::window_word(pos, ring_blocks) >> 1]);
    *new_pos = pos + 2u;
    *accepted = 1u;
    return RP_OK;
  }
  const uint32_t stride = rpd::draw_stride(kind);
  rpd::Try t[rpd::TRIES];
  for (uint32_t j = 0; j < rpd::TRIES; j++) {  // the kernel's ring_window
    for (uint32_t k = 0; k < rpd::WINDOW_WORDS / 2u; k++) t[j].v[k] = 0.0;
    for (uint32_t k = 0; k < stride / 2u; k++) t[j].v[k] = held[rpd::value_word(pos + stride * j, k, ring_blocks) >> 1];
  }
  rpd::Draw d{0.0, 0.0, 0.0, 0.0};
  uint32_t np = pos + stride * rpd::TRIES;
  *accepted = rpd::draw_pick(stride, pos, t, d, np) ? 1u : 0u;
  *new_pos = np;
  if (*accepted) {
    if (kind == rpd::DRAW_SPHERE) {  // the Lambert site's point (rp_device.h scatter_eval)
      const double f = 2.0 * std::sqrt(1.0 - d.s);
      out[0] = d.x * f; out[1] = d.y * f; out[2] = 1.0 - 2.0 * d.s;
    } else {
      out[0] = d.x; out[1] = d.y; out[2] = d.z;
    }
  }
  return RP_OK;
}

int rph_draw_values(const uint64_t* words, uint64_t n, double* stored, double* unit) {
  if (n && (!words || !stored || !unit)) return fail("rph_draw_values: non-NULL pointers");
  for (uint64_t i = 0; i < n; i++) {
    stored[i] = rpd::value_store((uint32_t)words[i], (uint32_t)(words[i] >> 32));
    unit[i] = rpd::unit_of(stored[i]);
  }
  return RP_OK;
}

}  // extern "C"
