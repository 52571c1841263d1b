// rp_draw.h -- the arithmetic of the render kernel's keystream draws, for host and device.
//
// Every draw on a path is a run of Standard f64 values read from the lane's keystream ring at its stream position.
// The rejection samplers (randomness.rs:21-73) differ only in how many values one try takes and when it is accepted:
//   UnitSphere (Lambert), UnitDisk (camera)  2 values per try (4 stream words), accepted when x^2 + y^2 < 1
//   UnitBall (Metal)                         3 values per try (6 words),        accepted when (x^2 + y^2) + z^2 < 1
// A round evaluates TRIES tries, try j at stream word a + stride j; the first accepted try wins and the position moves
// to a + stride (j + 1) -- the words consumed are exactly the sequential loop's.  A try's values are consecutive in the
// stream, so a ring with a mirror tail (the ring of 8 blocks) reads them as ONE window from one address (a dwordx4,
// plus a dwordx2 for the third value): the tail lets a window that starts in the ring's last words read straight on.
// A ring without one (the q8 kernel's 4 blocks) reads each value with its own wrapped address.
// Bernoulli (Dielectric, randomness.rs:78-82) is one Standard f64, the u64 at ring word a % ring.
// The ring holds every u64 already decoded, as the double 2 r - 1 (value_store below): a try's values are loaded, not
// computed, and a draw that wants r takes unit_of of the loaded double.
//
// The kernel (rp_device.h scatter_eval, start_sample) and the host test hook (rp_host.h rph_draw_round) both use this
// header, so the addressing, the accept rules and the position update tested on the CPU are the kernel's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RPD_FN __host__ __device__ __forceinline__
#define RPD_UNROLL _Pragma("unroll")
#else
#define RPD_FN inline
#define RPD_UNROLL
#endif

namespace rpd {

static constexpr uint32_t TRIES = 2;  // tries per round (1 or 3 tries: +0.6 / +0.9 %; 3 or 4 for Metal alone: +0.6 / +1.3 %)

// Ring image of a lane: 16 * rn words (block b in slot b % rn, rn a power of two), then, for the ring of 8 blocks,
// the mirror tail: the first TAIL_WORDS words of slot 0 stored again behind the last slot.  A try's window (at most
// WINDOW_WORDS words from its first word, which is even) then reads straight on from any start in the ring: it ends
// at most at word 16 rn + 3.  The tail is 8 words, not 4, so that the lane's slab stays a whole number of 32-B
// sectors (rp_device.h RngT).  The ring of 4 blocks (the q8-node kernel, config C5) has no tail: measured with one,
// C5 lost 0.6 %, while the ring of 8 gains 1.1 % on C3 and C2.
static constexpr uint32_t WINDOW_WORDS = 6, TAIL_WORDS = 8;
static_assert(WINDOW_WORDS - 2 <= TAIL_WORDS, "a window starting at the ring's last u64 ends inside the tail");
RPD_FN constexpr uint32_t ring_tail_words(uint32_t rn) { return rn > 4u ? TAIL_WORDS : 0u; }
RPD_FN constexpr uint32_t ring_image_words(uint32_t rn) { return 16u * rn + ring_tail_words(rn); }
// ring word of stream word a while its block is held
RPD_FN uint32_t window_word(uint32_t a, uint32_t rn) { return a & (16u * rn - 1u); }
// word of the ring image holding value k (0, 1, 2) of the try at stream word a: k u64 on from the try's first word
// where the tail allows it, else wrapped by itself
RPD_FN uint32_t value_word(uint32_t a, uint32_t k, uint32_t rn) {
  return ring_tail_words(rn) ? window_word(a, rn) + 2u * k : window_word(a + 2u * k, rn);
}

// Draw kinds; 1-3 are the scatter kinds of the materials that draw (rp.h RP_SCATTER_*).
enum : uint32_t { DRAW_SPHERE = 1, DRAW_BALL = 2, DRAW_UNIFORM = 3, DRAW_DISK = 4 };
// stream words per try of a rejection sampler (UnitBall: 3 values; the others: 2)
RPD_FN constexpr uint32_t draw_stride(uint32_t kind) { return kind == DRAW_BALL ? 6u : 4u; }
// the last keystream block a round starting at word a can consume
RPD_FN uint32_t round_last_block(uint32_t a, uint32_t stride) { return (a + stride * TRIES - 1u) >> 4; }

// rand 0.8 Standard f64, (u64 >> 11) * 2^-53, from the u64's two keystream words as hi * 2^-32 + (lo >> 11) * 2^-53:
// both terms and the sum k * 2^-53 (k < 2^53) are exact, so the FMA returns the identical double.
RPD_FN double words_unit(uint32_t lo, uint32_t hi) {
  return __builtin_fma((double)hi, 0x1p-32, (double)(lo >> 11) * 0x1p-53);
}
// 2 * words_unit - 1 (the samplers' `2.0 * r - 1.0`): with k = u64 >> 11, 2 r = k * 2^-52 is exact and so is
// k * 2^-52 - 1 (a multiple of 2^-52 of magnitude <= 1), whatever the order -- two exact FMAs.
RPD_FN double words_sym(uint32_t lo, uint32_t hi) {
  return __builtin_fma((double)hi, 0x1p-31, __builtin_fma((double)(lo >> 11), 0x1p-52, -1.0));
}


// What the ring holds.  The ring, its mirror tail and the jitter blocks keep, for every keystream u64, not the raw
// words but the double the rejection samplers want, 2 r - 1: the decode (a shift, two conversions, two FMAs) depends on
// nothing but the u64, so it runs once where the block is made -- in the refill pass, at most of a wave's lanes, for
// values their lanes will consume -- and not at the draw sites, the kernel's emptiest code, where a wave pays it per
// round whether nine lanes need it or sixty-four.  The double takes the u64's 8 bytes at its address.
RPD_FN double value_store(uint32_t lo, uint32_t hi) { return words_sym(lo, hi); }
// The Standard f64 r from a stored value v, for the draws that want r itself (the jitter, Bernoulli).  Exact:
// v = k * 2^-52 - 1 with k < 2^53, so v + 1 = k * 2^-52 is representable (k fits the significand) and the sum returns
// it; halving moves the exponent only (k * 2^-53 is 0 or >= 2^-53, far from subnormal).  So
// unit_of(value_store(lo, hi)) has the bits of words_unit(lo, hi) (tests/test_draw_values.py).
RPD_FN double unit_of(double v) { return (v + 1.0) * 0.5; }

struct Try {
  double v[WINDOW_WORDS / 2];  // the window's stored values; v[2] is loaded only for stride 6, 0 otherwise
};
struct Draw {
  double x, y, z;  // the accepted try (z = 0 for stride 4)
  double s;        // its squared norm: x x + y y, or (x x + y y) + z z
};

// One round at stream word a over the loaded windows t[j] (try j = words a + stride j ...), stride 4 or 6.  Returns
// whether a try was accepted; then `out` is the first accepted try and `pos` the stream position after it.
RPD_FN bool draw_pick(uint32_t stride, uint32_t a, const Try t[TRIES], Draw& out, uint32_t& pos) {
  bool done = false;
  RPD_UNROLL
  for (int j = (int)TRIES - 1; j >= 0; j--) {  // descending: the first accepted try wins
    const double x = t[j].v[0], y = t[j].v[1];
    double z = 0.0, s = x * x + y * y;
    if (stride == 6u) {
      z = t[j].v[2];
      s = s + z * z;
    }
    if (s < 1.0) {
      out.x = x; out.y = y; out.z = z; out.s = s;
      pos = a + stride * (uint32_t)(j + 1);
      done = true;
    }
  }
  return done;
}

}  // namespace rpd
