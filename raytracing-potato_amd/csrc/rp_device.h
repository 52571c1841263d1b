// rp_device.h -- device code of the gfx950 kernels (rp_kernel.hip: the persistent megakernel and the closest-hit
// query kernel): the rand 0.8 StdRng keystream, f64 vector math, the
// conservative-f32 wide-BVH traversal with exact f64 primitive tests, and the materials/textures.
//
// Arithmetic is IEEE binary64 in the reference's exact operation order (no contraction: the kernels are
// compiled with -ffp-contract=off and the pragma below), so paths -- and the RNG draws they consume --
// are the reference's.  References: render.rs:32-146, bvh.rs:93-124, hittable.rs:39-108,
// material.rs:27-179, texture.rs:21-118, randomness.rs:9-110, utility.rs:67-154.
#pragma once
#include <hip/hip_runtime.h>

#include "rp_kernel.h"

#pragma clang fp contract(off)

#include "rp_draw.h"
#include "rp_ray.h"
#include "rp_isect.h"
#include "rp_units.h"

// Every compile-time knob below changes timing only.  Experiments that change results (timing ablations
// with wrong streams or colours) are not kept in this file, and a build asking for one is refused so a
// library that writes wrong frames can never be produced from it.
#if defined(RPK_ABLATE_RNG) || defined(RPK_ABLATE_UV) || defined(RPK_ABLATE_TEX) || defined(RPK_ABLATE_METAL) || \
    defined(RPK_BATCH_LEAF)
#error "result-changing experiment macros are not part of the product kernel"
#endif
// Timing experiments are not compile-time switches of the product sources either: the kernel below is the
// product path only (plus the RPK_DIAG instrumentation).  tools/build_variant.sh builds an experiment from a
// patched copy of these sources; the switches of earlier rounds are refused so a stale command line cannot
// silently build something else.
#if defined(RPK_NT_STORE) || defined(RPK_NT_ALL) || defined(RPK_NT_TEX) || defined(RPK_NT_OUT) ||           \
    defined(RPK_SLAB_ALIGN) || defined(RPK_SLAB_PAD) || defined(RPK_COLD_SLAB) || defined(RPK_COLD_IN_SLAB) || \
    defined(RPK_W3) || defined(RPK_W4) || defined(RPK_WAVES) || defined(RPK_TRIES_BALL) ||             \
    defined(RPK_NO_SPECULATIVE) || defined(RPK_NODE_BREAK) || defined(RPK_TRIES) || defined(RPK_RING) ||       \
    defined(RPK_RNG_BATCH) || defined(RPK_RNG_CRIT) || defined(RPK_PRIM_BREAK) || defined(RPK_PRIO_TRAV) ||    \
    defined(RPK_PRIO_SHADE) || defined(RPK_PRIO_REFILL) || defined(RPK_SORT_Q) || defined(RPK_WF_REFILL)
#error "experiment macros are not part of the product kernel (tools/build_variant.sh patches a copy instead)"
#endif

namespace rpk {

#define RPK_INLINE __device__ __forceinline__

// Diagnostic build (-DRPK_DIAG, lib/librp_diag.so only): per-wave s_memtime phase stamps and lane
// utilisation counters into KArgs::diag.  The product build compiles none of it.
#ifdef RPK_DIAG
#define DIAG(...) __VA_ARGS__
RPK_INLINE uint64_t stamp() {
#ifdef RPK_DIAG_NOSTAMP
  return 0;
#endif
  const uint64_t t = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): s_memtime returns through the LGKM counter
  return t;
}
__shared__ unsigned long long g_dreg[2 * DREG_N];
// count one execution of region r by this wave and its active lanes (leader lane only; EXEC is read
// directly, no ballot)
#define DREG(r)                                                                        \
  {                                                                                    \
    const uint64_t ex_ = __builtin_amdgcn_read_exec();                                 \
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(ex_)) {                       \
      atomicAdd(&g_dreg[2 * (r)], 1ull);                                               \
      atomicAdd(&g_dreg[2 * (r) + 1], (unsigned long long)__popcll(ex_));             \
    }                                                                                  \
  }
// wave-cycles spent executing a code region (its lanes active, the others masked): s_memtime around it, added by
// the wave's first active lane into g_dcyc[r] (flushed to diag[DIAG_CYC + r] at the kernel's end)
__shared__ unsigned long long g_dcyc[DCYC_N];
#define DCYC_BEGIN(v) const uint64_t v = stamp();
#define DCYC_END(r, v)                                                                 \
  {                                                                                    \
    const uint64_t ex_ = __builtin_amdgcn_read_exec();                                 \
    const uint64_t d_ = stamp() - (v);                                                 \
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(ex_)) atomicAdd(&g_dcyc[r], (unsigned long long)d_); \
  }
#else
#define DIAG(...)
#define DREG(r)
#define DCYC_BEGIN(v)
#define DCYC_END(r, v)
#endif

static constexpr int BLOCK = RENDER_BLOCK;
typedef float f2 __attribute__((ext_vector_type(2)));
RPK_INLINE f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// The slab test's packed evaluation, two children at a time (v_pk_fma_f32: two fused FMAs with the same per-element
// rounding as rp_isect.h's plane_t and slab_pass).  q2: code bytes 2h and 2h + 1 of a word (v_cvt_f32_ubyte<b>);
// pk_pass_lhs: the pass test's left side.
RPK_INLINE f2 q2(uint32_t w, int h) {
  return f2{(float)((w >> (16 * h)) & 0xffu), (float)((w >> (16 * h + 8)) & 0xffu)};
}
RPK_INLINE f2 pk_pass_lhs(f2 tn) {
  return pk_fma(tn, f2{rpi::PASS_SCALE, rpi::PASS_SCALE}, f2{rpi::PASS_BIAS, rpi::PASS_BIAS});
}
// min(t, best32) for a t that is not NaN (a slab t^: finite, rp_isect.h "conservative f32 box test") and
// best32 = rpr::best_above(..), whose sign bit is clear: the signed-integer order of the bit patterns is then the
// floats' order (a negative t is a negative integer, below every best32; two non-negative floats order as their
// patterns), so v_min_i32 returns the same float as v_min_f32 -- without the v_max_f32 x, x the compiler puts in
// front of a float min to quiet a value it cannot prove canonical (best32 comes from integer arithmetic, once per
// step, and the quieting was redone at every node visit).
RPK_INLINE float min_best(float t, float best32) {
  return __int_as_float(min(__float_as_int(t), __float_as_int(best32)));
}
static constexpr uint32_t STACK_SLACK = 3;  // spare LDS stack entries for the branchless push (writes reach sp+2 <= cap+2)
static constexpr double RAY_EPSILON = 1e-3;  // utility.rs:30
static constexpr double PI_ = 3.14159265358979323846;
static constexpr double TAU_ = 6.28318530717958647692;
static constexpr double INF = __builtin_huge_val();

// ------------------------------------------------------------------ RNG (rand 0.8 StdRng) -------

RPK_INLINE uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define RPK_QR(a, b, c, d)              \
  a += b; d ^= a; d = rotl(d, 16);      \
  c += d; b ^= c; b = rotl(b, 12);      \
  a += b; d ^= a; d = rotl(d, 8);       \
  c += d; b ^= c; b = rotl(b, 7);

// ChaCha12 block (rand_chacha 0.3: 64-bit block counter in words 12-13, zero nonce).
RPK_INLINE void chacha12(const uint32_t k[8], uint32_t ctr, uint32_t o[16]) {
  uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
  uint32_t x4 = k[0], x5 = k[1], x6 = k[2], x7 = k[3], x8 = k[4], x9 = k[5], x10 = k[6], x11 = k[7];
  uint32_t x12 = ctr, x13 = 0, x14 = 0, x15 = 0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    RPK_QR(x0, x4, x8, x12);
    RPK_QR(x1, x5, x9, x13);
    RPK_QR(x2, x6, x10, x14);
    RPK_QR(x3, x7, x11, x15);
    RPK_QR(x0, x5, x10, x15);
    RPK_QR(x1, x6, x11, x12);
    RPK_QR(x2, x7, x8, x13);
    RPK_QR(x3, x4, x9, x14);
  }
  o[0] = x0 + 0x61707865u; o[1] = x1 + 0x3320646eu; o[2] = x2 + 0x79622d32u; o[3] = x3 + 0x6b206574u;
  o[4] = x4 + k[0]; o[5] = x5 + k[1]; o[6] = x6 + k[2]; o[7] = x7 + k[3];
  o[8] = x8 + k[4]; o[9] = x9 + k[5]; o[10] = x10 + k[6]; o[11] = x11 + k[7];
  o[12] = x12 + ctr; o[13] = x13; o[14] = x14; o[15] = x15;
}

// The same block computed by the four lanes of a DPP quad together (the coherent primary pass: four neighbouring
// samples of a pixel share a jitter block).  Lane c of the quad holds column c of the state -- words c, 4 + c, 8 + c,
// 12 + c -- so a column round is one quarter round per lane, and a diagonal round is one quarter round per lane after
// rotating rows 1, 2, 3 of the state by 1, 2, 3 lanes (quad_perm DPP moves), rotated back after it.  A quarter of a
// block's VALU per lane.  Every lane of the quad must be active and pass the same key and counter; returns the
// lane's column of the output block (words c, 4 + c, 8 + c, 12 + c).
RPK_INLINE uint32_t quad_rot(uint32_t v, int by) {  // lane c of a quad reads lane (c + by) & 3
  return by == 1 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x39, 0xF, 0xF, false)
       : by == 2 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false)
                 : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x93, 0xF, 0xF, false);
}
RPK_INLINE uint4 chacha12_quad(const uint32_t k[8], uint32_t ctr) {
  const uint32_t c = __lane_id() & 3u;
  const uint32_t a0 = c == 0 ? 0x61707865u : c == 1 ? 0x3320646eu : c == 2 ? 0x79622d32u : 0x6b206574u;
  const uint32_t b0 = c == 0 ? k[0] : c == 1 ? k[1] : c == 2 ? k[2] : k[3];
  const uint32_t c0 = c == 0 ? k[4] : c == 1 ? k[5] : c == 2 ? k[6] : k[7];
  const uint32_t d0 = c == 0 ? ctr : 0u;
  uint32_t a = a0, b = b0, x = c0, d = d0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    RPK_QR(a, b, x, d);  // column c
    b = quad_rot(b, 1);
    x = quad_rot(x, 2);
    d = quad_rot(d, 3);
    RPK_QR(a, b, x, d);  // diagonal starting at word c
    b = quad_rot(b, 3);
    x = quad_rot(x, 2);
    d = quad_rot(d, 1);
  }
  return make_uint4(a + a0, b + b0, x + c0, d + d0);
}
// Row `row` of a block held column-wise by a quad (chacha12_quad): words 4 row .. 4 row + 3.  Lane m of the quad holds
// word 4 row + m in component `row` of its column; each of the four components is read from every lane (DPP
// broadcasts within the quad) and the lane keeps its own row.
RPK_INLINE uint32_t quad_bcast(uint32_t v, int from) {  // every lane of a quad reads lane `from`
  return from == 0 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xF, 0xF, false)
       : from == 1 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xF, 0xF, false)
       : from == 2 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xF, 0xF, false)
                   : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xF, 0xF, false);
}
RPK_INLINE uint4 quad_row(uint4 col, uint32_t row) {
  uint32_t o[4];
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const uint32_t r0 = quad_bcast(col.x, m), r1 = quad_bcast(col.y, m), r2 = quad_bcast(col.z, m),
                   r3 = quad_bcast(col.w, m);
    o[m] = row == 0 ? r0 : row == 1 ? r1 : row == 2 ? r2 : r3;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// rand_core 0.6 seed_from_u64: PCG32 expansion of the u64 into the 8 key words.
RPK_INLINE void seed_key(uint64_t state, uint32_t key[8]) {
#pragma unroll
  for (int c = 0; c < 8; c++) {
    state = state * 6364136223846793005ull + 11634580027462260723ull;
    uint32_t xs = (uint32_t)(((state >> 18) ^ state) >> 27);
    uint32_t rot = (uint32_t)(state >> 59);
    key[c] = (xs >> rot) | (xs << ((32 - rot) & 31));
  }
}

// Main stream of one pixel.  Every draw on the path is a u64 (Standard f64), so the stream is the
// keystream read two words at a time from word `pos`: exactly rand_chacha's 4-block-buffered stream.
//
// Keystream blocks are produced ahead of use into a per-lane slab in global memory (L2/MALL resident,
// ~0.7 KB per lane): a ring of RING main-stream blocks and the two camera-jitter blocks the next
// samples need.  Production happens in ONE place per round of the render loop (rng_refill), for every
// lane that has room, so a ChaCha12 block (~600 VALU) runs with nearly all 64 lanes doing useful work;
// the draw sites only load 16-word blocks from the ring.  Generating at the draw sites instead made the
// wave pay a whole block whenever ANY lane crossed a block boundary (several per round at C3).  A draw
// that finds the ring empty still generates its block in place (rare: the refill pass keeps > RNG_CRIT
// blocks ahead of every lane).
//
// Slab layout per lane (uint4 units): [0,2) key words, [2, 2+4*RING) ring (block b in slot b % RING),
// [2+4*RING, +2) the ring's mirror tail (the first 8 words of slot 0 again, so a draw's window reads straight on past
// the ring's end: rp_draw.h; the ring of 8 blocks only), then 8 of jitter blocks (block b in slot b & 1).  A block is
// held decoded: each of its 8 u64 as the double 2 r - 1 in the same 8 bytes (ring_values below), in the ring, the tail
// and the jitter blocks alike.  Per-lane cursors (LDS): end = one
// past the newest ring block; jtag[2] = block held by each jitter slot.
static constexpr uint32_t RING = 8;  // slab ring capacity; a kernel keeps RngT::ring <= RING blocks ahead
static constexpr uint32_t SLAB_KEY = 0, SLAB_RING = 2;  // (the tail and the jitter blocks follow the ring: RngT)
// The pixel sum and path throughput (6 f64 per lane, read and written at every shade) live in LDS (in the
// slab: C3 +2.6 %, C5 +4.6 %); the host then keeps ~19 traversal-stack entries in LDS and spills deeper ones to
// the lane's global run (render_blocks_per_cu picks the split; bunny: 19 of 31, rarely reached).
// (v43-v47 kept the measured unit's start time in one more uint4 of the slab: 688 B per lane, and C3 wrote 70 GB per
// frame instead of 56 -- the stamp now lives in its own lane-indexed array, KScene::unit_t0)
// A refill pass runs when some lane is at or below RNG_CRIT blocks ahead, or RNG_BATCH lanes have room.
static constexpr uint32_t RNG_CRIT = 2, RNG_BATCH = 48;
// Traversal wave-level exits (trav_step): leave the inner-node loop once at most KScene::leaf_break lanes of
// the wave still look for a leaf (rp_scene_options.leaf_break; C3: 0 -> 3 was -2.7 % frame time, 8 is -0.8 %
// more; C5 wants 12-16), and the leaf loop once at most PRIM_BREAK lanes still test primitives (their
// remaining run is parked as a leaf entry; C3 0 -> 12: -3.7 %, C5 -0.8 %; 6-16 within 0.5 %).
static constexpr uint32_t PRIM_BREAK = 12;

// RN = ring blocks in use (a power of two <= RING): the render kernel of the quantized-node (large-scene)
// format keeps 4, the others 8 (rp_kernel.hip RingFor).
template <uint32_t RN>
struct RngT {
  static constexpr uint32_t ring = RN;
  // a lane's slab for this ring: key, RN ring blocks, the mirror tail, 2 jitter blocks (704 B; RN = 4: no tail, 416 B)
  static constexpr uint32_t tail_n = rpd::ring_tail_words(RN) / 4;  // uint4 units
  static constexpr uint32_t tail = SLAB_RING + 4 * RN, jit = tail + tail_n, lane_n = jit + 8;
  static_assert(RN > RNG_CRIT && RN <= RING && (RN & (RN - 1)) == 0,
                "ring: a power of two above the critical refill level (a full ring is never refilled), <= RING");
  // a lane stride of 16 B past a 32-B boundary (688 B, v43-v47) made every 64-B block dirty three 32-B sectors: +25 %
  // memory-side writes
  static_assert(lane_n % 2 == 0, "lane slab stride must be a multiple of 32 B (keystream blocks on whole sectors)");
  uint4* slab;     // global: this lane's slab
  uint32_t pos;    // next keystream word (even)
  uint32_t* end;   // LDS cursor: one past the newest ring block
  uint32_t* jtag;  // LDS cursors: jtag[0], jtag[BLOCK]
};
template <class Rng>
RPK_INLINE void store_key(Rng& r, const uint32_t k[8]) {
  r.slab[SLAB_KEY] = make_uint4(k[0], k[1], k[2], k[3]);
  r.slab[SLAB_KEY + 1] = make_uint4(k[4], k[5], k[6], k[7]);
}
// A stored block: the slab keeps every keystream u64 decoded (rp_draw.h value_store: the double 2 r - 1), in the u64's
// 8 bytes.  ring_values is the one place a ChaCha block becomes what the slab holds: every block store below takes its
// result (a lane's own block and an executor's in rng_refill, a fresh unit's second copy in jitter slot 0, gen_block),
// so the decode runs once per u64, where the block is made.  The slab stays an array of uint4: a double crosses as its
// two words (value_bits / bits_value: register names, no instruction).
RPK_INLINE void ring_values(const uint32_t w[16], double v[8]) {
#pragma unroll
  for (int q = 0; q < 8; q++) v[q] = rpd::value_store(w[2 * q], w[2 * q + 1]);
}
RPK_INLINE uint4 value_bits(double a, double b) {
  const uint64_t x = (uint64_t)__double_as_longlong(a), y = (uint64_t)__double_as_longlong(b);
  return make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
}
RPK_INLINE double bits_value(uint32_t lo, uint32_t hi) { return __longlong_as_double((long long)((uint64_t)hi << 32 | lo)); }
RPK_INLINE void store_block(uint4* dst, const double v[8]) {
#pragma unroll
  for (int q = 0; q < 4; q++) dst[q] = value_bits(v[2 * q], v[2 * q + 1]);
}
// Every store of a ring block goes through here (a lane's own block and an executor's in rng_refill, the in-place
// fallback gen_block): `tail` is the ring's mirror tail when the block's slot is 0 (ring_tail), else null -- the tail
// then stays the copy of slot 0's first values that the draw windows rely on.
RPK_INLINE void store_ring_block(uint4* dst, uint4* tail, const double v[8]) {
  store_block(dst, v);
  if (tail) {
#pragma unroll
    for (uint32_t q = 0; q < rpd::TAIL_WORDS / 4; q++) tail[q] = value_bits(v[2 * q], v[2 * q + 1]);
  }
}
template <uint32_t RN>
RPK_INLINE uint4* ring_slot(const RngT<RN>& r, uint32_t b) { return r.slab + SLAB_RING + 4 * (b & (RN - 1u)); }
// the mirror tail of the ring of the lane slab `slab` if it has one and block b lives in slot 0, else null
// (store_ring_block)
template <uint32_t RN>
RPK_INLINE uint4* ring_tail(uint4* slab, uint32_t b) {
  return RngT<RN>::tail_n != 0 && (b & (RN - 1u)) == 0u ? slab + RngT<RN>::tail : nullptr;
}
template <uint32_t RN>
RPK_INLINE uint4* jit_slot(const RngT<RN>& r, uint32_t b) { return r.slab + RngT<RN>::jit + 4 * (b & 1u); }

// The refill pass (wave-uniform call site).  `seed` is the lane's unit seed (the RNG contract's
// seed_from_u64 argument).  `s` is the lane's last sample whose jitter is consumed;
// samples s+1.. need jitter blocks (s+1)/4 and the one after.  A lane with a `fresh` unit (fetched last
// round, not started) gets its key from the unit's seed and keystream block 0 here, batched with the other
// lanes' ChaCha work -- at the fetch site the whole wave paid a ChaCha block for each fetching lane.
// Position of the n-th (0-based) set bit of m (n < popcount(m)).
RPK_INLINE uint32_t nth_set(uint64_t m, uint32_t n) {
  uint32_t pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const uint32_t c = (uint32_t)__popcll(m & ((1ull << w) - 1ull));
    if (n >= c) { n -= c; m >>= w; pos += (uint32_t)w; }
  }
  return pos;
}
static_assert(BLOCK == 64, "rng_refill: a block is one wave, so a lane's slab is the wave's lane index past the first");
template <uint32_t RN>
RPK_INLINE void rng_refill(RngT<RN>& r, bool alive, bool fresh, uint64_t seed, uint32_t s, uint32_t spp) {
  const uint32_t cur = r.pos >> 4, end = *r.end, have = end - cur;
  const uint32_t b1 = (s + 1) >> 2, b2 = b1 + 1;
  const bool j1 = alive && !fresh && 4 * b1 < spp && r.jtag[(b1 & 1u) * BLOCK] != b1;
  const bool j2 = alive && !fresh && 4 * b2 < spp && r.jtag[(b2 & 1u) * BLOCK] != b2;
  const bool crit = alive && (fresh || have <= RNG_CRIT);
  const bool room = alive && (fresh || have < RN || j1 || j2);
  if (__ballot(crit) == 0 && (uint32_t)__popcll(__ballot(room)) < RNG_BATCH) return;
  // This lane's own block (room): a fresh unit's block 0, else the next ring block or a missing jitter block.
  const bool main = fresh || crit || !(j1 || j2);  // crit: have <= RNG_CRIT < RN, so the ring has room
  const uint32_t b = fresh ? 0u : (main ? end : (j1 ? b1 : b2));
  const uint32_t end1 = !room ? end : (fresh ? 1u : (main ? end + 1u : end));  // ring end after it
  const uint32_t have1 = end1 - (fresh ? 0u : cur);
  // The lanes without a block of their own this pass (full rings, retired lanes) make ring blocks for the lanes still
  // at or below the critical level after it -- up to two each, the next blocks of their streams -- in the same ChaCha
  // pass: a fresh unit leaves the pass 3 blocks ahead instead of 1, so it does not force the next two passes, and the
  // in-place fallback (gen_block: one lane, a whole wave's ChaCha time) is rarer.  Requests are numbered lane by lane,
  // first blocks before second ones; executor x (the x-th lane without a block) takes request x.
  // (Topping up every other ring with room as well cost C3 +1.0 %, C5 +2.6 %: profiles/r4/c3_c5_refill_variants_ab.json.)
  const uint32_t want = alive && have1 <= RNG_CRIT ? min(RNG_CRIT + 1u - have1, RN - have1) : 0u;
  const uint64_t m1 = __ballot(want >= 1u), m2 = __ballot(want >= 2u), ex = __ballot(!room);
  const uint32_t lane = __lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t n1 = (uint32_t)__popcll(m1), nreq = n1 + (uint32_t)__popcll(m2), nex = (uint32_t)__popcll(ex);
  const uint32_t xr = (uint32_t)__popcll(ex & below);
  const bool sec = !room && xr < nreq;
  uint32_t owner = lane, j = 0u;
  if (sec) {
    if (xr < n1) owner = nth_set(m1, xr);
    else { owner = nth_set(m2, xr - n1); j = 1u; }
  }
  const uint32_t slo = __shfl((uint32_t)seed, (int)owner), shi = __shfl((uint32_t)(seed >> 32), (int)owner);
  const uint32_t oend = __shfl(end1, (int)owner);
  // this lane's requests that an executor took
  const uint32_t served = (uint32_t)(want >= 1u && (uint32_t)__popcll(m1 & below) < nex) +
                          (uint32_t)(want >= 2u && n1 + (uint32_t)__popcll(m2 & below) < nex);
  if (room || sec) {
    DREG(DREG_REFILL)
    uint32_t k[8], w[16];
    // The key is recomputed from the unit's seed (PCG32 seed_from_u64, ~100 VALU) rather than loaded from the
    // slab: a slab load that misses L2 stalls the whole pass before its ChaCha work (C3 -0.7 %, C5 -0.1 %,
    // ab48).  A fresh unit still stores it for the in-place fallback (gen_block).
    seed_key(room ? seed : ((uint64_t)shi << 32 | slo), k);
    if (fresh) {
      DREG(DREG_BEGIN_PIXEL)
      store_key(r, k);
    }
    const uint32_t bb = room ? b : oend + j;
    chacha12(k, bb, w);
    double v[8];
    ring_values(w, v);  // decoded here, once, for every site that draws from the block (rp_draw.h value_store)
    // an executor's block goes into its owner's ring (lane slabs are consecutive within the block)
    uint4* oslab = r.slab + ((int)owner - (int)lane) * (int)RngT<RN>::lane_n;  // room: owner == lane
    uint4* dst = room && !main ? jit_slot(r, b) : oslab + SLAB_RING + 4u * (bb & (RN - 1u));
    store_ring_block(dst, room && !main ? nullptr : ring_tail<RN>(oslab, bb), v);
    if (fresh) store_block(jit_slot(r, 0), v);  // block 0 is also the jitter block of samples 0-3 (render.rs:74-82)
  }
  if (room) {
    if (fresh) {
      r.pos = 0;
      r.jtag[0] = 0;
      r.jtag[BLOCK] = 0xFFFFFFFFu;
    } else if (!main) {
      r.jtag[(b & 1u) * BLOCK] = b;
    }
  }
  if (room || served) *r.end = end1 + served;
  // An executor lane stored blocks into its owner lane's slab above, and the owner reads them through ring_window later:
  // a cross-lane hand-off inside one wave.  One wave's memory operations stay in order, and this wavefront-scope fence
  // states the ordering for the memory model; it compiles to no instruction (the kernel's ISA is unchanged).
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Jitter words 4s..4s+3 of the pixel-start stream (block s/4).
// Keystream block b of the lane's key into dst, for the rare draw that finds its block not made yet.  Out
// of line: the kernel is ~50 KB of code against a 64 KB instruction cache shared by two CUs, and each
// inlined ChaCha12 is ~2.5 KB that only the fallback paths execute.
// `tail`: ring_tail of a ring block, null for a jitter block.
static __device__ __attribute__((noinline, unused)) void gen_block(const uint4* slab, uint32_t b, uint4* dst, uint4* tail) {
  const uint4 a = slab[SLAB_KEY], c = slab[SLAB_KEY + 1];
  const uint32_t k[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
  uint32_t w[16];
  chacha12(k, b, w);
  double v[8];
  ring_values(w, v);
  store_ring_block(dst, tail, v);
}

// The two stored values of sample s's jitter (2 r - 1 each; start_sample takes rpd::unit_of of them) in jv[0], jv[1].
template <uint32_t RN>
RPK_INLINE void rng_jitter(RngT<RN>& r, uint32_t s, double jv[2]) {
  const uint32_t b = s >> 2;
  if (r.jtag[(b & 1u) * BLOCK] != b) {
    DREG(DREG_JIT_FALLBACK)
    gen_block(r.slab, b, jit_slot(r, b), nullptr);
    r.jtag[(b & 1u) * BLOCK] = b;
  }
  const uint4 w = jit_slot(r, b)[s & 3u];
  jv[0] = bits_value(w.x, w.y);
  jv[1] = bits_value(w.z, w.w);
}

// Every draw reads the ring directly: the RN blocks of a lane are one circular run of 16 RN words in its slab
// (L2-resident), so stream word a sits at ring word a % (16 RN) while its block is held (blocks [end - RN, end)).
// A draw site makes sure every block it can consume this round is there (ring_ensure: generated in place when the
// refill pass has not made it yet, rare) and loads each try's window -- its 2 or 3 consecutive u64 -- with one
// dwordx4 (and one dwordx2 for a third value) from one address: the ring's mirror tail lets a window that starts in
// the ring's last words read straight on (rp_draw.h; one masked dwordx2 per value before: C3 and C2 +1.1 %; the ring
// of 4 blocks keeps those loads and has no tail: with one, C5 lost 0.6 %).  The rejection
// loops (UnitBall / UnitSphere / UnitDisk) load and evaluate TRIES tries at once and keep the first accepted one --
// the draws consumed, and so the stream, are exactly the sequential loop's (rpd::draw_pick).  A wave iterates until
// its slowest lane accepts: with acceptance p a lane needs a geometric number of tries, and the wave's maximum over its
// ~20 shading lanes is ~5 single tries for the ball (p = pi/6); each round pays one ring-load latency.
using rpd::TRIES;
static_assert((RING & (RING - 1)) == 0, "the ring is indexed as 16 * ring words (a power of two)");
typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));  // a window starts on an even word
template <uint32_t STRIDE, uint32_t RN>
RPK_INLINE void ring_window(const RngT<RN>& r, uint32_t a, rpd::Try& t) {  // stream words a .. a + STRIDE - 1
  t.v[2] = 0.0;
  if constexpr (RngT<RN>::tail_n != 0) {
    const char* p = reinterpret_cast<const char*>(r.slab + SLAB_RING) + 4u * rpd::value_word(a, 0, RN);
    const u32x4_a8 v = *reinterpret_cast<const u32x4_a8*>(p);
    t.v[0] = bits_value(v.x, v.y); t.v[1] = bits_value(v.z, v.w);
    if (STRIDE == 6u) {
      const uint2 z = *reinterpret_cast<const uint2*>(p + 16);
      t.v[2] = bits_value(z.x, z.y);
    }
  } else {  // no tail: one wrapped dwordx2 per value
    const uint2* ring = reinterpret_cast<const uint2*>(r.slab + SLAB_RING);
#pragma unroll
    for (uint32_t k = 0; k < STRIDE / 2u; k++) {
      const uint2 v = ring[rpd::value_word(a, k, RN) >> 1];
      t.v[k] = bits_value(v.x, v.y);
    }
  }
}
template <uint32_t RN>
RPK_INLINE void ring_ensure(RngT<RN>& r, uint32_t last_blk) {
  while (last_blk >= *r.end) {
    DREG(DREG_RNG_FALLBACK)
    const uint32_t b = *r.end;
    gen_block(r.slab, b, ring_slot(r, b), ring_tail<RN>(r.slab, b));
    *r.end = b + 1;
  }
}
// One round of a rejection sampler at stream word a: its blocks made sure of, the tries' windows loaded (try j at
// a + STRIDE j) and evaluated.  True when a try was accepted: q is it, and r.pos the position after it.
template <uint32_t STRIDE, uint32_t RN>
RPK_INLINE bool ring_round(RngT<RN>& r, uint32_t a, rpd::Draw& q) {
  ring_ensure(r, rpd::round_last_block(a, STRIDE));
  rpd::Try t[TRIES];
#pragma unroll
  for (uint32_t j = 0; j < TRIES; j++) ring_window<STRIDE>(r, a + STRIDE * j, t[j]);
  return rpd::draw_pick(STRIDE, a, t, q, r.pos);
}
// One Standard f64 draw (rand 0.8 gen::<f64>): from the stored value at the window address of r.pos
template <uint32_t RN>
RPK_INLINE double gen_f64(RngT<RN>& r) {
  ring_ensure(r, r.pos >> 4);
  const uint2 v = reinterpret_cast<const uint2*>(r.slab + SLAB_RING)[rpd::window_word(r.pos, RN) >> 1];
  r.pos += 2;
  return rpd::unit_of(bits_value(v.x, v.y));
}

// ------------------------------------------------------------------ math -------------------------

typedef rpi::V3 V3;
RPK_INLINE V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
RPK_INLINE V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RPK_INLINE V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RPK_INLINE V3 mulc(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
RPK_INLINE V3 smul(double s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
RPK_INLINE double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }    // nalgebra dot
RPK_INLINE double norm2(V3 a) { return (a.x * a.x + a.y * a.y) + a.z * a.z; }         // norm_squared
RPK_INLINE V3 normalize(V3 a) { double n = sqrt(norm2(a)); return v3(a.x / n, a.y / n, a.z / n); }
RPK_INLINE V3 reflect(V3 i, V3 n) { return sub(i, smul(2.0 * dot(i, n), n)); }         // utility.rs:106

// Rust `as` casts saturate, NaN -> 0
RPK_INLINE uint32_t sat_u32(double x) {
  if (!(x > 0.0)) return 0u;
  if (x >= 4294967295.0) return 4294967295u;
  return (uint32_t)x;
}
RPK_INLINE int64_t sat_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775807.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

// randomness.rs:91-105 (wrapping isize, arithmetic >> 13)
RPK_INLINE int64_t noise_integer(int64_t x, int64_t y, int64_t z, int64_t seed) {
  uint64_t h = 0x369E6D3B899E43CFull * (uint64_t)x + 0x53F89E7FFDA3B07Dull * (uint64_t)y +
               0x3B13C1CA4937E629ull * (uint64_t)z + 0x577C2C6E4019D645ull * (uint64_t)seed;
  h = (uint64_t)((int64_t)h >> 13) ^ h;
  h = h * (h * h * 60493ull + 19990303ull) + 1376312589ull;
  return (int64_t)h;
}
RPK_INLINE double noise_real(int64_t x, int64_t y, int64_t z, int64_t seed) {
  return (double)noise_integer(x, y, z, seed) / 9223372036854775807.0;
}

// ------------------------------------------------------------------ traversal --------------------

// The closest hit's primitive kind and material travel with it from the accepting test (bit 31 = triangle,
// bits 0-30 = material; scene_create caps materials below 2^31 - 1): the shading of a triangle hit then
// starts at the material and vertex loads instead of re-reading the primitive record first (one dependent
// L2 round trip less).  KM_UNKNOWN: read them from the record (the q8-node kernel, whose traversal would pay the register).
constexpr uint32_t KM_TRIANGLE = 0x80000000u, KM_UNKNOWN = 0xFFFFFFFFu;
struct HitRec {
  double t, u, v;  // u, v: barycentrics of hittable.rs:89-95 (triangles)
  int32_t prim;    // -1 = miss
  uint32_t km = KM_UNKNOWN;
};

struct TravDiag {
  uint32_t visits = 0, tests = 0, trips = 0;
};

// ---- conservative f32 box test: the test and the argument that it never culls a reachable box are rp_isect.h's
// ("conservative f32 box test"); rp_ray.h makes the ray's side of it.
struct Ray32 {
  float ix, iy, iz;     // rcp(fl(d))
  float nbx, nby, nbz;  // near-plane addends <= -oinv - D per axis (rp_ray.h)
  float fbx, fby, fbz;  // far-plane addends >= -oinv + D per axis
  float tmin;           // <= t_min
  uint32_t sx, sy, sz;  // per axis, by the sign of the slope: Node4 = byte offset of the near plane row
                        // (lo_* or hi_*; the far row is the other); Node4Q/Node8Q = v_perm_b32 selector picking
                        // the near plane codes out of the {hi, lo} word pair (the far codes out of {lo, hi})
  uint32_t oct;         // Node8Q: dir_octant(d), the children's rank order slot ^ oct
};

// A node frame's terms for the ray (frame origin c0.xyz, steps c0.w, sy, sz), each in both halves of a pair for the
// packed plane evaluation.  All A before the B: the instruction order of the node visit is part of its timing.
struct PkFrame {
  f2 ax, ay, az, bnx, bny, bnz, bfx, bfy, bfz;
};
RPK_INLINE PkFrame pk_frame(float4 c0, float sy, float sz, const Ray32& r) {
  const float Ax = rpi::frame_a(c0.w, r.ix), Ay = rpi::frame_a(sy, r.iy), Az = rpi::frame_a(sz, r.iz);
  const float Bnx = rpi::frame_b(c0.x, r.ix, r.nbx), Bny = rpi::frame_b(c0.y, r.iy, r.nby),
              Bnz = rpi::frame_b(c0.z, r.iz, r.nbz);
  const float Bfx = rpi::frame_b(c0.x, r.ix, r.fbx), Bfy = rpi::frame_b(c0.y, r.iy, r.fby),
              Bfz = rpi::frame_b(c0.z, r.iz, r.fbz);
  return {{Ax, Ax}, {Ay, Ay}, {Az, Az}, {Bnx, Bnx}, {Bny, Bny}, {Bnz, Bnz}, {Bfx, Bfx}, {Bfy, Bfy}, {Bfz, Bfz}};
}

// Octant of a direction: bit a set when d_a has its sign bit set (the sign of rcp(fl(d_a)) below).  Node8Q
// visits a node's children in rank order slot ^ octant (rp_layout.h); only the order depends on it.
RPK_INLINE uint32_t dir_octant(V3 d) {
  return (uint32_t)(__double_as_longlong(d.x) < 0) | (uint32_t)(__double_as_longlong(d.y) < 0) << 1 |
         (uint32_t)(__double_as_longlong(d.z) < 0) << 2;
}

// The per-axis slopes and addends, tmin32 and best32 are rp_ray.h's (shared with the host: the inequalities they keep
// and the argument are written there).
template <uint32_t NF>
RPK_INLINE void setup_ray32(V3 o, V3 d, double tmin, double qbound, Ray32& r) {
  constexpr bool FRAME = NF != rpl::NODES_F32;
  const rpr::Axis ax = rpr::axis_setup<FRAME>(o.x, d.x, qbound), ay = rpr::axis_setup<FRAME>(o.y, d.y, qbound),
                  az = rpr::axis_setup<FRAME>(o.z, d.z, qbound);
  r.ix = ax.inv; r.iy = ay.inv; r.iz = az.inv;
  r.nbx = ax.nb; r.nby = ay.nb; r.nbz = az.nb;
  r.fbx = ax.fb; r.fby = ay.fb; r.fbz = az.fb;
  r.tmin = rpr::f32_below(tmin);
  r.oct = dir_octant(d);
  if (NF != rpl::NODES_F32) {
    r.sx = r.ix < 0.0f ? 0x07060504u : 0x03020100u;
    r.sy = r.iy < 0.0f ? 0x07060504u : 0x03020100u;
    r.sz = r.iz < 0.0f ? 0x07060504u : 0x03020100u;
  } else {
    // Node4: lo_x at 0, hi_x at 16, lo_y at 32, hi_y at 48, lo_z at 64, hi_z at 80
    r.sx = r.ix < 0.0f ? 16u : 0u;
    r.sy = r.iy < 0.0f ? 48u : 32u;
    r.sz = r.iz < 0.0f ? 80u : 64u;
  }
}

// Closest hit over the 4-wide BVH (the reference's Hittable::Bvh::hit, bvh.rs:121-124 / hit_node
// bvh.rs:93-119: any tree shape and visit order returns the same closest hit up to exact-t ties,
// SURVEY.md 8a A9).  Primitive tests are the reference's exact f64 ones; t_max shrinks to the closest
// hit so far and acceptance is `t <= t_max`, so an equal-t primitive tested later wins
// (hittable.rs:52,99).  Structure: "while-while" -- descend inner nodes (near child first, the others
// pushed far-to-near on the LDS stack) until this lane holds a leaf, then test the leaf's primitives;
// the wave runs the expensive f64 leaf code once for every lane that reached a leaf.
//
// The traversal state is explicit (TravState) so a lane can stop between steps and resume later: the
// render kernel steps traversal until few lanes are still traversing, shades the finished ones and
// gives them new rays, then resumes (see render_kernel).
//
// Node8Q trees (trav_step_w8) keep groups instead of entries: cur/gy = a node group {W8_GROUP | family index,
// rank bits 0-7 | imask << 8} (the children still to visit, in rank order) or a primitive group {first primitive,
// primitive bits}; leaf/py = the parked primitive group (py = 0: none, and then leaf = 0).
struct TravState {
  double best, bu, bv;
  int32_t bestp;
  uint32_t bestm;  // the closest hit's kind and material (HitRec::km)
  uint32_t cur, sp;
  uint32_t leaf;  // parked leaf entry (speculative traversal), 0 = none (entry 0 is an inner node)
  uint32_t gy, py;  // Node8Q only (0 otherwise)
};
static constexpr uint32_t W8_GROUP = 0x80000000u;  // cur: a node group (prim groups: first primitive < 2^31)

RPK_INLINE bool trav_done(const TravState& t) { return t.cur == rpl::ENTRY_EMPTY && (t.leaf | t.py) == 0u; }

// A new ray from the root; `d` orders a Node8Q root's children.
template <uint32_t NF>
RPK_INLINE void trav_init(const KScene& S, double tmax, TravState& t, V3 d) {
  t.best = tmax;
  t.bu = 0.0;
  t.bv = 0.0;
  t.bestp = -1;
  t.bestm = KM_UNKNOWN;
  t.cur = S.root;
  t.sp = 0;
  t.leaf = 0;
  t.gy = 0;
  t.py = 0;
  if constexpr (NF == rpl::NODES_W8) {
    t.cur = W8_GROUP | S.root;              // the root as a group of one: slot 0, rank 0 ^ oct
    t.gy = (1u << dir_octant(d)) | 0x100u;  // imask = slot 0
  }
}

// One exact f64 primitive test (rp_isect.h: the reference's Hittable::hit for a leaf, hittable.rs:39-101): on
// acceptance `best` shrinks to t and the hit record is taken.  LEAF: a test of the leaf loop (trav_step, trav_step_w8),
// not of the always-tested site -- the diagnostic build counts the leaf loop's sphere branch (DREG_SPHERE_PATH: the
// iterations that run both kinds' paths); the product build compiles one text for both.
template <bool LEAF = true>
RPK_INLINE void prim_test(const KScene& S, uint32_t k, V3 o, V3 d, double tmin, double& best, TravState& ts) {
  // 32-bit byte offset from the wave-uniform base (scalar-base + vector-offset loads)
  const double2* q = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(S.prims) +
                                                      k * (uint32_t)sizeof(rpl::Prim));
  const double2 g01 = q[0], g23 = q[1], g45 = q[2], g67 = q[3];
  const double2 g8k = q[4];  // g[8], {kind, material}
  const uint64_t km = (uint64_t)__double_as_longlong(g8k.y);
  const uint32_t kind = (uint32_t)km, mat = (uint32_t)(km >> 32);
  const V3 g0 = v3(g01.x, g01.y, g23.x);  // the triangle's a, the sphere's centre
  if (kind == rpl::PRIM_TRIANGLE) {
    // One masked block takes the hit.  Early returns made five nested exec-mask regions, each copying the hit record
    // in and out, around skip branches a wave with a dozen lanes never takes; five selects instead of the block
    // measured 0.45 % slower on C3 (profiles/r9/c3_leaf_loop_ab.json).
    const V3 ba = v3(g23.y, g45.x, g45.y), ca = v3(g67.x, g67.y, g8k.x);
    rpi::tri_test(g0, ba, ca, o, d, tmin, best, [&](double t, double u, double v) {
      best = t; ts.bestp = (int32_t)k; ts.bu = u; ts.bv = v; ts.bestm = KM_TRIANGLE | mat;
    });
  } else {
    // (the words only the triangle reads count as read here too: all five loads of a test are then issued together in
    // front of the branch on the kind; with the triangle their only reader the compiler moves their loads into its
    // path, behind the wait for the kind, and a test waits for memory twice)
    asm volatile("" : : "v"(g45.x), "v"(g45.y), "v"(g67.x), "v"(g67.y), "v"(g8k.x));
    if constexpr (LEAF) {
      DREG(DREG_SPHERE_PATH)
    }
    rpi::sphere_test(g0, g23.y, o, d, tmin, best, [&](double t) {
      best = t; ts.bestp = (int32_t)k; ts.bestm = mat;
    });
  }
}

// A new ray: the always-tested primitives (KScene::n_always: boxes that dwarf the rest of the scene, kept
// out of the tree by the host builder) get their exact tests here, one wave-uniform loop over the same
// primitive for every starting lane, instead of a divergent leaf test deep in the prim loop; their hit
// also bounds the traversal from the root.  The closest hit is the tree's (any test order, up to exact-t
// ties).
//
// The list is the same for every lane and never written during a launch, so its records come through the constant
// address space: scalar loads into SGPRs, no per-lane copy of a record in VGPRs.  A sphere reads its centre, radius
// and {kind, material} (ten dwords); the next record's loads are issued in front of the current test, so the site
// waits for memory once, in front of its first test (waiting once per record instead measured the same on C3:
// profiles/r24/headline_ab.json).  The kind is a scalar and its branch wave-uniform: a sphere goes to
// rpi::sphere_test with its constants as scalar operands and the closest hit is taken in that test's one masked
// block, in place.  A record that is no sphere (a huge triangle the size rule listed) ends the sphere loop: it and the
// rest of the list, in list order, take prim_test as the leaf loop has it -- with that path inside the sphere loop the
// two paths' hit records meet behind every test, and the closest hit is copied in and out around each sphere's block.
typedef __attribute__((address_space(4))) const rpl::Prim cst_prim;
struct AlwaysRec {
  double cx, cy, cz, r;
  uint32_t kind, mat;
};
RPK_INLINE AlwaysRec always_load(const KScene& S, uint32_t k) {
  const cst_prim* p = (const cst_prim*)S.prims + k;
  return {p->g[0], p->g[1], p->g[2], p->g[3], p->kind, p->material};
}
RPK_INLINE void always_tests(const KScene& S, V3 o, V3 d, double tmin, double& best, TravState& ts) {
  if (S.n_always == 0) return;
  const uint32_t last = S.always_first + S.n_always - 1;
  uint32_t k = S.always_first;
  AlwaysRec nx = always_load(S, k);
  for (; k <= last; k++) {
    const AlwaysRec p = nx;
    if (p.kind != rpl::PRIM_SPHERE) break;
    nx = always_load(S, min(k + 1, last));
    DREG(DREG_ALWAYS)
    rpi::sphere_test(v3(p.cx, p.cy, p.cz), p.r, o, d, tmin, best, [&](double t) {
      best = t; ts.bestp = (int32_t)k; ts.bestm = p.mat;
    });
  }
  for (; k <= last; k++) {
    DREG(DREG_ALWAYS)
    prim_test<false>(S, k, o, d, tmin, best, ts);
  }
}

// SCALAR = false (the feature pass): the records through prim_test's per-lane loads.  That kernel keeps its KScene in
// SGPRs across its sample loop and spills them at the limit of 106; with the records in SGPRs as well its q8
// instantiation goes from 127 to 129 VGPRs and from 4 waves per SIMD to 3.
template <uint32_t NF, bool SCALAR = true>
RPK_INLINE void trav_begin(const KScene& S, V3 o, V3 d, double tmin, double tmax, TravState& t) {
  trav_init<NF>(S, tmax, t, d);
  double best = t.best;
  if constexpr (SCALAR) {
    always_tests(S, o, d, tmin, best, t);
  } else {
    for (uint32_t k = S.always_first; k < S.always_first + S.n_always; k++) {
      DREG(DREG_ALWAYS)
      prim_test<false>(S, k, o, d, tmin, best, t);
    }
  }
  t.best = best;
}

// Stack entry i of a lane: in its LDS column (entry i at stk[i * stride]) or, for SPILL kernels, entries
// >= S.lds_depth in the lane's global overflow run (S.spill[spl + i - lds_depth], L2-resident) -- a deep
// tree (config C5: 43 entries) then keeps the LDS of four blocks per CU.  The two parts are typed with
// their address spaces (LDS = 3, global = 1): with generic pointers the compiler merged the LDS and the
// spill store of a push into one FLAT store through a selected pointer (and the pops into FLAT loads),
// which waits on both memory counters at every node visit.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(1))) uint32_t glb_u32;
RPK_INLINE glb_u32* spill_ptr(const KScene& S) { return (glb_u32*)S.spill; }
template <bool SPILL>
RPK_INLINE void stk_put(const KScene& S, lds_u32* stk, uint32_t stride, uint32_t spl, uint32_t i, uint32_t v) {
  if (!SPILL || i < S.lds_depth) stk[i * stride] = v;
  else spill_ptr(S)[spl + i - S.lds_depth] = v;
}
template <bool SPILL>
RPK_INLINE uint32_t stk_get(const KScene& S, const lds_u32* stk, uint32_t stride, uint32_t spl, uint32_t i) {
  if (!SPILL || i < S.lds_depth) return stk[i * stride];
  return spill_ptr(S)[spl + i - S.lds_depth];
}

// One step: descend until a leaf is held, test the leaves.  Finished when t.cur == ENTRY_EMPTY and no leaf is
// parked (trav_done).  `spl`: the lane's first spill entry (SPILL kernels).  `work` (COUNT instantiations: the
// cost probe) accumulates the lane's traversal work in WORK_* units.
enum : uint32_t { WORK_VISIT = 2, WORK_TEST = 3, WORK_RAY = 16 };  // node visit : primitive test : shaded ray

// Node8Q step.  The lane descends while it holds a node group with children left: it takes the lowest rank
// (the nearest octant), pushes the rest of the group, and visits that child, whose hit inner children become
// the new node group and whose hit leaf children's primitives one primitive group -- parked if the lane has
// none parked (speculative traversal, as in the 4-wide step), else pushed.  Groups go on the stack as two
// words.  `w8_settle` pops until the lane holds a node group with work, a primitive group it cannot park yet
// (it waits for the leaf loop), or nothing.  The leaf loop tests one primitive per lane per iteration from the
// parked group (lowest bit first), then takes a waiting primitive group.  Same exits as trav_step.
template <bool SPILL>
RPK_INLINE void w8_settle(const KScene& S, lds_u32* stk, uint32_t stride, uint32_t spl, uint32_t& gx, uint32_t& gy,
                          uint32_t& px, uint32_t& py, uint32_t& sp) {
#pragma unroll
  for (int it = 0; it < 2; it++) {  // at most a primitive group and then anything: two pops
    if (gx & W8_GROUP) {
      if (gy & 0xFFu) return;
    } else {
      if (py) return;
      px = gx; py = gy;
    }
    if (sp == 0u) { gx = rpl::ENTRY_EMPTY; gy = 0u; return; }
    sp -= 2u;
    gx = stk_get<SPILL>(S, stk, stride, spl, sp);
    gy = stk_get<SPILL>(S, stk, stride, spl, sp + 1u);
  }
}

template <bool SPILL, bool COUNT>
RPK_INLINE void trav_step_w8(const KScene& S, lds_u32* stk, uint32_t stride, uint32_t spl, const Ray32& r, V3 o,
                             V3 d, double tmin, TravState& ts, bool& overflow, TravDiag* td, uint32_t* work) {
  uint32_t gx = ts.cur, gy = ts.gy, px = ts.leaf, py = ts.py, sp = ts.sp;
  double best = ts.best;
  const float best32 = rpr::best_above(best);
  const uint32_t cap = S.stack_depth - STACK_SLACK;  // words
  auto push = [&](uint32_t x, uint32_t y) {
    if (sp + 2u > cap) { overflow = true; return; }  // cannot happen for a stack sized from the tree depth
    stk_put<SPILL>(S, stk, stride, spl, sp, x);
    stk_put<SPILL>(S, stk, stride, spl, sp + 1u, y);
    sp += 2u;
  };
  w8_settle<SPILL>(S, stk, stride, spl, gx, gy, px, py, sp);
  // ---- inner nodes
  while ((gx & W8_GROUP) && (gy & 0xFFu) && (!COUNT || py == 0u)) {
    DIAG(if (td) td->visits++;)
    if constexpr (COUNT) *work += WORK_VISIT;
    DREG(DREG_NODE)
    const uint32_t slot = (uint32_t)__builtin_ctz(gy) ^ r.oct;
    gy &= gy - 1u;
    const uint32_t node = (gx & ~W8_GROUP) + (uint32_t)__builtin_popcount((gy >> 8) & ((1u << slot) - 1u));
    if (gy & 0xFFu) push(gx, gy);
    const char* nb = reinterpret_cast<const char*>(S.nodes);
    const uint32_t no = node << 7;
    const float4 c0 = *reinterpret_cast<const float4*>(nb + no);        // o.x o.y o.z s.x
    const uint4 c1 = *reinterpret_cast<const uint4*>(nb + (no + 16u));  // s.y s.z inner prim
    const uint4 cx = *reinterpret_cast<const uint4*>(nb + (no + 32u));  // lo_x[0-3] lo_x[4-7] hi_x[0-3] hi_x[4-7]
    const uint4 cy = *reinterpret_cast<const uint4*>(nb + (no + 48u));
    const uint4 cz = *reinterpret_cast<const uint4*>(nb + (no + 64u));
    const uint4 pa = *reinterpret_cast<const uint4*>(nb + (no + 80u));  // pmask[0-3]
    const uint4 pb = *reinterpret_cast<const uint4*>(nb + (no + 96u));  // pmask[4-7]
    const PkFrame f = pk_frame(c0, __uint_as_float(c1.x), __uint_as_float(c1.y), r);
    uint32_t hits = 0u, pm = 0u;
#pragma unroll
    for (int half = 0; half < 2; half++) {  // children 4 half .. 4 half + 3
      const uint32_t lx = half ? cx.y : cx.x, hx = half ? cx.w : cx.z;
      const uint32_t ly = half ? cy.y : cy.x, hy = half ? cy.w : cy.z;
      const uint32_t lz = half ? cz.y : cz.x, hz = half ? cz.w : cz.z;
      const uint32_t qnx = __builtin_amdgcn_perm(hx, lx, r.sx), qfx = __builtin_amdgcn_perm(lx, hx, r.sx);
      const uint32_t qny = __builtin_amdgcn_perm(hy, ly, r.sy), qfy = __builtin_amdgcn_perm(ly, hy, r.sy);
      const uint32_t qnz = __builtin_amdgcn_perm(hz, lz, r.sz), qfz = __builtin_amdgcn_perm(lz, hz, r.sz);
      const uint4 pq = half ? pb : pa;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const f2 NX = pk_fma(q2(qnx, q), f.ax, f.bnx), FX = pk_fma(q2(qfx, q), f.ax, f.bfx);
        const f2 NY = pk_fma(q2(qny, q), f.ay, f.bny), FY = pk_fma(q2(qfy, q), f.ay, f.bfy);
        const f2 NZ = pk_fma(q2(qnz, q), f.az, f.bnz), FZ = pk_fma(q2(qfz, q), f.az, f.bfz);
        f2 TN, TF;
#pragma unroll
        for (int e = 0; e < 2; e++) {
          TN[e] = fmaxf(fmaxf(NX[e], NY[e]), fmaxf(NZ[e], r.tmin));
          TF[e] = min_best(fminf(fminf(FX[e], FY[e]), FZ[e]), best32);
        }
        const f2 lhs = pk_pass_lhs(TN);
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const int c = 4 * half + 2 * q + e;
          const bool hit = lhs[e] <= TF[e];
          hits |= hit ? 1u << c : 0u;
          const uint32_t m = (2 * q + e) == 0 ? pq.x : (2 * q + e) == 1 ? pq.y : (2 * q + e) == 2 ? pq.z : pq.w;
          pm |= hit ? m : 0u;
        }
      }
    }
    // hit inner children in rank order: bit (slot ^ oct)
    const uint32_t imask = c1.z >> 24;
    uint32_t ih = hits & imask;
    if (r.oct & 1u) ih = ((ih & 0x55u) << 1) | ((ih >> 1) & 0x55u);
    if (r.oct & 2u) ih = ((ih & 0x33u) << 2) | ((ih >> 2) & 0x33u);
    if (r.oct & 4u) ih = ((ih & 0x0Fu) << 4) | ((ih >> 4) & 0x0Fu);
    if (pm) {
      if (py == 0u) { px = c1.w; py = pm; }
      else push(c1.w, pm);
    }
    gx = W8_GROUP | (c1.z & rpl::W8_INDEX);
    gy = ih | imask << 8;
    w8_settle<SPILL>(S, stk, stride, spl, gx, gy, px, py, sp);
    if (!COUNT && (uint32_t)__popcll(__ballot(py == 0u)) <= S.leaf_break) break;
  }
  // ---- leaves: one primitive per lane per iteration from the parked group, then a waiting one
  // (the loop runs on the wave's condition, a lane without a group skips the body: trav_step's leaf loop)
  uint32_t testing = (uint32_t)__popcll(__ballot(py != 0u));
  while (testing != 0u) {
    if (py != 0u) {
      DIAG(if (td) td->tests++;)
      if constexpr (COUNT) *work += WORK_TEST;
      DREG(DREG_PRIM)
      const uint32_t k = px + (uint32_t)__builtin_ctz(py);
      py &= py - 1u;
      prim_test(S, k, o, d, tmin, best, ts);
      if (py == 0u) {
        px = 0u;
        if (!(gx & W8_GROUP)) w8_settle<SPILL>(S, stk, stride, spl, gx, gy, px, py, sp);  // park the waiting group
      }
    }
    testing = (uint32_t)__popcll(__ballot(py != 0u));
    if (!COUNT && PRIM_BREAK > 0 && testing <= PRIM_BREAK) break;
  }
  ts.cur = gx;
  ts.gy = gy;
  ts.sp = sp;
  ts.best = best;
  ts.leaf = px;
  ts.py = py;
}

template <bool SPILL, uint32_t NF, bool COUNT = false>
RPK_INLINE void trav_step(const KScene& S, lds_u32* stk, uint32_t stride, uint32_t spl, const Ray32& r, V3 o, V3 d,
                          double tmin, TravState& ts, bool& overflow, TravDiag* td = nullptr,
                          uint32_t* work = nullptr) {
  if constexpr (NF == rpl::NODES_W8) {
    trav_step_w8<SPILL, COUNT>(S, stk, stride, spl, r, o, d, tmin, ts, overflow, td, work);
    return;
  }
  uint32_t cur = ts.cur, sp = ts.sp, leaf = ts.leaf;
  double best = ts.best;
  const float best32 = rpr::best_above(best);
  const uint32_t cap = S.stack_depth - STACK_SLACK;
  DCYC_BEGIN(cnode)
  // ---- inner nodes
  while (!(cur & rpl::ENTRY_LEAF)) {
    DIAG(if (td) td->visits++;)
    if constexpr (COUNT) *work += WORK_VISIT;
    DREG(DREG_NODE)
    // Near/far planes chosen per ray by the slope signs (octant), so each child costs one max3 + max for
    // t_near and one min3 + min for t_far: for a valid box the same pair of values the min/max slab form
    // picks (t^ is monotone in the plane coordinate).  Node4 picks the near/far rows by address; Node4Q
    // picks the four children's near (far) plane codes out of the {lo, hi} code words with one v_perm_b32
    // per axis and side.  32-bit byte offsets from the (wave-uniform) node base: scalar-base +
    // vector-offset addressing.
    const char* nb = reinterpret_cast<const char*>(S.nodes);
    f2 NX[2], FX[2], NY[2], FY[2], NZ[2], FZ[2];
    uint4 ch;
    if constexpr (NF == rpl::NODES_Q8) {
      const uint32_t no = cur << 6;
      const float4 c0 = *reinterpret_cast<const float4*>(nb + no);        // o.x o.y o.z s.x
      const uint4 c1 = *reinterpret_cast<const uint4*>(nb + (no + 16u));  // s.y s.z lo_x hi_x
      const uint4 c2 = *reinterpret_cast<const uint4*>(nb + (no + 32u));  // lo_y hi_y lo_z hi_z
      ch = *reinterpret_cast<const uint4*>(nb + (no + 48u));
      // per axis: A = s inv, B = fma(o, inv, nb | fb); plane t^ = fma(q, A, B)
      const PkFrame f = pk_frame(c0, __uint_as_float(c1.x), __uint_as_float(c1.y), r);
      const uint32_t qnx = __builtin_amdgcn_perm(c1.w, c1.z, r.sx), qfx = __builtin_amdgcn_perm(c1.z, c1.w, r.sx);
      const uint32_t qny = __builtin_amdgcn_perm(c2.y, c2.x, r.sy), qfy = __builtin_amdgcn_perm(c2.x, c2.y, r.sy);
      const uint32_t qnz = __builtin_amdgcn_perm(c2.w, c2.z, r.sz), qfz = __builtin_amdgcn_perm(c2.z, c2.w, r.sz);
#pragma unroll  // children (0,1) and (2,3) as packed pairs
      for (int q = 0; q < 2; q++) {
        NX[q] = pk_fma(q2(qnx, q), f.ax, f.bnx);
        FX[q] = pk_fma(q2(qfx, q), f.ax, f.bfx);
        NY[q] = pk_fma(q2(qny, q), f.ay, f.bny);
        FY[q] = pk_fma(q2(qfy, q), f.ay, f.bfy);
        NZ[q] = pk_fma(q2(qnz, q), f.az, f.bnz);
        FZ[q] = pk_fma(q2(qfz, q), f.az, f.bfz);
      }
    } else {
      const uint32_t no = cur << 7;
      const float4 nx = *reinterpret_cast<const float4*>(nb + (no + r.sx));
      const float4 fx = *reinterpret_cast<const float4*>(nb + (no + (r.sx ^ 16u)));
      const float4 ny = *reinterpret_cast<const float4*>(nb + (no + r.sy));
      const float4 fy = *reinterpret_cast<const float4*>(nb + (no + (r.sy ^ 16u)));
      const float4 nz = *reinterpret_cast<const float4*>(nb + (no + r.sz));
      const float4 fz = *reinterpret_cast<const float4*>(nb + (no + (r.sz ^ 16u)));
      ch = *reinterpret_cast<const uint4*>(nb + (no + 96u));
      const f2 ix = {r.ix, r.ix}, iy = {r.iy, r.iy}, iz = {r.iz, r.iz};
      const f2 nbx = {r.nbx, r.nbx}, nby = {r.nby, r.nby}, nbz = {r.nbz, r.nbz};
      const f2 fbx = {r.fbx, r.fbx}, fby = {r.fby, r.fby}, fbz = {r.fbz, r.fbz};
      NX[0] = pk_fma(f2{nx.x, nx.y}, ix, nbx); NX[1] = pk_fma(f2{nx.z, nx.w}, ix, nbx);
      FX[0] = pk_fma(f2{fx.x, fx.y}, ix, fbx); FX[1] = pk_fma(f2{fx.z, fx.w}, ix, fbx);
      NY[0] = pk_fma(f2{ny.x, ny.y}, iy, nby); NY[1] = pk_fma(f2{ny.z, ny.w}, iy, nby);
      FY[0] = pk_fma(f2{fy.x, fy.y}, iy, fby); FY[1] = pk_fma(f2{fy.z, fy.w}, iy, fby);
      NZ[0] = pk_fma(f2{nz.x, nz.y}, iz, nbz); NZ[1] = pk_fma(f2{nz.z, nz.w}, iz, nbz);
      FZ[0] = pk_fma(f2{fz.x, fz.y}, iz, fbz); FZ[1] = pk_fma(f2{fz.z, fz.w}, iz, fbz);
    }
    float tn[4];
    uint32_t n_hit = 0u;  // counted from the four test masks: off the sort's dependent chain
    uint32_t cc[4] = {ch.x, ch.y, ch.z, ch.w};
    f2 TN[2], TF[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
      for (int e = 0; e < 2; e++) {
        TN[q][e] = fmaxf(fmaxf(NX[q][e], NY[q][e]), fmaxf(NZ[q][e], r.tmin));
        TF[q][e] = min_best(fminf(fminf(FX[q][e], FY[q][e]), FZ[q][e]), best32);
      }
      // fma(tnear, 1 - 2^-19, -2^-100) <= tfar (section 4.2 of DESIGN.md): one packed FMA per pair
      const f2 lhs = pk_pass_lhs(TN[q]);
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int c = 2 * q + e;
        const bool hit = lhs[e] <= TF[q][e] && (NF != rpl::NODES_Q8 || cc[c] != rpl::ENTRY_EMPTY);
        tn[c] = hit ? TN[q][e] : __builtin_huge_valf();
        n_hit += hit ? 1u : 0u;
      }
    }
    // sort (tn, entry) ascending: misses (+inf) go last
#define RPK_CSWAP(a, b)                                   \
{                                                       \
  const bool sw = tn[b] < tn[a];                        \
  const float t_ = sw ? tn[b] : tn[a];                  \
  tn[b] = sw ? tn[a] : tn[b];                           \
  tn[a] = t_;                                           \
  const uint32_t c_ = sw ? cc[b] : cc[a];               \
  cc[b] = sw ? cc[a] : cc[b];                           \
  cc[a] = c_;                                           \
}
    RPK_CSWAP(0, 1) RPK_CSWAP(2, 3) RPK_CSWAP(0, 2) RPK_CSWAP(1, 3) RPK_CSWAP(1, 2)
#undef RPK_CSWAP
    // The hits are a prefix of the sorted entries (misses sort last as +inf; a hit's key is finite, so n_hit -- the
    // number of test masks set -- is the number of keys that are not +inf).  Push the k = hits - 1
    // farther ones far-to-near without branches: slots sp..sp+2 are written unconditionally (the stack
    // has STACK_SLACK spare entries; slots past the new top are garbage) and sp advances by k.
    const uint32_t k = n_hit > 1u ? n_hit - 1u : 0u;
    const uint32_t e0 = k == 3u ? cc[3] : (k == 2u ? cc[2] : cc[1]), e1 = k == 3u ? cc[2] : cc[1];
    // Whether every lane's pushes and pops of this visit stay in the LDS part of its stack: a wave-uniform branch
    // (SPILL kernels), so the common case runs no per-lane exec-mask juggling for the spill path.
    const bool lds_only = !SPILL || __ballot(sp + 2u >= S.lds_depth) == 0;
    if (lds_only) {
      stk[sp * stride] = e0;
      stk[(sp + 1u) * stride] = e1;
      stk[(sp + 2u) * stride] = cc[1];
    } else {
      stk_put<SPILL>(S, stk, stride, spl, sp, e0);
      stk_put<SPILL>(S, stk, stride, spl, sp + 1u, e1);
      stk_put<SPILL>(S, stk, stride, spl, sp + 2u, cc[1]);
    }
    sp += k;
    if (sp > cap) {  // cannot happen for a stack sized from the tree depth; flagged, never written past
      overflow = true;
      sp = cap;
    }
    // pops below read entries < the pushes' top (sp + 2 before the push), so an LDS-only visit pops from LDS
    const auto pop = [&]() -> uint32_t {
      --sp;
      return lds_only ? stk[sp * stride] : stk_get<SPILL>(S, stk, stride, spl, sp);
    };
    // Speculative traversal (Aila & Laine 2009): a lane that reaches a leaf parks it and keeps
    // descending, so lanes do not idle in this loop until every lane of the wave holds a leaf.  (Not in the
    // cost probe, COUNT: there a lane's node visits and primitive tests must not depend on its wave-mates, so
    // every rank of a balanced multi-GPU frame computes the same costs -- include/rp.h RP_SHARD_BALANCED.)
    if (lds_only) {
      // the next entry without a branch: the two entries under the top are read at once (indices clamped into the
      // column; an entry below the stack's bottom is read but never taken), then the pop for a visit that hit no
      // child and the pop behind a parked leaf are selects
      const uint32_t t1 = stk[min(sp - 1u, sp) * stride], t2 = stk[min(sp - 2u, sp) * stride];
      uint32_t npop = (!n_hit && sp) ? 1u : 0u;
      uint32_t c = n_hit ? cc[0] : (sp ? t1 : rpl::ENTRY_EMPTY);
      if constexpr (!COUNT) {
        const bool park = (c & rpl::ENTRY_LEAF) && c != rpl::ENTRY_EMPTY && leaf == 0u;
        const uint32_t left = sp - npop;
        leaf = park ? c : leaf;
        const uint32_t c2 = left ? (npop ? t2 : t1) : rpl::ENTRY_EMPTY;
        npop += (park && left) ? 1u : 0u;
        c = park ? c2 : c;
      }
      cur = c;
      sp -= npop;
    } else {
      if (n_hit) cur = cc[0];
      else cur = sp ? pop() : rpl::ENTRY_EMPTY;
      if constexpr (!COUNT) {
        if ((cur & rpl::ENTRY_LEAF) && cur != rpl::ENTRY_EMPTY && leaf == 0u) {
          leaf = cur;
          cur = sp ? pop() : rpl::ENTRY_EMPTY;
        }
      }
    }
    if constexpr (!COUNT) {
      // ... and once at most S.leaf_break lanes still look for one, the wave moves on to the leaves: the
      // last few descents ran with most of the wave idle (those lanes resume their descent next step)
      if ((uint32_t)__popcll(__ballot(leaf == 0u)) <= S.leaf_break) break;
    }
  }
  DCYC_END(DCYC_NODE_LOOP, cnode)
  DCYC_BEGIN(cprim)
  // the pops from here on only shrink sp: when no lane's stack reaches into its spill run, they all read LDS (a
  // wave-uniform branch, as in the node loop)
  const bool lds_pop = !SPILL || __ballot(sp > S.lds_depth) == 0;
  const auto pop = [&]() -> uint32_t {
    --sp;
    return lds_pop ? stk[sp * stride] : stk_get<SPILL>(S, stk, stride, spl, sp);
  };
  if (leaf == 0u && cur != rpl::ENTRY_EMPTY && (cur & rpl::ENTRY_LEAF)) {
    leaf = cur;
    cur = sp ? pop() : rpl::ENTRY_EMPTY;
  }
  // ---- leaves: the reference's exact f64 primitive tests, the parked leaf first, then the current
  // entry while it is a leaf as well.  One primitive per lane per iteration across those leaves, so
  // lanes with different leaf sizes advance together instead of the wave running every leaf's count.
  uint32_t k = leaf & rpl::LEAF_FIRST_MASK;
  uint32_t kend = k + ((leaf >> rpl::LEAF_SHIFT) & 7u) + 1u;
  // The loop runs on the wave's condition (the number of lanes that hold a leaf), a lane without one skips the body:
  // no lane leaves the loop before the others, so the closest hit, cur and sp stay in one set of registers from the
  // step's entry to its exit (a per-lane `while (leaf != 0u)` made the compiler keep a copy of all of them for the
  // lanes that had left, remade at the loop's header and at both ends of the step).
  uint32_t testing = (uint32_t)__popcll(__ballot(leaf != 0u));
  while (testing != 0u) {
    if (leaf != 0u) {
      DIAG(if (td) td->tests++;)
      if constexpr (COUNT) *work += WORK_TEST;
      DREG(DREG_PRIM)
      prim_test(S, k, o, d, tmin, best, ts);
      if (++k == kend) {
        if (cur != rpl::ENTRY_EMPTY && (cur & rpl::ENTRY_LEAF)) {
          leaf = cur;
          cur = sp ? pop() : rpl::ENTRY_EMPTY;
          k = leaf & rpl::LEAF_FIRST_MASK;
          kend = k + ((leaf >> rpl::LEAF_SHIFT) & 7u) + 1u;
        } else {
          leaf = 0u;
        }
      }
    }
    testing = (uint32_t)__popcll(__ballot(leaf != 0u));
    if (!COUNT && PRIM_BREAK > 0 && testing <= PRIM_BREAK) {
      // park the rest of the current run [k, kend) as a leaf entry; the next step tests it first
      if (leaf != 0u) leaf = rpl::ENTRY_LEAF | ((kend - k - 1u) << rpl::LEAF_SHIFT) | k;
      break;
    }
  }
  DCYC_END(DCYC_PRIM_LOOP, cprim)
  ts.cur = cur;
  ts.sp = sp;
  ts.best = best;
  ts.leaf = leaf;
}

template <uint32_t NF, bool SCALAR = true>
RPK_INLINE void traverse(const KScene& S, lds_u32* stk, uint32_t stride, V3 o, V3 d, double tmin, double tmax,
                         HitRec& hr, bool& overflow, TravDiag* td = nullptr) {
  Ray32 r;
  setup_ray32<NF>(o, d, tmin, S.qbound, r);
  TravState t;
  trav_begin<NF, SCALAR>(S, o, d, tmin, tmax, t);
  while (!trav_done(t)) trav_step<false, NF>(S, stk, stride, 0u, r, o, d, tmin, t, overflow, td);
  hr.t = t.best;
  hr.u = t.bu;
  hr.v = t.bv;
  hr.prim = t.bestp;
  hr.km = t.bestm;
}

// A word of a material, texture or per-primitive normals record: 32-bit byte offset from the wave-uniform table base
// (scalar-base + vector-offset loads, as nodes and primitives are read; the builder refuses tables beyond 4 GB).
template <class T>
RPK_INLINE T rec_load(const void* base, uint32_t off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + off);
}
// Two doubles of such a record as one 16 B load from an address that is 8-byte aligned only (rpl::TriNormals).  Its own
// function: as a template argument the typedef would lose its alignment.
typedef double double2a8 __attribute__((ext_vector_type(2), aligned(8)));
RPK_INLINE double2a8 rec_load_d2(const void* base, uint32_t off) {
  return *reinterpret_cast<const double2a8*>(reinterpret_cast<const char*>(base) + off);
}

// Hit record of the closest primitive (hittable.rs:59-62, 103-107).
struct Surf {
  V3 p, n;
  double u, v;
  uint32_t material;
};

// uv is computed only when the hit material reads it (rpl::Material::needs_uv): same values, and the
// f64 atan2/asin of a sphere hit are skipped for untextured spheres (the ground).
//
// surface_at is the record for a caller that already holds the hit's material (s.material) and can tell whether it
// reads uv (shade_ray: from the material's head, asked for only where a path needs the answer, so that the head's load
// is not waited for in front of the surface's own first load); surface() finds both itself.
RPK_INLINE uint32_t hit_material(const KScene& S, const HitRec& hr) {
  return hr.km != KM_UNKNOWN ? hr.km & ~KM_TRIANGLE : S.prims[hr.prim].material;
}
template <class F>
RPK_INLINE bool surface_at(const KScene& S, const HitRec& hr, V3 o, V3 d, Surf& s, F need_uv) {
  const rpl::Prim* p = S.prims + hr.prim;
  s.p = add(o, smul(hr.t, d));  // Ray::at (utility.rs:67)
  const bool known = hr.km != KM_UNKNOWN;
  s.u = 0.0;
  s.v = 0.0;
  if (known ? (hr.km & KM_TRIANGLE) != 0 : p->kind == rpl::PRIM_TRIANGLE) {
    const double u = hr.u, v = hr.v, w = 1.0 - u - v;
    // The three vertex normals: the primitive's own 72 B record (rp_layout.h TriNormals), five loads at a 32-bit byte
    // offset from the wave-uniform table base that depend on the hit record alone -- in shade_ray they go out with the
    // material head's, and shading waits for memory once in front of the interpolation.  (Through the vertex ids they
    // were two round trips: PrimRef, then nine loads from three rows of the vertex table.)
    const uint32_t toff = (uint32_t)hr.prim * (uint32_t)sizeof(rpl::TriNormals);
    const double2a8 q0 = rec_load_d2(S.tri_nrm, toff), q1 = rec_load_d2(S.tri_nrm, toff + 16u);
    const double2a8 q2 = rec_load_d2(S.tri_nrm, toff + 32u), q3 = rec_load_d2(S.tri_nrm, toff + 48u);
    const double q4 = rec_load<double>(S.tri_nrm, toff + 64u);
    // (all 18 words count as read here, where they are issued: the compiler neither splits the group nor sinks a part
    // of it behind a wait of its own)
    asm volatile("" : : "v"(q0.x), "v"(q0.y), "v"(q1.x), "v"(q1.y), "v"(q2.x), "v"(q2.y), "v"(q3.x), "v"(q3.y), "v"(q4));
    const V3 n0 = v3(q0.x, q0.y, q1.x), n1 = v3(q1.y, q2.x, q2.y), n2 = v3(q3.x, q3.y, q4);
    s.n = add(add(smul(w, n0), smul(u, n1)), smul(v, n2));
    if (need_uv()) {  // a textured mesh (rare): the ids, then the uvs -- two trips
      const rpl::PrimRef& pr = S.prim_refs[hr.prim];
      const uint32_t i0 = pr.v[0], i1 = pr.v[1], i2 = pr.v[2];
      s.u = (w * S.vuv[2 * i0] + u * S.vuv[2 * i1]) + v * S.vuv[2 * i2];
      s.v = (w * S.vuv[2 * i0 + 1] + u * S.vuv[2 * i1 + 1]) + v * S.vuv[2 * i2 + 1];
    }
  } else {
    const V3 c = v3(p->g[0], p->g[1], p->g[2]);
    s.n = normalize(sub(s.p, c));
    return need_uv();  // the caller computes the sphere uv (shared site)
  }
  return false;
}
RPK_INLINE bool surface(const KScene& S, const HitRec& hr, V3 o, V3 d, Surf& s, bool force_uv = false) {
  s.material = hit_material(S, hr);
  const bool need_uv = force_uv || S.mats[s.material].needs_uv != 0;
  return surface_at(S, hr, o, d, s, [&] { return need_uv; });
}

// ------------------------------------------------------------------ shading ----------------------

RPK_INLINE uint32_t mat_at(uint32_t material) { return material * (uint32_t)sizeof(rpl::Material); }

// x / 255.0 for a byte x, correctly rounded without a division: q0 = x * fl(1/255) is off by at most
// one ulp and one FMA residual step corrects it (exhaustively checked for all 256 x, tests/test_host.py).
RPK_INLINE double u8_unit(uint32_t x) {
  const double xd = (double)x, R = 1.0 / 255.0;
  const double q0 = xd * R;
  return __builtin_fma(__builtin_fma(-q0, 255.0, xd), R, q0);
}

// texture.rs:51-60: walk Checker indirections down to the texture that produces the value
// (validate() guarantees the walk terminates).
// A record's first four words {kind, odd, even, width} come as one 16 B load, so a level of the walk waits for memory
// once; `th` returns the resolved texture's, whose kind and width the callers go on with instead of reading them again.
RPK_INLINE uint32_t tex_at(uint32_t tid) { return tid * (uint32_t)sizeof(rpl::Texture); }
RPK_INLINE uint4 tex_head(const KScene& S, uint32_t tid) {
  static_assert(offsetof(rpl::Texture, kind) == 0 && offsetof(rpl::Texture, odd) == 4 && offsetof(rpl::Texture, even) == 8 &&
                offsetof(rpl::Texture, width) == 12, "Texture head");
  const uint4 t = rec_load<uint4>(S.texs, tex_at(tid));
  // (all four words count as read here: left to itself the compiler narrows the load to the kind and fetches the
  // children and the width by loads of their own, each behind its own wait)
  asm volatile("" : : "v"(t.x), "v"(t.y), "v"(t.z), "v"(t.w));
  return t;
}
RPK_INLINE uint32_t tex_resolve(const KScene& S, uint32_t tid, const Surf& h, uint4& th) {
  th = tex_head(S, tid);
  while (th.x == 4) {
    const double s = floor(h.p.x) + floor(h.p.y) + floor(h.p.z);
    tid = fmod(s, 2.0) == 0.0 ? th.z : th.y;
    th = tex_head(S, tid);
  }
  return tid;
}

// One RGBA8 texel (a non-temporal load, keeping the sky's random bounce lookups out of L2, cost +5 %)
RPK_INLINE uint32_t texel(const KScene& S, uint64_t i) { return S.texels[i]; }

// texture.rs:40-49 Image: clamp, then saturating `as u32` -> texel index
RPK_INLINE uint64_t image_texel(uint32_t width, uint32_t height, uint64_t texel_offset, const Surf& h) {
  const double w = (double)width, hh = (double)height;
  double x = h.u * w, y = h.v * hh;
  if (x < 0.0) x = 0.0;
  if (x > w - 1.0) x = w - 1.0;
  if (y < 0.0) y = 0.0;
  if (y > hh - 1.0) y = hh - 1.0;
  return texel_offset + (uint64_t)sat_u32(x) + (uint64_t)sat_u32(y) * width;
}

// The texel of a resolved Image texture (width from its head): its height and offset are two more loads, issued
// together, then the texel's.
RPK_INLINE uint32_t image_fetch(const KScene& S, uint32_t tid, uint32_t width, const Surf& h) {
  const uint32_t height = rec_load<uint32_t>(S.texs, tex_at(tid) + (uint32_t)offsetof(rpl::Texture, height));
  const uint64_t off = rec_load<uint64_t>(S.texs, tex_at(tid) + (uint32_t)offsetof(rpl::Texture, texel_offset));
  // (both count as read here, in the block that loads them: used only in the texel's block, one of them stays pending
  // in the compiler's books on the paths around it, and the scatter's first write to its register waits for memory --
  // for the texel too)
  asm volatile("" : : "v"(height), "v"(off));
  return texel(S, image_texel(width, height, off, h));
}

// texture.rs:21-118 value of a resolved (non-Checker) texture of kind `kind` (from its head: not read again);
// `px` is the Image texel, fetched by the caller ahead of use so its latency overlaps other shading work.
RPK_INLINE V3 tex_value(const KScene& S, uint32_t tid, uint32_t kind, const Surf& h, uint32_t px) {
  const rpl::Texture& t = *reinterpret_cast<const rpl::Texture*>(reinterpret_cast<const char*>(S.texs) + tex_at(tid));
  switch (kind) {
    case 1:  // DebugUVs
      return v3(h.u, h.v, 0.0);
    case 2:  // Solid
      return v3(t.color[0], t.color[1], t.color[2]);
    case 3:  // Image
      return v3(u8_unit(px & 0xffu), u8_unit((px >> 8) & 0xffu), u8_unit((px >> 16) & 0xffu));
      case 5: {  // Noise (texture.rs:62-68)
        double x = noise_real(sat_i64(floor(h.p.x)), sat_i64(floor(h.p.y)), sat_i64(floor(h.p.z)), t.seed);
        x = 0.5 * x + 0.5;
        return v3(x, x, x);
      }
      case 6: {  // Perlin (texture.rs:83-118)
        const V3 p = h.p;
        const V3 fp = v3(floor(p.x), floor(p.y), floor(p.z));
        const int64_t fx = sat_i64(fp.x), fy = sat_i64(fp.y), fz = sat_i64(fp.z);
        const int64_t cx = (int64_t)((uint64_t)fx + 1), cy = (int64_t)((uint64_t)fy + 1),
                      cz = (int64_t)((uint64_t)fz + 1);
        const int64_t s1 = (int64_t)((uint64_t)t.seed + 1), s2 = (int64_t)((uint64_t)t.seed + 2),
                      s3 = (int64_t)((uint64_t)t.seed + 3);
        double k[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          const int64_t X = (q & 1) ? cx : fx, Y = (q & 2) ? cy : fy, Z = (q & 4) ? cz : fz;
          const V3 g = v3(noise_real(X, Y, Z, s1), noise_real(X, Y, Z, s2), noise_real(X, Y, Z, s3));
          k[q] = dot(sub(p, v3((double)X, (double)Y, (double)Z)), g);
        }
        V3 tt = sub(p, fp);
        tt.x = (tt.x * (tt.x * 6.0 - 15.0) + 10.0) * tt.x * tt.x * tt.x;
        tt.y = (tt.y * (tt.y * 6.0 - 15.0) + 10.0) * tt.y * tt.y * tt.y;
        tt.z = (tt.z * (tt.z * 6.0 - 15.0) + 10.0) * tt.z * tt.z * tt.z;
        const double k12 = (k[1] - k[0]) * tt.x + k[0], k34 = (k[3] - k[2]) * tt.x + k[2];
        const double k56 = (k[5] - k[4]) * tt.x + k[4], k78 = (k[7] - k[6]) * tt.x + k[6];
        const double k1234 = (k34 - k12) * tt.y + k12, k5678 = (k78 - k56) * tt.y + k56;
        const double kk = (k5678 - k1234) * tt.z + k1234;
        const double x = 0.5 * kk + 0.5;
        return v3(x, x, x);
      }
      default:  // Missing
      return v3(0.0, 0.0, 0.0);
  }
}

RPK_INLINE V3 tex_sample(const KScene& S, uint32_t tid, const Surf& h) {
  uint4 th;
  tid = tex_resolve(S, tid, h, th);
  const uint32_t px = th.x == 3 ? image_fetch(S, tid, th.w, h) : 0u;
  return tex_value(S, tid, th.x, h, px);
}

// material.rs:49-60 Emit::evaluate (SkySphere's texture value sampled by the caller)
RPK_INLINE V3 emit_eval(uint32_t kind, V3 color, V3 tex, V3 d, const Surf& h) {
  switch (kind) {
    case 1: return h.n;                                  // DebugNormals
    case 2: return color;                                // Color
    case 3: {                                            // SkyGradient
      const double t = 0.5 * (d.y / sqrt(norm2(d)) + 1.0);
      return add(smul(1.0 - t, v3(1.0, 1.0, 1.0)), smul(t, v3(0.5, 0.7, 1.0)));
    }
    case 4: return tex;                                  // SkySphere
    default: return v3(0.0, 0.0, 0.0);                   // None
  }
}

// material.rs:74-81 Absorb::evaluate (AlbedoMap's texture value sampled by the caller)
RPK_INLINE V3 absorb_eval(uint32_t kind, V3 color, V3 tex) {
  switch (kind) {
    case 1: return v3(1.0, 1.0, 1.0);
    case 2: return color;
    case 3: return tex;
    default: return v3(0.0, 0.0, 0.0);
  }
}
RPK_INLINE V3 absorb_eval(const rpl::Material& m, V3 tex) {
  return absorb_eval(m.absorb_kind, v3(m.absorb_color[0], m.absorb_color[1], m.absorb_color[2]), tex);
}

// material.rs:27-34, 115-179 Scatter::evaluate.  Returns true and the new direction when scattered.
template <class R>
RPK_INLINE bool scatter_eval(uint32_t kind, double param, V3 d, const Surf& h, R& rng, V3& nd) {
  switch (kind) {
    case 1: {  // Lambert (material.rs:115-130)
      DREG(DREG_LAMBERT)
      if (dot(h.n, d) > 0.0) return false;
      // UnitSphere (randomness.rs:58-73): tries of 2 draws, TRIES per round (see ring_round)
      rpd::Draw q;
      for (uint32_t a = rng.pos;; a += 4u * TRIES) {
        DREG(DREG_LOOP_LAMBERT)
        if (ring_round<4u>(rng, a, q)) break;
      }
      const double f = 2.0 * sqrt(1.0 - q.s);
      nd = normalize(add(h.n, v3(q.x * f, q.y * f, 1.0 - 2.0 * q.s)));
      return true;
    }
    case 2: {  // Metal (material.rs:132-152)
      DREG(DREG_METAL)
      if (dot(h.n, d) > 0.0) return false;
      // UnitBall (randomness.rs:39-53): tries of 3 draws, TRIES per round (see ring_round)
      rpd::Draw q;
      for (uint32_t a = rng.pos;; a += 6u * TRIES) {
        DREG(DREG_LOOP_METAL)
        if (ring_round<6u>(rng, a, q)) break;
      }
      const V3 r = normalize(add(reflect(d, h.n), smul(param, v3(q.x, q.y, q.z))));
      if (dot(h.n, r) < 0.0) return false;
      nd = r;
      return true;
    }
    case 3: {  // Dielectric (material.rs:154-179)
      DREG(DREG_DIELEC)
      double eta;
      V3 n;
      if (dot(h.n, d) > 0.0) { eta = param; n = v3(-h.n.x, -h.n.y, -h.n.z); }
      else { eta = 1.0 / param; n = h.n; }
      double r0 = (1.0 - eta) / (1.0 + eta);
      r0 = r0 * r0;                                  // powi(2)
      const double x = 1.0 + dot(n, d);
      const double x2 = x * x;
      const double reflectance = r0 + (1.0 - r0) * (x * (x2 * x2));  // powi(5), LLVM binary expansion
      if (gen_f64(rng) < reflectance) {              // Bernoulli (randomness.rs:78-82)
        nd = reflect(d, n);
      } else {
        const double cos_theta = dot(n, d);          // refract (utility.rs:111-119)
        const double k = 1.0 - eta * eta * (1.0 - cos_theta * cos_theta);
        if (k < 0.0) nd = reflect(d, n);
        else nd = sub(smul(eta, d), smul(eta * cos_theta + sqrt(k), n));
      }
      return true;
    }
    default:
      return false;
  }
}

// Shading of one finished ray: the step of the reference's trace_path after the closest-hit query
// (render.rs:104-118 / 133-145, material.rs:104-110): the hit's surface record or the miss's
// Hit::at_infinity, textures, Scatter (the only RNG consumer), Absorb, Emit; T (*) emit goes into the sum
// (forward accumulation: main.rs:80 adds the sample's total, the association differs in the last ulp only).
// Returns true when the material scattered: (o, d) become the hit point and the new direction and T is
// multiplied by the absorption.  Hits and misses share one spherical-uv site and one texture site, so a
// wave with both pays for each f64 atan2/asin and texture walk once.
template <class R, class D, class U>
RPK_INLINE bool shade_ray(const KScene& S, const HitRec& hr, V3& o, V3& d, R& rng, D& T_x, D& T_y, D& T_z, D& sum_x,
                          D& sum_y, D& sum_z, bool first, U& hits) {
  const bool hit = hr.prim >= 0;
  Surf h;
  // A hit's material: its head (the control words, rp_layout.h) and scatter_param, two loads that depend on the hit
  // record alone and go out with the surface's first load, in front of shading's first wait.  Everything below
  // branches on the head's bits; the record's f64 colours follow the scatter.
  uint32_t moff = 0;
  rpl::MaterialHead mh = rpl::material_head_unpack(0u, 0u);
  double sparam = 0.0;
  bool sph_uv;
  if (hit) {
    DREG(DREG_SURF)
    DCYC_BEGIN(c0)
    h.material = hit_material(S, hr);
    moff = mat_at(h.material);
    const uint2 hw = rec_load<uint2>(S.mats, moff + (uint32_t)offsetof(rpl::Material, head));
    sparam = rec_load<double>(S.mats, moff + (uint32_t)offsetof(rpl::Material, scatter_param));
    sph_uv = surface_at(S, hr, o, d, h, [&] { return (hw.x & rpl::MH_NEEDS_UV) != 0; });
    mh = rpl::material_head_unpack(hw.x, hw.y);
    DCYC_END(DCYC_SURF, c0)
  } else {
    DREG(DREG_MISS)
    // background.evaluate(ray, Hit::at_infinity(dir)) (render.rs:118,144; utility.rs:93-100)
    h.p = d;
    h.n = d;
    h.u = 0.0;
    h.v = 0.0;
    h.material = 0;
    sph_uv = S.background.needs_uv != 0;
  }
  if (sph_uv) {  // hittable.rs:59-62 for a sphere hit, utility.rs:96-97 for a miss
    DREG(DREG_SPHUV)
    DCYC_BEGIN(c1)
    const V3 q = hit ? h.n : d;
    h.u = 0.5 - atan2(q.z, q.x) / TAU_;
    h.v = asin(q.y) / PI_ + 0.5;
    DCYC_END(DCYC_SPHUV, c1)
  }
  // Textures: each lane reads at most one here -- the absorb map of a hit or the sky sphere of a miss
  // (or of an emissive hit); its Checker walk and Image texel load are issued BEFORE the scatter so
  // the load latency overlaps it.  A hit reading both takes the second in a rare extra pass.
  const uint32_t emit_kind = hit ? mh.emit_kind : S.background.kind;
  uint32_t absorb_tex = mh.absorb_tex, emit_tex = hit ? mh.emit_tex : S.background.tex;
  if (mh.wide) {  // texture ids beyond 16 bits: the head holds none
    absorb_tex = rec_load<uint32_t>(S.mats, moff + (uint32_t)offsetof(rpl::Material, absorb_tex));
    emit_tex = rec_load<uint32_t>(S.mats, moff + (uint32_t)offsetof(rpl::Material, emit_tex));
  }
  const bool ta = hit && mh.absorb_kind == 3, te = emit_kind == 4;
  const bool t1 = ta || te;
  uint32_t tid1 = 0, px1 = 0, kind1 = 0;
  // a miss under an Image sky sphere: size and offset are kernel arguments (scalar registers), so the
  // texel load waits on no texture-table load
  const bool sky_img = !hit && S.background.img_w != 0;
  // Every load issued so far has been waited for by now on every path (the surface's own wait is a full one), but the
  // compiler's books still hold one as pending and put a full wait in front of the scatter, behind the texel's load:
  // the same wait here, where nothing is in flight, clears the books, and the texel then waits with the scatter's first
  // ring window.
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  DCYC_BEGIN(c2)
  if (t1) {
    if (sky_img) {
      tid1 = S.background.tex;
      px1 = texel(S, image_texel(S.background.img_w, S.background.img_h, S.background.img_off, h));
    } else {
      uint4 th;
      tid1 = tex_resolve(S, ta ? absorb_tex : emit_tex, h, th);
      kind1 = th.x;
      if (kind1 == 3) px1 = image_fetch(S, tid1, th.w, h);
    }
  }
  DCYC_END(DCYC_TEXISSUE, c2)
  // scatter (the only RNG consumer; material.rs order scatter, absorb, emit -- the textures draw none)
  V3 nd = v3(0.0, 0.0, 0.0);
  bool scattered = false;
  if (hit) {
    DCYC_BEGIN(c3)
    scattered = scatter_eval(mh.scatter_kind, sparam, d, h, rng, nd);
    DCYC_END(DCYC_SCATTER, c3)
  }
  V3 tex_ab = v3(0.0, 0.0, 0.0), tex_em = v3(0.0, 0.0, 0.0);
  DCYC_BEGIN(c4)
  if (t1) {
    DREG(DREG_TEX)
    const V3 tv = sky_img ? v3(u8_unit(px1 & 0xffu), u8_unit((px1 >> 8) & 0xffu), u8_unit((px1 >> 16) & 0xffu))
                          : tex_value(S, tid1, kind1, h, px1);
    if (ta) tex_ab = tv;
    else tex_em = tv;
  }
  if (ta && te) tex_em = tex_sample(S, emit_tex, h);
  DCYC_END(DCYC_TEXVAL, c4)
  DCYC_BEGIN(c5)
  // a hit's two colours (twelve registers, too many to hold across the scatter): four loads issued together and
  // waited for once -- counted as read here, or the compiler moves each into the branch that reads it, behind a wait
  // of its own
  V3 acol = v3(0.0, 0.0, 0.0), ecol = v3(S.background.color[0], S.background.color[1], S.background.color[2]);
  if (hit) {
    constexpr uint32_t A = (uint32_t)offsetof(rpl::Material, absorb_color), E = (uint32_t)offsetof(rpl::Material, emit_color);
    static_assert(A % 16 == 8 && E == A + 24, "absorb_color[1..2] and emit_color[0..1] as 16 B loads");
    const double a0 = rec_load<double>(S.mats, moff + A), e2 = rec_load<double>(S.mats, moff + E + 16);
    const double2 a12 = rec_load<double2>(S.mats, moff + A + 8), e01 = rec_load<double2>(S.mats, moff + E);
    asm volatile("" : : "v"(a0), "v"(a12.x), "v"(a12.y), "v"(e01.x), "v"(e01.y), "v"(e2));
    acol = v3(a0, a12.x, a12.y);
    ecol = v3(e01.x, e01.y, e2);
  }
  const V3 em = emit_eval(emit_kind, ecol, tex_em, d, h);
  // emit + absorb (*) trace_path_continue (render.rs:108-115, 135-142), accumulated forward: each
  // bounce's T (*) emit goes straight into the pixel sum (main.rs:80 adds the sample's total; the
  // association differs in the last ulp only)
  sum_x = sum_x + T_x * em.x;
  sum_y = sum_y + T_y * em.y;
  sum_z = sum_z + T_z * em.z;
  if (hit && first) hits++;
  if (scattered) {
    const V3 ab = absorb_eval(mh.absorb_kind, acol, tex_ab);
    T_x = T_x * ab.x;
    T_y = T_y * ab.y;
    T_z = T_z * ab.z;
    o = h.p;
    d = nd;
  }
  DCYC_END(DCYC_EMIT, c5)
  return scattered;
}

// ------------------------------------------------------------------ render kernel ----------------

RPK_INLINE V3 matvec(const double* m, V3 v) {  // nalgebra Matrix3 * Vector3 (column axpy)
  return v3((v.x * m[0] + v.y * m[3]) + v.z * m[6], (v.x * m[1] + v.y * m[4]) + v.z * m[7],
            (v.x * m[2] + v.y * m[5]) + v.z * m[8]);
}

RPK_INLINE KScene load_scene(KArgsPtr A) {
  KScene S;
  S.nodes = A->S.nodes;
  S.prims = A->S.prims;
  S.prim_refs = A->S.prim_refs;
  S.tri_nrm = A->S.tri_nrm;
  S.vuv = A->S.vuv;
  S.mats = A->S.mats;
  S.texs = A->S.texs;
  S.texels = A->S.texels;
  S.background.kind = A->S.background.kind;
  S.background.tex = A->S.background.tex;
  S.background.needs_uv = A->S.background.needs_uv;
  S.background.img_w = A->S.background.img_w;
  S.background.img_h = A->S.background.img_h;
  S.background.img_off = A->S.background.img_off;
  S.background.color[0] = A->S.background.color[0];
  S.background.color[1] = A->S.background.color[1];
  S.background.color[2] = A->S.background.color[2];
  S.root = A->S.root;
  S.always_first = A->S.always_first;
  S.n_always = A->S.n_always;
  S.qbound = A->S.qbound;
  S.node_format = A->S.node_format;
  S.leaf_break = A->S.leaf_break;
  S.stack_depth = A->S.stack_depth;
  S.lds_depth = A->S.lds_depth;
  S.spill = A->S.spill;
  S.rng_slab = A->S.rng_slab;
  S.unit_t0 = A->S.unit_t0;
  return S;
}

RPK_INLINE KArgsPtr kargs() {
  KArgsPtr p = (KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// What rp_units.h's unit fetch needs from the place it runs in, on the GPU (the host library has its own, rp_host_sched.cpp).
// All forced inline, so the fetch reaches the optimizer as the text it was when it stood here.
struct DevEnv {
  static RPK_INLINE KArgsPtr args() { return kargs(); }
  static RPK_INLINE uint32_t fetch_add(unsigned int* p) { return atomicAdd(p, 1u); }
  static RPK_INLINE bool any(bool x) { return __ballot(x) != 0; }
  static RPK_INLINE uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
  static RPK_INLINE uint32_t block() { return blockIdx.x; }
  static RPK_INLINE uint32_t numerator(uint32_t n) { return n; }
};

// Camera::shoot (render.rs:32-52) from the jittered frame coordinates (ju, jv) and the UnitDisk sample (dx, dy): one
// definition for the path loop (start_sample) and the coherent primary pass, which passes (0, 0) -- with lens_radius 0
// the disk is multiplied by 0 and only the signs of zeros could differ (the direction never: -focal - 0 and
// x - (+-0) for x != 0 are exact, and x = (2 ju - 1) ... is +0 when 2 ju - 1 = 0).
RPK_INLINE void camera_dir(KArgsPtr A, double ju, double jv, double dx, double dy, V3& o, V3& d) {
  // tan(fov/2) is computed on the host (render.rs:33 is a per-camera constant; same libm as the reference)
  const double lens = A->P.lens, tanf = A->P.tan_fov, focal = A->P.focal, aspect = A->P.aspect;
  const V3 lo = v3(lens * dx, lens * dy, 0.0);
  const V3 dl = normalize(sub(v3((2.0 * ju - 1.0) * tanf * focal * aspect, (2.0 * jv - 1.0) * tanf * focal, -focal), lo));
  double m[9];
#pragma unroll
  for (int q = 0; q < 9; q++) m[q] = A->P.orient[q];
  d = matvec(m, dl);
  o = add(matvec(m, lo), v3(A->P.pos[0], A->P.pos[1], A->P.pos[2]));
}

// One camera sample (main.rs:75-76): make_uv_jitter draws 2s, 2s+1 of a CLONE of the pixel-start
// stream (render.rs:74-82) = keystream words 4s..4s+3 = block s/4 at offset 4(s%4); Camera::shoot
// (render.rs:32-52) then draws its UnitDisk from the main stream (even when lens_radius == 0).
template <class R>
RPK_INLINE void start_sample(R& rng, uint32_t s, uint32_t pi, uint32_t pj, V3& o, V3& d) {
  DREG(DREG_START_SAMPLE)
  KArgsPtr A = kargs();
  double jw[2];
  rng_jitter(rng, s, jw);
  const double ju = ((double)pi + rpd::unit_of(jw[0])) / (double)A->P.W;
  const double jv = ((double)pj + rpd::unit_of(jw[1])) / (double)A->P.H;
  // UnitDisk (randomness.rs:21-34): tries of 2 draws, TRIES per round (see ring_round)
  rpd::Draw q;
  for (uint32_t a = rng.pos;; a += 4u * TRIES) {
    if (ring_round<4u>(rng, a, q)) break;
  }
  const double dx = q.x, dy = q.y;
  camera_dir(kargs(), ju, jv, dx, dy, o, d);
}

}  // namespace rpk
