// rp_ray.h -- the arithmetic that takes a ray into the conservative f32 slab test, for host and device.
//
// Per axis a the traversal needs the slope inv_a = clamp(rcp(fl(d_a)), +-2^64) and two FMA addends that move the
// axis's planes outward by D_a >= E_a (the absolute error terms of t^ = fma(P, inv, -oinv), rp_isect.h "conservative
// f32 box test" and DESIGN.md 4.2), and per ray tmin32 <= t_min and best32 >= best.  Five inequalities carry the
// proof (rp_isect.h: it is written next to the test) that no box the exact f64 test reaches is culled:
//     nb_a <= -oinv_a - D_a      fb_a >= -oinv_a + D_a      D_a >= E_a      tmin32 <= t_min      best32 >= best
// with oinv_a = fl(o32_a inv_a), o32_a = fl(o_a) and
//     E_a = |o_a - o32_a| |inv_a| (1 + 6u) + 2u |o32_a inv_a|                               (u = 2^-24)
//           + u (1 + u) |inv_a| (2 qbound + |o32_a|) + u^2 |o32_a inv_a|    (quantized frames: Node4Q, Node8Q)
//
// D_a is evaluated in f64 (each f64 rounding is 2^-53 relative; k = 1 + 2^-20 covers the (1 + 6u), the (1 + u) that
// takes |oinv| to |o32 inv| and every f64 rounding; the frame term uses 2u where u (1 + u) is needed):
//     D_a = ((|o - o32| |inv| k + |oinv| 2^-23) + frame) k,   frame = |inv| (2 qbound + |o32|) 2^-23 k  or  0
// |o - o32| is exact in f64 (Sterbenz), so an axis whose origin is an f32 value gets no origin term: the product
// 0 * |inv| * k is exactly 0 (|inv| is finite by the clamp), no select is needed for it.
//
// Directed roundings.  x = -oinv -+ D is a f64 value (one f64 rounding, 2^-53 relative: inside k); what the test
// needs is an f32 on the outer side of it.  f = fl(x) (round to nearest) is within half an ulp of x on either side;
// one unconditional step of f outward -- the neighbouring float, by integer arithmetic on the bit pattern -- is
// therefore on the outer side of x, and at most one float further out than the exact directed rounding (which is f
// or f's outer neighbour).  Cases: f = +-0 (|x| < 2^-150) steps to the smallest denormal of the outer sign (-0 is made
// +0 first by adding +0.0, so the step sees one zero); for any other f its sign decides whether the step adds one to
// the bit pattern or subtracts one, and a step from the smallest denormal towards zero lands on a zero, which is
// still on the outer side of x.  Every x here is finite and below 2^121 in magnitude (|o|, qbound <= 2^56, |inv| <= 2^64), so no step
// reaches infinity and every addend is finite.  t_min takes the same step downward.  (The exact roundings
// compared x against fl(x) in f64 and stepped on demand: ~8 instructions each, most of them f64-class; this is a
// convert and four integer-class ones.)
//
// best32: best is +inf for a ray without a hit yet, and then best32 must be +inf.  best_above adds one to the bit
// pattern of fl(best) and clamps it, as an unsigned number, at +inf's pattern: for 0 <= best < +inf that is the
// neighbouring float above fl(best) (+inf when fl(best) is the largest float or rounds to +inf), >= best; +inf stays;
// a negative (or NaN) best, for which no hit can be accepted at all, has its sign bit set, so the clamp returns
// +inf -- conservative (boxes are then culled by their slabs alone).  Three instructions.
//
// The kernel (rp_device.h setup_ray32, trav_step), the CPU model of the traversal (rp_host_tree.cpp
// rph_bvh_traversal_stats) and the host test hook (rp_host.h rph_ray_setup) all use this header, and rp_isect.h for
// what follows it -- the slab test's frame terms, plane t^ and pass test, and the exact primitive tests -- so the
// arithmetic tested on the CPU is the kernel's -- except the reciprocal: the device's v_rcp_f32 (<= 1 ulp) against the
// host's correctly rounded 1 / x; the proof takes inv as given, whatever its last bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RPR_FN __host__ __device__ __forceinline__
#else
#define RPR_FN inline
#endif

namespace rpr {

RPR_FN uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
RPR_FN float bits_f32(uint32_t b) { return __builtin_bit_cast(float, b); }

// The neighbouring float above a finite f (+-0: the smallest positive denormal).
RPR_FN float step_up(float f) {
  const int32_t b = (int32_t)f32_bits(f + 0.0f);  // -0 + +0 = +0: b >= 0 exactly when f >= 0
  return bits_f32((uint32_t)(b + ((b >> 31) | 1)));  // f >= 0: one up in magnitude; f < 0: one down
}
// An f32 >= x, at most one float above the exact upward rounding (finite x, |x| below the largest float).
RPR_FN float f32_above(double x) { return step_up((float)x); }
// An f32 <= x, likewise.
RPR_FN float f32_below(double x) { return -step_up((float)-x); }
// An f32 >= best, +inf for best = +inf (and for a negative or NaN best: see above).
RPR_FN float best_above(double best) {
  const uint32_t b = f32_bits((float)best) + 1u;
  return bits_f32(b < 0x7F800000u ? b : 0x7F800000u);
}

RPR_FN float rcp32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}

struct Axis {
  float inv;  // clamp(rcp(fl(d)), +-2^64)
  float nb;   // near-plane addend <= -oinv - D
  float fb;   // far-plane addend >= -oinv + D
};

// One axis of a ray with origin coordinate o and direction component d.  FRAME: the node format has quantized frames
// (qbound bounds every frame's |o| and 255 s, rp_layout.h); an axis-parallel axis through 0 (|inv| = 2^64 and
// o32 = 0) has exact A and B and no frame term.
template <bool FRAME>
RPR_FN Axis axis_setup(double o, double d, double qbound) {
  Axis a;
  const float o32 = (float)o;
  // |inv| clamped to 2^64: a zero direction component gives a huge finite slope instead of inf, so the
  // fma form never forms inf - inf; the slack term |o - o32| |inv| still covers an origin that rounded
  // across a slab plane, and a slab the ray never reaches still yields a huge t (a miss), as in f64.
  a.inv = __builtin_fminf(__builtin_fmaxf(rcp32((float)d), -0x1p64f), 0x1p64f);
  const float oinv = o32 * a.inv;
  const double k = 1.0 + 0x1p-20, u = 0x1p-23;
  const double e = __builtin_fabs(o - (double)o32), ai = __builtin_fabs((double)a.inv);
  const double oi = (double)oinv;
  double D = e * ai * k + __builtin_fabs(oi) * u;
  if (FRAME) {
    const bool exact = __builtin_fabsf(a.inv) == 0x1p64f && o32 == 0.0f;
    D = D + (exact ? 0.0 : ai * (2.0 * qbound + __builtin_fabs((double)o32)) * u * k);
  }
  D = D * k;
  a.nb = -f32_above(oi + D);  // = f32_below(-oi - D): the negation is exact
  a.fb = f32_above(D - oi);
  return a;
}

}  // namespace rpr
