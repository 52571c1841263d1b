// rp_isect.h -- the arithmetic that decides what a ray hits, for host and device: the two exact f64 primitive tests
// and the pieces of the conservative f32 slab test that culls boxes in front of them.
//
// ---- exact primitive tests
//
// tri_test and sphere_test are the reference's Hittable::hit for a leaf (hittable.rs:39-101) in its expression order,
// evaluated in f64 without contraction.  Each rejects through one predicate made of the reference's own comparisons
// (so a NaN rejects, or does not, exactly where it does there); an accepted test hands t (and u, v) to the caller's
// `take`, which takes the hit.  Acceptance is t <= best, so an equal-t primitive tested later wins (hittable.rs:52,99).
// Two things about the spelling keep the kernels' instruction stream what it was with the tests written out in
// rp_device.h (profiles/r10/MANIFEST.md): `take` is called under `if (!rej)` here -- a returned "accepted" flag is a
// negation the compiler folds into the comparisons of the sphere's second root, which changes them -- and points
// and vectors come by value (scalar arguments on the device), not through pointers.
//
// ---- conservative f32 box test
//
// Conservative f32 slab test.  The ray enters in f32 as o32 = fl(o_ray), inv = rcp(fl(d)) (<= 1 ulp),
// oinv = fl(o32 * inv).  Plane coordinates P are exact: f32 values rounded outward from the exact f64 boxes
// (Node4), or P = o + q s in a node frame (Node4Q, Node8Q: f32 o and s, 8-bit q, exact in f64).
//   Node4:  t^ = fma(P, inv, -oinv)
//   Node4Q: per node and axis A = fl(s inv), B = fma(o, inv, -oinv), and t^ = fma(q, A, B) =
//           (P inv - oinv)(1 + d3) + e,  |e| <= u (1 + u)(|q s inv| + |o inv - oinv|)
// The single-rounding form fma(P, inv, -oinv) errs by <= 5u |t| + |o_ray - o32| |inv| (1 + 6u) + u |o32 inv|
// against the exact t = (P - o_ray) / d (u = 2^-24); with every |o| and |q s| <= qbound (rp_layout.h),
// |e| <= u (1 + u) |inv| (2 qbound + |o32|) + u^2 |o32 inv|, and e = 0 when inv = +-2^64 (rp_ray.h's clamp)
// and o32 = 0 (A and B exact).  Call E_a the absolute terms of axis a.  Each axis's planes are moved
// outward by its own D_a >= E_a, folded into the FMA's addend: near planes use an nb_a <= -oinv_a - D_a, far
// planes an fb_a >= -oinv_a + D_a (frames: B_near = fma(o, inv, nb_a), B_far = fma(o, inv, fb_a), whose
// roundings the frame term covers), and the ray's interval enters as tmin32 <= t_min and best32 >= best.  These five
// inequalities are all the argument uses; rp_ray.h makes the values and shows they hold: D_a in f64, the addends and
// tmin32 by rounding to nearest and one unconditional step outward (at most one float wider than the exact directed
// rounding, a third of its instructions), best32 by a three-instruction form that keeps +inf.  A wider addend only
// passes more boxes.  A box whose exact interval meets [t_min, best] at some t* > 0 then has
// every near plane <= t*(1 + 6u) (those behind the origin or below tmin32 <= t* do not raise t_near) and
// every far plane >= t*(1 - 6u), so the test
//     fma(tnear^, 1 - 2^-19, -2^-100) <= tfar^
// passes it (2^-19 = 32u).  It may pass a few more boxes, never fewer: no primitive the reference's f64 test
// reaches is culled.  The error bound is per axis: a ray nearly parallel to an axis has a huge D on that
// axis only (|inv| is huge there), which widens that slab alone -- with one scalar slack (max over the
// axes, round 1) such a ray passed every box near the plane it runs in, up to 43 k node visits on C5.
// Empty slots fail (Node4: lo = +inf, hi = -inf gives t_near = +inf; frames: masked by their entry).  Slopes
// are clamped to |inv| <= 2^64 (axis-parallel rays) and frames to |o|, 255 s <= 2^56 (rp_layout.h
// COORD_MAX), so every A, B and t^ is finite; an A that underflows errs by < 2^-118, inside the 2^-100 term.
//
// The kernel (rp_device.h prim_test, trav_step, trav_step_w8), the CPU model of the traversal (rp_host_tree.cpp
// rph_bvh_traversal_stats) and the host test hook (rp_host.h rph_prim_test) all use this header.  The device evaluates
// plane_t and the pass test two children at a time (v_pk_fma_f32: the same fused operation per element) and takes the
// near and far planes by the slope's sign where the host takes min and max of both (the same pair of values: t^ is
// monotone in the plane coordinate).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RPI_FN __host__ __device__ __forceinline__
#else
#define RPI_FN inline
#endif

namespace rpi {

static constexpr double SMOL = 1e-7;  // utility.rs:31

struct V3 {
  double x, y, z;
};

// hittable.rs:65-101; ba = a - b and ca = a - c (pre-subtracted: the same IEEE operation).  A |det| below SMOL rejects
// whatever its inv_det gave.  Accepted: take(t, u, v).
template <class Take>
RPI_FN void tri_test(V3 a, V3 ba, V3 ca, V3 o, V3 d, double tmin, double best, Take take) {
  const V3 pa = {a.x - o.x, a.y - o.y, a.z - o.z};
  const double det = ba.x * ca.y * d.z + ba.y * ca.z * d.x + ba.z * ca.x * d.y
                   - ba.x * ca.z * d.y - ba.y * ca.x * d.z - ba.z * ca.y * d.x;
  const double inv_det = 1.0 / det;
  const double t = (pa.x * (ba.y * ca.z - ba.z * ca.y)
                  + pa.y * (ba.z * ca.x - ba.x * ca.z)
                  + pa.z * (ba.x * ca.y - ba.y * ca.x)) * inv_det;
  const double u = (pa.x * (ca.y * d.z - ca.z * d.y)
                  + pa.y * (ca.z * d.x - ca.x * d.z)
                  + pa.z * (ca.x * d.y - ca.y * d.x)) * inv_det;
  const double v = (pa.x * (ba.z * d.y - ba.y * d.z)
                  + pa.y * (ba.x * d.z - ba.z * d.x)
                  + pa.z * (ba.y * d.x - ba.x * d.y)) * inv_det;
  const double w = 1.0 - u - v;
  const bool rej = (fabs(det) < SMOL) | (t < tmin) | (t > best) | (u < 0.0) | (v < 0.0) | (w < 0.0);
  if (!rej) take(t, u, v);
}

// hittable.rs:39-57; the second root stays under its branch (a division that whole waves skip).  Accepted: take(t).
template <class Take>
RPI_FN void sphere_test(V3 c, double radius, V3 o, V3 d, double tmin, double best, Take take) {
  const V3 tc = {o.x - c.x, o.y - c.y, o.z - c.z};
  const double a = (d.x * d.x + d.y * d.y) + d.z * d.z;
  const double half_b = (d.x * tc.x + d.y * tc.y) + d.z * tc.z;
  const double cq = ((tc.x * tc.x + tc.y * tc.y) + tc.z * tc.z) - radius * radius;
  const double delta = half_b * half_b - a * cq;
  bool rej = delta <= 0.0;
  const double sq = sqrt(delta);
  double t = (-half_b - sq) / a;
  if (!rej && ((t < tmin) | (t > best))) {
    t = (-half_b + sq) / a;
    rej = (t < tmin) | (t > best);
  }
  if (!rej) take(t);
}

// The pass test fma(tnear, 1 - 2^-19, -2^-100) <= tfar.
static constexpr float PASS_SCALE = 1.0f - 0x1p-19f;
static constexpr float PASS_BIAS = -0x1p-100f;
RPI_FN bool slab_pass(float tnear, float tfar) { return fmaf(tnear, PASS_SCALE, PASS_BIAS) <= tfar; }

// One axis of a quantized frame (origin o, step s) for a ray with slope inv and addends nb, fb (rp_ray.h):
// A = fl(s inv), B = fma(o, inv, nb | fb).  (The kernel calls the two pieces, all A of a node before its B: the
// instruction order of its node visit is part of its timing.)
RPI_FN float frame_a(float s, float inv) { return s * inv; }
RPI_FN float frame_b(float o, float inv, float addend) { return fmaf(o, inv, addend); }
struct FrameAxis {
  float A, Bn, Bf;
};
RPI_FN FrameAxis frame_axis(float o, float s, float inv, float nb, float fb) {
  return {frame_a(s, inv), frame_b(o, inv, nb), frame_b(o, inv, fb)};
}
// t^ of the plane with code q (Node4: the plane coordinate itself, with A = inv and B = nb or fb).
RPI_FN float plane_t(float q, float A, float B) { return fmaf(q, A, B); }

}  // namespace rpi
