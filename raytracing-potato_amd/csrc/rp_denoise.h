// rp_denoise.h -- the arithmetic of the guided denoiser (include/rp.h rp_denoise*), for host and device:
// the parameters' defaults and ranges, a pixel's setup, the weight of one tap and the step of one pixel through one
// level of the edge-avoiding a-trous filter (Dammertz et al. 2010).
//
// Every value is IEEE binary64 and every expression uses + - * /, comparisons and max(|a|, |b|) only, written in the
// operation order include/rp.h gives and compiled without contraction (-ffp-contract=off), so the kernel
// (rp_denoise.hip), the CPU loop behind rph_denoise (rp_host.cpp) and the numpy model of the tests
// (tests/denoise_ref.py, written from the definition and not from this file) agree to the last bit.
//
// A caller hands level_step the pixel's own record and a `tap(dx, dy, q)` that fills q with the record of the pixel at
// p + s (dx, dy) and returns false where that lies outside the frame: the kernel reads a dense LDS tile of the pixel's
// residue class mod s, the host loop reads the frame.  Records come by value and by reference to locals only (scalar
// registers on the device after inlining: 0 B of scratch per lane).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/rp.h"

#if defined(__HIPCC__)
#define RPDN_FN __host__ __device__ __forceinline__
#else
#define RPDN_FN inline
#endif

namespace rpdn {

// ---- parameters: a zero field takes its default; false = out of range (RP_EINVAL)
static constexpr uint32_t DEF_ITERATIONS = 3, DEF_NORMAL_POWER = 6, MAX_ITERATIONS = 8, MAX_NORMAL_POWER = 8;
static constexpr double DEF_SIGMA_DEPTH = 0.05, DEF_SIGMA_ALBEDO = 0.1, DEF_SIGMA_COLOR = 1.0, DEF_ALBEDO_EPS = 1e-2;

inline void defaults(rp_denoise_params& p) {
  p.iterations = DEF_ITERATIONS;
  p.normal_power = DEF_NORMAL_POWER;
  p.sigma_depth = DEF_SIGMA_DEPTH;
  p.sigma_albedo = DEF_SIGMA_ALBEDO;
  p.sigma_color = DEF_SIGMA_COLOR;
  p.albedo_eps = DEF_ALBEDO_EPS;
}

// in (NULL = the defaults) with its zero fields replaced.  sigma_color < 0 stays: it disables the colour term.
inline bool resolve(const rp_denoise_params* in, rp_denoise_params& p) {
  defaults(p);
  if (!in) return true;
  if (in->iterations) p.iterations = in->iterations;
  if (in->normal_power) p.normal_power = in->normal_power;
  if (in->sigma_depth != 0.0) p.sigma_depth = in->sigma_depth;
  if (in->sigma_albedo != 0.0) p.sigma_albedo = in->sigma_albedo;
  if (in->sigma_color != 0.0) p.sigma_color = in->sigma_color;
  if (in->albedo_eps != 0.0) p.albedo_eps = in->albedo_eps;
  if (p.iterations > MAX_ITERATIONS || p.normal_power > MAX_NORMAL_POWER) return false;
  // positive and finite (x - x is NaN for an infinity or a NaN); only sigma_color may be negative
  const double pos[3] = {p.sigma_depth, p.sigma_albedo, p.albedo_eps};
  for (double x : pos)
    if (!(x > 0.0) || x - x != 0.0) return false;
  return p.sigma_color - p.sigma_color == 0.0;
}

// ---- one level's constants (made on the host for both sides)
enum : uint32_t { HAS_NORMAL = 1, HAS_ALBEDO = 2, HAS_DEPTH = 4, HAS_COLOR = 8 };
struct Level {
  uint32_t flags;    // HAS_*: the guides given and the colour term enabled
  uint32_t squares;  // e_n - 1: how often (d d) / ab is squared
  int32_t step;      // s = 2^l
  double sz;         // sigma_z
  double sa2;        // sigma_a sigma_a
  double sc2;        // sigma_c,l sigma_c,l with sigma_c,l = sigma_c / 2^l
  double eps;
};
inline Level make_level(const rp_denoise_params& p, uint32_t l, bool normal, bool albedo, bool depth) {
  Level L;
  L.flags = (normal ? HAS_NORMAL : 0u) | (albedo ? HAS_ALBEDO : 0u) | (depth ? HAS_DEPTH : 0u) |
            (p.sigma_color < 0.0 ? 0u : HAS_COLOR);
  L.squares = p.normal_power - 1u;
  L.step = (int32_t)(1u << l);
  L.sz = p.sigma_depth;
  L.sa2 = p.sigma_albedo * p.sigma_albedo;
  const double scl = p.sigma_color / (double)(1u << l);
  L.sc2 = scl * scl;
  L.eps = p.albedo_eps;
  return L;
}

// ---- a pixel: the level's input colour c and the guides (a missing guide's fields are never read)
struct Px {
  double cx, cy, cz;
  double nx, ny, nz, nn;
  double ax, ay, az;
  double z;
};

RPDN_FN double len2(double x, double y, double z) { return (x * x + y * y) + z * z; }
RPDN_FN double rat(double x2) {
  const double t = 1.0 + x2;
  return 1.0 / (t * t);
}
// demodulation and its inverse, per channel
RPDN_FN double demod(double rgb, double albedo, double eps) { return rgb / (albedo + eps); }
RPDN_FN double remod(double c, double albedo, double eps) { return c * (albedo + eps); }
// the kernel k = {3/8, 1/4, 1/16} at |d|
RPDN_FN double kern(int d) {
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375 : (a == 1 ? 0.25 : 0.0625);
}
// a pixel the filter leaves alone (background, misses): its normal is zero
RPDN_FN bool passes(const Level& L, const Px& p) { return (L.flags & HAS_NORMAL) && p.nn == 0.0; }

// w = (((h w_n) w_z) w_a) w_c of the tap q of pixel p
RPDN_FN double tap_weight(const Level& L, const Px& p, const Px& q, double h, bool centre) {
  double wn = 1.0, wz = 1.0, wa = 1.0, wc = 1.0;
  if ((L.flags & HAS_NORMAL) && !centre) {
    const double d = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
    const double ab = p.nn * q.nn;
    wn = 0.0;
    if (ab > 0.0 && d > 0.0) {
      wn = (d * d) / ab;
      for (uint32_t i = 0; i < L.squares; i++) wn = wn * wn;
    }
  }
  if (L.flags & HAS_DEPTH) {
    const double m = fmax(fabs(p.z), fabs(q.z));
    const double x = m > 0.0 ? (p.z - q.z) / (L.sz * m) : 0.0;
    wz = rat(x * x);
  }
  if (L.flags & HAS_ALBEDO) wa = rat(len2(p.ax - q.ax, p.ay - q.ay, p.az - q.az) / L.sa2);
  if (L.flags & HAS_COLOR) wc = rat(len2(p.cx - q.cx, p.cy - q.cy, p.cz - q.cz) / L.sc2);
  return (((h * wn) * wz) * wa) * wc;
}

// c' of pixel p: the 5 x 5 taps at step s, dy outer and dx inner, sums from 0.0 in tap order
template <class Tap>
RPDN_FN void level_step(const Level& L, const Px& p, Tap tap, double& ox, double& oy, double& oz) {
  if (passes(L, p)) {
    ox = p.cx;
    oy = p.cy;
    oz = p.cz;
    return;
  }
  double sw = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; dx++) {
      Px q;
      if (!tap(dx, dy, q)) continue;
      const double h = kern(dx) * kern(dy);
      const double w = tap_weight(L, p, q, h, dx == 0 && dy == 0);
      sw = sw + w;
      ax = ax + w * q.cx;
      ay = ay + w * q.cy;
      az = az + w * q.cz;
    }
  }
  ox = ax / sw;
  oy = ay / sw;
  oz = az / sw;
}

}  // namespace rpdn
