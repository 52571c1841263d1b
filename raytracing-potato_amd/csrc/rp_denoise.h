// rp_denoise.h -- the arithmetic of the guided denoiser (include/rp.h rp_denoise*), for host and device:
// the parameters' defaults and ranges, a pixel's setup, the weight of one tap and the step of one pixel through one
// level of the edge-avoiding a-trous filter (Dammertz et al. 2010).
//
// Every value is IEEE binary64 and every expression uses + - * /, comparisons and max(|a|, |b|) only, written in the
// operation order include/rp.h gives and compiled without contraction (-ffp-contract=off), so the kernel
// (rp_denoise.hip), the CPU loop behind rph_denoise (rp_host_passes.cpp) and the numpy model of the tests
// (tests/denoise_ref.py, written from the definition and not from this file) agree to the last bit.
//
// A caller hands level_step the pixel's own record and a `tap(dx, dy, q)` that fills q with the record of the pixel at
// p + s (dx, dy) and returns false where that lies outside the frame: the kernel reads a dense LDS tile of the pixel's
// residue class mod s, the host loop reads the frame.  Records come by value and by reference to locals only (scalar
// registers on the device after inlining: 0 B of scratch per lane).
//
// The variance-guided filter (include/rp.h rp_denoise_var*) is the same step with VAR = true: a pixel
// also carries the variance v of its colour, the colour stop's scale comes from a 3 x 3 prefilter of v on the level's
// own taps instead of sigma_color, and v is filtered along with the colour.  VAR = false is the guided denoiser, its
// expressions untouched.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/rp.h"
#include "rp_overlap.h"

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

// the variance-guided filter's: base.sigma_color is ignored, sigma_var and var_eps are positive and finite
static constexpr double DEF_SIGMA_VAR = 3.0, DEF_VAR_EPS = 1e-6;
inline void defaults(rp_denoise_var_params& p) {
  defaults(p.base);
  p.sigma_var = DEF_SIGMA_VAR;
  p.var_eps = DEF_VAR_EPS;
}
inline bool resolve(const rp_denoise_var_params* in, rp_denoise_var_params& p) {
  rp_denoise_params base{};
  if (in) base = in->base;
  base.sigma_color = 0.0;
  if (!resolve(&base, p.base)) return false;
  p.sigma_var = in && in->sigma_var != 0.0 ? in->sigma_var : DEF_SIGMA_VAR;
  p.var_eps = in && in->var_eps != 0.0 ? in->var_eps : DEF_VAR_EPS;
  const double pos[2] = {p.sigma_var, p.var_eps};
  for (double x : pos)
    if (!(x > 0.0) || x - x != 0.0) return false;
  return true;
}

// ---- what every entry point refuses about its frames, device and host; NULL = fine
inline const char* check_size(uint32_t width, uint32_t height) {
  if (width == 0 || height == 0 || width > 65535 || height > 65535) return "width and height must be 1..65535";
  return nullptr;
}
// var NULL: the guided denoiser (the variance-guided one refuses a NULL var itself).
inline const char* check_frames(uint32_t width, uint32_t height, const double* rgb, const double* var, const double* normal,
                                const double* albedo, const double* depth, const double* out) {
  if (const char* why = check_size(width, height)) return why;
  if (!rgb || !out) return "rgb and out must be non-NULL";
  const uint64_t b1 = 8 * (uint64_t)width * height, b3 = 3 * b1;
  using rpo::overlaps;
  if (overlaps(out, b3, rgb, b3) || overlaps(out, b3, normal, b3) || overlaps(out, b3, albedo, b3) ||
      overlaps(out, b3, depth, b1) || overlaps(out, b3, var, b3))
    return "out must not alias an input";
  return nullptr;
}

// ---- one level's constants (made on the host for both sides)
enum : uint32_t { HAS_NORMAL = 1, HAS_ALBEDO = 2, HAS_DEPTH = 4, HAS_COLOR = 8 };
struct Level {
  uint32_t flags;    // HAS_*: the guides given and the colour term enabled
  uint32_t squares;  // e_n - 1: how often (d d) / ab is squared
  int32_t step;      // s = 2^l
  double sz;         // sigma_z
  double sa2;        // sigma_a sigma_a
  double sc2;        // sigma_c,l sigma_c,l with sigma_c,l = sigma_c / 2^l; variance-guided: sigma_v sigma_v
  double eps;
  double veps;       // variance-guided: var_eps
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
  L.veps = 0.0;
  return L;
}
// the variance-guided filter's level: the colour term is always on and its scale is the same at every level
inline Level make_level(const rp_denoise_var_params& p, uint32_t l, bool normal, bool albedo, bool depth) {
  Level L = make_level(p.base, l, normal, albedo, depth);
  L.flags |= HAS_COLOR;
  L.sc2 = p.sigma_var * p.sigma_var;
  L.veps = p.var_eps;
  return L;
}

// ---- a pixel: the level's input colour c and the guides (a missing guide's fields are never read)
struct Px {
  double cx, cy, cz;
  double nx, ny, nz, nn;
  double ax, ay, az;
  double z;
  double v;  // variance-guided: the variance of c, summed over the channels
};

RPDN_FN double len2(double x, double y, double z) { return (x * x + y * y) + z * z; }
RPDN_FN double rat(double x2) {
  const double t = 1.0 + x2;
  return 1.0 / (t * t);
}
// demodulation and its inverse, per channel
RPDN_FN double demod(double rgb, double albedo, double eps) { return rgb / (albedo + eps); }
RPDN_FN double remod(double c, double albedo, double eps) { return c * (albedo + eps); }
// variance-guided: a channel's variance under demodulation, and a pixel's initial v from its three
RPDN_FN double demod_var(double var, double albedo, double eps) { return var / ((albedo + eps) * (albedo + eps)); }
RPDN_FN double sum3(double x, double y, double z) { return (x + y) + z; }
// the kernel k = {3/8, 1/4, 1/16} at |d|
RPDN_FN double kern(int d) {
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375 : (a == 1 ? 0.25 : 0.0625);
}
// variance-guided: the prefilter's kernel kg = {1/2, 1/4} at |d| <= 1
RPDN_FN double kern_g(int d) { return d == 0 ? 0.5 : 0.25; }
// a pixel the filter leaves alone (background, misses): its normal is zero
RPDN_FN bool passes(const Level& L, const Px& p) { return (L.flags & HAS_NORMAL) && p.nn == 0.0; }

// w = (((h w_n) w_z) w_a) w_c of the tap q of pixel p; sc2 divides the squared colour distance
RPDN_FN double tap_weight(const Level& L, const Px& p, const Px& q, double h, bool centre, double sc2) {
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
  if (L.flags & HAS_COLOR) wc = rat(len2(p.cx - q.cx, p.cy - q.cy, p.cz - q.cz) / sc2);
  return (((h * wn) * wz) * wa) * wc;
}

// c' (and, VAR, v') of pixel p: the 5 x 5 taps at step s, dy outer and dx inner, sums from 0.0 in tap order.
// VAR: first vf = g / gw over the 3 x 3 taps at the same step that lie in the frame and are no pass-through pixels,
// weights kg kg; the colour distance is divided by (sigma_v sigma_v) (vf + var_eps); vacc sums (w w) v_q and
// v' = vacc / (sw sw).
template <bool VAR, class Tap>
RPDN_FN void level_step_v(const Level& L, const Px& p, Tap tap, double& ox, double& oy, double& oz, double& ov) {
  if (passes(L, p)) {
    ox = p.cx;
    oy = p.cy;
    oz = p.cz;
    if (VAR) ov = p.v;
    return;
  }
  double sc2 = L.sc2;
  if (VAR) {
    double g = 0.0, gw = 0.0;
    for (int dy = -1; dy <= 1; dy++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int dx = -1; dx <= 1; dx++) {
        Px q;
        if (!tap(dx, dy, q)) continue;
        if ((L.flags & HAS_NORMAL) && !(q.nn > 0.0)) continue;
        const double k = kern_g(dx) * kern_g(dy);
        g = g + k * q.v;
        gw = gw + k;
      }
    }
    sc2 = L.sc2 * (g / gw + L.veps);
  }
  double sw = 0.0, ax = 0.0, ay = 0.0, az = 0.0, av = 0.0;
  for (int dy = -2; dy <= 2; dy++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; dx++) {
      Px q;
      if (!tap(dx, dy, q)) continue;
      const double h = kern(dx) * kern(dy);
      const double w = tap_weight(L, p, q, h, dx == 0 && dy == 0, sc2);
      sw = sw + w;
      ax = ax + w * q.cx;
      ay = ay + w * q.cy;
      az = az + w * q.cz;
      if (VAR) av = av + (w * w) * q.v;
    }
  }
  ox = ax / sw;
  oy = ay / sw;
  oz = az / sw;
  if (VAR) ov = av / (sw * sw);
}
template <class Tap>
RPDN_FN void level_step(const Level& L, const Px& p, Tap tap, double& ox, double& oy, double& oz) {
  double ov;
  level_step_v<false>(L, p, tap, ox, oy, oz, ov);
}

}  // namespace rpdn
