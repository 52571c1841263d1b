// rp_reproject.h -- the arithmetic of temporal reprojection (include/rp.h rp_reproject_device), for
// host and device: where a pixel's surface lay in the previous pose's frame, which of the four taps around that place
// may speak for it, and the accumulation state (mean, m2, count) it inherits from them.
//
// Every value is IEEE binary64, every expression is written in the operation order include/rp.h gives and compiled
// without contraction (-ffp-contract=off), only + - * /, comparisons, floor and sqrt (correctly rounded on both sides,
// as rp_isect.h's sphere test relies on), so the kernel (rp_reproject.hip), the CPU loop behind rph_reproject
// (rp_host_passes.cpp) and the numpy model of the tests (tests/reproject_ref.py, written from the definition and not from this
// file) agree to the last bit.  The two tangents per camera are taken on the host (make_camera): no lane calls tan.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rp_overlap.h"

#if defined(__HIPCC__)
#define RPRJ_FN __host__ __device__ __forceinline__
#else
#define RPRJ_FN inline
#endif

namespace rprj {

// The four statistics of a pass (RP_REPROJECT_STATS_LEN): order-free integer sums.
enum { STAT_PIXELS = 0, STAT_KEPT = 1, STAT_COUNT = 2, STAT_OFF = 3, STATS_LEN = 4 };

// A camera as the pass sees it: orientation R[3 * col + row], position, and the half-extents of the image plane at
// unit distance, ty = tan(fov / 2) and tx = ty * aspect.
struct Camera {
  double R[9], pos[3], tx, ty;
};

// rp_reproject_params resolved: sigma_depth, normal_cos * normal_cos, max_history.
struct Params {
  double sigma_depth, cos2;
  uint32_t max_history;
};

// The frame, both cameras and the previous pose's guides and state.
struct Frame {
  uint32_t W, H;
  Camera cur, prev;
  Params P;
  const double* depth_prev;
  const double* normal_prev;
  const double* mean_prev;
  const double* m2_prev;
  const uint32_t* count_prev;
};

struct Result {
  double mean[3], m2[3];
  uint32_t count;
  bool off;
};

// Neither NaN nor an infinity, by comparisons alone.
RPRJ_FN bool finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

RPRJ_FN double sum3(double x, double y, double z) { return (x + y) + z; }

// Pixel (i, j) of the current frame, its depth z and normal n: the definition's steps 1 to 9.
RPRJ_FN Result reproject_pixel(const Frame& F, uint32_t i, uint32_t j, double z, double nx, double ny, double nz) {
  Result r;
  r.count = 0, r.off = true;
  for (int c = 0; c < 3; c++) r.mean[c] = 0.0, r.m2[c] = 0.0;
  const double Wd = (double)F.W, Hd = (double)F.H;
  // 1. the pixel's ray in the current camera
  const double u = ((double)i + 0.5) / Wd, v = ((double)j + 0.5) / Hd;
  const double sx = (2.0 * u - 1.0) * F.cur.tx, sy = (2.0 * v - 1.0) * F.cur.ty;
  const double l = sqrt((sx * sx + sy * sy) + 1.0);
  // 2. geometry or sky
  const double nn = sum3(nx * nx, ny * ny, nz * nz);
  const bool geo = nn > 0.0 && z > 0.0;
  // 3. the world vector from the previous camera (sky: a direction, no translation)
  double Lx = sx, Ly = sy, Lz = -1.0;
  if (geo) {
    const double g = z / l;
    Lx = sx * g, Ly = sy * g, Lz = -g;
  }
  const double* R = F.cur.R;
  double Ex = (R[0] * Lx + R[3] * Ly) + R[6] * Lz;
  double Ey = (R[1] * Lx + R[4] * Ly) + R[7] * Lz;
  double Ez = (R[2] * Lx + R[5] * Ly) + R[8] * Lz;
  if (geo) {
    Ex = (Ex + F.cur.pos[0]) - F.prev.pos[0];
    Ey = (Ey + F.cur.pos[1]) - F.prev.pos[1];
    Ez = (Ez + F.cur.pos[2]) - F.prev.pos[2];
  }
  // 4. into the previous frame
  const double* Q = F.prev.R;
  const double qx = (Q[0] * Ex + Q[1] * Ey) + Q[2] * Ez;
  const double qy = (Q[3] * Ex + Q[4] * Ey) + Q[5] * Ez;
  const double qz = (Q[6] * Ex + Q[7] * Ey) + Q[8] * Ez;
  const double m = -qz;
  const double fx = ((qx / (m * F.prev.tx) + 1.0) * 0.5) * Wd - 0.5;
  const double fy = ((qy / (m * F.prev.ty) + 1.0) * 0.5) * Hd - 0.5;
  // 5. off the previous frame (a NaN fails a comparison)
  if (!(m > 0.0 && fx > -1.0 && fx < Wd && fy > -1.0 && fy < Hd)) return r;
  r.off = false;
  // 6. the taps' corner and weights
  const double fi = floor(fx), fj = floor(fy);
  const double a = fx - fi, b = fy - fj;
  const int64_t i0 = (int64_t)fi, j0 = (int64_t)fj;  // -1 .. W - 1, -1 .. H - 1
  const double z_exp = geo ? sqrt(sum3(qx * qx, qy * qy, qz * qz)) : 0.0;
  // 7., 8. the counting taps, in order
  double sw = 0.0, best = 0.0, acc[3] = {0.0, 0.0, 0.0}, sacc[3] = {0.0, 0.0, 0.0};
  uint32_t n_best = 0;
  for (int dy = 0; dy < 2; dy++)
    for (int dx = 0; dx < 2; dx++) {
      const int64_t ti = i0 + dx, tj = j0 + dy;
      if (ti < 0 || ti >= (int64_t)F.W || tj < 0 || tj >= (int64_t)F.H) continue;
      const double w = (dx ? a : 1.0 - a) * (dy ? b : 1.0 - b);
      if (!(w > 0.0)) continue;
      const uint64_t t = (uint64_t)tj * F.W + (uint64_t)ti;
      const uint32_t ct = F.count_prev[t];
      if (ct < 1) continue;
      const double tx = F.normal_prev[3 * t], ty = F.normal_prev[3 * t + 1], tz = F.normal_prev[3 * t + 2];
      const double nnt = sum3(tx * tx, ty * ty, tz * tz);
      if (geo) {
        if (!(nnt > 0.0)) continue;
        const double d = F.depth_prev[t] - z_exp;
        if (!((d < 0.0 ? -d : d) <= F.P.sigma_depth * z_exp)) continue;
        const double c = sum3(nx * tx, ny * ty, nz * tz);
        if (!(c > 0.0 && c * c >= F.P.cos2 * (nn * nnt))) continue;
      } else if (!(nnt == 0.0)) {
        continue;
      }
      sw += w;
      const double div = ct >= 2 ? (double)(ct - 1u) : 1.0;
      for (int ch = 0; ch < 3; ch++) {
        acc[ch] += w * F.mean_prev[3 * t + ch];
        const double s = ct >= 2 ? F.m2_prev[3 * t + ch] / div : 0.0;
        sacc[ch] += w * s;
      }
      if (w > best) best = w, n_best = ct;
    }
  // 9. the inherited state
  if (n_best == 0) return r;
  r.count = n_best < F.P.max_history ? n_best : F.P.max_history;
  const double df = (double)(r.count - 1u);
  for (int ch = 0; ch < 3; ch++) {
    r.mean[ch] = acc[ch] / sw;
    r.m2[ch] = (sacc[ch] / sw) * df;
  }
  return r;
}

// Host side.  rp_reproject_params with the zeros replaced by the defaults; false: out of range.
template <class P>
inline bool resolve(const P* in, Params& out) {
  out.sigma_depth = in && in->sigma_depth != 0.0 ? in->sigma_depth : 0.05;
  const double nc = in && in->normal_cos != 0.0 ? in->normal_cos : 0.9;
  out.cos2 = nc * nc;
  out.max_history = in && in->max_history ? in->max_history : 32u;
  return out.sigma_depth > 0.0 && finite(out.sigma_depth) && nc > 0.0 && nc <= 1.0 && out.max_history <= 0x7fffffffu;
}
template <class P>
inline void defaults(P& p) {
  p.sigma_depth = 0.05, p.normal_cos = 0.9, p.max_history = 32, p.reserved = 0;
}

// An rp_camera as the pass sees it; false: a field that is not finite, or a field of view whose tangent is not > 0.
template <class C>
inline bool make_camera(const C& c, Camera& out) {
  bool ok = finite(c.aspect_ratio) && finite(c.fov) && finite(c.focal_dist) && finite(c.lens_radius);
  for (int k = 0; k < 9; k++) ok = ok && finite(c.orientation[k]), out.R[k] = c.orientation[k];
  for (int k = 0; k < 3; k++) ok = ok && finite(c.position[k]), out.pos[k] = c.position[k];
  if (!ok) return false;
  out.ty = tan(0.5 * c.fov);
  out.tx = out.ty * c.aspect_ratio;
  return out.ty > 0.0 && finite(out.ty);
}

// What rp_reproject_device and rph_reproject refuse about their frame and buffers; NULL = fine.
inline const char* check_buffers(uint32_t width, uint32_t height, const void* depth_cur, const void* normal_cur,
                                 const void* depth_prev, const void* normal_prev, const void* mean_prev,
                                 const void* m2_prev, const void* count_prev, const void* mean, const void* m2,
                                 const void* count, const void* stats) {
  if (width == 0 || height == 0 || width > 65535 || height > 65535) return "width and height must be 1..65535";
  if (!depth_cur || !normal_cur || !depth_prev || !normal_prev || !mean_prev || !m2_prev || !count_prev || !mean || !m2 ||
      !count || !stats)
    return "every buffer must be non-NULL";
  const uint64_t n = (uint64_t)width * height;
  struct Range {
    const void* p;
    uint64_t bytes;
  };
  const Range in[7] = {{depth_cur, 8 * n},  {normal_cur, 24 * n}, {depth_prev, 8 * n}, {normal_prev, 24 * n},
                       {mean_prev, 24 * n}, {m2_prev, 24 * n},    {count_prev, 4 * n}};
  const Range out[4] = {{mean, 24 * n}, {m2, 24 * n}, {count, 4 * n}, {stats, 8 * (uint64_t)STATS_LEN}};
  auto overlaps = [](const Range& a, const Range& b) { return rpo::overlaps(a.p, a.bytes, b.p, b.bytes); };
  for (int o = 0; o < 4; o++) {
    for (int k = 0; k < 7; k++)
      if (overlaps(out[o], in[k])) return "an output must not alias an input (a gather: in place is wrong)";
    for (int k = o + 1; k < 4; k++)
      if (overlaps(out[o], out[k])) return "the outputs must not alias one another";
  }
  return nullptr;
}

}  // namespace rprj
