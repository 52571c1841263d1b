// rp_denoise.hip -- the guided denoiser (include/rp.h rp_denoise*): an edge-avoiding a-trous wavelet
// filter (Dammertz et al. 2010) over a frame-order beauty frame and the feature pass's guides.  The arithmetic is
// rp_denoise.h's, shared with the CPU loop behind rph_denoise; this file is the kernel, its launches and the C-ABI.
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like rp_aov.hip, not part of the
// rp_build_id hash: it decides no ray of a render.
//
// Kernel: one launch per level.  Level l's taps lie s = 2^l pixels apart, so a pixel only ever reads pixels of its own
// residue class (i mod s, j mod s).  A block of TX x TY lanes takes a TX x TY tile of ONE class's sub-lattice: there the
// 5 x 5 stencil is dense, and the tile with its halo of 2 -- (TX + 4) x (TY + 4) pixel records, the same for every level
// -- is read from global memory once, into LDS, instead of 25 gathers of 80 bytes per lane.  TX = 32: a half-wave (the
// group a ds_read_b64 is banked in) reads 32 consecutive doubles of one row of one field (structure of arrays), which is
// conflict-free at any row pitch, and at s = 1 a row of the tile is 768 contiguous bytes of each input.  Blocks of the
// s x s classes over the same tile are neighbours in the grid (they share cache lines).  The first level demodulates as
// it loads (rgb / (albedo + eps), once per loaded pixel), the last one remodulates as it stores and copies the
// pass-through pixels' rgb; levels in between ping-pong between two colour buffers in the caller's scratch.  nn is made
// once per loaded pixel.  No allocation, no synchronisation, nothing but launches on the caller's stream.
//
// The variance-guided filter (rp_denoise_var*) is the instantiation VAR = true of the same kernel: the
// pixel record grows from 11 to 12 doubles by the variance v (made from var and the albedo as the first level loads,
// ping-ponged in scratch beside the colour after it), and the 3 x 3 prefilter of v reads taps the tile already holds.
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers rp_denoise.h uses

#include "rp_denoise.h"

#pragma clang fp contract(off)

namespace rpdn {

constexpr int TX = 32, TY = 8, HALO = 2, LW = TX + 2 * HALO, LH = TY + 2 * HALO, LN = LW * LH;
constexpr int DN_BLOCK = TX * TY;
enum { F_CX, F_CY, F_CZ, F_NX, F_NY, F_NZ, F_NN, F_AX, F_AY, F_AZ, F_Z, F_N, F_V = F_N, F_NV };  // VAR: one more

struct DnArgs {
  Level L;
  uint32_t W, H;
  uint32_t tiles_x;      // tiles across the widest class's sub-lattice: the grid is (tiles_x s) x (tiles_y s) blocks
  uint32_t first, last;  // the level demodulates its input / writes the frame
  const double* rgb;     // the frame (the last level's pass-through pixels)
  const double* in;      // the level's input colour: rgb for the first level, a scratch buffer after it
  const double* normal;
  const double* albedo;
  const double* depth;
  double* out;
  // VAR: the frame's variance (3 per pixel; the first level's input), the later levels' input v and this level's v'
  // (1 per pixel, scratch; the last level writes none)
  const double* var;
  const double* vin;
  double* vout;
};

template <bool VAR>
__device__ __forceinline__ Px lds_px(const double (*t)[LN], int e, uint32_t flags) {
  Px q = {};
  q.cx = t[F_CX][e], q.cy = t[F_CY][e], q.cz = t[F_CZ][e];
  if (flags & HAS_NORMAL) q.nx = t[F_NX][e], q.ny = t[F_NY][e], q.nz = t[F_NZ][e], q.nn = t[F_NN][e];
  if (flags & HAS_ALBEDO) q.ax = t[F_AX][e], q.ay = t[F_AY][e], q.az = t[F_AZ][e];
  if (flags & HAS_DEPTH) q.z = t[F_Z][e];
  if (VAR) q.v = t[F_V][e];
  return q;
}

template <bool VAR>
__global__ void __launch_bounds__(DN_BLOCK) denoise_level(const DnArgs A) {
  __shared__ double tile[VAR ? F_NV : F_N][LN];
  const Level L = A.L;
  const uint32_t s = (uint32_t)L.step, flags = L.flags;
  // block -> residue class (ri, rj) and tile (tx, ty) of its sub-lattice; the class's pixels are (ri + s u, rj + s v)
  const uint32_t gx = A.tiles_x * s, bx = blockIdx.x % gx, by = blockIdx.x / gx;
  const uint32_t ri = bx % s, tx = bx / s, rj = by % s, ty = by / s;
  const int sw = ri < A.W ? (int)((A.W - ri + s - 1) / s) : 0, sh = rj < A.H ? (int)((A.H - rj + s - 1) / s) : 0;
  const int u0 = (int)tx * TX, v0 = (int)ty * TY;
  if (u0 >= sw || v0 >= sh) return;  // the whole block: a class narrower than the widest one, or outside a small frame
  for (int e = (int)threadIdx.x; e < LN; e += DN_BLOCK) {
    const int u = u0 + e % LW - HALO, v = v0 + e / LW - HALO;
    if (u < 0 || u >= sw || v < 0 || v >= sh) continue;  // outside the frame: a tap the lanes skip, never read
    const uint64_t px = (uint64_t)(rj + s * (uint32_t)v) * A.W + (ri + s * (uint32_t)u);
    double cx = A.in[3 * px], cy = A.in[3 * px + 1], cz = A.in[3 * px + 2];
    double vx = 0.0, vy = 0.0, vz = 0.0;
    if (VAR && A.first) vx = A.var[3 * px], vy = A.var[3 * px + 1], vz = A.var[3 * px + 2];
    if (flags & HAS_ALBEDO) {
      const double ax = A.albedo[3 * px], ay = A.albedo[3 * px + 1], az = A.albedo[3 * px + 2];
      tile[F_AX][e] = ax, tile[F_AY][e] = ay, tile[F_AZ][e] = az;
      if (A.first) cx = demod(cx, ax, L.eps), cy = demod(cy, ay, L.eps), cz = demod(cz, az, L.eps);
      if (VAR && A.first) vx = demod_var(vx, ax, L.eps), vy = demod_var(vy, ay, L.eps), vz = demod_var(vz, az, L.eps);
    }
    if (VAR) tile[F_V][e] = A.first ? sum3(vx, vy, vz) : A.vin[px];
    tile[F_CX][e] = cx, tile[F_CY][e] = cy, tile[F_CZ][e] = cz;
    if (flags & HAS_NORMAL) {
      const double nx = A.normal[3 * px], ny = A.normal[3 * px + 1], nz = A.normal[3 * px + 2];
      tile[F_NX][e] = nx, tile[F_NY][e] = ny, tile[F_NZ][e] = nz;
      tile[F_NN][e] = len2(nx, ny, nz);
    }
    if (flags & HAS_DEPTH) tile[F_Z][e] = A.depth[px];
  }
  __syncthreads();
  const int lx = (int)threadIdx.x % TX, ly = (int)threadIdx.x / TX;
  const int u = u0 + lx, v = v0 + ly;
  if (u >= sw || v >= sh) return;
  const int e0 = (ly + HALO) * LW + lx + HALO;
  const Px p = lds_px<VAR>(tile, e0, flags);
  double ox, oy, oz, ov;
  level_step_v<VAR>(
      L, p,
      [&](int dx, int dy, Px& q) {
        const int uu = u + dx, vv = v + dy;
        if (uu < 0 || uu >= sw || vv < 0 || vv >= sh) return false;
        q = lds_px<VAR>(tile, e0 + dy * LW + dx, flags);
        return true;
      },
      ox, oy, oz, ov);
  const uint64_t px = (uint64_t)(rj + s * (uint32_t)v) * A.W + (ri + s * (uint32_t)u);
  if (A.last) {
    if (passes(L, p)) {  // rgb itself, bit for bit
      ox = A.rgb[3 * px], oy = A.rgb[3 * px + 1], oz = A.rgb[3 * px + 2];
    } else if (flags & HAS_ALBEDO) {
      ox = remod(ox, p.ax, L.eps), oy = remod(oy, p.ay, L.eps), oz = remod(oz, p.az, L.eps);
    }
  }
  A.out[3 * px] = ox, A.out[3 * px + 1] = oy, A.out[3 * px + 2] = oz;
  if (VAR && !A.last) A.vout[px] = ov;
}

}  // namespace rpdn

namespace {

using rpp::overlaps;

// Doubles of scratch per pixel: two colour buffers (3 each) and, with the variance, two variance buffers (1 each).
constexpr uint64_t scratch_doubles(bool var) { return var ? 2 * (3 + 1) : 2 * 3; }

// The device's own refusals, after rp_denoise.h's check_frames: the scratch of rp_denoise_device and
// rp_denoise_var_device (d_var NULL: the former).
int check_scratch(uint32_t width, uint32_t height, const double* d_rgb, const double* d_var, const double* d_normal,
                  const double* d_albedo, const double* d_depth, const double* d_out, const void* d_scratch) {
  const uint64_t n = (uint64_t)width * height, b3 = 3 * n * sizeof(double), b1 = n * sizeof(double);
  const uint64_t scratch_bytes = scratch_doubles(d_var != nullptr) * b1;
  if (overlaps(d_scratch, scratch_bytes, d_out, b3) || overlaps(d_scratch, scratch_bytes, d_rgb, b3) ||
      overlaps(d_scratch, scratch_bytes, d_normal, b3) || overlaps(d_scratch, scratch_bytes, d_albedo, b3) ||
      overlaps(d_scratch, scratch_bytes, d_depth, b1) || overlaps(d_scratch, scratch_bytes, d_var, b3))
    return fail(RP_EINVAL, "scratch must not alias an input or out");
  if (reinterpret_cast<uintptr_t>(d_scratch) % sizeof(double)) return fail(RP_EINVAL, "scratch must be 8-byte aligned");
  return RP_OK;
}

// One launch per level of P (resolved: rp_denoise_params, or rp_denoise_var_params with VAR), ping-ponging between the
// two colour buffers -- and, VAR, the two variance buffers behind them -- of d_scratch.
template <bool VAR, class Params>
int launch_levels(const Params& P, uint32_t iterations, uint32_t width, uint32_t height, const double* d_rgb,
                  const double* d_var, const double* d_normal, const double* d_albedo, const double* d_depth,
                  double* d_out, void* d_scratch, void* stream) {
  const uint64_t n = (uint64_t)width * height;
  double* const base = static_cast<double*>(d_scratch);
  double* buf[2] = {base, base + 3 * n};
  double* vbuf[2] = {VAR ? base + 6 * n : nullptr, VAR ? base + 7 * n : nullptr};
  const double* in = d_rgb;
  const double* vin = nullptr;
  for (uint32_t l = 0; l < iterations; l++) {
    rpdn::DnArgs a;
    a.L = rpdn::make_level(P, l, d_normal != nullptr, d_albedo != nullptr, d_depth != nullptr);
    const uint32_t s = (uint32_t)a.L.step;
    a.W = width, a.H = height;
    a.tiles_x = ((width + s - 1) / s + rpdn::TX - 1) / rpdn::TX;
    const uint32_t tiles_y = ((height + s - 1) / s + rpdn::TY - 1) / rpdn::TY;
    a.first = l == 0, a.last = l + 1 == iterations;
    a.rgb = d_rgb, a.in = in;
    a.normal = d_normal, a.albedo = d_albedo, a.depth = d_depth;
    a.out = a.last ? d_out : buf[l & 1u];
    a.var = d_var, a.vin = vin;
    a.vout = VAR && !a.last ? vbuf[l & 1u] : nullptr;
    const uint64_t grid = (uint64_t)a.tiles_x * s * tiles_y * s;  // < 2^31: at most (2048 + 128) x (8192 + 128) blocks
    hipLaunchKernelGGL(rpdn::denoise_level<VAR>, dim3((unsigned)grid), dim3(rpdn::DN_BLOCK), 0, (hipStream_t)stream, a);
    RP_HIP(hipGetLastError());
    in = a.out;
    vin = a.vout;
  }
  return RP_OK;
}

// rp_denoise and rp_denoise_var: the frames up, `enqueue(buffers..., stream)` as a synchronous call, the result down.
// var NULL: rp_denoise.
template <class Enqueue>
int denoise_sync(int device, uint32_t width, uint32_t height, const double* rgb, const double* var, const double* normal,
                 const double* albedo, const double* depth, double* out, double* seconds, Enqueue enqueue) {
  if (const char* why = rpdn::check_frames(width, height, rgb, var, normal, albedo, depth, out)) return fail(RP_EINVAL, why);
  const uint64_t n = (uint64_t)width * height;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(RP_ENODEV, "no HIP device");
  if (device < 0 || device >= count) return fail(RP_EINVAL, "device out of range");
  DeviceGuard g(device);
  DevBuf<double> d_rgb, d_var, d_normal, d_albedo, d_depth, d_out, d_scratch;
  if (!d_rgb.alloc(3 * n) || !d_out.alloc(3 * n) || !d_scratch.alloc(scratch_doubles(var != nullptr) * n) ||
      (var && !d_var.alloc(3 * n)) || (normal && !d_normal.alloc(3 * n)) || (albedo && !d_albedo.alloc(3 * n)) ||
      (depth && !d_depth.alloc(n)))
    return fail(RP_ENOMEM, "hipMalloc frame buffers");
  RP_HIP(hipMemcpy(d_rgb.get(), rgb, 24 * n, hipMemcpyHostToDevice));
  if (var) RP_HIP(hipMemcpy(d_var.get(), var, 24 * n, hipMemcpyHostToDevice));
  if (normal) RP_HIP(hipMemcpy(d_normal.get(), normal, 24 * n, hipMemcpyHostToDevice));
  if (albedo) RP_HIP(hipMemcpy(d_albedo.get(), albedo, 24 * n, hipMemcpyHostToDevice));
  if (depth) RP_HIP(hipMemcpy(d_depth.get(), depth, 8 * n, hipMemcpyHostToDevice));
  double s = 0.0;
  const int rc = rpp::sync_call(device, "denoise", &s, [&](void* st) {
    return enqueue(d_rgb.get(), d_var.get(), d_normal.get(), d_albedo.get(), d_depth.get(), d_out.get(), d_scratch.get(), st);
  });
  if (rc) return rc;
  RP_HIP(hipMemcpy(out, d_out.get(), 24 * n, hipMemcpyDeviceToHost));
  if (seconds) *seconds = s;
  return RP_OK;
}

const char* const VAR_RANGE = "denoise params out of range: iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo, "
                              "albedo_eps, sigma_var and var_eps > 0 and finite";

}  // namespace

extern "C" {

int rp_denoise_params_init(rp_denoise_params* p) {
  if (!p) return fail(RP_EINVAL, "params is NULL");
  rpdn::defaults(*p);
  return RP_OK;
}

int rp_denoise_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes) {
  if (const char* why = rpdn::check_size(width, height)) return fail(RP_EINVAL, why);
  if (!bytes) return fail(RP_EINVAL, "bytes is NULL");
  *bytes = scratch_doubles(false) * sizeof(double) * width * height;
  return RP_OK;
}

int rp_denoise_device(const rp_denoise_params* params, uint32_t width, uint32_t height, const double* d_rgb,
                      const double* d_normal, const double* d_albedo, const double* d_depth, double* d_out,
                      void* d_scratch, void* stream) {
  if (const char* why = rpdn::check_frames(width, height, d_rgb, nullptr, d_normal, d_albedo, d_depth, d_out))
    return fail(RP_EINVAL, why);
  if (!d_scratch) return fail(RP_EINVAL, "scratch must be non-NULL");
  rp_denoise_params P;
  if (!rpdn::resolve(params, P))
    return fail(RP_EINVAL, "denoise params out of range: iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo "
                           "and albedo_eps > 0 and finite, sigma_color finite (negative disables)");
  if (const int rc = check_scratch(width, height, d_rgb, nullptr, d_normal, d_albedo, d_depth, d_out, d_scratch)) return rc;
  return launch_levels<false>(P, P.iterations, width, height, d_rgb, nullptr, d_normal, d_albedo, d_depth, d_out,
                              d_scratch, stream);
}

int rp_denoise(const rp_denoise_params* params, int device, uint32_t width, uint32_t height, const double* rgb,
               const double* normal, const double* albedo, const double* depth, double* out, double* seconds) {
  rp_denoise_params P;
  if (!rpdn::resolve(params, P)) return fail(RP_EINVAL, "denoise params out of range");
  return denoise_sync(device, width, height, rgb, nullptr, normal, albedo, depth, out, seconds,
                      [&](const double* d_rgb, const double*, const double* d_normal, const double* d_albedo,
                          const double* d_depth, double* d_out, void* d_scratch, void* st) {
                        return rp_denoise_device(&P, width, height, d_rgb, d_normal, d_albedo, d_depth, d_out, d_scratch, st);
                      });
}

int rp_denoise_var_params_init(rp_denoise_var_params* p) {
  if (!p) return fail(RP_EINVAL, "params is NULL");
  rpdn::defaults(*p);
  return RP_OK;
}

int rp_denoise_var_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes) {
  if (const char* why = rpdn::check_size(width, height)) return fail(RP_EINVAL, why);
  if (!bytes) return fail(RP_EINVAL, "bytes is NULL");
  *bytes = scratch_doubles(true) * sizeof(double) * width * height;
  return RP_OK;
}

int rp_denoise_var_device(const rp_denoise_var_params* params, uint32_t width, uint32_t height, const double* d_rgb,
                          const double* d_var, const double* d_normal, const double* d_albedo, const double* d_depth,
                          double* d_out, void* d_scratch, void* stream) {
  if (const char* why = rpdn::check_frames(width, height, d_rgb, d_var, d_normal, d_albedo, d_depth, d_out))
    return fail(RP_EINVAL, why);
  if (!d_var || !d_scratch) return fail(RP_EINVAL, "var and scratch must be non-NULL");
  rp_denoise_var_params P;
  if (!rpdn::resolve(params, P)) return fail(RP_EINVAL, VAR_RANGE);
  if (const int rc = check_scratch(width, height, d_rgb, d_var, d_normal, d_albedo, d_depth, d_out, d_scratch)) return rc;
  return launch_levels<true>(P, P.base.iterations, width, height, d_rgb, d_var, d_normal, d_albedo, d_depth, d_out,
                             d_scratch, stream);
}

int rp_denoise_var(const rp_denoise_var_params* params, int device, uint32_t width, uint32_t height, const double* rgb,
                   const double* var, const double* normal, const double* albedo, const double* depth, double* out,
                   double* seconds) {
  if (!var) return fail(RP_EINVAL, "var must be non-NULL");
  rp_denoise_var_params P;
  if (!rpdn::resolve(params, P)) return fail(RP_EINVAL, VAR_RANGE);
  return denoise_sync(device, width, height, rgb, var, normal, albedo, depth, out, seconds,
                      [&](const double* d_rgb, const double* d_var, const double* d_normal, const double* d_albedo,
                          const double* d_depth, double* d_out, void* d_scratch, void* st) {
                        return rp_denoise_var_device(&P, width, height, d_rgb, d_var, d_normal, d_albedo, d_depth, d_out,
                                                     d_scratch, st);
                      });
}

}  // extern "C"
