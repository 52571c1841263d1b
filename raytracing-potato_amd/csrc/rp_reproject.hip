// rp_reproject.hip -- temporal reprojection (include/rp.h rp_reproject_device and rp_reproject): the
// accumulation state of the previous camera pose -- running mean, m2 and a per-pixel frame count -- carried to where its
// surfaces appear from the current pose, with the depth and normal guides of the feature pass deciding which of the
// four taps around the reprojected place may speak for a pixel.  No ray is traced.  The arithmetic is rp_reproject.h's,
// shared with the CPU loop behind rph_reproject; this file is the kernel, its launch and the C-ABI.
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like rp_denoise.hip and rp_accum.hip, not
// part of the rp_build_id hash: it runs between renders and decides no ray of them.
//
// reproject_kernel: a gather, one lane per pixel of the current frame.  A block is RJ_BX x RJ_BY = 64 x 4 lanes, a wave
// 64 consecutive pixels of one row, so the current guides are read and the state written as contiguous runs; the four
// taps are plain global loads that neighbouring lanes share in L1 and L2 (a small camera move maps a row's run to a
// near-row run of the previous frame), no LDS staging.  The tangents arrive as arguments.  The four statistics are
// order-free integers: ballots and a wave sum of the counts, then the block's waves through 128 bytes of LDS, then one
// vector atomic per block and statistic, as rp_accum.hip's error pass.  zero_stats_kernel clears them first.
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers the shared headers use

#include "rp_reproject.h"

#pragma clang fp contract(off)

namespace rprj {

constexpr int RJ_BX = 64, RJ_BY = 4, RJ_BLOCK = RJ_BX * RJ_BY, RJ_WAVES = RJ_BLOCK / 64;

struct RjArgs {
  Frame F;
  const double* depth_cur;
  const double* normal_cur;
  double* mean;
  double* m2;
  uint32_t* count;
  unsigned long long* stats;  // STATS_LEN
};

// The statistics start at zero: a kernel of its own ahead of reproject_kernel on the stream, not a memset -- a captured
// graph replays a kernel node with the arguments it was captured with.
__global__ void __launch_bounds__(64) zero_stats_kernel(unsigned long long* stats) {
  if (threadIdx.x < STATS_LEN) stats[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(RJ_BLOCK) reproject_kernel(const RjArgs A) {
  __shared__ unsigned long long part[RJ_WAVES][STATS_LEN];
  const uint32_t i = blockIdx.x * RJ_BX + threadIdx.x, j = blockIdx.y * RJ_BY + threadIdx.y;
  const bool inside = i < A.F.W && j < A.F.H;  // no early return: every lane reaches the ballots and the barrier
  bool kept = false, off = false;
  unsigned long long n = 0;
  if (inside) {
    const uint64_t px = (uint64_t)j * A.F.W + i;
    const Result r = reproject_pixel(A.F, i, j, A.depth_cur[px], A.normal_cur[3 * px], A.normal_cur[3 * px + 1],
                                     A.normal_cur[3 * px + 2]);
    A.mean[3 * px] = r.mean[0], A.mean[3 * px + 1] = r.mean[1], A.mean[3 * px + 2] = r.mean[2];
    A.m2[3 * px] = r.m2[0], A.m2[3 * px + 1] = r.m2[1], A.m2[3 * px + 2] = r.m2[2];
    A.count[px] = r.count;
    kept = r.count >= 1, off = r.off, n = r.count;
  }
  const unsigned long long n_inside = __popcll(__ballot(inside)), n_kept = __popcll(__ballot(kept)),
                           n_off = __popcll(__ballot(off));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);  // lane 0: the wave's sum (64 counts below 2^31)
  const uint32_t lane = threadIdx.x, wave = threadIdx.y;    // RJ_BX = 64: a wave is a row of the block
  if (lane == 0) {
    part[wave][STAT_PIXELS] = n_inside;
    part[wave][STAT_KEPT] = n_kept;
    part[wave][STAT_COUNT] = n;
    part[wave][STAT_OFF] = n_off;
  }
  __syncthreads();
  if (wave == 0 && lane < STATS_LEN) {
    unsigned long long v = part[0][lane];
#pragma unroll
    for (int k = 1; k < RJ_WAVES; k++) v += part[k][lane];
    if (v) atomicAdd(A.stats + lane, v);
  }
}

}  // namespace rprj

namespace {

// Parameters, cameras and buffers checked, and the kernel's arguments.
int reproject_args(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                   const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                   const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                   double* mean, double* m2, uint32_t* count, uint64_t* stats, rprj::RjArgs& a) {
  if (!cur || !prev) return fail(RP_EINVAL, "cur and prev must be non-NULL");
  if (const char* why = rprj::check_buffers(width, height, depth_cur, normal_cur, depth_prev, normal_prev, mean_prev,
                                            m2_prev, count_prev, mean, m2, count, stats))
    return fail(RP_EINVAL, why);
  if (!rprj::resolve(params, a.F.P))
    return fail(RP_EINVAL, "reproject params out of range: sigma_depth > 0 and finite, normal_cos in (0, 1], max_history "
                           "1 .. 2^31 - 1");
  if (!rprj::make_camera(*cur, a.F.cur) || !rprj::make_camera(*prev, a.F.prev))
    return fail(RP_EINVAL, "a camera field is not finite, or tan(fov / 2) is not > 0");
  a.F.W = width, a.F.H = height;
  a.F.depth_prev = depth_prev, a.F.normal_prev = normal_prev;
  a.F.mean_prev = mean_prev, a.F.m2_prev = m2_prev, a.F.count_prev = count_prev;
  a.depth_cur = depth_cur, a.normal_cur = normal_cur;
  a.mean = mean, a.m2 = m2, a.count = count;
  a.stats = reinterpret_cast<unsigned long long*>(stats);
  return RP_OK;
}

}  // namespace

extern "C" {

int rp_reproject_params_init(rp_reproject_params* p) {
  if (!p) return fail(RP_EINVAL, "params is NULL");
  rprj::defaults(*p);
  return RP_OK;
}

int rp_reproject_device(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                        const rp_camera* prev, const double* d_depth_cur, const double* d_normal_cur,
                        const double* d_depth_prev, const double* d_normal_prev, const double* d_mean_prev,
                        const double* d_m2_prev, const uint32_t* d_count_prev, double* d_mean, double* d_m2,
                        uint32_t* d_count, uint64_t* d_stats, void* stream) {
  static_assert(RP_REPROJECT_STATS_LEN == rprj::STATS_LEN, "include/rp.h and rp_reproject.h disagree");
  rprj::RjArgs a;
  const int rc = reproject_args(params, width, height, cur, prev, d_depth_cur, d_normal_cur, d_depth_prev, d_normal_prev,
                                d_mean_prev, d_m2_prev, d_count_prev, d_mean, d_m2, d_count, d_stats, a);
  if (rc) return rc;
  hipLaunchKernelGGL(rprj::zero_stats_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a.stats);
  RP_HIP(hipGetLastError());
  const dim3 grid((width + rprj::RJ_BX - 1) / rprj::RJ_BX, (height + rprj::RJ_BY - 1) / rprj::RJ_BY);  // <= 1024 x 16384
  hipLaunchKernelGGL(rprj::reproject_kernel, grid, dim3(rprj::RJ_BX, rprj::RJ_BY), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

int rp_reproject(const rp_reproject_params* params, int device, uint32_t width, uint32_t height, const rp_camera* cur,
                 const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                 const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                 double* mean, double* m2, uint32_t* count, uint64_t* stats, double* seconds) {
  rprj::RjArgs unused;
  int rc = reproject_args(params, width, height, cur, prev, depth_cur, normal_cur, depth_prev, normal_prev, mean_prev,
                          m2_prev, count_prev, mean, m2, count, stats, unused);
  if (rc) return rc;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(RP_ENODEV, "no HIP device");
  if (device < 0 || device >= n_dev) return fail(RP_EINVAL, "device out of range");
  DeviceGuard g(device);
  const uint64_t n = (uint64_t)width * height;
  DevBuf<double> d_zc, d_nc, d_zp, d_np, d_mp, d_qp, d_m, d_q;
  DevBuf<uint32_t> d_cp, d_c;
  DevBuf<uint64_t> d_st;
  if (!d_zc.alloc(n) || !d_nc.alloc(3 * n) || !d_zp.alloc(n) || !d_np.alloc(3 * n) || !d_mp.alloc(3 * n) ||
      !d_qp.alloc(3 * n) || !d_m.alloc(3 * n) || !d_q.alloc(3 * n) || !d_cp.alloc(n) || !d_c.alloc(n) ||
      !d_st.alloc(rprj::STATS_LEN))
    return fail(RP_ENOMEM, "hipMalloc frame buffers");
  RP_HIP(hipMemcpy(d_zc.get(), depth_cur, 8 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_nc.get(), normal_cur, 24 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_zp.get(), depth_prev, 8 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_np.get(), normal_prev, 24 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_mp.get(), mean_prev, 24 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_qp.get(), m2_prev, 24 * n, hipMemcpyHostToDevice));
  RP_HIP(hipMemcpy(d_cp.get(), count_prev, 4 * n, hipMemcpyHostToDevice));
  double s = 0.0;
  rc = rpp::sync_call(device, "reproject", &s, [&](void* st) {
    return rp_reproject_device(params, width, height, cur, prev, d_zc.get(), d_nc.get(), d_zp.get(), d_np.get(),
                               d_mp.get(), d_qp.get(), d_cp.get(), d_m.get(), d_q.get(), d_c.get(), d_st.get(), st);
  });
  if (rc) return rc;
  RP_HIP(hipMemcpy(mean, d_m.get(), 24 * n, hipMemcpyDeviceToHost));
  RP_HIP(hipMemcpy(m2, d_q.get(), 24 * n, hipMemcpyDeviceToHost));
  RP_HIP(hipMemcpy(count, d_c.get(), 4 * n, hipMemcpyDeviceToHost));
  RP_HIP(hipMemcpy(stats, d_st.get(), 8 * rprj::STATS_LEN, hipMemcpyDeviceToHost));
  if (seconds) *seconds = s;
  return RP_OK;
}

}  // extern "C"
