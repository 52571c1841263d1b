// rp_accum.hip -- progressive accumulation (include/rp.h rp_accum_frames_device and rp_accum_error_device_ws,
// DESIGN.md 4.13): the frames of multi-frame launches folded into a running mean and the variance of that mean, and the
// count of pixels whose relative standard error is still above a tolerance.  No ray is traced.  The arithmetic is
// rp_accum.h's, shared with the CPU loops behind rph_accum_frames and rph_accum_error; this file is the kernels,
// their launches and the C-ABI.
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like rp_aov.hip, rp_denoise.hip and
// rp_variance.hip, not part of the rp_build_id hash: it runs after the render and decides no ray of it.
//
// accum_kernel: a streaming reduction over frames.  One lane owns two consecutive words and moves them with 16-byte
// loads and stores when every pointer is 16-byte aligned and the frame stride is even; otherwise, and for an odd last
// word, it walks its words one by one.  The loads of ACC_GROUP frames are issued before the Welford chain that consumes
// them in frame order; 1 / k is one division per frame, the same in every lane.  The grid is ceil(n_words / 2) lanes.
// accum_tiles_kernel (rp_accum_frames_tiles_device): the same per-lane body with a block indirection --
// the words of listed block k of every frame folded into state block tiles[k], an entry at or above the state's block
// count skipped; the wide path needs an even block size as well, so that every block starts on an even word.
// accum_counts_kernel (rp_accum_frames_counts_device): the fold with the frame number taken per pixel --
// a lane owns one pixel, reads its count c once, folds its words with k = c + 1 .., one division per frame, and writes
// c + n_frames back; three words per pixel (rgb) and one are unrolled, any other number walks word by word.
// error_kernel: a lane per shard slot, several slots per lane above 2048 blocks (rp_units.h slot_pixel's decode, as
// rp_variance.hip); the four statistics are
// reduced in the wave, then in the block through LDS, then one vector atomic per block and statistic -- integer sums and
// an integer maximum, so the result does not depend on the order of arrival.  zero_stats_kernel clears them first.
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers the shared headers use

#include "rp_accum.h"
#include "rp_units.h"

#pragma clang fp contract(off)

namespace rpa {

constexpr int ACC_BLOCK = 256;
constexpr int ACC_GROUP = 4;  // frames whose loads are in flight together: 4 x 16 B per lane
constexpr int ERR_BLOCK = 256;
constexpr int ERR_WAVES = ERR_BLOCK / 64;
constexpr uint64_t ERR_GRID_MAX = 2048;  // 256 CUs x 8 blocks: above it a block takes several slots per lane, so the
                                         // atomics on the four statistics words stay at 2048 per word

struct AccArgs {
  uint64_t n_words, stride;
  uint32_t n_prior, n_frames;
  uint32_t vec;  // every pointer 16-byte aligned and the stride even: a lane's two words move as one
  const double* frames;
  double* mean;
  double* m2;
  double* var;  // NULL: not wanted
};

template <int W>
struct Words {
  double v[W];
};
template <int W>
__device__ __forceinline__ Words<W> load(const double* p);
template <>
__device__ __forceinline__ Words<1> load<1>(const double* p) {
  return {{*p}};
}
template <>
__device__ __forceinline__ Words<2> load<2>(const double* p) {
  const double2 t = *reinterpret_cast<const double2*>(p);
  return {{t.x, t.y}};
}
__device__ __forceinline__ void store(double* p, const Words<1>& w) { *p = w.v[0]; }
__device__ __forceinline__ void store(double* p, const Words<2>& w) {
  *reinterpret_cast<double2*>(p) = make_double2(w.v[0], w.v[1]);
}

// Words ws .. ws + W - 1 of every frame of the call, in frame order, into the state words w .. w + W - 1 (the plain
// fold: ws = w; the tile fold: ws inside listed block k, w inside state block tiles[k]).
template <int W>
__device__ __forceinline__ void fold(const AccArgs& A, uint64_t ws, uint64_t w) {
  Words<W> mean, m2;
  if (A.n_prior) {
    mean = load<W>(A.mean + w);
    m2 = load<W>(A.m2 + w);
  } else {
#pragma unroll
    for (int c = 0; c < W; c++) mean.v[c] = 0.0, m2.v[c] = 0.0;
  }
  const double* src = A.frames + ws;
  uint32_t k = A.n_prior;  // frames folded in so far
  uint32_t f = 0;
  for (; f + ACC_GROUP <= A.n_frames; f += ACC_GROUP) {
    Words<W> x[ACC_GROUP];
#pragma unroll
    for (int u = 0; u < ACC_GROUP; u++) x[u] = load<W>(src + (uint64_t)(f + u) * A.stride);
#pragma unroll
    for (int u = 0; u < ACC_GROUP; u++) {
      const double r = frame_weight(++k);
#pragma unroll
      for (int c = 0; c < W; c++) welford(x[u].v[c], r, mean.v[c], m2.v[c]);
    }
  }
  for (; f < A.n_frames; f++) {
    const Words<W> x = load<W>(src + (uint64_t)f * A.stride);
    const double r = frame_weight(++k);
#pragma unroll
    for (int c = 0; c < W; c++) welford(x.v[c], r, mean.v[c], m2.v[c]);
  }
  store(A.mean + w, mean);
  store(A.m2 + w, m2);
  if (A.var) {
    const double nn = mean_divisor(k);
    Words<W> var;
#pragma unroll
    for (int c = 0; c < W; c++) var.v[c] = mean_variance(m2.v[c], nn);
    store(A.var + w, var);
  }
}

__global__ void __launch_bounds__(ACC_BLOCK) accum_kernel(const AccArgs A) {
  const uint64_t w = 2 * ((uint64_t)blockIdx.x * ACC_BLOCK + threadIdx.x);
  if (w >= A.n_words) return;
  if (A.vec && w + 1 < A.n_words) {
    fold<2>(A, w, w);
  } else {
    fold<1>(A, w, w);
    if (w + 1 < A.n_words) fold<1>(A, w + 1, w + 1);
  }
}

// The tile fold (rp_accum_frames_tiles_device): A.n_words is a block's words here.  A lane owns two consecutive words
// of one listed block; an entry at or above n_state would address words past the state and is skipped.
struct TileArgs {
  AccArgs A;
  const uint32_t* tiles;
  uint32_t n_listed, n_state;
  uint64_t lanes_per_tile;  // ceil(A.n_words / 2)
};

__global__ void __launch_bounds__(ACC_BLOCK) accum_tiles_kernel(const TileArgs T) {
  const uint64_t id = (uint64_t)blockIdx.x * ACC_BLOCK + threadIdx.x;
  const uint64_t k = id / T.lanes_per_tile;
  if (k >= T.n_listed) return;
  const uint32_t t = T.tiles[k];
  if (t >= T.n_state) return;
  const uint64_t w = 2 * (id - k * T.lanes_per_tile), tw = T.A.n_words;
  const uint64_t src = k * tw + w, dst = (uint64_t)t * tw + w;
  if (T.A.vec && w + 1 < tw) {  // (vec: tw is even, so src and dst are)
    fold<2>(T.A, src, dst);
  } else {
    fold<1>(T.A, src, dst);
    if (w + 1 < tw) fold<1>(T.A, src + 1, dst + 1);
  }
}

// The per-pixel fold (rp_accum_frames_counts_device).  A pixel's state is not read when its count is zero.
struct CountArgs {
  uint64_t n_pixels, stride;
  uint32_t wpp, n_frames;
  const double* frames;
  uint32_t* count;
  double* mean;
  double* m2;
  double* var;  // NULL: not wanted
  double var_one;
};

// Words w0 .. w0 + W - 1 of the lane's pixel: frames outermost, so 1 / k is made once per frame for the W words.
template <int W>
__device__ __forceinline__ void fold_counts(const CountArgs& A, uint64_t w0, uint32_t c) {
  double mean[W], m2[W];
#pragma unroll
  for (int i = 0; i < W; i++) mean[i] = c ? A.mean[w0 + i] : 0.0, m2[i] = c ? A.m2[w0 + i] : 0.0;
  uint32_t k = c;
  for (uint32_t f = 0; f < A.n_frames; f++) {
    const double* x = A.frames + (uint64_t)f * A.stride + w0;
    const double r = frame_weight(++k);
#pragma unroll
    for (int i = 0; i < W; i++) welford(x[i], r, mean[i], m2[i]);
  }
#pragma unroll
  for (int i = 0; i < W; i++) A.mean[w0 + i] = mean[i], A.m2[w0 + i] = m2[i];
  if (A.var) {
    const double nn = mean_divisor(k);
#pragma unroll
    for (int i = 0; i < W; i++) A.var[w0 + i] = k >= 2 ? mean_variance(m2[i], nn) : A.var_one;
  }
}

__global__ void __launch_bounds__(ACC_BLOCK) accum_counts_kernel(const CountArgs A) {
  const uint64_t p = (uint64_t)blockIdx.x * ACC_BLOCK + threadIdx.x;
  if (p >= A.n_pixels) return;
  const uint32_t c = A.count[p];
  const uint64_t w0 = p * A.wpp;
  if (A.wpp == 3) {
    fold_counts<3>(A, w0, c);
  } else {
    for (uint32_t i = 0; i < A.wpp; i++) fold_counts<1>(A, w0 + i, c);
  }
  A.count[p] = c + A.n_frames;
}

struct ErrArgs {
  rpp::ShardView v;
  const double* mean;        // 3 per slot
  const double* var;         // 3 per slot
  double tol2, eps;
  unsigned long long* stats;  // STATS_LEN
};

// The statistics start at zero: a kernel of its own ahead of error_kernel on the stream, not a memset -- a captured
// graph replays a kernel node with the arguments it was captured with.
__global__ void __launch_bounds__(64) zero_stats_kernel(unsigned long long* stats) {
  if (threadIdx.x < STATS_LEN) stats[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(ERR_BLOCK) error_kernel(const ErrArgs A) {
  __shared__ unsigned long long part[ERR_WAVES][STATS_LEN];
  unsigned long long n_counted = 0, n_over = 0, n_nonfinite = 0, bits = 0;
  // a block walks the slots in steps of the grid (the same trip count for all its lanes: the ballots and the barrier
  // below are reached by every lane); the counts are the wave's, the same in all its lanes
  for (uint64_t base = (uint64_t)blockIdx.x * ERR_BLOCK; base < A.v.n_slots; base += (uint64_t)gridDim.x * ERR_BLOCK) {
    const uint64_t slot = base + threadIdx.x;
    bool counted = false, over = false, nonfinite = false;
    uint32_t pi, pj;
    if (slot < A.v.n_slots && rpk::slot_pixel(A.v, slot, pi, pj)) {
      const double e2 = error2(A.mean + 3 * slot, A.var + 3 * slot, A.eps);
      counted = true;
      over = e2 > A.tol2;
      if (!finite(e2)) {
        nonfinite = true;
      } else if (e2 > 0.0) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(e2);
        bits = b > bits ? b : bits;
      }
    }
    n_counted += __popcll(__ballot(counted));
    n_over += __popcll(__ballot(over));
    n_nonfinite += __popcll(__ballot(nonfinite));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_down(bits, off);
    bits = other > bits ? other : bits;
  }
  const uint32_t wave = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) {
    part[wave][STAT_PIXELS] = n_counted;
    part[wave][STAT_OVER] = n_over;
    part[wave][STAT_MAX_BITS] = bits;
    part[wave][STAT_NONFINITE] = n_nonfinite;
  }
  __syncthreads();
  if (threadIdx.x < STATS_LEN) {
    const uint32_t s = threadIdx.x;
    unsigned long long v = part[0][s];
#pragma unroll
    for (int i = 1; i < ERR_WAVES; i++) {
      const unsigned long long o = part[i][s];
      v = s == STAT_MAX_BITS ? (o > v ? o : v) : v + o;
    }
    if (v) {
      if (s == STAT_MAX_BITS)
        atomicMax(A.stats + s, v);
      else
        atomicAdd(A.stats + s, v);
    }
  }
}

// The kernel's arguments of both folds, once rp_accum.h's check_fold has admitted the call; listed: the tile fold.
static void fold_args(bool listed, uint64_t block_words, uint32_t n_prior, uint32_t n_frames, const double* d_frames,
                      uint64_t frame_stride, double* d_mean, double* d_m2, double* d_var, AccArgs& a) {
  a.n_words = block_words, a.stride = frame_stride;
  a.n_prior = n_prior, a.n_frames = n_frames;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(d_frames) | reinterpret_cast<uintptr_t>(d_mean) |
                         reinterpret_cast<uintptr_t>(d_m2) | reinterpret_cast<uintptr_t>(d_var);
  // the wide path: every block starts on an even word of 16-byte aligned buffers, in the frames and in the state (the
  // plain fold's one block starts each frame: an even stride is enough)
  a.vec = bits % 16 == 0 && frame_stride % 2 == 0 && (!listed || block_words % 2 == 0);
  a.frames = d_frames, a.mean = d_mean, a.m2 = d_m2, a.var = d_var;
}

}  // namespace rpa

extern "C" {

int rp_accum_frames_device(uint64_t n_words, uint32_t n_prior, uint32_t n_frames, const double* d_frames,
                           uint64_t frame_stride, double* d_mean, double* d_m2, double* d_var, void* stream) {
  if (const char* why = rpa::check_fold(false, n_words, 1, 1, nullptr, n_prior, n_frames, d_frames, frame_stride, d_mean,
                                        d_m2, d_var))
    return fail(RP_EINVAL, why);
  const uint64_t lanes = (n_words + 1) / 2, grid = (lanes + rpa::ACC_BLOCK - 1) / rpa::ACC_BLOCK;
  if (grid > 0x7fffffffu) return fail(RP_EINVAL, "more than 2^31 - 1 blocks");
  rpa::AccArgs a;
  rpa::fold_args(false, n_words, n_prior, n_frames, d_frames, frame_stride, d_mean, d_m2, d_var, a);
  hipLaunchKernelGGL(rpa::accum_kernel, dim3((unsigned)grid), dim3(rpa::ACC_BLOCK), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

int rp_accum_frames_tiles_device(uint64_t tile_words, uint32_t n_state_tiles, const uint32_t* d_tiles, uint32_t n_listed,
                                 uint32_t n_prior, uint32_t n_frames, const double* d_frames, uint64_t frame_stride,
                                 double* d_mean, double* d_m2, double* d_var, void* stream) {
  if (const char* why = rpa::check_fold(true, tile_words, n_listed, n_state_tiles, d_tiles, n_prior, n_frames, d_frames,
                                        frame_stride, d_mean, d_m2, d_var))
    return fail(RP_EINVAL, why);
  if (n_listed == 0) return RP_OK;  // nothing listed: nothing folded, nothing launched
  rpa::TileArgs t;
  rpa::fold_args(true, tile_words, n_prior, n_frames, d_frames, frame_stride, d_mean, d_m2, d_var, t.A);
  t.tiles = d_tiles, t.n_listed = n_listed, t.n_state = n_state_tiles;
  t.lanes_per_tile = (tile_words + 1) / 2;
  const uint64_t lanes = t.lanes_per_tile * n_listed, grid = (lanes + rpa::ACC_BLOCK - 1) / rpa::ACC_BLOCK;
  if (grid > 0x7fffffffu) return fail(RP_EINVAL, "more than 2^31 - 1 blocks");
  hipLaunchKernelGGL(rpa::accum_tiles_kernel, dim3((unsigned)grid), dim3(rpa::ACC_BLOCK), 0, (hipStream_t)stream, t);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

int rp_accum_frames_counts_device(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* d_frames,
                                  uint64_t frame_stride, uint32_t* d_count, double* d_mean, double* d_m2, double* d_var,
                                  double var_one, void* stream) {
  if (const char* why = rpa::check_fold_counts(n_pixels, words_per_pixel, n_frames, d_frames, frame_stride, d_count, d_mean,
                                               d_m2, d_var, var_one))
    return fail(RP_EINVAL, why);
  const uint64_t grid = (n_pixels + rpa::ACC_BLOCK - 1) / rpa::ACC_BLOCK;  // < 2^32: n_pixels is below 2^40
  if (grid > 0x7fffffffu) return fail(RP_EINVAL, "more than 2^31 - 1 blocks");
  rpa::CountArgs a;
  a.n_pixels = n_pixels, a.stride = frame_stride;
  a.wpp = words_per_pixel, a.n_frames = n_frames;
  a.frames = d_frames, a.count = d_count, a.mean = d_mean, a.m2 = d_m2, a.var = d_var;
  a.var_one = var_one;
  hipLaunchKernelGGL(rpa::accum_counts_kernel, dim3((unsigned)grid), dim3(rpa::ACC_BLOCK), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

int rp_accum_error_device_ws(rp_scene* s, rp_workspace* w, const rp_render_params* p, const rp_error_params* e,
                             const double* d_shard_mean, const double* d_shard_var, uint64_t* d_stats, void* stream) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!d_shard_mean || !d_shard_var || !d_stats)
    return fail(RP_EINVAL, "d_shard_mean, d_shard_var and d_stats must be non-NULL");
  double tol, eps;
  if (!rpa::resolve(e, tol, eps))
    return fail(RP_EINVAL, "error params out of range (tol > 0; eps > 0 and finite)");
  Tiling t;
  rpa::ErrArgs a;
  if ((rc = rpp::shard_view(w, p, t, a.v))) return rc;
  DeviceGuard g(s->device);
  static_assert(RP_ERROR_STATS_LEN == rpa::STATS_LEN, "include/rp.h and rp_accum.h disagree");
  hipLaunchKernelGGL(rpa::zero_stats_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<unsigned long long*>(d_stats));
  RP_HIP(hipGetLastError());
  if (t.n_slots == 0) return RP_OK;
  a.mean = d_shard_mean, a.var = d_shard_var;
  a.tol2 = tol * tol, a.eps = eps;
  a.stats = reinterpret_cast<unsigned long long*>(d_stats);
  const uint64_t blocks = (t.n_slots + rpa::ERR_BLOCK - 1) / rpa::ERR_BLOCK;
  const uint64_t grid = blocks < rpa::ERR_GRID_MAX ? blocks : rpa::ERR_GRID_MAX;
  hipLaunchKernelGGL(rpa::error_kernel, dim3((unsigned)grid), dim3(rpa::ERR_BLOCK), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

}  // extern "C"
