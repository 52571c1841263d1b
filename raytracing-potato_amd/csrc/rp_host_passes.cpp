// rp_host_passes.cpp -- librp_host.so (include/rp_host.h): the CPU loops of the passes around the render kernel --
// denoise, batch variance, accumulation, tile selection, reprojection -- over the arithmetic headers the kernels compile
// (rp_denoise.h, rp_variance.h, rp_accum.h, rp_reproject.h).  What an entry point refuses is those headers' checks, the
// same text as the device's behind an `rph_<name>: ` prefix.
#include <cstring>
#include <string>
#include <vector>

#include "rp_accum.h"
#include "rp_denoise.h"
#include "rp_host_util.h"
#include "rp_reproject.h"
#include "rp_schedule.h"
#include "rp_variance.h"

using rph::fail;

// The denoiser's levels as a plain loop over rp_denoise.h (what rp_denoise.hip's kernel does per lane): demodulate once,
// every level from one colour buffer into the other, remodulate (or copy a pass-through pixel's rgb) at the end.
// VAR (rph_denoise_var, P an rp_denoise_var_params): the variance v travels with the colour.
template <bool VAR, class Params>
static void denoise_loop(const Params& P, uint32_t iterations, double eps, uint32_t width, uint32_t height,
                         const double* rgb, const double* var, const double* normal, const double* albedo,
                         const double* depth, double* out) {
  const uint64_t n = (uint64_t)width * height;
  std::vector<double> cur(3 * n), nxt(3 * n), vcur(VAR ? n : 0), vnxt(VAR ? n : 0);
  auto pixel = [&](const std::vector<double>& c, const std::vector<double>& v, uint64_t i) {
    rpdn::Px p = {};
    p.cx = c[3 * i], p.cy = c[3 * i + 1], p.cz = c[3 * i + 2];
    if (normal) {
      p.nx = normal[3 * i], p.ny = normal[3 * i + 1], p.nz = normal[3 * i + 2];
      p.nn = rpdn::len2(p.nx, p.ny, p.nz);
    }
    if (albedo) p.ax = albedo[3 * i], p.ay = albedo[3 * i + 1], p.az = albedo[3 * i + 2];
    if (depth) p.z = depth[i];
    if (VAR) p.v = v[i];
    return p;
  };
  for (uint64_t i = 0; i < 3 * n; i++) cur[i] = albedo ? rpdn::demod(rgb[i], albedo[i], eps) : rgb[i];
  if (VAR)
    for (uint64_t i = 0; i < n; i++) {
      double v[3];
      for (int k = 0; k < 3; k++) v[k] = albedo ? rpdn::demod_var(var[3 * i + k], albedo[3 * i + k], eps) : var[3 * i + k];
      vcur[i] = rpdn::sum3(v[0], v[1], v[2]);
    }
  rpdn::Level L{};
  for (uint32_t l = 0; l < iterations; l++) {
    L = rpdn::make_level(P, l, normal != nullptr, albedo != nullptr, depth != nullptr);
    const int64_t s = L.step;
    for (uint32_t j = 0; j < height; j++)
      for (uint32_t i = 0; i < width; i++) {
        const uint64_t at = (uint64_t)j * width + i;
        double ov = 0.0;
        rpdn::level_step_v<VAR>(
            L, pixel(cur, vcur, at),
            [&](int dx, int dy, rpdn::Px& q) {
              const int64_t qi = (int64_t)i + s * dx, qj = (int64_t)j + s * dy;
              if (qi < 0 || qi >= (int64_t)width || qj < 0 || qj >= (int64_t)height) return false;
              q = pixel(cur, vcur, (uint64_t)qj * width + (uint64_t)qi);
              return true;
            },
            nxt[3 * at], nxt[3 * at + 1], nxt[3 * at + 2], ov);
        if (VAR) vnxt[at] = ov;
      }
    cur.swap(nxt);
    vcur.swap(vnxt);
  }
  for (uint64_t at = 0; at < n; at++) {
    const rpdn::Px p = pixel(cur, vcur, at);
    for (int k = 0; k < 3; k++) {
      const uint64_t i = 3 * at + k;
      out[i] = rpdn::passes(L, p) ? rgb[i] : (albedo ? rpdn::remod(cur[i], albedo[i], eps) : cur[i]);
    }
  }
}

// rp_accum.h's Welford update per word of every listed block, frame after frame: listed block k of every frame into
// state block tiles[k] (tiles NULL: block k), an entry at or above n_state skipped -- what rp_accum.hip's accum_kernel
// (one block, no list) and accum_tiles_kernel do per lane.
static void fold_blocks(uint64_t block_words, uint32_t n_in, uint32_t n_state, const uint32_t* tiles, uint32_t n_prior,
                        uint32_t n_frames, const double* frames, uint64_t frame_stride, double* mean, double* m2,
                        double* var) {
  const double nn = var ? rpa::mean_divisor(n_prior + n_frames) : 0.0;
  for (uint32_t k = 0; k < n_in; k++) {
    const uint32_t t = tiles ? tiles[k] : k;
    if (t >= n_state) continue;
    double* mk = mean + (uint64_t)t * block_words;
    double* qk = m2 + (uint64_t)t * block_words;
    if (!n_prior)
      for (uint64_t w = 0; w < block_words; w++) mk[w] = 0.0, qk[w] = 0.0;
    for (uint32_t f = 0; f < n_frames; f++) {
      const double r = rpa::frame_weight(n_prior + f + 1);
      const double* x = frames + (uint64_t)f * frame_stride + (uint64_t)k * block_words;
      for (uint64_t w = 0; w < block_words; w++) rpa::welford(x[w], r, mk[w], qk[w]);
    }
    if (var) {
      double* vk = var + (uint64_t)t * block_words;
      for (uint64_t w = 0; w < block_words; w++) vk[w] = rpa::mean_variance(qk[w], nn);
    }
  }
}

extern "C" {

int rph_denoise(const rp_denoise_params* params, uint32_t width, uint32_t height, const double* rgb, const double* normal,
                const double* albedo, const double* depth, double* out) {
  if (const char* why = rpdn::check_frames(width, height, rgb, nullptr, normal, albedo, depth, out))
    return fail(std::string("rph_denoise: ") + why);
  rp_denoise_params P;
  if (!rpdn::resolve(params, P))
    return fail("rph_denoise: params out of range (iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo and "
                "albedo_eps > 0 and finite, sigma_color finite)");
  denoise_loop<false>(P, P.iterations, P.albedo_eps, width, height, rgb, nullptr, normal, albedo, depth, out);
  return RP_OK;
}

int rph_denoise_var(const rp_denoise_var_params* params, uint32_t width, uint32_t height, const double* rgb,
                    const double* var, const double* normal, const double* albedo, const double* depth, double* out) {
  if (const char* why = rpdn::check_frames(width, height, rgb, var, normal, albedo, depth, out))
    return fail(std::string("rph_denoise_var: ") + why);
  if (!var) return fail("rph_denoise_var: var must be non-NULL");
  rp_denoise_var_params P;
  if (!rpdn::resolve(params, P))
    return fail("rph_denoise_var: params out of range (iterations 1..8, normal_power 1..8, sigma_depth, sigma_albedo, "
                "albedo_eps, sigma_var and var_eps > 0 and finite)");
  denoise_loop<true>(P, P.base.iterations, P.base.albedo_eps, width, height, rgb, var, normal, albedo, depth, out);
  return RP_OK;
}

// rp_variance.h's batch_variance per pixel and channel: what rp_variance.hip's kernel does per lane.
int rph_batch_variance(uint32_t spp, uint32_t samples_per_stream, uint64_t n_pixels, const double* sums, double* var) {
  if (!sums || !var) return fail("rph_batch_variance: sums and var must be non-NULL");
  const uint32_t sps = samples_per_stream ? samples_per_stream : RP_SAMPLES_PER_STREAM;
  const uint32_t B = rpv::batches(spp, sps);
  if (B < 2) return fail("rph_batch_variance: needs at least two sample batches per pixel (spp > samples_per_stream)");
  for (uint64_t i = 0; i < n_pixels; i++)
    for (uint32_t c = 0; c < 3; c++) var[3 * i + c] = rpv::batch_variance(sums + 3 * i * B + c, 3, B, spp, sps);
  return RP_OK;
}

int rph_accum_frames(uint64_t n_words, uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride,
                     double* mean, double* m2, double* var) {
  if (const char* why = rpa::check_fold(false, n_words, 1, 1, nullptr, n_prior, n_frames, frames, frame_stride, mean, m2, var))
    return fail(std::string("rph_accum_frames: ") + why);
  fold_blocks(n_words, 1, 1, nullptr, n_prior, n_frames, frames, frame_stride, mean, m2, var);
  return RP_OK;
}

// rp_accum.h's error2 per pixel and the four order-free statistics: what rp_accum.hip's error_kernel reduces.
int rph_accum_error(const rp_error_params* params, uint64_t n_pixels, const double* mean, const double* var,
                    uint64_t* stats) {
  if (!mean || !var || !stats) return fail("rph_accum_error: mean, var and stats must be non-NULL");
  double tol, eps;
  if (!rpa::resolve(params, tol, eps))
    return fail("rph_accum_error: error params out of range (tol > 0; eps > 0 and finite)");
  const double tol2 = tol * tol;
  for (int k = 0; k < rpa::STATS_LEN; k++) stats[k] = 0;
  for (uint64_t i = 0; i < n_pixels; i++) {
    const double e2 = rpa::error2(mean + 3 * i, var + 3 * i, eps);
    stats[rpa::STAT_PIXELS]++;
    if (e2 > tol2) stats[rpa::STAT_OVER]++;
    if (!rpa::finite(e2)) {
      stats[rpa::STAT_NONFINITE]++;
    } else if (e2 > 0.0) {
      uint64_t bits;
      std::memcpy(&bits, &e2, sizeof bits);
      if (bits > stats[rpa::STAT_MAX_BITS]) stats[rpa::STAT_MAX_BITS] = bits;
    }
  }
  return RP_OK;
}

// rp_accum_frames_tiles_device on host buffers.
int rph_accum_frames_tiles(uint64_t tile_words, uint32_t n_state_tiles, const uint32_t* tiles, uint32_t n_listed,
                           uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride, double* mean,
                           double* m2, double* var) {
  if (const char* why = rpa::check_fold(true, tile_words, n_listed, n_state_tiles, tiles, n_prior, n_frames, frames,
                                        frame_stride, mean, m2, var))
    return fail(std::string("rph_accum_frames_tiles: ") + why);
  fold_blocks(tile_words, n_listed, n_state_tiles, tiles, n_prior, n_frames, frames, frame_stride, mean, m2, var);
  return RP_OK;
}

// rp_accum_tiles_select_device on host buffers: rp_accum.h's pixel_over per in-frame pixel of every listed tile, the
// tile's count, tile_active, and the active tiles in list order (what rp_tiles.hip's two kernels do).
int rph_accum_tiles_select(const rp_render_params* params, const rp_error_params* error, double tile_share,
                           const double* mean, const double* var, const uint32_t* tiles_in, uint32_t n_in, uint32_t* over,
                           uint32_t* tiles_out, uint32_t* count) {
  if (!mean || !var || !tiles_out || !count)
    return fail("rph_accum_tiles_select: mean, var, tiles_out and count must be non-NULL");
  rps::Tiling t;
  const rps::Refusal r = rps::make_tiling(params, t);
  if (r.code) return fail(std::string("rph_accum_tiles_select: ") + r.msg);
  double tol, eps;
  if (const char* why = rpa::check_select(t.shards, params->shard_map, error, tile_share, n_in, tol, eps))
    return fail(std::string("rph_accum_tiles_select: ") + why);
  const double tol2 = tol * tol;
  const uint32_t W = params->width, H = params->height, tile_px = t.tw * t.th;
  uint32_t n_out = 0;
  for (uint32_t k = 0; k < n_in; k++) {
    const uint32_t tile = tiles_in ? tiles_in[k] : k;
    uint32_t n_over = 0;
    const bool in_frame = tile < t.n_tiles;
    if (in_frame) {
      const uint32_t ox = (tile % t.tiles_x) * t.tw, oy = (tile / t.tiles_x) * t.th;
      for (uint32_t lj = 0; lj < t.th && oy + lj < H; lj++)
        for (uint32_t li = 0; li < t.tw && ox + li < W; li++) {
          const uint64_t slot = (uint64_t)tile * tile_px + (uint64_t)lj * t.tw + li;
          n_over += rpa::pixel_over(mean + 3 * slot, var + 3 * slot, eps, tol2);
        }
    }
    if (over) over[k] = n_over;
    // (tiles_out may be tiles_in here: position n_out is never beyond entry k, which has been read)
    if (in_frame && rpa::tile_active(n_over, rpa::tile_pixels(tile, W, H, t.tw, t.th, t.tiles_x), tile_share))
      tiles_out[n_out++] = tile;
  }
  count[0] = n_out;
  return RP_OK;
}

// rp_reproject.h's reproject_pixel per pixel and the four order-free statistics: what rp_reproject.hip's kernel does
// per lane and reduces.
int rph_reproject(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                  const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                  const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                  double* mean, double* m2, uint32_t* count, uint64_t* stats) {
  if (!cur || !prev) return fail("rph_reproject: cur and prev must be non-NULL");
  if (const char* why = rprj::check_buffers(width, height, depth_cur, normal_cur, depth_prev, normal_prev, mean_prev,
                                            m2_prev, count_prev, mean, m2, count, stats))
    return fail(std::string("rph_reproject: ") + why);
  rprj::Frame F;
  if (!rprj::resolve(params, F.P))
    return fail("rph_reproject: params out of range (sigma_depth > 0 and finite, normal_cos in (0, 1], max_history "
                "1 .. 2^31 - 1)");
  if (!rprj::make_camera(*cur, F.cur) || !rprj::make_camera(*prev, F.prev))
    return fail("rph_reproject: a camera field is not finite, or tan(fov / 2) is not > 0");
  F.W = width, F.H = height;
  F.depth_prev = depth_prev, F.normal_prev = normal_prev;
  F.mean_prev = mean_prev, F.m2_prev = m2_prev, F.count_prev = count_prev;
  for (int k = 0; k < rprj::STATS_LEN; k++) stats[k] = 0;
  for (uint32_t j = 0; j < height; j++)
    for (uint32_t i = 0; i < width; i++) {
      const uint64_t px = (uint64_t)j * width + i;
      const rprj::Result r = rprj::reproject_pixel(F, i, j, depth_cur[px], normal_cur[3 * px], normal_cur[3 * px + 1],
                                                   normal_cur[3 * px + 2]);
      for (int ch = 0; ch < 3; ch++) mean[3 * px + ch] = r.mean[ch], m2[3 * px + ch] = r.m2[ch];
      count[px] = r.count;
      stats[rprj::STAT_PIXELS]++;
      stats[rprj::STAT_KEPT] += r.count >= 1;
      stats[rprj::STAT_COUNT] += r.count;
      stats[rprj::STAT_OFF] += r.off;
    }
  return RP_OK;
}

// rp_accum.h's Welford update with the frame number taken per pixel: what rp_accum.hip's accum_counts_kernel does per
// lane.
int rph_accum_frames_counts(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* frames,
                            uint64_t frame_stride, uint32_t* count, double* mean, double* m2, double* var, double var_one) {
  if (const char* why = rpa::check_fold_counts(n_pixels, words_per_pixel, n_frames, frames, frame_stride, count, mean, m2,
                                               var, var_one))
    return fail(std::string("rph_accum_frames_counts: ") + why);
  for (uint64_t p = 0; p < n_pixels; p++) {
    const uint32_t c = count[p], n = c + n_frames;
    double* mp = mean + p * words_per_pixel;
    double* qp = m2 + p * words_per_pixel;
    if (!c)
      for (uint32_t w = 0; w < words_per_pixel; w++) mp[w] = 0.0, qp[w] = 0.0;
    for (uint32_t f = 0; f < n_frames; f++) {
      const double r = rpa::frame_weight(c + f + 1);
      const double* x = frames + (uint64_t)f * frame_stride + p * words_per_pixel;
      for (uint32_t w = 0; w < words_per_pixel; w++) rpa::welford(x[w], r, mp[w], qp[w]);
    }
    if (var) {
      const double nn = rpa::mean_divisor(n);
      for (uint32_t w = 0; w < words_per_pixel; w++)
        var[p * words_per_pixel + w] = n >= 2 ? rpa::mean_variance(qp[w], nn) : var_one;
    }
    count[p] = n;
  }
  return RP_OK;
}

}  // extern "C"
