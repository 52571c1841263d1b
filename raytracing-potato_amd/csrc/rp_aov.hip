// rp_aov.hip -- the first-hit feature pass (include/rp.h rp_render_aov*): the noiseless guide buffers a denoiser or
// compositor takes beside the beauty frame -- normal, albedo and depth of the camera rays' first hits, and the
// foreground fraction.  render.rs:101 plans for them ("the first ray of the path tracing provides additional noiseless
// data like albedo and normal", PathTraceOutput::normal, render.rs:87-91, zero on a miss at :119).
//
// A pass of its own, beside the render kernel and not in it: the megakernel sits at its register budget for 4 waves per
// SIMD (seven more f64 sums per lane would cost the headline), and its machine code is what rp_build_id hashes.  This
// translation unit is linked into librp.so but is not part of that hash.
//
// Kernel: one lane per shard slot (the render's compact shard order), the lane loops over the pixel's spp camera
// samples, so every buffer's sum is added in sample order by construction.  Sample k of pixel (i, j) is sample 0 of
// the stream seed_from_u64(seed + k W H + j W + i) -- the RNG contract at samples_per_stream = 1 -- so there is no
// queue, no persistent loop and no keystream slab: a sample derives its key, makes keystream block 0 (the jitter and
// the first four UnitDisk tries) and further blocks only if all four tries are rejected.  Then camera_dir, one
// traverse<NF> on an LDS stack sized as the closest-hit query's (launch_intersect), and the hit's surface record.
//
// Arithmetic is IEEE binary64 in the reference's operation order (-ffp-contract=off and the pragma below), as in
// rp_kernel.hip: the camera rays are the render's bit for bit.
#include <cmath>
#include <vector>

#include "rp_device.h"
#include "rp_pass.h"

#pragma clang fp contract(off)

namespace rpk {

// The kernarg segment begins with a KArgs, so the kargs() readers (rp_device.h camera_dir and load_scene, rp_units.h
// unit_seed) find their fields where the render kernel keeps them; the pass's own outputs follow (each nullable).
struct AovArgs {
  KArgs k;
  double* normal;  // 3 per slot
  double* albedo;  // 3 per slot
  double* depth;   // 1 per slot
  float* fg;       // 1 per slot
};

template <uint32_t NF>
__global__ void __launch_bounds__(BLOCK) aov_kernel(const AovArgs args) {
  extern __shared__ uint32_t lds_stack[];
  KArgsPtr A = kargs();
  const uint64_t slot64 = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (slot64 >= A->P.n_slots) return;
  // slot -> shard tile -> frame tile -> pixel; slots of edge tiles outside the frame are not written
  const uint32_t slot = (uint32_t)slot64;
  uint32_t pi, pj;
  if (!slot_pixel(A->P, slot, pi, pj)) return;
  const uint32_t spp = A->P.spp;
  unsigned long long* ctr = A->ctr;
  if (ctr) {  // rays = samples = spp x pixels: one atomic per wave and counter
    const uint64_t live = __ballot(true);
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(live)) {
      const unsigned long long n = (unsigned long long)__popcll(live);
      atomicAdd(&ctr[CTR_RAYS], n * spp);
      atomicAdd(&ctr[CTR_SAMPLES], n * spp);
      atomicAdd(&ctr[CTR_PIXELS], n);
    }
  }
  const KScene S = load_scene(A);
  lds_u32* stk = (lds_u32*)(lds_stack + threadIdx.x);
  // wave-uniform: no albedo buffer, no texture work; neither albedo nor normal, no surface record
  const bool want_alb = args.albedo != nullptr, want_surf = want_alb || args.normal != nullptr;
  double nx = 0.0, ny = 0.0, nz = 0.0, ax = 0.0, ay = 0.0, az = 0.0, dep = 0.0;
  uint32_t hits = 0;
  bool overflow = false;
  for (uint32_t s = 0; s < spp; s++) {
    // the sample's own stream (RNG contract, batch s at one sample per stream)
    uint32_t key[8], w[16];
    seed_key(unit_seed(A, pi, pj, s), key);
    chacha12(key, 0u, w);
    // make_uv_jitter: the first two draws of a clone of the stream (render.rs:74-82)
    const double ju = ((double)pi + rpd::words_unit(w[0], w[1])) / (double)A->P.W;
    const double jv = ((double)pj + rpd::words_unit(w[2], w[3])) / (double)A->P.H;
    // Camera::shoot's UnitDisk from the stream's start (randomness.rs:21-34; drawn even at lens_radius == 0, where it
    // is multiplied by zero): try j is stream words 4 j .. 4 j + 3, the first accepted one wins -- four tries per
    // keystream block, further blocks on demand
    double dx = 0.0, dy = 0.0;
    for (uint32_t b = 0;;) {
      bool done = false;
#pragma unroll
      for (int j = 3; j >= 0; j--) {  // descending: the first accepted try wins (rp_draw.h draw_pick)
        const double x = rpd::words_sym(w[4 * j], w[4 * j + 1]), y = rpd::words_sym(w[4 * j + 2], w[4 * j + 3]);
        if (x * x + y * y < 1.0) {
          dx = x;
          dy = y;
          done = true;
        }
      }
      if (done) break;
      chacha12(key, ++b, w);
    }
    V3 o, d;
    camera_dir(A, ju, jv, dx, dy, o, d);
    HitRec hr;
    // root.hit(ray), t_min 1e-3, t_max +inf (the always-tested records per lane: rp_device.h trav_begin)
    traverse<NF, false>(S, stk, BLOCK, o, d, RAY_EPSILON, INF, hr, overflow);
    if (hr.prim >= 0) {  // a miss adds zero to every sum (render.rs:119)
      hits++;
      dep = dep + hr.t;
      if (want_surf) {
        Surf h;
        const bool sph_uv = surface(S, hr, o, d, h);
        nx = nx + h.n.x;
        ny = ny + h.n.y;
        nz = nz + h.n.z;
        if (want_alb) {
          // material.absorb.evaluate(ray, hit) (material.rs:74-81), whether or not the material scatters
          if (sph_uv) {  // hittable.rs:59-62: the sphere's uv, where a texture of the material reads it
            h.u = 0.5 - atan2(h.n.z, h.n.x) / TAU_;
            h.v = asin(h.n.y) / PI_ + 0.5;
          }
          const rpl::Material& m = S.mats[h.material];
          V3 tex = v3(0.0, 0.0, 0.0);
          if (m.absorb_kind == 3) tex = tex_sample(S, m.absorb_tex, h);
          const V3 ab = absorb_eval(m, tex);
          ax = ax + ab.x;
          ay = ay + ab.y;
          az = az + ab.z;
        }
      }
    }
  }
  const double n = (double)spp;
  if (args.normal) {
    args.normal[3 * (uint64_t)slot + 0] = nx / n;
    args.normal[3 * (uint64_t)slot + 1] = ny / n;
    args.normal[3 * (uint64_t)slot + 2] = nz / n;
  }
  if (args.albedo) {
    args.albedo[3 * (uint64_t)slot + 0] = ax / n;
    args.albedo[3 * (uint64_t)slot + 1] = ay / n;
    args.albedo[3 * (uint64_t)slot + 2] = az / n;
  }
  if (args.depth) args.depth[slot] = dep / n;
  if (args.fg) args.fg[slot] = (float)((double)hits / n);
  if (ctr && overflow) atomicOr(&ctr[CTR_STATUS], (unsigned long long)STATUS_STACK_OVERFLOW);
}

// One block per 64 shard slots, the whole traversal stack in LDS (launch_intersect's size and bound).
static int launch_aov(const KScene& s, const KParams& p, double* normal, double* albedo, double* depth, float* fg,
                      uint64_t* counters, void* stream) {
  if (p.n_slots == 0) return 0;
  AovArgs a;
  a.k.S = s;
  a.k.P = p;
  a.k.out = nullptr;
  a.k.out_fg = nullptr;
  a.k.ctr = reinterpret_cast<unsigned long long*>(counters);
  a.k.queue = nullptr;
  a.k.diag = reinterpret_cast<unsigned long long*>(s.diag);
  a.normal = normal;
  a.albedo = albedo;
  a.depth = depth;
  a.fg = fg;
  const size_t lds = (size_t)s.stack_depth * BLOCK * sizeof(uint32_t);
  const uint64_t grid = (p.n_slots + BLOCK - 1) / BLOCK;
  const hipStream_t st = (hipStream_t)stream;
  if (s.node_format == rpl::NODES_W8)
    hipLaunchKernelGGL(aov_kernel<rpl::NODES_W8>, dim3((unsigned)grid), dim3(BLOCK), lds, st, a);
  else if (s.node_format == rpl::NODES_Q8)
    hipLaunchKernelGGL(aov_kernel<rpl::NODES_Q8>, dim3((unsigned)grid), dim3(BLOCK), lds, st, a);
  else
    hipLaunchKernelGGL(aov_kernel<rpl::NODES_F32>, dim3((unsigned)grid), dim3(BLOCK), lds, st, a);
  return (int)hipGetLastError();
}

}  // namespace rpk

extern "C" {

int rp_render_aov_device_ws(rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p,
                            double* d_normal, double* d_albedo, double* d_depth, float* d_fg, uint64_t* d_counters,
                            void* stream) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!cam) return fail(RP_EINVAL, "camera is NULL");
  if (!d_normal && !d_albedo && !d_depth && !d_fg) return fail(RP_EINVAL, "every output is NULL");
  Tiling t;
  rpk::KParams kp{};
  if ((rc = rpp::shard_view(w, p, t, kp))) return rc;
  DeviceGuard g(s->device);
  const hipStream_t st = (hipStream_t)stream;
  if (d_counters) RP_HIP(hipMemsetAsync(d_counters, 0, sizeof(uint64_t) * rpk::CTR_N, st));
  if (t.n_slots == 0) return RP_OK;
  if (p->spp == 0) {
    // every sum / 0.0 is NaN, as rp_render's frame of no samples (main.rs:86-87); all-ones bits are a NaN
    if (d_normal) RP_HIP(hipMemsetAsync(d_normal, 0xff, sizeof(double) * 3 * t.n_slots, st));
    if (d_albedo) RP_HIP(hipMemsetAsync(d_albedo, 0xff, sizeof(double) * 3 * t.n_slots, st));
    if (d_depth) RP_HIP(hipMemsetAsync(d_depth, 0xff, sizeof(double) * t.n_slots, st));
    if (d_fg) RP_HIP(hipMemsetAsync(d_fg, 0xff, sizeof(float) * t.n_slots, st));
    return RP_OK;
  }
  rpp::set_camera(kp, cam);
  kp.seed = p->seed, kp.spp = p->spp, kp.n_shard_tiles = t.n_shard_tiles;
  RP_LAUNCH("feature pass", rpk::launch_aov(s->ks, kp, d_normal, d_albedo, d_depth, d_fg, d_counters, stream));
  return RP_OK;
}

int rp_render_aov(rp_scene* s, const rp_camera* cam, const rp_render_params* p, double* out_normal, double* out_albedo,
                  double* out_depth, float* out_fg, rp_stats* stats) {
  if (!s || !cam) return fail(RP_EINVAL, "scene and camera must be non-NULL");
  if (!out_normal && !out_albedo && !out_depth && !out_fg) return fail(RP_EINVAL, "every output is NULL");
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  DeviceGuard g(s->device);
  const uint64_t n = t.n_slots ? t.n_slots : 1;
  std::vector<double> normal(out_normal ? 3 * n : 0), albedo(out_albedo ? 3 * n : 0), depth(out_depth ? n : 0);
  std::vector<float> fg(out_fg ? n : 0);
  uint64_t ctr[rpk::CTR_N] = {0};
  double seconds = 0.0;
  DevBuf<double> d_normal, d_albedo, d_depth;
  DevBuf<float> d_fg;
  DevBuf<uint64_t> d_ctr;
  if ((out_normal && !d_normal.alloc(3 * n)) || (out_albedo && !d_albedo.alloc(3 * n)) ||
      (out_depth && !d_depth.alloc(n)) || (out_fg && !d_fg.alloc(n)) || !d_ctr.alloc(rpk::CTR_N))
    return fail(RP_ENOMEM, "hipMalloc output");
  if ((rc = rpp::sync_call(s->device, "feature pass", &seconds, [&](void* st) {
         return rp_render_aov_device_ws(s, nullptr, cam, p, d_normal.get(), d_albedo.get(), d_depth.get(), d_fg.get(),
                                        d_ctr.get(), st);
       })))
    return rc;
  if ((out_normal && hipMemcpy(normal.data(), d_normal.get(), sizeof(double) * 3 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (out_albedo && hipMemcpy(albedo.data(), d_albedo.get(), sizeof(double) * 3 * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (out_depth && hipMemcpy(depth.data(), d_depth.get(), sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      (out_fg && hipMemcpy(fg.data(), d_fg.get(), sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
      hipMemcpy(ctr, d_ctr.get(), sizeof ctr, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RP_EHIP, "copy back");
  if ((rc = rpp::check_status(ctr, "feature pass"))) return rc;
  if (t.n_slots) {
    std::vector<uint32_t> map;
    if (t.balanced) {
      map.resize(t.n_tiles);
      if ((rc = rp_workspace_tile_map(s, nullptr, p, map.data(), t.n_tiles))) return rc;
    }
    const uint32_t* m = t.balanced ? map.data() : nullptr;
    if (out_normal) rpp::unpack_host(p, t, m, normal.data(), sizeof(double), 3, out_normal);
    if (out_albedo) rpp::unpack_host(p, t, m, albedo.data(), sizeof(double), 3, out_albedo);
    if (out_depth) rpp::unpack_host(p, t, m, depth.data(), sizeof(double), 1, out_depth);
    if (out_fg) rpp::unpack_host(p, t, m, fg.data(), sizeof(float), 1, out_fg);
  }
  rpp::fill_stats(ctr, seconds, stats);
  return RP_OK;
}

}  // extern "C"
