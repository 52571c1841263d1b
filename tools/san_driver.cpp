// san_driver.cpp -- native driver of the host code for the sanitizer builds ("Host ASan/UBSan build of the
// C++ oracle").  Built by `make -C raytracing-potato_amd sanitize` with -fsanitize=thread (TSan) and with
// -fsanitize=address,undefined, linked with the host library's sources (rp_host_*.cpp, rp_bvh.cpp) and the oracle
// (oracle/rp_oracle.c) directly -- no Python and no LD_PRELOAD between the sanitizer and the code.  It exercises:
//   - the multi-threaded binned-SAH builder and its SAH-optimal / greedy 4-wide collapse at 1, 3, 8 and 16 threads
//     (rph_bvh_tree_hash: the tree must not depend on the thread count) and the structural self-check, on a random
//     triangle soup, a mesh with shared vertices and degenerate (zero-area, duplicated) triangles, and spheres;
//   - the CPU traversal model (rph_bvh_traversal_stats_ex) and the exact primitive tests (rph_prim_test) over random rays;
//   - the render kernel's unit fetch in its host environment (rph_unit_walk: csrc/rp_units.h);
//   - the passes' host loops on exactly sized buffers: denoisers, variance, accumulation, tile selection, and temporal
//     reprojection with its per-pixel fold (rph_reproject, rph_accum_frames_counts);
//   - the OBJ and TGA readers (mesh.rs:145-183, image.rs:73-114) on files this driver writes, including truncated and
//     malformed ones (they must fail cleanly), and the TGA writer;
//   - the bulk StdRng (rph_stdrng_u64, threaded) against the oracle's sequential stream;
//   - the oracle's threaded renderer (or_render, the reference driver's tile queue) at 1 and 8 threads: same image.
// Exit status 0 = every check passed and the sanitizer reported nothing (a report aborts with a non-zero status).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/rp_host.h"
#include "../oracle/rp_oracle.h"

static int g_fail = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail = 1;                                                     \
    }                                                                 \
  } while (0)

struct MeshScene {
  std::vector<double> pos, nrm, uv;
  std::vector<uint32_t> idx;
  std::vector<rp_hittable> hit;
  rp_mesh mesh{};
  rp_material mat[2]{};
  rp_scene_desc desc{};
  void finish(uint32_t n_spheres, std::mt19937_64& rng) {
    mesh.n_vertices = (uint32_t)(pos.size() / 3);
    mesh.n_indices = (uint32_t)idx.size();
    mesh.positions = pos.data();
    mesh.normals = nrm.data();
    mesh.uvs = uv.data();
    mesh.indices = idx.data();
    mesh.material = 0;
    for (uint32_t t = 0; t < mesh.n_indices / 3; t++) {
      rp_hittable h{};
      h.kind = RP_HITTABLE_TRIANGLE;
      h.mesh = 0;
      h.triangle = 3 * t;
      hit.push_back(h);
    }
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (uint32_t k = 0; k < n_spheres; k++) {
      rp_hittable h{};
      h.kind = RP_HITTABLE_SPHERE;
      h.material = 1;
      h.center[0] = u(rng);
      h.center[1] = u(rng);
      h.center[2] = u(rng);
      h.radius = k == 0 ? 1000.0 : 0.05 + 0.1 * (u(rng) + 1.0);  // one huge sphere: an always-tested primitive
      if (k == 0) h.center[1] = -1001.0;
      hit.push_back(h);
    }
    mat[0].scatter.kind = RP_SCATTER_LAMBERT;
    mat[0].absorb.kind = RP_ABSORB_ALBEDO;
    mat[0].absorb.color[0] = mat[0].absorb.color[1] = mat[0].absorb.color[2] = 0.6;
    mat[1].scatter.kind = RP_SCATTER_METAL;
    mat[1].scatter.param = 0.2;
    mat[1].absorb.kind = RP_ABSORB_WHITE_BODY;
    desc.root_kind = RP_ROOT_BVH;
    desc.n_hittables = (uint32_t)hit.size();
    desc.hittables = hit.data();
    desc.n_meshes = 1;
    desc.meshes = &mesh;
    desc.n_materials = 2;
    desc.materials = mat;
    desc.n_textures = 0;
    desc.textures = nullptr;
    desc.background.kind = RP_EMIT_SKY_GRADIENT;
  }
};

static void add_vertex(MeshScene& s, double x, double y, double z) {
  s.pos.insert(s.pos.end(), {x, y, z});
  const double n = std::sqrt(x * x + y * y + z * z) + 1e-9;
  s.nrm.insert(s.nrm.end(), {x / n, y / n, z / n});
  s.uv.insert(s.uv.end(), {0.5 * (x + 1.0), 0.5 * (y + 1.0)});
}

static MeshScene soup(uint32_t n, uint64_t seed) {  // random small triangles in [-1, 1]^3 (config C5's construction)
  MeshScene s;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (uint32_t t = 0; t < n; t++) {
    const double cx = u(rng), cy = u(rng), cz = u(rng);
    for (int v = 0; v < 3; v++) {
      add_vertex(s, cx + 0.02 * u(rng), cy + 0.02 * u(rng), cz + 0.02 * u(rng));
      s.idx.push_back(3 * t + v);
    }
  }
  s.finish(8, rng);
  return s;
}

static MeshScene grid_with_degenerates(uint32_t side, uint64_t seed) {  // shared vertices, zero-area + duplicates
  MeshScene s;
  std::mt19937_64 rng(seed);
  for (uint32_t j = 0; j <= side; j++)
    for (uint32_t i = 0; i <= side; i++) add_vertex(s, (double)i / side - 0.5, 0.0, (double)j / side - 0.5);
  for (uint32_t j = 0; j < side; j++)
    for (uint32_t i = 0; i < side; i++) {
      const uint32_t a = j * (side + 1) + i, b = a + 1, c = a + side + 1, d = c + 1;
      s.idx.insert(s.idx.end(), {a, b, c, b, d, c});
      if ((i + j) % 7 == 0) s.idx.insert(s.idx.end(), {a, a, b});  // zero-area triangle
      if ((i + j) % 11 == 0) s.idx.insert(s.idx.end(), {a, b, c});  // duplicate triangle (exact-t ties)
    }
  s.finish(3, rng);
  return s;
}

static void check_tree(const char* name, const rp_scene_desc& d) {
  for (uint32_t fmt : {1u, 2u, 3u}) {    // RP_NODES_F32, Q8, W8
    for (uint32_t col : {1u, 2u}) {      // RP_COLLAPSE_GREEDY, SAH
      uint64_t st[16] = {0};
      const int rc = rph_bvh_selfcheck_ex(&d, fmt, col, st);
      if (rc != RP_OK) std::fprintf(stderr, "%s fmt %u collapse %u: %s\n", name, fmt, col, rph_last_error());
      CHECK(rc == RP_OK);
    }
    uint64_t h0 = 0;
    for (uint32_t threads : {1u, 3u, 8u, 16u}) {
      uint64_t h = 0;
      CHECK(rph_bvh_tree_hash(&d, fmt, threads, &h) == RP_OK);
      if (threads == 1) h0 = h;
      CHECK(h == h0);
    }
  }
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> u(-1.5, 1.5);
  const uint32_t n = 4096;
  std::vector<double> rays(8 * n);
  for (uint32_t r = 0; r < n; r++) {
    double* q = &rays[8 * r];
    q[0] = u(rng); q[1] = u(rng); q[2] = 3.0;
    q[3] = 0.1 * u(rng); q[4] = 0.1 * u(rng); q[5] = -1.0;
    if (r % 17 == 0) q[3] = 0.0;  // axis-parallel components
    q[6] = 1e-3;
    q[7] = (r % 5 == 0) ? 2.5 : INFINITY;
  }
  std::vector<uint64_t> per(4 * n);
  for (uint32_t fmt : {1u, 2u, 3u}) CHECK(rph_bvh_traversal_stats_ex(&d, rays.data(), n, fmt, 2u, per.data()) == RP_OK);
  // the exact primitive tests through their hook: a triangle across the rays' path and a sphere around their origins
  const double tri[9] = {-4.0, -4.0, 0.0, -16.0, 0.0, 0.0, 0.0, -16.0, 0.0}, sph[9] = {0.0, 0.0, 3.0, 5.0};
  std::vector<double> hit(4 * n);
  for (const double* g : {tri, sph}) {
    CHECK(rph_prim_test(g == tri ? 1u : 0u, g, rays.data(), n, hit.data()) == RP_OK);
    uint32_t acc = 0;
    for (uint32_t r = 0; r < n; r++) acc += hit[4 * r] == 1.0;
    CHECK(acc > n / 2);
  }
  CHECK(rph_prim_test(2u, tri, rays.data(), n, hit.data()) == RP_EINVAL);
  std::printf("%s: %u hittables, trees deterministic at 1/3/8/16 threads, self-checks pass\n", name, d.n_hittables);
}

static void write_file(const std::string& path, const std::string& bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  std::fwrite(bytes.data(), 1, bytes.size(), f);
  std::fclose(f);
}

static void check_io(const std::string& dir) {
  const std::string obj = dir + "/t.obj";
  write_file(obj, "# test\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvn 0 0 1\nvt 0 0\nvt 1 0\nvt 0 1\nvt 1 1\n"
                  "f 1/1/1 2/2/1 3/3/1\nf 2/2/1 4/4/1 3/3/1\n");
  rph_mesh m{};
  CHECK(rph_obj_load(obj.c_str(), &m) == RP_OK);
  CHECK(m.n_indices == 6);
  rph_mesh_free(&m);
  or_mesh_data om{};
  CHECK(or_obj_load(obj.c_str(), &om) == 0);
  or_mesh_free(&om);
  // malformed: an index past the vertices, a truncated face, garbage numbers, an empty file
  const char* bad[] = {"v 0 0 0\nvn 0 0 1\nvt 0 0\nf 1/1/1 2/1/1 3/1/1\n", "v 0 0 0\nf 1/1/1 1/1\n",
                       "v x y z\nf a b c\n", ""};
  for (const char* b : bad) {
    write_file(dir + "/bad.obj", b);
    rph_mesh mb{};
    if (rph_obj_load((dir + "/bad.obj").c_str(), &mb) == RP_OK) rph_mesh_free(&mb);
    or_mesh_data ob{};
    if (or_obj_load((dir + "/bad.obj").c_str(), &ob) == 0) or_mesh_free(&ob);
  }
  CHECK(rph_obj_load((dir + "/missing.obj").c_str(), &m) != RP_OK);
  // TGA: write, read back, and truncated / unsupported headers
  const uint32_t w = 37, h = 11;
  std::vector<uint8_t> img(4 * w * h);
  for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)(i * 31 + 7);
  for (size_t i = 3; i < img.size(); i += 4) img[i] = 255;
  const std::string tga = dir + "/t.tga";
  CHECK(rph_tga_save(tga.c_str(), w, h, img.data()) == RP_OK);
  uint32_t rw = 0, rh = 0;
  uint8_t* back = nullptr;
  CHECK(rph_tga_load(tga.c_str(), &rw, &rh, &back) == RP_OK);
  CHECK(rw == w && rh == h && back && std::memcmp(back, img.data(), img.size()) == 0);
  rph_free(back);
  uint8_t* ob2 = nullptr;
  CHECK(or_tga_load(tga.c_str(), &rw, &rh, &ob2) == 0);
  or_free(ob2);
  FILE* f = std::fopen(tga.c_str(), "rb");
  std::string all;
  char buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) all.append(buf, k);
  std::fclose(f);
  for (size_t cut : {size_t(0), size_t(5), size_t(17), size_t(18), all.size() / 2, all.size() - 1}) {
    write_file(dir + "/cut.tga", all.substr(0, cut));
    uint8_t* p = nullptr;
    if (rph_tga_load((dir + "/cut.tga").c_str(), &rw, &rh, &p) == RP_OK) rph_free(p);
    p = nullptr;
    if (or_tga_load((dir + "/cut.tga").c_str(), &rw, &rh, &p) == 0) or_free(p);
  }
  std::string rle = all;
  rle[2] = 10;  // RLE: unsupported
  write_file(dir + "/rle.tga", rle);
  uint8_t* p = nullptr;
  CHECK(rph_tga_load((dir + "/rle.tga").c_str(), &rw, &rh, &p) != RP_OK);
  std::printf("OBJ/TGA readers and writer: round trip exact, malformed inputs refused\n");
}

static void check_rng() {
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i * 13 + 1);
  const uint64_t n = 3u << 20;
  std::vector<uint64_t> bulk(n), seq(n);
  CHECK(rph_stdrng_u64(seed, 0, n, bulk.data()) == RP_OK);
  or_rng r;
  or_rng_from_seed(&r, seed, 12);
  for (uint64_t i = 0; i < n; i++) seq[i] = or_rng_next_u64(&r);
  CHECK(bulk == seq);
  std::printf("threaded bulk StdRng == the oracle's sequential stream (%llu draws)\n", (unsigned long long)n);
}

static void check_oracle_render(const MeshScene& s) {
  or_scene* os = or_scene_create(&s.desc);
  CHECK(os != nullptr);
  if (!os) return;
  rp_camera cam{};
  cam.aspect_ratio = 1.0;
  cam.fov = 1.2;
  cam.focal_dist = 1.0;
  const double p[3] = {0.0, 0.5, 3.0}, t[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};
  or_lookat(p, t, up, cam.orientation);
  std::memcpy(cam.position, p, sizeof p);
  rp_render_params rp{};
  rp.width = 48;
  rp.height = 32;
  rp.spp = 4;
  rp.max_bounce = 8;
  rp.seed = 7;
  rp.tile_w = rp.tile_h = 8;
  std::vector<double> a(3 * 48 * 32), b(3 * 48 * 32);
  uint64_t ca[OR_C_N] = {0}, cb[OR_C_N] = {0};
  CHECK(or_render(os, &cam, &rp, a.data(), nullptr, ca, 1) == 0);
  CHECK(or_render(os, &cam, &rp, b.data(), nullptr, cb, 8) == 0);
  CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
  CHECK(ca[OR_C_RAYS] == cb[OR_C_RAYS]);
  // the same frame with the shading census: all OR_C_N counters and the per-pixel event mask, 8 threads
  std::vector<uint64_t> mask(48 * 32, 0);
  uint64_t ce[OR_C_N] = {0};
  CHECK(or_render_events(os, &cam, &rp, b.data(), nullptr, ce, mask.data(), 8) == 0);
  CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
  CHECK(ce[OR_C_RAYS] == ca[OR_C_RAYS] && ce[OR_E_HIT_TRI] + ce[OR_E_HIT_SPH] + ce[OR_E_HIT_MISS] == ce[OR_C_RAYS]);
  const double secs = or_render_baseline(os, &cam, 32, 32, 2, 8, 16, 8, 11, nullptr, ca);
  CHECK(secs >= 0.0);
  or_scene_destroy(os);
  std::printf("oracle render at 1 and 8 threads: identical frames; threaded baseline driver ran\n");
}

// the render's launch arithmetic (csrc/rp_schedule.h, through the host library's hook): ragged and extreme shapes
static void check_plan() {
  rph_launch_plan o;
  int planned = 0, refused = 0;
  for (uint32_t w : {1u, 75u, 1920u, 65535u})
    for (uint32_t tile : {1u, 16u, 32u, 65535u})
      for (uint32_t spp : {0u, 1u, 40u, 1024u, 0xffffffffu})
        for (uint32_t nf : {1u, 20u, 64u})
          for (uint32_t q = 0; q < 4; q++) {
            const int rc = rph_plan_launch(w, w / 2 + 1, spp, 8, tile, tile, 2, 3, 32, q & 1, nf, q, q, q * 7, 262144, &o);
            CHECK(rc == RP_OK || rc == RP_EINVAL);
            if (rc == RP_OK) CHECK(o.queue_chunk >= 1 && o.grid >= 1 && o.n_queue < (1ull << 31));
            (rc == RP_OK ? planned : refused)++;
          }
  CHECK(planned > 0 && refused > 0);
  std::printf("launch plans: %d planned, %d refused\n", planned, refused);
}

// the render kernel's unit fetch in the host environment (csrc/rp_units.h, rph_unit_walk): the ragged frame, three
// frames per launch in pixel order over the per-XCD queues, with the wave-mate vote forced; and its cost probe
static void check_unit_walk() {
  const uint32_t W = 37, H = 21, nbatch = 3, frames = 3, blocks = 11;
  std::vector<uint32_t> units((size_t)RPH_UNIT_WORDS * 30 * 32 * nbatch * frames), words(RPH_QUEUE_WORDS),
      entries(RPH_QUEUE_WORDS);
  const uint64_t cap = units.size() / RPH_UNIT_WORDS;
  uint64_t n = 0, forced = 0;
  for (uint32_t lattice : {0u, 3u}) {
    CHECK(rph_unit_walk(W, H, 5, 8, 8, 4, 0, 1, 2, 0, frames, RP_FRAME_ORDER_PIXEL, RP_QUEUES_XCD_TILES, 3, nullptr, nullptr,
                        nullptr, lattice, 0, blocks, lattice ? 0 : 1, units.data(), cap, &n, words.data(), entries.data(),
                        &forced) == RP_OK);
    CHECK(n == (lattice ? 30ull * lattice * lattice : (uint64_t)W * H * nbatch * frames));
    for (uint64_t u = 0; u < n; u++) CHECK(units[RPH_UNIT_WORDS * u + 1] < W && units[RPH_UNIT_WORDS * u + 2] < H);
    if (!lattice) CHECK(forced >= 1);
  }
  CHECK(rph_unit_walk(W, H, 5, 8, 8, 4, 0, 1, 2, 0, frames, RP_FRAME_ORDER_PIXEL, RP_QUEUES_XCD_TILES, 3, nullptr, nullptr,
                      nullptr, 0, 0, blocks, 0, units.data(), 10, &n, words.data(), entries.data(), &forced) == RP_EINVAL);
  std::printf("unit walk: every unit of three ragged frames fetched, probe lattice walked, a short buffer refused\n");
}

// the guided denoiser's host loop (csrc/rp_denoise.h, rph_denoise) on a 7 x 5 frame at L = 5: most taps leave the frame,
// two pixels are misses (zero normal), and a depth is zero
static void check_denoise() {
  const uint32_t W = 7, H = 5;
  std::vector<double> rgb(3 * W * H), nrm(3 * W * H), alb(3 * W * H), dep(W * H), out(3 * W * H), out2(3 * W * H);
  for (uint32_t i = 0; i < W * H; i++) {
    const bool miss = i == 3 || i == 17;
    for (int k = 0; k < 3; k++) {
      rgb[3 * i + k] = 0.1 + 0.01 * ((i * 7 + k * 3) % 11);
      nrm[3 * i + k] = miss ? 0.0 : (k == (int)(i / 12) % 3 ? 1.0 : 0.1);
      alb[3 * i + k] = miss ? 0.0 : 0.5 + 0.1 * k;
    }
    dep[i] = miss || i == 9 ? 0.0 : 2.0 + 0.05 * i;
  }
  rp_denoise_params p{};
  p.iterations = 5;
  CHECK(rph_denoise(&p, W, H, rgb.data(), nrm.data(), alb.data(), dep.data(), out.data()) == RP_OK);
  for (uint32_t i : {3u, 17u})
    for (int k = 0; k < 3; k++) CHECK(out[3 * i + k] == rgb[3 * i + k]);
  for (double x : out) CHECK(x > 0.0 && x < 1.0);
  CHECK(rph_denoise(nullptr, W, H, rgb.data(), nullptr, nullptr, nullptr, out2.data()) == RP_OK);
  CHECK(rph_denoise(&p, W, H, rgb.data(), nrm.data(), alb.data(), dep.data(), rgb.data()) == RP_EINVAL);
  p.iterations = 9;
  CHECK(rph_denoise(&p, W, H, rgb.data(), nrm.data(), alb.data(), dep.data(), out.data()) == RP_EINVAL);
  std::printf("denoise: 7 x 5 at five levels, misses passed through, aliasing and a bad level count refused\n");
  // the variance pass's and the variance-guided filter's host loops (csrc/rp_variance.h rph_batch_variance,
  // rph_denoise_var) on the same frame: spp 10 in batches of 4, 4 and 2, some variances zero
  const uint32_t B = 3;
  std::vector<double> sums(3 * B * W * H), var(3 * W * H);
  for (uint32_t i = 0; i < W * H; i++)
    for (uint32_t b = 0; b < B; b++)
      for (int k = 0; k < 3; k++)
        sums[3 * (i * B + b) + k] = (b == 2 ? 2.0 : 4.0) * rgb[3 * i + k] * (i % 4 ? 1.0 + 0.1 * b : 1.0);
  CHECK(rph_batch_variance(10, 4, W * H, sums.data(), var.data()) == RP_OK);
  for (uint32_t i = 0; i < 3 * W * H; i++) CHECK(var[i] >= 0.0 && var[i] < 1.0 && (i / 3 % 4 ? var[i] > 0.0 : var[i] < 1e-30));
  CHECK(rph_batch_variance(4, 4, W * H, sums.data(), var.data()) == RP_EINVAL);
  rp_denoise_var_params v{};
  v.base.iterations = 5;
  CHECK(rph_denoise_var(&v, W, H, rgb.data(), var.data(), nrm.data(), alb.data(), dep.data(), out.data()) == RP_OK);
  for (uint32_t i : {3u, 17u})
    for (int k = 0; k < 3; k++) CHECK(out[3 * i + k] == rgb[3 * i + k]);
  for (double x : out) CHECK(x > 0.0 && x < 1.0);
  CHECK(rph_denoise_var(nullptr, W, H, rgb.data(), var.data(), nullptr, nullptr, nullptr, out2.data()) == RP_OK);
  CHECK(rph_denoise_var(&v, W, H, rgb.data(), var.data(), nrm.data(), alb.data(), dep.data(), var.data()) == RP_EINVAL);
  CHECK(rph_denoise_var(&v, W, H, rgb.data(), nullptr, nrm.data(), alb.data(), dep.data(), out.data()) == RP_EINVAL);
  v.sigma_var = -1.0;
  CHECK(rph_denoise_var(&v, W, H, rgb.data(), var.data(), nrm.data(), alb.data(), dep.data(), out.data()) == RP_EINVAL);
  std::printf("variance: batches of 4, 4 and 2; variance-guided denoise: misses passed through, aliasing, a missing\n"
              "variance and a negative sigma_var refused\n");
  // progressive accumulation's host loops (csrc/rp_accum.h rph_accum_frames, rph_accum_error): the three batch frames
  // at a stride with a gap, folded 1 + 2 with exactly sized buffers, then the error statistics of the result
  const uint64_t nw = 3 * W * H, stride = nw + 5;
  std::vector<double> fr(2 * stride + nw), mean(nw), m2(nw), avar(nw);
  for (uint32_t b = 0; b < B; b++)
    for (uint64_t i = 0; i < nw; i++) fr[b * stride + i] = sums[3 * (i / 3 * B + b) + i % 3] / (b == 2 ? 2.0 : 4.0);
  CHECK(rph_accum_frames(nw, 0, 1, fr.data(), stride, mean.data(), m2.data(), nullptr) == RP_OK);
  for (uint64_t i = 0; i < nw; i++) CHECK(mean[i] == fr[i] && m2[i] == 0.0);
  CHECK(rph_accum_frames(nw, 1, 2, fr.data() + stride, stride, mean.data(), m2.data(), avar.data()) == RP_OK);
  for (uint64_t i = 0; i < nw; i++) CHECK(avar[i] >= 0.0 && avar[i] < 1.0 && (i / 3 % 4 ? avar[i] > 0.0 : avar[i] == 0.0));
  CHECK(rph_accum_frames(nw, 0, 1, fr.data(), stride, mean.data(), m2.data(), avar.data()) == RP_EINVAL);
  CHECK(rph_accum_frames(nw, 0, 3, fr.data(), stride, fr.data() + nw, m2.data(), avar.data()) == RP_EINVAL);
  uint64_t st[RP_ERROR_STATS_LEN];
  CHECK(rph_accum_error(nullptr, W * H, mean.data(), avar.data(), st) == RP_OK);
  CHECK(st[0] == W * H && st[1] <= st[0] && st[2] > 0 && st[3] == 0);
  rp_error_params ep{-1.0, 0.0};
  CHECK(rph_accum_error(&ep, W * H, mean.data(), avar.data(), st) == RP_EINVAL);
  std::printf("accumulate: three frames at a gapped stride folded 1 + 2, error statistics; one-frame variance, aliasing\n"
              "and a negative tolerance refused\n");
}

// tile-adaptive progressive rendering's host code (csrc/rp_accum.h and csrc/rp_schedule.h: rph_accum_frames_tiles,
// rph_accum_tiles_select, rph_plan_tiles_launch, rph_tiles_unit_walk) on a 37 x 21 frame in 8 x 4 tiles (5 x 6 tiles,
// both edges ragged), every buffer exactly sized: the fold and the select over a shuffled list with an entry outside
// the frame, the compaction in place, the plan over every list length and the fetch over the foreign list
static void check_tiles() {
  const uint32_t W = 37, H = 21, tw = 8, th = 4, n_tiles = 30, tile_px = tw * th, tile_words = 3 * tile_px;
  std::vector<uint32_t> list = {29, 3, 30, 17, 0, 4, 24};  // 30: not a tile of the frame
  const uint32_t n_listed = (uint32_t)list.size(), frames = 3;
  const uint64_t state = (uint64_t)n_tiles * tile_words, stride = (uint64_t)n_listed * tile_words;
  std::vector<double> fr(frames * stride), mean(state, 0.5), m2(state, 0.0), var(state, 0.0);
  for (uint64_t i = 0; i < fr.size(); i++) fr[i] = 0.25 + 0.001 * (double)((i * 2654435761ull) % 997);
  CHECK(rph_accum_frames_tiles(tile_words, n_tiles, list.data(), n_listed, 0, frames, fr.data(), stride, mean.data(),
                               m2.data(), var.data()) == RP_OK);
  CHECK(mean[(uint64_t)29 * tile_words] != 0.5 && mean[(uint64_t)1 * tile_words] == 0.5 && var[0] > 0.0);
  CHECK(rph_accum_frames_tiles(tile_words, n_tiles, list.data(), n_listed, 3, 1, fr.data(), stride, mean.data(), m2.data(),
                               nullptr) == RP_OK);
  CHECK(rph_accum_frames_tiles(tile_words, 6, list.data(), n_listed, 0, frames, fr.data(), stride, mean.data(), m2.data(),
                               var.data()) == RP_EINVAL);
  CHECK(rph_accum_frames_tiles(tile_words, n_tiles, list.data(), n_listed, 0, frames, fr.data(), stride - 1, mean.data(),
                               m2.data(), var.data()) == RP_EINVAL);
  rp_render_params p{};
  p.width = W, p.height = H, p.spp = 4, p.max_bounce = 8, p.tile_w = tw, p.tile_h = th, p.samples_per_stream = 4;
  std::vector<uint32_t> over(n_listed), out(n_listed);
  uint32_t count = 99;
  CHECK(rph_accum_tiles_select(&p, nullptr, 0.0, mean.data(), var.data(), list.data(), n_listed, over.data(), out.data(),
                               &count) == RP_OK);
  CHECK(count <= n_listed - 1 && over[2] == 0);
  for (uint32_t i = 0; i < count; i++) CHECK(out[i] < n_tiles);
  std::vector<uint32_t> all(n_tiles);
  CHECK(rph_accum_tiles_select(&p, nullptr, 0.5, mean.data(), var.data(), nullptr, n_tiles, nullptr, all.data(), &count) == RP_OK);
  CHECK(rph_accum_tiles_select(&p, nullptr, 0.0, mean.data(), var.data(), list.data(), n_listed, nullptr, list.data(),
                               &count) == RP_OK);  // in place
  CHECK(rph_accum_tiles_select(&p, nullptr, 1.0, mean.data(), var.data(), nullptr, n_tiles, nullptr, all.data(), &count) == RP_EINVAL);
  CHECK(rph_accum_tiles_select(&p, nullptr, 0.0, mean.data(), var.data(), nullptr, 16385, nullptr, all.data(), &count) == RP_EINVAL);
  list = {29, 3, 30, 17, 0, 4, 24};
  rph_launch_plan o;
  for (uint32_t n = 0; n <= n_tiles + 1; n++)
    for (uint32_t q = 0; q < 4; q++) {
      const int rc = rph_plan_tiles_launch(W, H, 4, 8, tw, th, 4, n, 1 + 5 * q, q, q, q * 3, 262144, &o);
      CHECK(rc == (n <= n_tiles ? RP_OK : RP_EINVAL));
      if (rc == RP_OK) CHECK(o.queue_chunk >= 1 && o.grid >= 1 && o.n_slots == (uint64_t)n * tile_px);
    }
  CHECK(rph_plan_tiles_launch(W, H, 4, 8, tw, th, 2, 3, 1, 0, 0, 0, 262144, &o) == RP_EINVAL);
  std::vector<uint32_t> units((size_t)RPH_UNIT_WORDS * n_listed * tile_px * frames), words(RPH_QUEUE_WORDS),
      entries(RPH_QUEUE_WORDS);
  uint64_t n = 0, want = 0;
  for (uint32_t t : list)
    if (t < n_tiles) want += (uint64_t)std::min(tw, W - (t % 5) * tw) * std::min(th, H - (t / 5) * th);
  for (uint32_t order : {RP_FRAME_ORDER_SEQUENTIAL, RP_FRAME_ORDER_INTERLEAVED, RP_FRAME_ORDER_PIXEL}) {
    CHECK(rph_tiles_unit_walk(W, H, 4, 8, tw, th, 4, frames, order, RP_QUEUES_XCD_TILES, 3, list.data(), n_listed, 11,
                              units.data(), units.size() / RPH_UNIT_WORDS, &n, words.data(), entries.data()) == RP_OK);
    CHECK(n == want * frames);
    for (uint64_t u = 0; u < n; u++)
      CHECK(units[RPH_UNIT_WORDS * u] < n_listed * tile_px && units[RPH_UNIT_WORDS * u + 1] < W && units[RPH_UNIT_WORDS * u + 2] < H);
  }
  CHECK(rph_tiles_unit_walk(W, H, 4, 8, tw, th, 4, frames, 0, 0, 0, list.data(), n_listed, 11, units.data(), 10, &n,
                            words.data(), entries.data()) == RP_EINVAL);
  std::printf("tiles: a shuffled list with an entry outside the frame folded, selected (in place too), planned and walked;\n"
              "a short state, a short stride, a full tile share, 16385 entries and a short unit buffer refused\n");
}

// temporal reprojection's host loops (csrc/rp_reproject.h rph_reproject; csrc/rp_accum.h rph_accum_frames_counts) on a
// 9 x 7 frame with exactly sized buffers: a camera that steps sideways over a plane with two sky pixels and two pixels
// without history, a previous camera that faces away (every pixel off), then the per-pixel fold of two frames
static void check_reproject() {
  const uint32_t W = 9, H = 7, n = W * H;
  std::vector<double> dep(n), nrm(3 * n), mean0(3 * n), m20(3 * n), mean(3 * n), m2(3 * n), var(3 * n), fr(2 * 3 * n);
  std::vector<uint32_t> cnt0(n), cnt(n);
  for (uint32_t i = 0; i < n; i++) {
    const bool sky = i == 5 || i == 40;
    dep[i] = sky ? 0.0 : 4.0 + 0.01 * (i % W);
    for (int k = 0; k < 3; k++) {
      nrm[3 * i + k] = sky ? 0.0 : (k == 2 ? 1.0 : 0.05);
      mean0[3 * i + k] = 0.2 + 0.01 * ((i * 5 + k) % 13);
      m20[3 * i + k] = 0.001 * ((i + k) % 7);
    }
    cnt0[i] = i == 11 || i == 30 ? 0 : 1 + i % 40;  // some above max_history = 32
  }
  for (size_t i = 0; i < fr.size(); i++) fr[i] = 0.3 + 0.01 * (i % 17);
  rp_camera cur{}, prev{};
  cur.aspect_ratio = (double)W / H, cur.fov = 0.8, cur.focal_dist = 1.0;
  cur.orientation[0] = cur.orientation[4] = cur.orientation[8] = 1.0;
  cur.position[2] = 4.0;
  prev = cur;
  prev.position[0] = 0.6;  // 1.2 pixels at this depth: the first column leaves the previous frame
  uint64_t st[RP_REPROJECT_STATS_LEN];
  CHECK(rph_reproject(nullptr, W, H, &cur, &prev, dep.data(), nrm.data(), dep.data(), nrm.data(), mean0.data(), m20.data(),
                      cnt0.data(), mean.data(), m2.data(), cnt.data(), st) == RP_OK);
  CHECK(st[0] == n && st[1] > n / 2 && st[1] < n && st[2] >= st[1] && st[3] > 0 && st[3] < n);
  for (uint32_t i = 0; i < n; i++) CHECK(cnt[i] <= 32 && (cnt[i] || (mean[3 * i] == 0.0 && m2[3 * i] == 0.0)));
  CHECK(rph_accum_frames_counts(n, 3, 2, fr.data(), 3 * n, cnt.data(), mean.data(), m2.data(), var.data(), 0.5) == RP_OK);
  for (uint32_t i = 0; i < n; i++) CHECK(cnt[i] >= 2 && cnt[i] <= 34 && var[3 * i] >= 0.0 && mean[3 * i] > 0.0);
  prev.orientation[0] = prev.orientation[8] = -1.0;  // turned about y: the scene lies behind it
  CHECK(rph_reproject(nullptr, W, H, &cur, &prev, dep.data(), nrm.data(), dep.data(), nrm.data(), mean0.data(), m20.data(),
                      cnt0.data(), mean.data(), m2.data(), cnt.data(), st) == RP_OK);
  CHECK(st[1] == 0 && st[2] == 0 && st[3] == n);
  std::vector<uint32_t> one(n, 0);
  CHECK(rph_accum_frames_counts(n, 3, 1, fr.data(), 3 * n, one.data(), mean.data(), m2.data(), var.data(), 0.5) == RP_OK);
  for (uint32_t i = 0; i < 3 * n; i++) CHECK(mean[i] == fr[i] && m2[i] == 0.0 && var[i] == 0.5);
  CHECK(rph_reproject(nullptr, W, H, &cur, &prev, dep.data(), nrm.data(), dep.data(), nrm.data(), mean0.data(), m20.data(),
                      cnt0.data(), mean0.data(), m2.data(), cnt.data(), st) == RP_EINVAL);
  rp_reproject_params rp{};
  rp.normal_cos = 1.5;
  CHECK(rph_reproject(&rp, W, H, &cur, &prev, dep.data(), nrm.data(), dep.data(), nrm.data(), mean0.data(), m20.data(),
                      cnt0.data(), mean.data(), m2.data(), cnt.data(), st) == RP_EINVAL);
  CHECK(rph_accum_frames_counts(n, 3, 2, fr.data(), 3 * n, cnt.data(), mean.data(), m2.data(), var.data(), -1.0) == RP_EINVAL);
  std::printf("reproject: a sideways step with sky, empty and long histories, then the per-pixel fold; a camera facing away;\n"
              "one frame from nothing; in-place, a cosine above 1 and a negative var_one refused\n");
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  check_plan();
  check_unit_walk();
  check_denoise();
  check_tiles();
  check_reproject();
  MeshScene a = soup(200000, 11);  // >= 2^16 primitives: the parallel build form (rp_bvh.cpp ParallelBuild) runs
  check_tree("soup", a.desc);
  MeshScene b = grid_with_degenerates(40, 3);
  check_tree("grid+degenerates", b.desc);
  check_io(dir);
  check_rng();
  check_oracle_render(b);
  std::printf(g_fail ? "FAILED\n" : "ALL CHECKS PASSED\n");
  return g_fail;
}
