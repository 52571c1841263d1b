/*
 * rp_host.h -- C-ABI of librp_host.so: the host pieces around the hot path, in C++ (the reference's
 * Rust host -- example_scenes.rs, mesh.rs obj::load, image.rs tga::load/save, utility.rs lookat /
 * to_srgb_u8 -- cannot be built in this image).  A Rust host keeps its own; these exist so that C/C++
 * and Python callers (tests, bench.py) can build the reference scenes without Rust.
 * No GPU code: this library loads and runs on any host.
 */
#ifndef RP_HOST_H
#define RP_HOST_H

#include <stdint.h>

#include "rp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mesh.rs:145-183 obj::load: v/vn/vt/f lines, 1-based indices, (p, n, t) tuples deduplicated in
 * first-use order, missing normal -> (0,0,0), missing uv -> (0,0), non-triangular faces rejected.
 * Arrays are allocated by the library; release with rph_mesh_free. */
typedef struct rph_mesh {
  uint32_t n_vertices, n_indices;
  double* positions; /* 3 * n_vertices */
  double* normals;   /* 3 * n_vertices */
  double* uvs;       /* 2 * n_vertices */
  uint32_t* indices; /* n_indices */
} rph_mesh;

int rph_obj_load(const char* path, rph_mesh* out);  /* RP_OK or RP_EINVAL (message: rph_last_error) */
void rph_mesh_free(rph_mesh* m);

/* image.rs:73-114 tga::load: uncompressed 24/32-bit only; returns RGBA8 with row 0 = bottom row. */
int rph_tga_load(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgba);
/* image.rs:116-137 tga::save: 32-bit BGRA, bottom-left origin. */
int rph_tga_save(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba);
void rph_free(void* p);

/* utility.rs:212-220 to_srgb_u8 over n pixels of linear RGB (f64) -> RGBA8 (alpha 255). */
void rph_to_srgb_u8(const double* rgb, uint64_t n_pixels, uint8_t* rgba);

/* utility.rs:172-177 Transformation::lookat -> column-major orientation for rp_camera. */
void rph_lookat(const double position[3], const double target[3], const double up[3], double orientation[9]);

/* Deterministic stand-in for assets/sky_panorama.tga, which is missing from the reference mount
 * (.MISSING_LARGE_BLOBS:1): an equirectangular RGBA8 sky (gradient, sun disc, hashed value-noise
 * clouds built on randomness.rs noise::integer).  Row 0 = bottom (nadir), as tga::load stores it.
 * Pure integer and +,-,*,/,sqrt arithmetic: bit-identical on every IEEE host. */
int rph_sky_panorama(uint32_t width, uint32_t height, uint8_t* rgba);

/* Self-check of the acceleration-structure builder used by librp.so on a scene (CPU only):
 * validates the scene, builds the host tree in `node_format` (RP_NODES_*, AUTO = librp.so's size rule)
 * and checks its invariants.  stats (nullable, 4 values): {nodes, leaves, max_depth, primitives}. */
int rph_bvh_selfcheck(const rp_scene_desc* desc, uint32_t node_format, uint64_t* stats);

/* CPU model of the device traversal over the same packed tree in `node_format` (diagnostics): for n rays
 * (layout of rp_intersect) writes n x 3 {node records visited, primitive tests, closest hittable id or
 * 2^64-1}. */
int rph_bvh_traversal_stats(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                            uint64_t* per_ray);
/* The two above with the 4-wide collapse chosen (RP_COLLAPSE_*, include/rp.h: the library's AUTO is SAH). */
int rph_bvh_selfcheck_ex(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, uint64_t* stats);
int rph_bvh_traversal_stats_ex(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                               uint32_t collapse, uint64_t* per_ray);

/* Hash (FNV-1a) of the packed host tree (node records and leaf-ordered primitive references) built with
 * `threads` build threads (0 = the machine's, at most 16): the tree does not depend on the thread count. */
int rph_bvh_tree_hash(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, uint64_t* hash);

/* The three above with the always-tested list chosen, so the CPU model sees the tree librp.so renders with:
 * always_max as rp_scene_options.always_max (< 0: the default, 0: every hittable in the tree), and always_minor != 0
 * for the rule librp.so applies to every host-built tree -- a mesh scene's few non-triangle hittables are tested
 * first for every ray too, and the tree's leaves hold triangles only (the hooks above build without it).
 * stats (nullable) has 6 values here: {nodes, leaves, max_depth, primitives, always-tested primitives, non-triangle
 * primitives inside the tree}. */
int rph_bvh_selfcheck_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t collapse, int32_t always_max,
                          uint32_t always_minor, uint64_t* stats);
int rph_bvh_traversal_stats_opt(const rp_scene_desc* desc, const double* rays, uint64_t n, uint32_t node_format,
                                uint32_t collapse, int32_t always_max, uint32_t always_minor, uint64_t* per_ray);
int rph_bvh_tree_hash_opt(const rp_scene_desc* desc, uint32_t node_format, uint32_t threads, int32_t always_max,
                          uint32_t always_minor, uint64_t* hash);

/* rand 0.8 StdRng (ChaCha12, rand_chacha 0.3 stream: 64-bit block counter, zero nonce) keyed by the 32-byte
 * seed (StdRng::from_seed; seed_from_u64 seeds come from its PCG32 expansion): n consecutive next_u64
 * draws starting at draw index `first` (two keystream words each, little-endian).  Host bulk scene
 * generation (the synthetic C5 mesh: 120 M draws); multi-threaded. */
int rph_stdrng_u64(const uint8_t seed[32], uint64_t first, uint64_t n, uint64_t* out);

/* Test hook: the magic numbers of the render kernel's unit decode (raytracing-potato_amd/csrc/rp_kernel.h
 * rpk::make_div32, the same header the library's launches use): for a divisor d >= 1, m and s such that
 * floor(n / d) == (n * m) >> s (64-bit product) for every n < 2^31.  RP_EINVAL for d == 0. */
int rph_make_div32(uint32_t d, uint32_t* m, uint32_t* s);

/* Test hook: what a render decides before its first launch (raytracing-potato_amd/csrc/rp_schedule.h rps::plan_launch,
 * the same header librp.so's render_shard calls), for n_frames frames of an rp_render_params given field by field, the
 * scheduling fields of the scene's resolved options and the render lanes the scene keeps resident.  The tiling's
 * outputs (n_shard_tiles .. block_words) are filled whenever the params are valid.  Returns the render's own refusal
 * (RP_EINVAL, message: rph_last_error) or RP_OK. */
typedef struct rph_launch_plan {
  uint32_t n_shard_tiles, nbatch;
  uint32_t plan_block;     /* rps::plan_block(frame tiles, num_shards) */
  uint64_t n_slots;
  uint64_t gather_stride;  /* rps::stage_slots: rp_gather_stride */
  uint64_t block_words;    /* rps::pack_words(t, true, n_frames): rp_frames_block_words */
  uint32_t queue_groups, queue_chunk, frames_inter, sortable, measure;
  uint32_t grid;           /* blocks of the launch (rps::grid_for) */
  uint64_t n_queue, out_stride;
  uint32_t dv_units[2], dv_tiles_x[2], dv_chunk[2]; /* the launch's make_div32 constants, {m, s} */
} rph_launch_plan;
int rph_plan_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                    uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                    uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes, rph_launch_plan* out);

/* Test hook: one round of a draw of the render kernel (raytracing-potato_amd/csrc/rp_draw.h, the same header the
 * kernel's scatter and camera draws use: window addressing with the ring's mirror tail, the stride, the accept rules,
 * "first accepted try wins", the position update).  kind: 1 UnitSphere (Lambert), 2 UnitBall (Metal), 3 the
 * Bernoulli draw's Standard f64 (Dielectric), 4 UnitDisk (camera).  ring_image: a lane's ring laid out as its slab
 * holds it, in raw keystream words (the hook decodes every u64 to the double the slab keeps, as the kernel does where
 * it makes a block: rph_draw_values) -- 16 * ring_blocks words (ring_blocks 4 or 8; keystream block b in slot b % ring_blocks), then, for
 * ring_blocks 8, the tail, the first 8 words of slot 0 again (the ring of 4 has none: 64 words are read, wrapping) --
 * which must hold every block the round can consume from the even stream word
 * `pos` on (two tries of 4 words for kinds 1 and 4, of 6 for kind 2; 2 words for kind 3).  On return *accepted tells
 * whether a try of the round was accepted (always, for kind 3); if so out[0..2] are the values -- the sphere point
 * (x n, y n, 1 - 2 s), the ball point, the Standard f64 (out[1], out[2] zero), the disk point (out[2] zero) -- and
 * *new_pos the stream position after the accepted try; if not, *new_pos is the next round's position.  RP_EINVAL
 * for a bad kind, ring size or odd pos. */
int rph_draw_round(uint32_t kind, uint32_t ring_blocks, const uint32_t* ring_image, uint32_t pos, double out[3],
                   uint32_t* new_pos, uint32_t* accepted);

/* Test hook: what the kernel's keystream ring holds for a keystream u64 and what a Standard f64 draw makes of it
 * (rp_draw.h value_store / unit_of, the pair the kernel compiles).  The kernel decodes a block once, where it is made:
 * with k = u64 >> 11, stored[i] = k 2^-52 - 1 (the rejection samplers' 2 r - 1), and unit[i] = (stored[i] + 1) / 2 =
 * k 2^-53 (r itself: the jitter, the Bernoulli draw), both exact.  words: n u64 (low word = the first keystream word).
 * rph_draw_round takes the raw image and decodes it the same way.  RP_EINVAL for a NULL pointer with n > 0. */
int rph_draw_values(const uint64_t* words, uint64_t n, double* stored, double* unit);

/* Test hook: how a ray enters the conservative f32 box test (raytracing-potato_amd/csrc/rp_ray.h, the same header the
 * kernels' setup_ray32 and trav_step use, except that the reciprocal is a correctly rounded 1 / x here).  rays: n x 8
 * {o, d, t_min, best}, as rph_bvh_traversal_stats takes them; node_format RP_NODES_F32, _Q8 or _W8 (the quantized
 * formats add their frame term, with qbound the scene's bound on every frame's |o| and 255 s).  out: n x 11 floats
 * {inv[3], nb[3], fb[3], tmin32, best32}: per axis the clamped slope and the near- and far-plane addends,
 * nb <= -oinv - D and fb >= -oinv + D; tmin32 <= t_min; best32 >= best (+inf for best = +inf). */
int rph_ray_setup(uint32_t node_format, double qbound, const double* rays, uint64_t n, float* out);

/* Test hook: the exact f64 primitive tests (raytracing-potato_amd/csrc/rp_isect.h tri_test / sphere_test, the same
 * header the kernels' prim_test and the CPU traversal model call).  kind: 0 sphere, 1 triangle; g: the nine doubles of
 * geometry as the packed primitive holds them (triangle: a, a - b, a - c; sphere: centre, radius, the rest unread);
 * rays: n x 8 {o, d, t_min, best}.  out: n x 4 doubles {accepted (1 or 0), t, u, v}: t, u, v of an accepted test
 * (a sphere's u and v are 0), zeros for a rejected one.  RP_EINVAL for a NULL pointer or an unknown kind. */
int rph_prim_test(uint32_t kind, const double g[9], const double* rays, uint64_t n, double* out);

/* Test hooks: the packed head of a device material record (raytracing-potato_amd/csrc/rp_layout.h material_head_pack /
 * material_head_unpack, the one pair the scene builder and the render kernel's shading compile).
 * rph_material_head packs fields = {scatter_kind, absorb_kind, emit_kind, needs_uv, absorb_tex, emit_tex} into
 * packed = {head, head_tex} and unpacks those again into unpacked = {the same six, wide}; with wide = 1 the head holds
 * no texture ids (one of them needs more than 16 bits) and unpacked[4..5] mean nothing.
 * rph_scene_materials builds desc's shading tables and writes, for the first min(cap, n) of its n materials, the
 * record's first eight words as the device gets them: {scatter_kind, absorb_kind, emit_kind, absorb_tex, emit_tex,
 * needs_uv, head, head_tex}; *n_materials = n.  RP_EINVAL for a NULL pointer or a scene the builder refuses. */
int rph_material_head(const uint32_t fields[6], uint32_t packed[2], uint32_t unpacked[7]);
int rph_scene_materials(const rp_scene_desc* desc, uint64_t cap, uint32_t* words, uint64_t* n_materials);

/* Test hook: the per-primitive normals table (raytracing-potato_amd/csrc/rp_layout.h TriNormals) the host builder
 * makes for desc beside its primitive records -- the table librp.so uploads for a host-built tree, and the statement
 * (tri_normals_fill) the device builders' gather kernel compiles.  The tree is rph_bvh_tree_hash_opt's (node_format,
 * always_max, always_minor).  For the first min(cap, n) of the n primitives in leaf order: normals gets 9 doubles
 * {n0.xyz, n1.xyz, n2.xyz} (a sphere: zeros), refs 4 words {v0, v1, v2, src} (the PrimRef: global vertex ids, source
 * hittable), kinds one word (0 sphere, 1 triangle); each of the three may be NULL.  *n_prims = n.  RP_EINVAL for a NULL
 * desc or n_prims or a scene the builder refuses. */
int rph_tri_normals(const rp_scene_desc* desc, uint32_t node_format, int32_t always_max, uint32_t always_minor, uint64_t cap,
                    double* normals, uint32_t* refs, uint32_t* kinds, uint64_t* n_prims);

/* Test hook: the render kernel's unit fetch, run on the CPU (raytracing-potato_amd/csrc/rp_units.h fetch_pixel, unit_frame
 * and unit_spp: the same header the kernel compiles, in a host environment that stands in for the kernarg segment, the
 * atomics and the wave).  The launch is planned by rps::plan_launch from the arguments rph_plan_launch takes (and must
 * pass rps::launch_limits with n_blocks lanes); tile_order (n_shard_tiles entries), tile_map (the frame's tiles, a deal
 * order) and unit_order (n_slots * nbatch entries) are optional (NULL) and set as render_shard's stages set them.
 * probe_lattice > 0 walks the cost probe of the shard's tiles with that lattice side instead of the render.
 * queue_groups > 0 replaces the plan's queue count (1 or 8) by another up to 8: the fetch serves any.
 *
 * n_blocks blocks of one lane each fetch in rounds -- every block not yet retired fetches once per round, and retires on
 * its first failed fetch, as a lane does.  units: 8 words per unit in fetch order {slot, pi, pj, global batch, fetching
 * block, the queue it came from, unit_frame(batch), unit_spp(batch)}, units_cap units of room, *n_units the count.  queue_words and entries:
 * RPH_QUEUE_WORDS words each -- the final queue words, and per word the fetches that got an entry.
 *
 * any_every = n > 0: on every n-th wave vote of the walk, a wave-mate that found the queue drained while this lane did
 * not is put beside the lane (the vote is forced true).  Such a mate exists only where the lane took its queue's last
 * entry (the mate's increment, the next of the same wave atomic, is then the first drained one), so the vote is forced
 * only there; *forced counts the votes that were.
 *
 * The environment checks every queue word the fetch touches (a queue below queue_groups, or the probe's word) and every
 * numerator of a launch-constant division (< 2^31): a violation ends the walk with RP_EINVAL and a message, as do a
 * refused launch, an order or map entry out of range and more than units_cap units. */
enum { RPH_QUEUE_WORDS = 288, RPH_UNIT_WORDS = 8 };
int rph_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w, uint32_t tile_h,
                  uint32_t shard, uint32_t num_shards, uint32_t samples_per_stream, uint32_t shard_map, uint32_t n_frames,
                  uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tile_order,
                  const uint32_t* tile_map, const uint32_t* unit_order, uint32_t probe_lattice, uint32_t queue_groups,
                  uint32_t n_blocks, uint32_t any_every, uint32_t* units, uint64_t units_cap, uint64_t* n_units,
                  uint32_t* queue_words, uint32_t* entries, uint64_t* forced);

/* The guided denoiser on the CPU (include/rp.h rp_denoise: the definition): a plain loop over
 * raytracing-potato_amd/csrc/rp_denoise.h, the same header the device kernel compiles, so the two agree bit for bit.
 * Host buffers, full frames in frame order; params, normal, albedo and depth nullable as rp_denoise's.  RP_EINVAL for
 * NULL rgb or out, a zero size, a side above 65535, out aliasing an input and parameters out of range. */
int rph_denoise(const rp_denoise_params* params, uint32_t width, uint32_t height, const double* rgb, const double* normal,
                const double* albedo, const double* depth, double* out);
/* The variance-guided denoiser on the CPU (include/rp.h rp_denoise_var: the definition), the same loop over the same
 * header with the variance carried along.  var: a full frame, 3 doubles per pixel, required; the rest as rph_denoise. */
int rph_denoise_var(const rp_denoise_var_params* params, uint32_t width, uint32_t height, const double* rgb,
                    const double* var, const double* normal, const double* albedo, const double* depth, double* out);

/* The per-pixel variance pass on the CPU (include/rp.h rp_render_variance_device_ws: the definition): a plain loop over
 * raytracing-potato_amd/csrc/rp_variance.h, the header the device kernel compiles.  sums: n_pixels x B x 3 doubles,
 * pixel i's batch b at (i*B + b)*3 with B = ceil(spp / samples_per_stream) (0: RP_SAMPLES_PER_STREAM); var: n_pixels x 3.
 * RP_EINVAL for B < 2 and NULL buffers. */
int rph_batch_variance(uint32_t spp, uint32_t samples_per_stream, uint64_t n_pixels, const double* sums, double* var);

/* Progressive accumulation on the CPU (include/rp.h rp_accum_frames_device and rp_accum_error_device_ws: the
 * definitions): plain loops over raytracing-potato_amd/csrc/rp_accum.h, the header the device kernels compile, so the
 * two agree bit for bit.  rph_accum_frames: rp_accum_frames_device on host buffers, with its arguments and its RP_EINVAL
 * cases.  rph_accum_error: mean and var are full frames of n_pixels pixels, 3 doubles each (every pixel is counted);
 * stats: RP_ERROR_STATS_LEN words, as rp_accum_error_device_ws defines them.  RP_EINVAL for NULL buffers and parameters
 * out of range. */
int rph_accum_frames(uint64_t n_words, uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride,
                     double* mean, double* m2, double* var);
int rph_accum_error(const rp_error_params* params, uint64_t n_pixels, const double* mean, const double* var,
                    uint64_t* stats);

/* Tile-adaptive progressive rendering on the CPU (include/rp.h rp_accum_frames_tiles_device and
 * rp_accum_tiles_select_device: the definitions): plain loops over raytracing-potato_amd/csrc/rp_accum.h, the header the
 * device kernels compile, so values agree bit for bit and counts, list and order exactly.  Host buffers, the device
 * calls' arguments and RP_EINVAL cases; rph_accum_tiles_select also serves tiles_out == tiles_in (compaction in place). */
int rph_accum_frames_tiles(uint64_t tile_words, uint32_t n_state_tiles, const uint32_t* tiles, uint32_t n_listed,
                           uint32_t n_prior, uint32_t n_frames, const double* frames, uint64_t frame_stride, double* mean,
                           double* m2, double* var);
int rph_accum_tiles_select(const rp_render_params* params, const rp_error_params* error, double tile_share,
                           const double* mean, const double* var, const uint32_t* tiles_in, uint32_t n_in, uint32_t* over,
                           uint32_t* tiles_out, uint32_t* count);

/* Temporal reprojection on the CPU (include/rp.h rp_reproject_device and rp_accum_frames_counts_device: the
 * definitions): plain loops over raytracing-potato_amd/csrc/rp_reproject.h and rp_accum.h, the headers the device
 * kernels compile, so the two agree bit for bit.  Host buffers, the device calls' arguments and RP_EINVAL cases. */
int rph_reproject(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                  const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                  const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                  double* mean, double* m2, uint32_t* count, uint64_t* stats);
int rph_accum_frames_counts(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* frames,
                            uint64_t frame_stride, uint32_t* count, double* mean, double* m2, double* var, double var_one);

/* Test hooks: what rp_render_tiles_device_ws launches with (raytracing-potato_amd/csrc/rp_schedule.h
 * rps::plan_tiles_launch, the header librp.so's rp_tiles.hip calls), in the pattern of rph_plan_launch and rph_unit_walk
 * for a whole-frame params given field by field (shard 0 of 1, interleave).  rph_plan_tiles_launch fills the
 * rph_launch_plan of a launch over n_listed tiles (n_shard_tiles = n_listed; plan_block 1, gather_stride and block_words
 * 0: no gather), and returns the launch's own refusal.  rph_tiles_unit_walk runs rp_units.h's fetch on the CPU with the
 * list `tiles` (n_listed entries) as the launch's tile map: units, units_cap, n_units, queue_words and entries as
 * rph_unit_walk's.  An entry at or above the frame's tile count must simply yield no unit; one at or above 2^31 ends the
 * walk with RP_EINVAL (the fetch's division). */
int rph_plan_tiles_launch(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                          uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_listed, uint32_t n_frames,
                          uint32_t frame_order, uint32_t unit_queues, uint32_t queue_chunk, uint64_t lanes,
                          rph_launch_plan* out);
int rph_tiles_unit_walk(uint32_t width, uint32_t height, uint32_t spp, uint32_t max_bounce, uint32_t tile_w,
                        uint32_t tile_h, uint32_t samples_per_stream, uint32_t n_frames, uint32_t frame_order,
                        uint32_t unit_queues, uint32_t queue_chunk, const uint32_t* tiles, uint32_t n_listed,
                        uint32_t n_blocks, uint32_t* units, uint64_t units_cap, uint64_t* n_units, uint32_t* queue_words,
                        uint32_t* entries);

/* The CPU model of the refit (include/rp.h rp_scene_refit_device; raytracing-potato_amd/csrc/rp_refit.h, the header
 * the device kernels compile): the plan, the primitive pass and the levels, in place on records laid out as
 * rp_scene_tree returns them -- nodes: n_nodes Node4 (RP_NODES_F32) or Node4Q (RP_NODES_Q8) records, pads included;
 * prims (80 B each) and refs (16 B each): n_prims of each in leaf order, the always-tested tail included; tri_normals
 * (72 B each, nullable unless normals are given): the per-primitive normals.  positions, normals (3 doubles per vertex,
 * n_vertices of them) and spheres (4 doubles each, n_spheres of them) as rp_scene_refit_device takes them, each nullable;
 * bound: the coordinate bound B; status: one word, RP_REFIT_OUT_OF_BOUND or 0.  RP_EINVAL: the device's refusals
 * (RP_NODES_W8, all inputs NULL, geometry named in part, a NULL status), and -- what the device cannot see -- fewer
 * vertices than the triangles name, or a sphere count that is not the scene's; records that are no tree (an index out of
 * range, a node reached twice).  Nothing is written by a refused call. */
int rph_refit_records(uint32_t node_format, void* nodes, uint64_t n_nodes, uint32_t root, void* prims, const void* refs,
                      void* tri_normals, uint64_t n_prims, const double* positions, const double* normals,
                      const double* spheres, uint64_t n_vertices, uint64_t n_spheres, double bound, uint32_t* status);
/* The plan alone: levels_out (nullable, n_nodes words) a node's level -- 0 without inner children, else 1 + the highest
 * among them; 0xFFFFFFFF for a record that is not reachable from root (a pad) --, order_out (nullable, n_nodes words)
 * the reachable nodes sorted by (level, index), then 0xFFFFFFFF, and *n_levels the number of levels. */
int rph_refit_plan(uint32_t node_format, const void* nodes, uint64_t n_nodes, uint32_t root, uint32_t* levels_out,
                   uint32_t* order_out, uint32_t* n_levels);
/* The host builder's own tree of `before` (node_format, always_max, always_minor as rph_bvh_selfcheck_opt) refit to the
 * geometry of `after` -- the same hittables over the same meshes' triangles, only positions, normals, centres and radii
 * may differ (else RP_EINVAL) -- with the bound of both geometries, then held to the builder's check() against the
 * after-geometry: RP_EINTERNAL with check's message when the refit tree fails it.  hashes (nullable, 2 values): FNV-1a
 * of the node, primitive, reference and normal records before and after the refit (equal when after == before);
 * status: the refit's status word. */
int rph_bvh_refit_check(const rp_scene_desc* before, const rp_scene_desc* after, uint32_t node_format, int32_t always_max,
                        uint32_t always_minor, uint64_t* hashes, uint32_t* status);

const char* rph_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
