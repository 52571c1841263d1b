/*
 * rp.h -- C-ABI of the MI355X path-tracing hot path (librp.so).
 *
 * Drop-in boundary for alucas2/raytracing-potato ("scaling-potato", crate raytracing2).
 * The reference has no FFI; its seam is the per-pixel worker loop
 *   main.rs:61-92  (make_uv_jitter -> Camera::shoot -> trace_path -> accumulate -> average)
 * calling
 *   render.rs:94-146 trace_path / trace_path_first / trace_path_continue
 * over the scene types
 *   hittable.rs:10-15 (Hittable), mesh.rs:18-22 (Mesh), material.rs:19-91 (Scatter/Emit/Absorb/Material),
 *   texture.rs:10-18 (Texture), render.rs:10-25 (SceneData, Camera).
 * rp_render() replaces that whole per-pixel loop for one frame (or one shard of it); the host keeps
 * scene construction, OBJ/TGA loading and image output (example_scenes.rs, mesh.rs:145, image.rs:73,116).
 *
 * Conventions
 *   - Plain C types only; no HIP/C++ types or exceptions cross this boundary.
 *   - Every function returning int returns RP_OK (0) or a negative rp_status; rp_last_error() gives a
 *     thread-local message for the last failure on the calling thread.  Nothing aborts or panics.
 *   - Ownership: the caller owns every buffer it passes.  rp_scene_create deep-copies the scene into
 *     device memory (HBM); afterwards only a refit (rp_scene_refit_device, below) changes it: the geometry
 *     moves, everything else stays.
 *   - Determinism (the RNG contract): the samples of pixel (i, j) are drawn in batches of
 *     N = params.samples_per_stream (0 -> RP_SAMPLES_PER_STREAM = 32); batch b (samples N*b .. N*b+N-1)
 *     is rendered with its own StdRng::seed_from_u64(params.seed + b*width*height + j*width + i)
 *     (rand 0.8 StdRng = ChaCha12) and the unchanged per-pixel body of main.rs:70-85 over its samples
 *     (make_uv_jitter from a clone of the batch stream's start).  The pixel value is (S_0 + S_1 + ...) /
 *     spp, batch sums added in batch order (main.rs:80,86).  With N >= spp (e.g. samples_per_stream =
 *     spp) this is SURVEY.md 8c's one stream per pixel, seed + j*width + i, for any spp.  Output depends
 *     only on (scene, camera, seed, width, height, spp, max_bounce, samples_per_stream) -- never on
 *     tiling, sharding, device count, scheduling or the environment.  (The reference draws every pixel of
 *     a worker's tiles from one from_entropy() stream, main.rs:52, so its output is not reproducible; a
 *     pixel's samples are sequential in a stream, so batching them is what lets one pixel's work spread
 *     over lanes/GPUs: the default 32 keeps an 8-GPU shard's longest unit short.)
 *   - No allocation happens inside the asynchronous calls (rp_render_device*, rp_frame_gather,
 *     rp_render_gather): device memory they need is reserved up front (rp_workspace_reserve), so they
 *     can be captured into a hipGraph and never synchronise the device.
 *   - Arithmetic is IEEE binary64 throughout, as the reference (utility.rs:14 `type Real = f64`).
 *   - Image layout: row-major, pixel (i, j) at index j*width + i, row j = 0 is the BOTTOM row
 *     (image.rs:31-33, main.rs:119, tga::save writes bottom-left origin).  RGB are linear f64 averages
 *     (main.rs:86), i.e. before to_srgb_u8 (utility.rs:212).
 */
#ifndef RP_H
#define RP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_ABI_VERSION 9

/* Default samples per RNG stream (see "Determinism" above; rp_render_params.samples_per_stream = 0). */
#define RP_SAMPLES_PER_STREAM 32

/* Device counter block of the asynchronous renders: RP_COUNTERS_LEN uint64 {rays, samples, pixels,
 * status}.  Nothing else is written through the pointer (the unit queue lives in the workspace). */
#define RP_COUNTERS_LEN 4
enum { RP_CTR_RAYS = 0, RP_CTR_SAMPLES = 1, RP_CTR_PIXELS = 2, RP_CTR_STATUS = 3 };
/* status bits (OR-ed over the ranks of a frame gather, never summed) */
#define RP_STATUS_STACK_OVERFLOW 1u  /* a lane's traversal stack overflowed (entries dropped: the frame is wrong) */
#define RP_STATUS_PLAN_MISMATCH 2u   /* ranks of a balanced frame made different tile plans (frame invalid) */

/* Bytes of an RCCL unique id (rp_comm_unique_id). */
#define RP_COMM_ID_BYTES 128

typedef enum rp_status {
  RP_OK = 0,
  RP_EINVAL = -1,    /* bad argument / malformed scene (the reference would panic: index out of range, etc.) */
  RP_EHIP = -2,      /* HIP runtime error */
  RP_ENOMEM = -3,    /* host or device allocation failed */
  RP_ENODEV = -4,    /* no usable gfx950 device */
  RP_EINTERNAL = -5, /* kernel reported an internal error (e.g. traversal stack overflow) */
  RP_ERCCL = -6      /* RCCL (collective communication) error */
} rp_status;

/* ---------------------------------------------------------------- scene description ----------- */

/* hittable.rs:10-15.  List/Bvh aggregates are expressed by rp_scene_desc.root_kind. */
enum { RP_HITTABLE_SPHERE = 0, RP_HITTABLE_TRIANGLE = 1 };

typedef struct rp_hittable {
  uint32_t kind;       /* RP_HITTABLE_* */
  uint32_t material;   /* Sphere {material: MaterialId} */
  uint32_t mesh;       /* Triangle {mesh: MeshId} */
  uint32_t triangle;   /* Triangle {triangle: TriangleId} = offset of the first of 3 indices (mesh.rs:33) */
  double center[3];    /* Sphere {center} */
  double radius;       /* Sphere {radius} */
} rp_hittable;

/* mesh.rs:7-22: Vertex {position, normal, uv} stored as three interleaved arrays. */
typedef struct rp_mesh {
  uint32_t n_vertices;
  uint32_t n_indices;      /* multiple of 3 */
  const double* positions; /* 3 * n_vertices (x, y, z per vertex) */
  const double* normals;   /* 3 * n_vertices */
  const double* uvs;       /* 2 * n_vertices */
  const uint32_t* indices; /* n_indices */
  uint32_t material;       /* Mesh.material (MaterialId) */
  uint32_t reserved;
} rp_mesh;

/* material.rs:19-24 */
enum { RP_SCATTER_NONE = 0, RP_SCATTER_LAMBERT = 1, RP_SCATTER_METAL = 2, RP_SCATTER_DIELECTRIC = 3 };
/* material.rs:66-71 */
enum { RP_ABSORB_BLACK_BODY = 0, RP_ABSORB_WHITE_BODY = 1, RP_ABSORB_ALBEDO = 2, RP_ABSORB_ALBEDO_MAP = 3 };
/* material.rs:40-46 */
enum { RP_EMIT_NONE = 0, RP_EMIT_DEBUG_NORMALS = 1, RP_EMIT_COLOR = 2, RP_EMIT_SKY_GRADIENT = 3,
       RP_EMIT_SKY_SPHERE = 4 };
/* texture.rs:10-18 */
enum { RP_TEXTURE_MISSING = 0, RP_TEXTURE_DEBUG_UVS = 1, RP_TEXTURE_SOLID = 2, RP_TEXTURE_IMAGE = 3,
       RP_TEXTURE_CHECKER = 4, RP_TEXTURE_NOISE = 5, RP_TEXTURE_PERLIN = 6 };

typedef struct rp_scatter {
  uint32_t kind;       /* RP_SCATTER_* */
  uint32_t reserved;
  double param;        /* Metal {fuzziness} | Dielectric {refraction_index} */
} rp_scatter;

typedef struct rp_absorb {
  uint32_t kind;       /* RP_ABSORB_* */
  uint32_t texture;    /* AlbedoMap(TextureId) */
  double color[3];     /* Albedo(Color) */
} rp_absorb;

typedef struct rp_emit {
  uint32_t kind;       /* RP_EMIT_* */
  uint32_t texture;    /* SkySphere(TextureId) */
  double color[3];     /* Color(Color) */
} rp_emit;

/* material.rs:87-91; evaluation order scatter -> absorb -> emit (material.rs:104-110) */
typedef struct rp_material {
  rp_scatter scatter;
  rp_absorb absorb;
  rp_emit emit;
} rp_material;

typedef struct rp_texture {
  uint32_t kind;         /* RP_TEXTURE_* */
  uint32_t odd, even;    /* Checker {odd, even} (TextureId) */
  uint32_t width, height;/* Image: Array2d<[u8;4]> dimensions */
  uint32_t reserved;
  int64_t seed;          /* Noise {seed} | Perlin {seed} (isize) */
  double color[3];       /* Solid(Color) */
  const uint8_t* rgba;   /* Image: width*height*4 bytes, texel (i, j) at 4*(i + j*width), j = 0 bottom row */
} rp_texture;

enum { RP_ROOT_BVH = 0, RP_ROOT_LIST = 1 };

/* render.rs:10-14 SceneData + example_scenes.rs:14-19 root/background. */
typedef struct rp_scene_desc {
  uint32_t root_kind;                  /* Hittable::Bvh (any tree shape) or Hittable::List */
  uint32_t n_hittables;
  const rp_hittable* hittables;
  uint32_t n_meshes;
  const rp_mesh* meshes;
  uint32_t n_materials;
  const rp_material* materials;
  uint32_t n_textures;
  const rp_texture* textures;
  rp_emit background;
} rp_scene_desc;

/* render.rs:19-25 + utility.rs:160-163.  orientation is column-major as nalgebra's Matrix3
 * (columns x, y, z of Transformation::lookat, utility.rs:172-177). */
typedef struct rp_camera {
  double aspect_ratio, fov, focal_dist, lens_radius;
  double orientation[9];
  double position[3];
} rp_camera;

/* One frame (or one shard of it).  The frame is cut into tile_w x tile_h tiles in row-major tile
 * order (image.rs:151-167), and the tiles are dealt to the S shards (GPUs) by shard_map:
 *   RP_SHARD_INTERLEAVE: shard s renders tiles t with t % S == s, its k-th tile is t = s + k*S.
 *   RP_SHARD_BALANCED: a tile plan deals them by cost.  The render of a shard first traces a cost probe of the
 *     WHOLE frame (sample 0 of a lattice of pixels per tile, traversal work counted without any dependence on
 *     the scheduling, so every rank measures the same costs) and deals the tiles, costliest first, in rounds of
 *     S alternating direction; shard s's k-th tile is the deal order's entry s + k*S.  Every shard holds exactly
 *     the interleave's number of tiles (same buffer sizes and gather strides), and every rank computes the same
 *     plan (the frame gather compares their hashes: RP_STATUS_PLAN_MISMATCH).  The plan lives in the workspace of
 *     the render; rp_workspace_tile_map returns it.  Frames of more than 16384 tiles are dealt as the interleave.
 * Neither choice changes a pixel (per-pixel seeding): only which GPU renders it. */
enum { RP_SHARD_INTERLEAVE = 0, RP_SHARD_BALANCED = 1 };
typedef struct rp_render_params {
  uint32_t width, height;   /* Multisampler {width, height} */
  uint32_t spp;             /* Multisampler {num_samples} */
  uint32_t max_bounce;      /* trace_path depth (main.rs:25); >= 1 (render.rs:97) */
  uint64_t seed;            /* base seed of the RNG contract */
  uint32_t tile_w, tile_h;  /* 0 -> 32 (main.rs:26) */
  uint32_t shard, num_shards;/* num_shards 0 -> 1 */
  uint32_t samples_per_stream; /* RNG contract batch size N, 0 -> RP_SAMPLES_PER_STREAM; N >= spp: one
                                  stream per pixel */
  uint32_t shard_map;       /* RP_SHARD_INTERLEAVE (0) or RP_SHARD_BALANCED */
} rp_render_params;
/* A shard holds at most 2^31 - 1 (pixel, sample stream) units -- its pixels x ceil(spp / samples_per_stream) -- and
 * with the default per-XCD unit queues half the 32-bit queue word less the resident lanes; larger shards are refused
 * with RP_EINVAL (e.g. 8192 x 8192 pixels at 1024 spp: split the frame into shards). */

/* Scene build and kernel tuning options (rp_scene_create_ex).  None of them changes an image beyond
 * exact-t ties between primitives (the closest hit does not depend on the tree).
 * Zero-initialised fields take the defaults; rp_scene_options_init fills them in explicitly. */
/* Builders: HOST = multi-threaded binned SAH on the CPU; DEVICE = LBVH on the GPU (Karras 2012: fastest build,
 * Morton-split tree); PLOC = agglomerative clustering on the GPU (Meister & Bittner 2018: SAH-quality tree). */
enum { RP_BUILDER_AUTO = 0, RP_BUILDER_HOST = 1, RP_BUILDER_DEVICE = 2, RP_BUILDER_PLOC = 3 };
/* Wide-node formats: 128 B f32 child boxes, or 64 B child boxes quantized to 8 bits per plane in a per-node
 * f32 frame (half the node bytes, more ALU per visit).  AUTO = Q8 for host-built trees of >= 2^21 hittables,
 * F32 otherwise. */
enum { RP_NODES_AUTO = 0, RP_NODES_F32 = 1, RP_NODES_Q8 = 2, RP_NODES_W8 = 3 };
/* Tile orders: PLAIN = shard order (row-major); COST = the costliest tiles go first (short frame tail), by the
 * workspace's learned costs of the previous frame (see rp_workspace_tile_costs) or, without them, by a probe
 * launch that traces sample 0 of a lattice of pixels per tile; PROBE = COST always from the probe; MORTON = Z-order
 * of the tiles (neighbouring tiles run together: a small cache working set; a balanced multi-GPU plan then deals
 * square blocks of tiles).  AUTO = COST (round 4; rounds 2-3: MORTON for scenes past the 256 MB Infinity Cache). */
enum { RP_TILES_AUTO = 0, RP_TILES_PLAIN = 1, RP_TILES_COST = 2, RP_TILES_MORTON = 3, RP_TILES_PROBE = 4 };
/* Unit queues: SINGLE = one device-wide queue over the tile order; XCD_TILES = eight queues, one per group of
 * render blocks sharing an XCD (and its L2), tile k of the order served by queue k mod 8 (a tile's pixels
 * run on one XCD); XCD_REGIONS = queue g serves the g-th eighth of the tile order (a compact region per XCD
 * under Z-order).  A drained queue's blocks take units from the others.  AUTO = XCD_TILES. */
enum { RP_QUEUES_AUTO = 0, RP_QUEUES_SINGLE = 1, RP_QUEUES_XCD_TILES = 2, RP_QUEUES_XCD_REGIONS = 3 };
/* How the binary SAH tree is collapsed into 4-wide nodes (host builder; ABI v6): AUTO = SAH; GREEDY opens the child
 * of largest surface area until a node has 4 children; SAH takes the cut through the binary subtree that minimises
 * the 4-wide tree's SAH cost (dynamic program).  Never changes an image beyond exact-t ties. */
enum { RP_COLLAPSE_AUTO = 0, RP_COLLAPSE_GREEDY = 1, RP_COLLAPSE_SAH = 2 };
/* rp_scene_options.node_layout (ABI v7): the memory order of a device-built (PLOC) tree's wide nodes.  DFS: depth-first,
 * a node's inner children as one consecutive family; DFS_LINE: the same with every family starting on a 128-B cache
 * line (64-B quantized nodes: a pad slot after odd families; f32 nodes are one line each, so the same as DFS).  Speed
 * only: the image never depends on it. */
enum { RP_LAYOUT_AUTO = 0, RP_LAYOUT_DFS = 1, RP_LAYOUT_DFS_LINE = 2 };
/* rp_scene_options.unit_order (ABI v8): the order the unit queues hand out a shard's (pixel, sample stream) units.
 * TILES: tile by tile (tile_order), a tile's pixels row-major.  LEARNED: every render of one frame per launch stores each
 * unit's duration, and the next such frame of the same shape on the same workspace hands out its units longest first
 * (log-spaced buckets, shard order inside; a frame ends with its longest unit), on one device or interleaved shards (a
 * balanced plan's tiles may move between frames: those frames keep TILES).  AUTO (ABI v9) = LEARNED for one stream per
 * pixel (samples_per_stream >= spp: lone C3 frames 220 vs 261 ms), TILES for several streams per pixel (32-sample streams:
 * +4.4 %) and for launches of several frames (their interleaved tile order, rp_render_frames_device_ws);
 * LEARNED also orders such launches, a unit's frames handed out together.  Results never depend on it. */
enum { RP_UNITS_AUTO = 0, RP_UNITS_TILES = 1, RP_UNITS_LEARNED = 2 };
typedef struct rp_scene_options {
  uint32_t builder;         /* RP_BUILDER_*: AUTO = HOST (multi-threaded binned SAH); DEVICE = LBVH (faster
                               build, ~24 % slower traversal on 10 M triangles); PLOC */
  uint32_t max_leaf;        /* primitives per leaf, 1..8 (0 -> 4) */
  double cost_traverse;     /* SAH node cost relative to a primitive test (0 -> 0.7) */
  int32_t always_max;       /* most primitives tested before the tree for every ray: giant ones and, in a mesh scene with no more than this many, its spheres (-1 -> 4; 0 = none) */
  uint32_t lds_depth;       /* traversal-stack entries kept in LDS (0 -> automatic; >= 8 forces a split) */
  uint32_t self_check;      /* 1: structural self-check of a device-built tree (slow; tests) */
  uint32_t trav_threshold;  /* lanes of a wave still traversing before the finished ones shade (0 -> 24 for
                               scenes within the 256 MB Infinity Cache, 32 above; 1..64) */
  uint32_t tile_order;      /* RP_TILES_*: the order the unit queue hands out a shard's tiles */
  uint32_t probe_n;         /* cost probe lattice n x n per tile (0 -> 16) */
  uint32_t node_format;     /* RP_NODES_* */
  uint32_t leaf_break;      /* speculative traversal: a wave moves to the leaf tests once at most this many of its
                               lanes still look for a leaf (0 -> 8 for scenes within the 256 MB Infinity Cache,
                               16 above; 1..64) */
  uint32_t unit_queues;     /* RP_QUEUES_*: how the render blocks share out the units */
  uint32_t queue_chunk;     /* XCD_TILES: consecutive tiles of the order dealt to one queue at a time (0: up to 8 while
                               every queue gets >= 16 chunks; a launch of n interleaved frames: rounded up to a multiple
                               of n, whole tiles of every frame) */
  uint32_t debug_stack_depth; /* TESTS ONLY (0 = off): traversal-stack entries per lane, 8..4096, instead of the
                               depth the tree needs.  Too small a stack drops entries -- wrong frames -- and the
                               render reports RP_STATUS_STACK_OVERFLOW / RP_EINTERNAL: the error path made reachable. */
  uint32_t collapse;        /* RP_COLLAPSE_*: the 4-wide collapse of the host-built tree (ABI v6) */
  uint32_t node_layout;     /* RP_LAYOUT_*: node order of a device-built (PLOC) tree (ABI v7) */
  uint32_t unit_order;      /* RP_UNITS_*: tile order or the learned per-unit order (ABI v8) */
} rp_scene_options;
/* ABI v9 removed the measured-and-lost options of v5-v8: `engine` / `wf_slots` (the stage-split
 * engine) and `primary` (the coherent primary pass). */

typedef struct rp_stats {
  uint64_t rays;      /* root scene.hit() calls, primary + secondary (render.rs:105,133) */
  uint64_t samples;   /* camera samples traced */
  uint64_t pixels;    /* pixels written */
  double seconds;     /* device time of the render (HIP events) */
} rp_stats;

typedef struct rp_scene rp_scene;   /* opaque: device-resident scene + acceleration structure */
typedef struct rp_workspace rp_workspace;  /* opaque: per-frame device state of a render (see below) */

/* Library / device queries.  rp_build_id: a hash of the machine code that decides a frame's per-ray work -- the render
 * kernel, the tree builders and the scheduling code -- this library was built from (profile records of the kernel carry
 * it; a record of another build is stale). */
int rp_abi_version(void);
const char* rp_build_id(void);
const char* rp_last_error(void);
int rp_device_count(int* count);

/* Build the acceleration structure and copy the scene to device `device`.  Validates every index the
 * reference would bounds-check (material/mesh/texture ids, triangle offsets, checker recursion).
 * rp_scene_create uses the default options; the library reads no environment variables. */
int rp_scene_create(const rp_scene_desc* desc, int device, rp_scene** out);
int rp_scene_options_init(rp_scene_options* opt);
int rp_scene_create_ex(const rp_scene_desc* desc, int device, const rp_scene_options* opt, rp_scene** out);
void rp_scene_destroy(rp_scene* scene);
/* Acceleration-structure statistics: node count, leaf count, max depth, primitive count. */
int rp_scene_info(const rp_scene* scene, uint64_t* n_nodes, uint64_t* n_leaves, uint32_t* max_depth,
                  uint64_t* n_prims, uint64_t* device_bytes);

/* Host wall-clock seconds of rp_scene_create's phases: {validation, host tree (or the shading tables alone for a
 * device build), device builder input (primitive records and boxes), device build (or the host tree's upload),
 * vertex/shading tables upload, workspace}.  RP_BUILD_PHASES values; n may be smaller. */
#define RP_BUILD_PHASES 6
int rp_scene_build_times(const rp_scene* scene, double* seconds, uint32_t n);

/* Number of pixels in shard params->shard (the length of the compact shard buffer). */
int rp_shard_pixel_count(const rp_render_params* params, uint64_t* count);
/* Scatter a compact shard buffer (shard order: its tiles in deal order k = 0, 1, ..., row-major inside a
 * tile) into a full frame; `channels` values per pixel.  RP_SHARD_INTERLEAVE frames only (a balanced frame is
 * refused with RP_EINVAL): rp_shard_unpack_map takes the deal order of a balanced frame (rp_workspace_tile_map;
 * NULL = the interleave). */
int rp_shard_unpack(const rp_render_params* params, const double* shard_buf, uint32_t channels,
                    double* frame);
int rp_shard_unpack_map(const rp_render_params* params, const uint32_t* tile_map, const double* shard_buf,
                        uint32_t channels, double* frame);

/* Render synchronously into host memory.  out_rgb: width*height*3 doubles (only the shard's pixels are
 * written).  out_foreground (nullable): width*height floats, fraction of samples whose first ray hit
 * geometry (main.rs:81-87).  stats nullable.  Reserves the scene workspace for params as needed. */
int rp_render(rp_scene* scene, const rp_camera* camera, const rp_render_params* params,
              double* out_rgb, float* out_foreground, rp_stats* stats);

/* Asynchronous device-resident render on `stream` (a hipStream_t, NULL = default stream) of the scene's
 * device.  d_shard_rgb: shard_pixel_count*3 doubles in device memory, compact shard order.
 * d_shard_fg (nullable): shard_pixel_count floats.  d_counters (nullable): RP_COUNTERS_LEN uint64 in
 * device memory that receive {rays, samples, pixels, status}; they are zeroed on the stream before the
 * launch.  No host synchronisation, copy or allocation happens inside.  A frame of more than one sample
 * batch (spp > samples_per_stream) keeps 3 doubles + 1 uint32 per pixel and batch in the workspace:
 * reserve them first (rp_workspace_reserve), else the call returns RP_EINVAL. */
int rp_render_device(rp_scene* scene, const rp_camera* camera, const rp_render_params* params,
                     double* d_shard_rgb, float* d_shard_fg, uint64_t* d_counters, void* stream);

/* Frames in flight.  A render's per-frame device state -- the keystream cache of the resident lanes,
 * the unit queues, the cost-probe and tile-order buffers, the multi-batch sums, the gather staging of
 * rp_frame_gather -- lives in a workspace.  The scene owns one, which rp_render and rp_render_device use
 * (their frames must therefore be ordered on one stream).  Frames rendered with different workspaces may
 * run concurrently on different streams: the end of one frame, when its last units leave most of the GPU
 * idle, then overlaps the start of the next.  A workspace serves one frame at a time (the caller orders
 * its reuse on streams); destroy workspaces before their scene.  Same arguments and results as
 * rp_render_device. */
int rp_workspace_create(rp_scene* scene, rp_workspace** out);
void rp_workspace_destroy(rp_workspace* workspace);
int rp_render_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_camera* camera,
                        const rp_render_params* params, double* d_shard_rgb, float* d_shard_fg,
                        uint64_t* d_counters, void* stream);
/* Reserve the device memory renders of `params`' shape need in `workspace` (NULL = the scene's own):
 * the multi-batch sums of the shard and, when params->num_shards > 1, the staging buffers rp_frame_gather
 * uses for this frame size.  Synchronous (allocates; may free a smaller reservation); idempotent for a
 * shape it already covers.  rp_render reserves for itself. */
int rp_workspace_reserve(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params);
/* Scheduling costs.  Every render of the megakernel measures its units' durations per tile; a workspace that
 * rendered a whole frame on one device (num_shards = 1), or gathered one with rp_frame_gather, keeps them as a
 * learned per-tile cost table, and its next frame of the same geometry orders its tiles -- and deals them
 * (RP_SHARD_BALANCED) -- from that table instead of tracing a cost probe.  A balanced plan over N ranks only uses a
 * table gathered from N ranks (identical bytes on every rank, hence identical plans).  Callers that move shards
 * with their own collective get a render's measured costs with rp_workspace_tile_costs (2 x the shard's tile
 * count: summed unit durations per shard tile, then the longest unit; synchronises the device) and install a
 * frame's table, assembled through the deal order, with rp_workspace_set_tile_costs (2 x the frame's tile count:
 * sums, then longest units, by frame tile; `ranks` = how many ranks' renders it combines).  Results never
 * depend on any of it. */
int rp_workspace_tile_costs(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                            uint32_t* costs, uint32_t n);
int rp_workspace_set_tile_costs(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                                const uint32_t* costs, uint32_t ranks);
/* Several frames in ONE persistent launch (ABI v8).  Frame f = 0 .. n_frames - 1 is exactly the frame of `params` with
 * its sample batches numbered f * B .. f * B + B - 1, B = ceil(spp / samples_per_stream) -- i.e. the frame rp_render_device
 * renders with params.seed + f * B * width * height (the RNG contract's seeds of batches past the frame's own): n_frames
 * independent frames of the same scene, camera and sampling.  The queues hand out the frames' units one frame after
 * the other, so the lanes a frame's tail leaves take the next frame's units at once instead of idling in sparse waves
 * (a frame's tail: ~4 % of a C3 frame, ~20 % of an 8-way C3 shard).  d_shard_rgb holds n_frames shard
 * buffers back to back (3 x rp_shard_pixel_count doubles each), d_shard_fg (nullable) n_frames x pixel count floats;
 * d_counters: the n_frames frames' counts summed (status bits OR-ed).  The workspace must be reserved for n_frames
 * (rp_workspace_reserve_frames; it also reserves what rp_workspace_reserve does).  The shard's tiles (a balanced plan)
 * and their order are made once for the launch: from the workspace's learned cost table, or from a probe of frame 0 --
 * a probed plan follows its seed, so a balanced shard of frame f > 1 may hold other tiles than rp_render_device's frame
 * of that seed would (the pixels are the same; rp_workspace_tile_map gives the launch's deal).  n_frames <= RP_MAX_FRAMES.
 * frame_order (RP_FRAME_ORDER_*): SEQUENTIAL hands out frame 0's units, then frame 1's, ...; INTERLEAVED hands out the
 * frames' k-th tiles of the cost order together, for k = 0, 1, ... -- the units in flight at any moment come from a
 * narrower band of the cost order (fewer lanes idle in a wave whose neighbours run longer paths), every frame ends near
 * the launch's end.  PIXEL (ABI v9) is INTERLEAVED with a tile's units handed out pixel by pixel, each pixel's frames
 * consecutive (a wave holds a few pixels x their frames).  AUTO = INTERLEAVED.  The frames' pixels do not depend on it. */
#define RP_MAX_FRAMES 64
enum { RP_FRAME_ORDER_AUTO = 0, RP_FRAME_ORDER_SEQUENTIAL = 1, RP_FRAME_ORDER_INTERLEAVED = 2, RP_FRAME_ORDER_PIXEL = 3 };
int rp_workspace_reserve_frames(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                                uint32_t n_frames);
int rp_render_frames_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_camera* camera,
                               const rp_render_params* params, uint32_t n_frames, uint32_t frame_order,
                               double* d_shard_rgb,
                               float* d_shard_fg, uint64_t* d_counters, void* stream);
/* How the last render enqueued with `workspace` (NULL = the scene's) was scheduled (ABI v8): RP_FRAME_* bits (0 after
 * a render that launched nothing: spp = 0, an empty shard, a refused call).  Host state only (no device
 * synchronisation); results never depend on any of it.  (Bit 1 belonged to the coherent primary pass, removed in v9.) */
enum {
  RP_FRAME_LEARNED_ORDER = 2, /* tiles ordered / dealt from the workspace's learned cost table */
  RP_FRAME_PROBED = 4,        /* a cost probe launch ran */
  RP_FRAME_UNIT_ORDER = 8     /* units handed out in the learned per-unit order (rp_scene_options.unit_order) */
};
int rp_workspace_frame_info(const rp_scene* scene, const rp_workspace* workspace, uint32_t* flags);
/* Inspection of the learned per-unit order (ABI v9; tests and tools): the last render with `workspace` (NULL = the
 * scene's) stored each of its units' durations in 100 MHz ticks -- unit u = slot * nbatch + batch in shard order --
 * when it could learn them (one frame per launch, unit_order LEARNED or AUTO with one stream per pixel, a reserved
 * workspace), and handed its units out in `order` when its frame_info has RP_FRAME_UNIT_ORDER.  Copies n entries of each
 * (NULL = skip) to the host; n must not exceed the workspace's reservation.  Synchronises the device. */
int rp_workspace_unit_order(rp_scene* scene, rp_workspace* workspace, uint32_t* durations, uint32_t* order, uint64_t n);
/* The deal order of params' frame (one entry per frame tile; shard s's k-th tile is tile_map[s + k*num_shards]):
 * for RP_SHARD_BALANCED the plan the last render of this frame in `workspace` (NULL = the scene's) made, for the
 * interleave 0, 1, 2, ...  n >= the frame's tile count.  Synchronises the device. */
int rp_workspace_tile_map(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                          uint32_t* tile_map, uint32_t n);

/* First-hit feature pass: the noiseless guide buffers a denoiser or compositor takes beside the beauty frame
 * (render.rs:101 "the first ray of the path tracing provides additional noiseless data like albedo and normal";
 * PathTraceOutput::normal, render.rs:87-91, zero on a miss at :119).  A pass of its own beside the render, which it
 * never changes.
 *   Definition.  The pass traces camera rays only.  Sample k = 0 .. spp-1 of pixel (i, j) is the first camera sample
 *   of the stream StdRng::seed_from_u64(seed + k*width*height + j*width + i): its uv jitter is the first two draws of a
 *   clone of that stream (render.rs:74-82), Camera::shoot then draws its UnitDisk from the stream's start
 *   (render.rs:32-52, drawn even at lens_radius == 0), and root.hit(ray) follows with t_min = 1e-3, t_max = +inf.  That
 *   is exactly sample 0 of batch k of the RNG contract at samples_per_stream = 1: beside a beauty frame rendered with
 *   samples_per_stream = 1 the buffers describe the very same camera rays; under any other contract sample 0 is the same
 *   ray and the rest are fresh camera rays of the same distribution -- what a guide buffer needs.
 *   params.samples_per_stream and params.max_bounce are ignored.
 *   Every buffer is (sum over k of [sample k hit ? x_k : 0]) / (double)spp, the sum started at 0.0 and added in k
 *   order (the batch order of the contract; a miss adds the reference's zero):
 *     normal (3 f64)  hit.normal as Hittable::hit returns it (a triangle's interpolated normal is not normalised, and
 *                     never flipped towards the ray);
 *     albedo (3 f64)  material.absorb.evaluate(ray, hit) (material.rs:74-81: BlackBody, WhiteBody, Albedo, AlbedoMap
 *                     over every texture kind), evaluated whether or not the material scatters;
 *     depth  (1 f64)  hit.t;
 *     fg     (1 f32)  (float)((double)hits / spp), as rp_render's foreground.
 *   spp = 0: every value is 0 / 0 = NaN, as rp_render's.
 * rp_render_aov_device_ws: asynchronous on `stream`, never allocates or synchronises (capturable, like
 * rp_render_device).  Every output is nullable (all four NULL: RP_EINVAL); each is a compact shard buffer in device
 * memory, rp_shard_pixel_count slots of 3, 3, 1 doubles and 1 float, in the render's shard order (a buffer that is not
 * asked for costs nothing: without albedo no texture is read).  d_counters (nullable): RP_COUNTERS_LEN uint64, zeroed
 * on the stream, then {rays = samples = spp x the shard's pixels, pixels, status}.  params.shard, num_shards, tile_w and
 * tile_h are honoured.  RP_SHARD_INTERLEAVE always works; RP_SHARD_BALANCED uses the plan `workspace` (NULL = the
 * scene's) holds for this frame shape, so the shard holds the same tiles as the beauty shard rendered before it on that
 * workspace (the caller orders the two on streams), and without such a plan is RP_EINVAL.  The workspace is read for
 * nothing else.  spp = 0 or an empty shard launches no kernel and returns RP_OK.
 * rp_render_aov: the synchronous version into host memory; the buffers are full frames (width*height slots, only the
 * shard's pixels written, row 0 = bottom), like rp_render's.  stats (nullable): the counters and seconds = device time
 * of the pass (HIP events).  Any status bit returns RP_EINTERNAL.
 * Multi-GPU: gathered shards assemble with rp_frame_assemble[_ws] at words_per_slot = 6 (normal, albedo), 2 (depth) or
 * 1 (fg); on the host rp_shard_unpack[_map] unpacks normal, albedo (channels = 3) and depth (1). */
int rp_render_aov_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_camera* camera,
                            const rp_render_params* params, double* d_shard_normal, double* d_shard_albedo,
                            double* d_shard_depth, float* d_shard_fg, uint64_t* d_counters, void* stream);
int rp_render_aov(rp_scene* scene, const rp_camera* camera, const rp_render_params* params, double* out_normal,
                  double* out_albedo, double* out_depth, float* out_fg, rp_stats* stats);

/* Guided denoiser for low-spp frames: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) that
 * takes the beauty frame and the feature pass's noiseless guides (rp_render_aov) and returns a picture.  The reference
 * has none (render.rs:101 only leaves the hook), so the definition is this project's own; DESIGN.md 4.11.
 *   Buffers are FULL FRAMES IN FRAME ORDER: row-major, pixel (i, j) at j*width + i, row 0 = bottom, as
 *   rp_frame_assemble leaves them -- rgb, normal, albedo 3 doubles per pixel, depth 1, exactly as rp_render and
 *   rp_render_aov define them.  Everything is IEEE binary64, uses only + - * /, comparisons and max, and is evaluated
 *   in the order written here without contraction: the device, librp_host.so's rph_denoise and a numpy model agree to
 *   the last bit.
 *   Parameters: a zero field takes its default (rp_denoise_params_init fills them in), params = NULL means all defaults.
 *     iterations    3     L, 1..8
 *     normal_power  6     e_n, 1..8: the normal weight is cos^(2^e_n)
 *     sigma_depth   0.05  sigma_z   (> 0)
 *     sigma_albedo  0.1   sigma_a   (> 0)
 *     sigma_color   1.0   sigma_c; negative disables the colour term
 *     albedo_eps    1e-2  eps       (> 0)
 *   Per pixel: nn = (n.x*n.x + n.y*n.y) + n.z*n.z; c = rgb / (albedo + eps) per channel (demodulation);
 *   rat(x2) = 1 / ((1 + x2) * (1 + x2)).  Squared lengths and dot products are summed as nn is.
 *   Level l = 0 .. L-1 has step s = 2^l and colour scale sigma_c,l = sigma_c / 2^l.  For pixel p the taps run
 *   dy = -2..2 (outer), dx = -2..2 (inner), q = p + s*(dx, dy); a tap outside the frame is skipped;
 *   h = k[|dx|] * k[|dy|], k = {3/8, 1/4, 1/16}.
 *     w_n: d = n_p . n_q, ab = nn_p * nn_q; ab > 0 and d > 0: (d*d)/ab squared e_n - 1 times; else 0; centre tap: 1.
 *     w_z: m = max(|z_p|, |z_q|); x = m > 0 ? (z_p - z_q) / (sigma_z * m) : 0; w_z = rat(x*x).
 *     w_a = rat(|a_p - a_q|^2 / (sigma_a*sigma_a)).
 *     w_c = rat(|c_p - c_q|^2 / (sigma_c,l*sigma_c,l)) with c the level's input, or 1 when disabled.
 *     w = (((h * w_n) * w_z) * w_a) * w_c; sw += w and acc += w * c_q from 0.0 in tap order; c' = acc / sw.
 *   A pixel with nn == 0 (background, misses: its radiance is the emission itself) keeps its c through every level and
 *   is never a neighbour's tap (w_n = 0).  After the last level out = c * (albedo + eps); a pixel with nn == 0 gets rgb
 *   itself, bit for bit.  Missing guides: albedo NULL -- no demodulation, w_a = 1; normal NULL -- w_n = 1 and no
 *   pass-through; depth NULL -- w_z = 1.  NaN inputs propagate.
 *   Known limit: first-hit guides say nothing about what a mirror or a glass surface shows, so there sigma_c is the only
 *   edge stop, and on such frames at 16 spp the filter can lose to the noisy frame.
 * rp_denoise_device: asynchronous on `stream` on the CURRENT device (as rp_frame_assemble); one kernel launch per level,
 * no allocation and no synchronisation inside (capturable, like rp_render_device).  d_scratch: rp_denoise_scratch_bytes
 * bytes of device memory, 8-byte aligned (two colour buffers the levels ping-pong between; host only, needs no device).
 * d_out must not alias an input (nor scratch anything): RP_EINVAL, as are NULL rgb, out or scratch, a zero size, a side
 * above 65535 and parameters out of range.
 * rp_denoise: the synchronous version from and to host buffers on `device`; seconds (nullable) = device time of the
 * levels (HIP events). */
typedef struct rp_denoise_params {
  uint32_t iterations, normal_power;
  double sigma_depth, sigma_albedo, sigma_color, albedo_eps;
} rp_denoise_params;
int rp_denoise_params_init(rp_denoise_params* params);
int rp_denoise_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
int rp_denoise_device(const rp_denoise_params* params, uint32_t width, uint32_t height, const double* d_rgb,
                      const double* d_normal, const double* d_albedo, const double* d_depth, double* d_out,
                      void* d_scratch, void* stream);
int rp_denoise(const rp_denoise_params* params, int device, uint32_t width, uint32_t height, const double* rgb,
               const double* normal, const double* albedo, const double* depth, double* out, double* seconds);

/* Per-pixel variance from the batch sums: the variance of every pixel's mean, estimated from the spread of its sample
 * batches.  It costs no ray: a frame of more than one batch per pixel (spp > samples_per_stream) leaves every batch's
 * sample sum in its workspace, and this pass reads them there.  For error maps, stopping rules and rp_denoise_var.
 * DESIGN.md 4.12 has the derivation.
 *   Definition.  N = samples_per_stream (0: RP_SAMPLES_PER_STREAM), B = ceil(spp / N) batches, batch b holds
 *   n_b = min(N, spp - b*N) samples and S_b is the sum of its samples' radiance.  Per channel, in IEEE binary64, in the
 *   order written and without contraction:
 *     x   = (((0.0 + S_0) + S_1) + ...) / spp            -- rp_render's pixel, bit for bit
 *     e_b = S_b / spp - x * ((double)n_b / spp)
 *     acc = the sum of e_b * e_b from 0.0 in b order
 *     var = acc * ((double)B / (double)(B - 1))
 *   With equal batches e_b = (m_b - x) / B for the batch means m_b = S_b / N, and var = sum (m_b - x)^2 / (B (B - 1)):
 *   the unbiased estimate of the variance of the mean of B independent batch means.
 * rp_render_variance_device_ws reads the sums that the LAST render of `params` on `workspace` (NULL = the scene's) left
 * there -- rp_render_device[_ws] with one frame per launch; the caller orders the pass after that render on streams, and
 * before the workspace's next render.  d_shard_var: 3 doubles per slot in the render's compact shard order
 * (rp_shard_pixel_count slots); slots of edge tiles outside the frame are not written.  Asynchronous on `stream`, never
 * allocates or synchronises (capturable); an empty shard launches nothing.  params.shard, num_shards, tile_w, tile_h and
 * shard_map are honoured: a balanced shard uses the plan the beauty render left in the workspace, as rp_render_aov does.
 * RP_EINVAL: B < 2 (nothing to take a spread of), a workspace whose batch reservation (rp_workspace_reserve) does not
 * cover the shard's slots x B, a balanced shard without a plan, NULL d_shard_var.  The sums of a multi-frame launch
 * (rp_render_frames_device_ws) are not supported: rp_accum_frames_device takes the variance over such a launch's frames.
 * The shard buffer is laid out like the render's rgb: gathered shards assemble with rp_frame_assemble[_ws] at
 * words_per_slot = 6, and rp_shard_unpack[_map] unpacks it with channels = 3. */
int rp_render_variance_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                                 double* d_shard_var, void* stream);

/* Variance-guided denoiser: rp_denoise with the colour stop scaled by each pixel's measured noise instead of one
 * sigma_color.  Where a reflection or a sky seen through glass is deterministic the variance is about zero, the stop is
 * tight and the detail stays; where a pixel is noisy it blurs.  var is a full frame in frame order,
 * 3 doubles per pixel: the variance of rgb's pixel per channel, as rp_render_variance_device_ws defines it.
 *   Parameters: base is rp_denoise's, with base.sigma_color ignored; a zero field takes its default, params = NULL
 *   means all defaults.
 *     sigma_var  3.0   sigma_v  (> 0, finite)
 *     var_eps    1e-6  eps_v    (> 0, finite)
 *   Definition.  Everything in rp_denoise's definition stands, except:
 *     Every pixel also carries v, the variance of its c summed over the channels.  Initially
 *       v = (x + y) + z of var / ((albedo + eps) * (albedo + eps)) per channel; albedo NULL: of var itself.
 *     Level l (step s), pixel p, first a prefilter of v: the taps dy = -1..1 (outer), dx = -1..1 (inner) at
 *       q = p + s*(dx, dy); a tap counts if it lies inside the frame and nn_q > 0 (normal NULL: every tap inside the
 *       frame); its weight is kg[|dx|] * kg[|dy|], kg = {1/2, 1/4}; g += weight * v_q and gw += weight from 0.0 in tap
 *       order; vf = g / gw.
 *     w_c = rat(|c_p - c_q|^2 / ((sigma_v*sigma_v) * (vf + eps_v))), at every level and never disabled.
 *     Beside sw and acc, every tap adds (w*w) * v_q to vacc (from 0.0); v' = vacc / (sw*sw).
 *     A pixel with nn == 0 keeps its c and its v.
 *   The prefilter lies on the level's own sub-lattice (step s, not 1): its taps are among the 5 x 5 taps.
 * rp_denoise_var_device, rp_denoise_var: as rp_denoise_device and rp_denoise, with d_var / var beside rgb (NULL:
 * RP_EINVAL; out and scratch must not alias it).  d_scratch: rp_denoise_var_scratch_bytes bytes, 8-byte aligned: two
 * colour and two variance buffers, 2 x (24 + 8) bytes per pixel. */
typedef struct rp_denoise_var_params {
  rp_denoise_params base;
  double sigma_var, var_eps;
} rp_denoise_var_params;
int rp_denoise_var_params_init(rp_denoise_var_params* params);
int rp_denoise_var_scratch_bytes(uint32_t width, uint32_t height, uint64_t* bytes);
int rp_denoise_var_device(const rp_denoise_var_params* params, uint32_t width, uint32_t height, const double* d_rgb,
                          const double* d_var, const double* d_normal, const double* d_albedo, const double* d_depth,
                          double* d_out, void* d_scratch, void* stream);
int rp_denoise_var(const rp_denoise_var_params* params, int device, uint32_t width, uint32_t height, const double* rgb,
                   const double* var, const double* normal, const double* albedo, const double* depth, double* out,
                   double* seconds);

/* Progressive rendering: the frames of successive launches folded, on the device, into a running mean and the variance
 * of that mean, and the count of pixels whose error is still above a tolerance -- the stopping rule.  Frame f of
 * rp_render_frames_device_ws is the frame of seed + f*B*W*H (B = ceil(spp / samples_per_stream)), so the n frames of a
 * launch are n independent estimates of every pixel and the next launch at seed + n*B*W*H continues them without
 * repeating a stream: the one-stream-per-pixel fast path gets a variance, with n - 1 degrees of freedom, that
 * rp_render_variance_device_ws cannot give it.  DESIGN.md 4.13.
 *   Definition.  A word is one double of a buffer, whatever it holds.  Its state is (mean, m2); frame number k counts
 *   from 1 over all frames ever folded in.  In IEEE binary64, in the order written and without contraction:
 *     r_k  = 1.0 / (double)k
 *     d    = x - mean
 *     mean = mean + d * r_k
 *     m2   = m2 + d * (x - mean)            -- the new mean
 *   (Welford 1962).  With n_prior = 0 the state is not read: it starts at mean = 0.0, m2 = 0.0 and k at 1, hence after
 *   one frame mean == x bit for bit and m2 == 0.  After n >= 2 frames the variance of the mean is
 *     var = m2 / ((double)n * (double)(n - 1))
 *   NaN and infinities propagate.
 * rp_accum_frames_device is purely elementwise: it knows nothing of scenes, shards or channels, and serves compact shard
 * buffers (slots outside the frame just carry their garbage along), full frames, rgb or anything else laid out as
 * n_frames blocks.  d_frames: frame f's n_words doubles at f * frame_stride (in doubles, >= n_words); they are folded in
 * the order f = 0 .. n_frames - 1 into (d_mean, d_m2), n_words doubles each, which already hold n_prior frames (0: they
 * are only written).  d_var (nullable): n_words doubles, the variance of the mean for n = n_prior + n_frames.
 * Asynchronous on `stream` on the CURRENT device (as rp_frame_assemble); one kernel launch, no allocation and no
 * synchronisation (capturable, like rp_render_device).  Any n_words >= 1, stride and alignment are served; 16-byte
 * aligned buffers with an even stride take the wide path.  RP_EINVAL: NULL d_frames, d_mean or d_m2; n_words or n_frames
 * of zero; frame_stride < n_words; d_var with n < 2; n above 2^31 - 1; n_words above 2^40 - 512; an output that aliases
 * the frames or another output. */
int rp_accum_frames_device(uint64_t n_words, uint32_t n_prior, uint32_t n_frames, const double* d_frames,
                           uint64_t frame_stride, double* d_mean, double* d_m2, double* d_var, void* stream);

/* The error measure of a pixel, from the three words of its mean m and the three of its variance v:
 *     s  = (v.r + v.g) + v.b
 *     q  = ((m.r*m.r + m.g*m.g) + m.b*m.b) + eps
 *     e2 = s / q
 *   the squared relative standard error; eps makes it an absolute error for dark pixels.  A pixel is "over" when
 *   e2 > tol*tol.  A zero field takes its default (tol 0.05, eps 1e-4), params = NULL means both; tol must be > 0 and eps
 *   > 0 and finite.
 * rp_accum_error_device_ws: d_shard_mean and d_shard_var are compact shard buffers of `params`' shard, 3 doubles per slot
 * (the render's shard order, as rp_render_variance_device_ws writes them); slots of edge tiles outside the frame are
 * never read or counted.  d_stats (RP_ERROR_STATS_LEN uint64, 8-byte aligned) is zeroed on `stream`, then receives
 *     [0] the pixels counted              [1] the pixels over
 *     [2] the bit pattern of the largest finite e2 (of the positive ones; 0 when there is none)
 *     [3] the pixels whose e2 is not finite (NaN: never over; +inf: also over)
 * All four are order-free -- integer sums and an integer maximum of positive doubles' bits -- so the result is exact and
 * the same on every run.  Shards add up: pixels, over and non-finite sum over the shards of a frame, the maximum is the
 * maximum of theirs.  params.shard, num_shards, tile_w, tile_h and shard_map are honoured; a balanced shard uses the plan
 * the beauty render left in the workspace (NULL = the scene's).  Asynchronous on `stream`, never allocates or
 * synchronises (capturable): one small launch that clears d_stats and the pass's own; an empty shard leaves the zeros.  RP_EINVAL: a
 * NULL buffer, parameters out of range, a balanced shard without a plan. */
#define RP_ERROR_STATS_LEN 4
typedef struct rp_error_params {
  double tol, eps;
} rp_error_params;
int rp_accum_error_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                             const rp_error_params* error, const double* d_shard_mean, const double* d_shard_var,
                             uint64_t* d_stats, void* stream);

/* Tile-adaptive progressive rendering: further launches trace only the tiles that are still over the
 * tolerance.  Three calls: a render launch over a list of frame tiles, the selection of the tiles still over, and the
 * fold of a tile-list launch into whole-frame state.  The RNG contract makes the result well defined: pixel (i, j)'s
 * k-th frame is the frame of seed + k*W*H whoever renders it, a tile that leaves the list never returns (its state no
 * longer changes), so every listed tile has the same number of frames folded in and one seed per launch suffices.
 *
 * rp_render_tiles_device_ws: n_frames frames of the n_listed frame tiles d_tiles names (device memory; row-major tile
 * indices of `params`' frame, as everywhere else).  `params` describes the whole frame on one device: num_shards 0 or 1,
 * shard 0, RP_SHARD_INTERLEAVE; one stream per pixel (samples_per_stream >= spp >= 1).  Frame f (0 .. n_frames - 1) is the
 * frame of seed + f*W*H, exactly as rp_render_frames_device_ws's.  Output: listed tile k occupies the slots
 * k*tw*th .. (k + 1)*tw*th - 1, row-major inside the tile; frame f starts at f * 3 * n_listed*tw*th doubles of d_rgb and
 * at f * n_listed*tw*th floats of d_fg (nullable).
 *   Defined property: every value written is bit-identical to what rp_render_frames_device_ws writes for that pixel and
 *   frame with the same params, for every frame_order.
 *   Not written and not counted: the slots of edge tiles outside the frame, and the slots of an entry e at or above the
 *   frame's tile count.  The render kernel's in-frame test skips the latter by itself: slot_pixel and the unit fetch
 *   (rp_units.h) place tile e's pixels at row (e / tiles_x) * tile_h >= tiles_y * tile_h >= height.  That holds while
 *   e < 2^31 (the fetch's division) and e * tile_h < 2^32 (the row does not wrap); beyond that range the entry's own
 *   slots are unspecified -- still nothing outside the entry's slots is written.  Duplicates render twice, each into its
 *   own slots.
 *   d_counters (RP_COUNTERS_LEN, required): zeroed on `stream`, then samples = spp x in-frame pixels of the listed tiles x
 *   n_frames, rays and pixels likewise, status bits as rp_render_device.
 * Asynchronous on `stream`; never allocates or synchronises.  It uses what a workspace (NULL = the scene's) has from its
 * creation -- queues, keystream slabs, spill, start times -- and needs no reservation (the batch workspace is for
 * several streams per pixel, which it refuses).  It leaves the workspace's learned state exactly as it found it: no tile
 * is measured, no unit duration stored, no plan or cost table read or written; rp_workspace_frame_info reports 0 after it.
 * It waits on a pending frame gather as a render does.  The tiles go out in list order, in the queue chunks and frame
 * order of a shard of n_listed tiles (raytracing-potato_amd/csrc/rp_schedule.h).  n_listed = 0: the counters are
 * zeroed, nothing is launched, RP_OK.  RP_EINVAL: a NULL camera, params, d_rgb, d_counters or (n_listed > 0) d_tiles; a
 * sharded or balanced params; spp = 0; samples_per_stream < spp; n_listed above the frame's tile count; n_frames outside
 * 1..RP_MAX_FRAMES; a bad frame_order; what rp_render_frames_device_ws refuses about params and the launch's size. */
int rp_render_tiles_device_ws(rp_scene* scene, rp_workspace* workspace, const rp_camera* camera,
                              const rp_render_params* params, const uint32_t* d_tiles, uint32_t n_listed,
                              uint32_t n_frames, uint32_t frame_order, double* d_rgb, float* d_fg, uint64_t* d_counters,
                              void* stream);

/* rp_accum_tiles_select_device: which tiles of a list are still over.  d_mean and d_var are whole-frame compact shard
 * buffers (one shard, interleave: frame tile t at slot t*tw*th, 3 doubles per slot) -- the layout a whole-frame render
 * and rp_accum_frames_device keep.  d_tiles_in: n_in tile indices, NULL = the identity list 0 .. n_in - 1.  Per listed
 * tile k:
 *     over_k = the number of its in-frame pixels with e2 > tol*tol  (e2, tol, eps: as rp_accum_error_device_ws; NaN is
 *              never over, +inf is)
 *     px_k   = its in-frame pixel count
 *     active iff (double)over_k > tile_share * (double)px_k          (tile_share in [0, 1); 0: any pixel over)
 *   An entry at or above the frame's tile count has over = 0 and is never active.
 * d_tiles_out (room for n_in entries) receives the active tiles in the order of the input list -- a stable compaction,
 * the same on every run --, d_count[0] their number, d_over (nullable, n_in entries) the counts.  d_tiles_out is also the
 * pass's scratch: entries past the count hold leftovers.  Asynchronous on `stream` on the CURRENT device, two small
 * launches (one block per listed tile; one block for the scan), no atomics, no allocation, no synchronisation.
 * RP_EINVAL: a NULL d_mean, d_var, d_tiles_out or d_count; sharded or balanced params; error params out of range;
 * tile_share outside [0, 1); n_in above 16384 (the limit balanced plans have); d_tiles_out aliasing d_tiles_in or d_over,
 * d_count inside either output. */
int rp_accum_tiles_select_device(const rp_render_params* params, const rp_error_params* error, double tile_share,
                                 const double* d_mean, const double* d_var, const uint32_t* d_tiles_in, uint32_t n_in,
                                 uint32_t* d_over, uint32_t* d_tiles_out, uint32_t* d_count, void* stream);

/* rp_accum_frames_tiles_device: rp_accum_frames_device's fold with a block indirection, as ignorant of scenes.  The
 * state (d_mean, d_m2, d_var nullable) is n_state_tiles blocks of tile_words doubles; d_frames holds n_frames frames of
 * n_listed blocks, word w of listed block k of frame f at d_frames[f*frame_stride + k*tile_words + w].  Listed block k
 * is folded in frame order, with frame numbers n_prior + 1 .., into the state words d_tiles[k]*tile_words + w; d_var is
 * written for the listed blocks only, with n = n_prior + n_frames.  The arithmetic is the definition above, unchanged;
 * every other state word is untouched (with n_prior = 0 the listed blocks' state is not read, the others' is kept).
 * An entry at or above n_state_tiles is skipped.  Duplicate entries give an unspecified result for that block and for
 * nothing else.  tile_words even, 16-byte aligned buffers and an even stride take the wide path, anything else the
 * 8-byte one.  Asynchronous on `stream` on the CURRENT device; one launch (none for n_listed = 0, which is RP_OK).
 * RP_EINVAL: as rp_accum_frames_device (tile_words for n_words; the state's n_state_tiles*tile_words above 2^40 - 512),
 * and n_listed > n_state_tiles, frame_stride < n_listed*tile_words, a NULL d_tiles with n_listed > 0, an output aliasing
 * the list. */
int rp_accum_frames_tiles_device(uint64_t tile_words, uint32_t n_state_tiles, const uint32_t* d_tiles, uint32_t n_listed,
                                 uint32_t n_prior, uint32_t n_frames, const double* d_frames, uint64_t frame_stride,
                                 double* d_mean, double* d_m2, double* d_var, void* stream);

/* Temporal reprojection: the accumulation state kept across a camera move -- the temporal half of SVGF
 * (Schied et al. 2017).  rp_reproject_device carries the previous pose's running mean, m2 and per-pixel frame count to
 * where its surfaces appear from the current pose, guided by the depth and normal buffers of rp_render_aov at both
 * poses; rp_accum_frames_counts_device then folds the new pose's frames in with the frame number taken per pixel.  A
 * disoccluded pixel starts over (count 0), the others continue what they had.
 *   Buffers are full frames in frame order (pixel (i, j) at j*W + i, row 0 at the bottom, as rp_denoise_device's): depth
 *   1 double per pixel, normal, mean and m2 3 doubles, count 1 uint32 (the frames folded into that pixel).  The pass runs
 *   on the CURRENT device and knows nothing of scenes or shards.
 *   Definition.  IEEE binary64, in the order written, without contraction; floor is exact and sqrt correctly rounded.
 *   Per camera c, on the host: ty_c = tan(0.5*fov), tx_c = ty_c * aspect_ratio.  R = orientation, R[3*col + row];
 *   R.v = ((R[0]*v.x + R[3]*v.y) + R[6]*v.z, ...), Rt.v = ((R[0]*v.x + R[1]*v.y) + R[2]*v.z, ...), Rt taken as R's
 *   inverse (lookat builds orthonormal columns).  Dot products and squared lengths are summed (x + y) + z.  For the
 *   current pixel (i, j) with depth z_cur, normal n_cur, nn_cur = n_cur.n_cur:
 *     1. u = ((double)i + 0.5) / W, v = ((double)j + 0.5) / H; sx = (2.0*u - 1.0) * tx_cur, sy = (2.0*v - 1.0) * ty_cur;
 *        l = sqrt((sx*sx + sy*sy) + 1.0).
 *     2. The pixel is geometry iff nn_cur > 0 and z_cur > 0, else sky.
 *     3. Geometry: g = z_cur / l, L = (sx*g, sy*g, -g), D = R_cur.L, E = (D + pos_cur) - pos_prev per component.
 *        Sky: L = (sx, sy, -1.0), E = R_cur.L (the background is at infinity: no translation).
 *     4. q = Rt_prev.E, m = -q.z; fx = ((q.x / (m*tx_prev) + 1.0) * 0.5) * W - 0.5, fy likewise with q.y, ty_prev, H.
 *     5. The pixel is off unless m > 0 and fx > -1.0 and fx < W and fy > -1.0 and fy < H (a NaN is off).
 *     6. i0 = floor(fx), a = fx - i0; j0 = floor(fy), b = fy - j0; geometry: z_exp = sqrt(q.q).
 *     7. Taps dy = 0, 1 (outer), dx = 0, 1 (inner): t = (i0 + dx, j0 + dy), w = (dx ? a : 1.0 - a) * (dy ? b : 1.0 - b).
 *        A tap counts iff it lies inside the frame, w > 0, count_prev[t] >= 1 and its class matches -- sky: nn_t == 0;
 *        geometry: nn_t > 0, and with d = z_t - z_exp, (d < 0 ? -d : d) <= sigma_depth * z_exp, and with c = n_cur.n_t,
 *        c > 0 and c*c >= (normal_cos*normal_cos) * (nn_cur*nn_t).
 *     8. From 0.0, in tap order: sw += w; acc[ch] += w * mean_t[ch]; sacc[ch] += w * s_t[ch], s_t[ch] = count_t >= 2 ?
 *        m2_t[ch] / (double)(count_t - 1) : 0.0 (the per-frame variance); the first tap with a strictly larger w than
 *        all before it gives n_best = count_t.
 *     9. No counting tap: count = 0, mean = m2 = 0.0.  Otherwise count = min(n_best, max_history), mean = acc / sw,
 *        m2 = (sacc / sw) * (double)(count - 1): "count frames with this mean and this per-frame variance", which the
 *        fold below continues.  NaN in a counting tap's state propagates; a tap that does not count is never read into
 *        the sums.
 *   A zero field of rp_reproject_params takes its default: sigma_depth 0.05 (> 0, finite), normal_cos 0.9 (in (0, 1]),
 *   max_history 32 (1 .. 2^31 - 1); params = NULL means all three.
 *   d_stats (RP_REPROJECT_STATS_LEN uint64, 8-byte aligned) is zeroed on `stream`, then receives
 *     [0] the pixels   [1] the pixels with count >= 1   [2] the sum of the counts   [3] the off pixels
 *   -- order-free integer sums, exact and the same on every run.
 * rp_reproject_device: asynchronous on `stream`, two launches, no allocation and no synchronisation (capturable).
 * rp_reproject: the same on host buffers through the kernel on `device`, synchronous; *seconds (nullable) the device time.
 * RP_EINVAL: a NULL pointer; a zero size or a side above 65535; parameters out of range; a camera field that is not
 * finite or a fov with tan(0.5*fov) <= 0; an output aliasing an input or another output (a gather: in place is wrong). */
#define RP_REPROJECT_STATS_LEN 4
typedef struct rp_reproject_params {
  double sigma_depth, normal_cos;
  uint32_t max_history, reserved;
} rp_reproject_params;
int rp_reproject_params_init(rp_reproject_params* params);
int rp_reproject_device(const rp_reproject_params* params, uint32_t width, uint32_t height, const rp_camera* cur,
                        const rp_camera* prev, const double* d_depth_cur, const double* d_normal_cur,
                        const double* d_depth_prev, const double* d_normal_prev, const double* d_mean_prev,
                        const double* d_m2_prev, const uint32_t* d_count_prev, double* d_mean, double* d_m2,
                        uint32_t* d_count, uint64_t* d_stats, void* stream);
int rp_reproject(const rp_reproject_params* params, int device, uint32_t width, uint32_t height, const rp_camera* cur,
                 const rp_camera* prev, const double* depth_cur, const double* normal_cur, const double* depth_prev,
                 const double* normal_prev, const double* mean_prev, const double* m2_prev, const uint32_t* count_prev,
                 double* mean, double* m2, uint32_t* count, uint64_t* stats, double* seconds);

/* rp_accum_frames_counts_device: rp_accum_frames_device with the frame number taken per pixel.  Word w of pixel p of
 * frame f sits at d_frames[f*frame_stride + p*words_per_pixel + w]; the state words of pixel p at p*words_per_pixel + w
 * of d_mean and d_m2.  For pixel p with c = d_count[p], frames f = 0 .. n_frames - 1 are folded with k = c + f + 1,
 * r = 1.0 / (double)k, by the Welford lines above, unchanged; with c == 0 the state is not read and starts at 0.0.
 * Afterwards d_count[p] = c + n_frames.  d_var (nullable): with n = c + n_frames, m2 / ((double)n * (double)(n - 1)) for
 * n >= 2, else var_one -- the caller's stand-in for "one frame, spread unknown", finite and >= 0 (a non-finite one would
 * put 0 * inf into the variance-guided filter).  The caller keeps every count below 2^31 - n_frames (max_history does
 * that for reprojected state).
 *   Defined property: with every count equal to c, mean, m2 and (n >= 2) var equal rp_accum_frames_device's with
 *   n_prior = c bit for bit.
 * Asynchronous on `stream` on the CURRENT device; one launch, no allocation, no synchronisation.  RP_EINVAL: as
 * rp_accum_frames_device (n_pixels*words_per_pixel for n_words), and words_per_pixel of zero, a NULL d_count, a var_one
 * that is negative or not finite, d_count aliasing the frames or the state. */
int rp_accum_frames_counts_device(uint64_t n_pixels, uint32_t words_per_pixel, uint32_t n_frames, const double* d_frames,
                                  uint64_t frame_stride, uint32_t* d_count, double* d_mean, double* d_m2, double* d_var,
                                  double var_one, void* stream);

/* Output stage on the device: the reference's to_srgb_u8 (utility.rs:212-220, alpha 255) of every slot of
 * a compact shard buffer, bytes in tga::save's pixel order B, G, R, A (image.rs:116-137), so a gathered
 * and de-interleaved frame is the body of the reference's output.tga (18-byte header: rph_tga_save).
 * d_shard_bgra: shard_pixel_count * 4 bytes, 4-byte aligned.  Asynchronous on `stream`.  Bytes are
 * identical to to_srgb_u8 evaluated with the host libm's pow: the device looks x up in the 255
 * thresholds of that step function (rp_srgb_thresholds), it evaluates no pow of its own. */
int rp_shard_to_bgra8(rp_scene* scene, const rp_render_params* params, const double* d_shard_rgb,
                      uint8_t* d_shard_bgra, void* stream);
/* The threshold table of rp_shard_to_bgra8: out[k] (k = 1..255) is the smallest x whose to_srgb_u8 byte
 * is >= k; out[0] = -inf.  256 doubles.  Host only (no device needed). */
int rp_srgb_thresholds(double* out);

/* Closest-hit query (Hittable::hit on the root, hittable.rs:18 / bvh.rs:121) for n rays, synchronous,
 * host buffers.  rays: n * 8 doubles {origin xyz, direction xyz, t_min, t_max} (utility.rs:52-57).
 * out_hit: n * 9 doubles {t, position xyz, normal xyz, u, v} (utility.rs:84-89), t = +inf on a miss.
 * out_material: n uint32 (MaterialId, 0xffffffff on a miss).  Used to test the traversal in isolation. */
int rp_intersect(rp_scene* scene, const double* rays, uint64_t n, double* out_hit, uint32_t* out_material);

/* Diagnostic counters accumulated by renders since the last reset (non-zero only in the diagnostic
 * build lib/librp_diag.so, whose kernel carries s_memtime phase stamps): wave-cycles per phase
 * {fetch, new sample, traverse, shade, tail}, wave loop iterations, active lanes at traversal,
 * traversal wave-trips, lane node visits, lane primitive tests.  Synchronises the device. */
int rp_diagnostics(rp_scene* scene, uint64_t* out, uint32_t n, int reset);

/* ---------------------------------------------------------------- multi-GPU -- */
/* Image tiles are dealt across the GPUs (params.shard = rank, params.shard_map: the interleave tile t -> rank
 * t % nranks, or the balanced plan), every GPU holds its own copy of the scene, and one RCCL all-gather over xGMI
 * per frame moves the shards; each rank then de-interleaves them into frame order on its device.  This replaces the reference's
 * thread tile queue (main.rs:36-106, num_workers main.rs:27).  The per-pixel RNG contract makes the
 * gathered frame bitwise identical for any number of GPUs. */
typedef struct rp_comm rp_comm;     /* opaque: one rank's RCCL communicator (one device) */
typedef struct rp_multi rp_multi;   /* opaque: a scene on several devices of this process + communicator */

/* One process per GPU (torch.distributed / MPI style): rank 0 makes the id, every rank receives its bytes
 * out of band and joins.  `device` is the rank's HIP device (the scene's). */
int rp_comm_unique_id(uint8_t id[RP_COMM_ID_BYTES]);
int rp_comm_create(const uint8_t id[RP_COMM_ID_BYTES], int nranks, int rank, int device, rp_comm** out);
void rp_comm_destroy(rp_comm* comm);
int rp_comm_info(const rp_comm* comm, int* nranks, int* rank, int* device);

/* Collective over all ranks of `comm`, asynchronous on `stream` (every rank must call it, in the same
 * order relative to its other collectives on comm).  params: this rank's shard (shard = rank, num_shards
 * = nranks), the workspace reserved for it (rp_workspace_reserve) -- for RP_SHARD_BALANCED the workspace that
 * rendered the shard (it holds the plan).  d_shard_rgb: the rank's finished shard (rp_render_device_ws output).
 * Outputs (either nullable, on the rank's device, frame order, row 0 = bottom): d_frame_bgra width*height*4
 * bytes = to_srgb_u8 in tga::save byte order (rp_shard_to_bgra8) -- the body of output.tga; d_frame_rgb
 * width*height*3 linear f64.  Every rank must pass the same NULL / non-NULL combination of d_frame_bgra and
 * d_frame_rgb: the collectives issued are, in this order, ONE all-gather of every rank's packed block -- its counter
 * block, its measured tile costs (zeros for frames of more than 16384 tiles) and, with d_frame_bgra, its BGRA8
 * shard -- and, with d_frame_rgb, one of the f64 shards.  d_counters (nullable): the rank's
 * RP_COUNTERS_LEN counters in, the frame's out -- rays, samples and pixels summed over the ranks, status bits
 * OR-ed over them, plus RP_STATUS_PLAN_MISMATCH when the ranks' balanced plans differ.  A caller that does not
 * pass counters does not learn the status.  Tile costs (the collectives also all-gather every rank's measured
 * tile costs for frames of <= 16384 tiles) and the balanced plan live in the workspace: the gather reads the
 * workspace's plan and measured costs and writes its learned cost table on `stream`, and the next render with the
 * same workspace rewrites the first two and reads the third on ITS stream.  The library orders the two itself: the
 * gather records an event in the workspace at its end, and the next render with that workspace makes its stream wait
 * on it (a caller with separate render and gather streams cannot race them).  Frames in flight use one workspace
 * per frame. */
int rp_frame_gather(rp_comm* comm, rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                    const double* d_shard_rgb, uint8_t* d_frame_bgra, double* d_frame_rgb,
                    uint64_t* d_counters, void* stream);
/* rp_frame_gather for the n_frames shards of one rp_render_frames_device_ws launch (d_shard_rgb: its n_frames shard
 * buffers back to back) in ONE all-gather: every rank's packed block carries its counter block (the launch's sums),
 * its measured tile costs and the n_frames shards' BGRA8 bytes one after the other; d_frames_bgra (nullable) receives
 * n_frames assembled frames of width*height*4 bytes back to back.  BGRA8 only (rp_frame_gather gathers f64 frames).
 * One collective per launch instead of one per frame: an RCCL all-gather kernel waits for a CU the render waves leave
 * (DESIGN.md 6).  The workspace must be reserved with rp_workspace_reserve_frames for n_frames. */
int rp_frames_gather(rp_comm* comm, rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                     uint32_t n_frames, const double* d_shard_rgb, uint8_t* d_frames_bgra, uint64_t* d_counters,
                     void* stream);
/* rp_frames_gather in two halves around a collective of the caller's own (ABI v9; MPI, a torch.distributed
 * all-gather, tests): rp_frames_block_words gives the words (uint32) of one rank's packed block for n_frames frames of
 * params' shape -- the counter block and plan hash, the measured tile costs, then frame f's to_srgb_u8 bytes at a fixed
 * offset per frame; rp_frames_pack writes this rank's block (params.shard of params.num_shards) into d_send; the caller
 * all-gathers the num_shards blocks rank by rank into d_recv (rank r's block at r * words); rp_frames_unpack then does
 * what rp_frames_gather does after its collective: counters reduced into d_counters (sums, status OR-ed, plan hashes
 * compared), the gathered tile costs learned, and the n_frames frames assembled into d_frames_bgra.  Same workspace
 * reservation and rules as rp_frames_gather; asynchronous on `stream`. */
int rp_frames_block_words(const rp_render_params* params, uint32_t n_frames, uint64_t* words);
int rp_frames_pack(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params, uint32_t n_frames,
                   const double* d_shard_rgb, const uint64_t* d_counters, uint32_t* d_send, void* stream);
int rp_frames_unpack(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params, uint32_t n_frames,
                     const uint32_t* d_recv, uint8_t* d_frames_bgra, uint64_t* d_counters, void* stream);
/* The frame assembly step alone, for callers that move the shards with their own collective (MPI, a
 * torch.distributed all-gather): d_gathered holds params->num_shards shard buffers of `stride` slots each
 * (rp_gather_stride: the largest shard, shard 0), rank r's at slot r * stride, `words_per_slot` 32-bit words
 * per slot (1 for the BGRA8 bytes of rp_shard_to_bgra8, 6 for f64 RGB); d_frame receives width*height
 * slots in frame order.  Asynchronous on `stream`, on the current device. */
int rp_gather_stride(const rp_render_params* params, uint64_t* stride);
/* RP_SHARD_INTERLEAVE frames; a balanced frame is refused (RP_EINVAL): rp_frame_assemble_ws assembles with the
 * plan held by the workspace that rendered this rank's shard of the frame. */
int rp_frame_assemble(const rp_render_params* params, const void* d_gathered, uint32_t words_per_slot,
                      void* d_frame, void* stream);
int rp_frame_assemble_ws(rp_scene* scene, rp_workspace* workspace, const rp_render_params* params,
                         const void* d_gathered, uint32_t words_per_slot, void* d_frame, void* stream);

/* rp_render_device_ws into the workspace's shard buffer, then rp_frame_gather, on one stream. */
int rp_render_gather(rp_comm* comm, rp_scene* scene, rp_workspace* workspace, const rp_camera* camera,
                     const rp_render_params* params, uint8_t* d_frame_bgra, double* d_frame_rgb,
                     uint64_t* d_counters, void* stream);

/* One process, several GPUs (the reference's single-process model): a scene copy per device, one
 * communicator over them (ncclCommInitAll), one stream per device. */
int rp_multi_create(const rp_scene_desc* desc, const int* devices, int n_devices, const rp_scene_options* opt,
                    rp_multi** out);
void rp_multi_destroy(rp_multi* multi);
/* Synchronous frame on every device of `multi` (params.shard / num_shards are ignored: device k renders
 * shard k of n_devices; params.shard_map applies -- RP_SHARD_BALANCED is the better split).  out_rgb
 * (nullable): width*height*3 doubles on the host, frame order; out_bgra (nullable): width*height*4 bytes
 * (to_srgb_u8, tga::save order).  stats (nullable): summed counters, seconds = wall time of the frame.  Returns
 * RP_EINTERNAL when any device reported a status bit (stack overflow, plan mismatch). */
int rp_render_multi(rp_multi* multi, const rp_camera* camera, const rp_render_params* params,
                    double* out_rgb, uint8_t* out_bgra, rp_stats* stats);

/* ---------------------------------------------------------------- test hook: the packed tree -- */
/* Copies a scene's acceleration structure to the host as it lies in device memory, whatever built it (host SAH, device
 * LBVH or PLOC): the wide node records -- raytracing-potato_amd/csrc/rp_layout.h Node4 (128 B, RP_NODES_F32), Node4Q
 * (64 B, RP_NODES_Q8) or Node8Q (128 B, RP_NODES_W8); rp_scene_info's n_nodes of them, the pad records of
 * RP_LAYOUT_DFS_LINE included --, the primitives in leaf order (Prim, 80 B each, rp_scene_info's n_prims of them) and
 * their references (PrimRef, 16 B each; src = the source hittable).  node_format and root (each nullable) receive the
 * resolved RP_NODES_* and the root's node index.  A NULL buffer is not copied: all three NULL query the format and the
 * root, and the sizes follow from rp_scene_info.  RP_EINVAL, with the bytes needed in the message and nothing written
 * to any buffer: a buffer smaller than its records.  Synchronises the device.  Added without an ABI bump: a library
 * without it still serves every other call. */
int rp_scene_tree(const rp_scene* scene, void* nodes, uint64_t node_bytes, void* prims, uint64_t prim_bytes,
                  void* prim_refs, uint64_t ref_bytes, uint32_t* node_format, uint32_t* root);

/* ---------------------------------------------------------------- moving geometry: refit in place -- */
/* New vertex positions, vertex normals and sphere records for a scene, without building it again: the primitive
 * records, the per-primitive normals and the boxes of the EXISTING tree are rewritten on the device.  The topology is
 * kept -- which primitives share a leaf, the entries, the node order, RP_LAYOUT_DFS_LINE's pad records, the stack depth
 * -- and so are materials, textures, uvs, workspaces and everything they have learned (tile costs, unit orders, plans:
 * results never depend on them).  A refit node stores exactly the boxes the builders would store for the same tree over
 * the new geometry, so a refit with unchanged geometry changes no byte.  What a refit does not keep is
 * the tree's QUALITY: the tree was chosen for the old geometry, and the further the geometry moves, the more node visits
 * a ray costs compared with a fresh build (profiles/r32/refit_time.json).  Images stay exact.
 *
 * rp_refit_create (synchronous, allocates): the plan of a scene's tree -- its reachable nodes by level -- and 48 bytes
 * of scratch per primitive and per node record.  RP_EINVAL: a NULL scene; an RP_NODES_W8 scene (a Node8Q slot encodes
 * where a child lies relative to its node's centre, which moved geometry invalidates: rebuild such scenes); coord_max
 * negative, not finite or above 2^54.  The handle belongs to the scene: destroy it before the scene.  An rp_multi has
 * no accessor for its per-device scenes and cannot be refit.
 *
 * The coordinate bound B = max(coord_max, the largest |coordinate| of the scene's primitive boxes at create time, taken
 * from the records with a few ulps of slack; coord_max = 0 keeps the build's bound) holds for all later updates.  The
 * quantized traversal (RP_NODES_Q8) takes its slab slack from a bound on every node frame; create raises the scene's to
 * cover B.  That only widens a conservative box test: no image changes, with or without an update, and
 * rp_refit_destroy leaves the widened bound in place.  A render captured in a graph before the create keeps the bound
 * it was captured with.
 *
 * rp_scene_refit_device: asynchronous on `stream` on the scene's device; it never allocates or synchronises and may be
 * captured in a graph.  d_positions, d_normals: 3 doubles per global vertex -- the meshes' vertices concatenated in mesh
 * order (rp_refit_info's n_vertices of them); d_spheres: 4 doubles {center.xyz, radius} per sphere, the sphere hittables
 * numbered in hittable order (n_spheres of them).  Each is nullable and means "unchanged"; all three NULL is RP_EINVAL.
 * d_normals alone rewrites only the per-primitive normals.  An update of the geometry names ALL of it -- d_positions
 * when the scene has triangles, d_spheres when it has spheres, else RP_EINVAL: the handle keeps no copy of the current
 * positions to complete a partial update from (DeviceScene.geometry() is the starting point of a deformation).
 * d_status (required, one word, zeroed on the stream first) receives RP_REFIT_OUT_OF_BOUND when a primitive's box has a
 * finite coordinate beyond B.  After an RP_NODES_Q8 refit that reported it, the scene's images are unspecified until a
 * refit within the bound; RP_NODES_F32 scenes are unaffected by the bound.  In neither case can a traversal leave the
 * buffers: the topology is untouched.  NaN coordinates behave as in the builders (never hit, nothing repaired).
 * The caller orders a refit against renders, feature passes and queries of the same scene with streams and events: a
 * refit while a render of the scene is in flight is a race.  The host's scene description is not involved.
 *
 * rp_scene_refit: the same from host buffers, synchronous; seconds (nullable) = device time of the kernels.
 * Reprojecting the history of MOVING surfaces (rp_reproject_device) needs motion vectors and is not part of this.
 * Added without an ABI bump: a library without these calls still serves every other call. */
#define RP_REFIT_OUT_OF_BOUND 1u
typedef struct rp_refit rp_refit;   /* opaque: a scene's refit plan and scratch */
int rp_refit_create(rp_scene* scene, double coord_max, rp_refit** out);
void rp_refit_destroy(rp_refit* refit);
int rp_refit_info(const rp_refit* refit, uint64_t* n_vertices, uint64_t* n_spheres, uint32_t* n_levels, double* bound);
int rp_scene_refit_device(rp_refit* refit, const double* d_positions, const double* d_normals, const double* d_spheres,
                          uint32_t* d_status, void* stream);
int rp_scene_refit(rp_refit* refit, const double* positions, const double* normals, const double* spheres,
                   uint32_t* status, double* seconds);

#ifdef __cplusplus
}
#endif

#endif /* RP_H */
