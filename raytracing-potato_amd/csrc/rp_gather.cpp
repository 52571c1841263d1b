// rp_gather.cpp -- the multi-GPU side of the C-ABI in include/rp.h (librp.so): frame assembly, the RCCL communicator,
// the frame gathers and rp_multi (one thread driving several devices).
//
// A frame is assembled in three phases so one thread can drive several devices (rp_multi):
// (1) stage the rank's shard (to_srgb_u8 bytes and/or a padded f64 copy), (2) the RCCL collectives,
// (3) de-interleave the gathered shards into frame order.
#include <chrono>

#include "rp_state.h"

static_assert(sizeof(ncclUniqueId) == RP_COMM_ID_BYTES, "RCCL unique id size");

struct rp_comm {
  Comm comm;
  int nranks = 0, rank = 0, device = 0;
};

struct rp_multi {
  struct Rank {  // one device's share (members are released last to first: the communicator before the scene)
    int device = 0;
    Guarded<rp_scene> scene;
    DevBuf<double> d_frame_rgb;  // rank 0: the assembled frame
    DevBuf<uint32_t> d_frame_bgra;
    DevBuf<uint64_t> d_ctr;  // CTR_N
    Stream stream;
    Comm comm;
  };
  std::vector<Guarded<Rank>> ranks;
};

namespace {

using rps::bgra_words;
using rps::pack_words;
using rps::stage_slots;

struct GatherPlan {
  Tiling t;
  uint64_t stride;  // slots per rank buffer
  uint32_t stride_tiles;  // tiles per rank buffer (shard 0's count)
  uint64_t head;          // words of the packed block before the BGRA8 bytes (pack_head)
  uint32_t nf;            // frames whose BGRA8 bytes the block carries (rp_frames_gather; 1 otherwise)
  rpk::FrameGeom geom;
  const uint32_t* plan_hash;  // the workspace's plan hash (balanced frames), NULL = interleave
};

int gather_plan(rp_scene* s, rp_workspace* w, int nranks, int rank, const rp_render_params* p, GatherPlan& gp,
                uint32_t nf = 1) {
  if (!s || !w || w->scene != s) return fail(RP_EINVAL, "scene / workspace mismatch");
  gp.nf = nf;
  int rc = frame_tiling(p, gp.t);
  if (rc) return rc;
  if ((int)gp.t.shards != nranks || (int)gp.t.shard != rank)
    return fail(RP_EINVAL, "params.shard / num_shards must be the communicator's rank / size");
  gp.stride = stage_slots(gp.t);
  gp.stride_tiles = (gp.t.n_tiles + gp.t.shards - 1) / gp.t.shards;
  gp.head = rps::pack_head(gp.t);
  const uint64_t pw = pack_words(gp.t, true, nf);
  if (3 * gp.stride > w->d_gs_rgb.capacity() || 3 * gp.stride * (uint64_t)nranks > w->d_gather_rgb.capacity() ||
      pw > w->d_pack_send.capacity() || pw * nranks > w->d_pack_recv.capacity())
    return fail(RP_EINVAL, nf > 1 ? "workspace not reserved for these frames' gather: call rp_workspace_reserve_frames"
                                  : "workspace not reserved for this frame's gather: call rp_workspace_reserve");
  gp.geom = rpk::FrameGeom{p->width, p->height, gp.t.tw, gp.t.th, gp.t.tiles_x, (uint32_t)nranks, gp.stride, 0, nullptr};
  gp.plan_hash = nullptr;
  if (gp.t.balanced) {
    if (!w->plan_matches(p, gp.t))
      return fail(RP_EINVAL, "balanced frame: render this rank's shard with the same workspace before gathering it");
    gp.geom.tile_pos = w->d_plan.get() + gp.t.n_tiles;
    gp.plan_hash = w->d_plan.get() + 2 * gp.t.n_tiles;
  }
  return RP_OK;
}

// (1) this rank's packed block for the one collective -- its counters (and plan hash), its measured tile costs, its
// to_srgb_u8 bytes -- and/or a padded f64 copy of the shard
int gather_stage(rp_scene* s, rp_workspace* w, const GatherPlan& gp, const double* d_shard_rgb, bool bgra, bool rgb,
                 const uint64_t* d_counters, hipStream_t st) {
  DeviceGuard g(s->device);
  // the measured costs travel only for frames whose tiles fit the table (gather_learn's condition)
  const uint32_t* meas = gp.t.n_tiles <= (uint32_t)rpk::TILE_SORT_MAX ? w->d_meas.get() : nullptr;
  RP_LAUNCH("gather pack", rpk::launch_gather_pack(d_counters, gp.plan_hash, meas, gp.stride_tiles, w->d_pack_send.get(), st));
  for (uint32_t f = 0; bgra && gp.t.n_slots && f < gp.nf; f++)  // frame f's bytes at head + f x bgra_words
    RP_LAUNCH("output stage",
              rpk::launch_srgb_bgra(srgb_table(), d_shard_rgb + 3 * gp.t.n_slots * (uint64_t)f, gp.t.n_slots,
                                    reinterpret_cast<uint8_t*>(w->d_pack_send.get() + gp.head + bgra_words(gp.t) * f), st));
  if (rgb && gp.t.n_slots && d_shard_rgb != w->d_gs_rgb.get())
    RP_HIP(hipMemcpyAsync(w->d_gs_rgb.get(), d_shard_rgb, sizeof(double) * 3 * gp.t.n_slots, hipMemcpyDeviceToDevice, st));
  return RP_OK;
}

// (2) the collectives: ONE all-gather of the packed blocks (counters -- status bits are OR-ed, not summed, and the plan
// hashes compared --, measured tile costs, BGRA8 bytes), then the f64 shards when asked for (rp.h: every rank passes
// the same NULL / non-NULL outputs, so every rank gathers the same block size).  One collective instead of four: an
// RCCL all-gather kernel on gfx950 needs 37.7 KB of LDS and 256 VGPRs per lane, so with frames in flight each one
// waits ~8-24 ms for a CU the render waves leave (profiles/r5/c3_gather_lds_wait.json).
int gather_collectives(ncclComm_t comm, rp_workspace* w, const GatherPlan& gp, bool bgra, bool rgb, hipStream_t st) {
  RP_NCCL(ncclAllGather(w->d_pack_send.get(), w->d_pack_recv.get(), pack_words(gp.t, bgra, gp.nf), ncclUint32, comm, st));
  if (rgb) RP_NCCL(ncclAllGather(w->d_gs_rgb.get(), w->d_gather_rgb.get(), 3 * gp.stride, ncclFloat64, comm, st));
  return RP_OK;
}

// (3a) the gathered tile costs -> the workspace's learned table (on every device of the frame)
int gather_learn(rp_scene* s, rp_workspace* w, const GatherPlan& gp, const rp_render_params* p, bool bgra,
                 hipStream_t st) {
  DeviceGuard g(s->device);
  if (!w->meas_on || gp.t.n_tiles > (uint32_t)rpk::TILE_SORT_MAX) {
    w->fcost_valid = false;
  } else {
    // rank r's sums at r * block + 2 GATHER_CTR, its maxima stride_tiles further
    const uint32_t* sums = w->d_pack_recv.get() + 2 * rpk::GATHER_CTR;
    RP_LAUNCH("cost table", rpk::launch_learn_costs(sums, sums + gp.stride_tiles, (uint32_t)pack_words(gp.t, bgra, gp.nf),
                                                    gp.geom.nranks, gp.t.n_tiles, gp.t.balanced ? w->d_plan.get() : nullptr,
                                                    w->d_fcost.get(), st));
    w->set_fcost(p, gp.t, gp.geom.nranks);
  }
  // the next render on this workspace waits for the collectives (which read d_meas) and the table (ev_gathered)
  RP_HIP(hipEventRecord(w->ev_gathered.get(), st));
  w->gathered_pending = true;
  return RP_OK;
}

// (3) counters reduced (sums, status OR), shards de-interleaved into frame order
int gather_assemble(rp_scene* s, rp_workspace* w, const GatherPlan& gp, uint8_t* d_frame_bgra, double* d_frame_rgb,
                    uint64_t* d_counters, hipStream_t st) {
  DeviceGuard g(s->device);
  const uint64_t block = pack_words(gp.t, d_frame_bgra != nullptr, gp.nf);
  RP_LAUNCH("counter reduce", rpk::launch_counters_reduce(reinterpret_cast<const uint64_t*>(w->d_pack_recv.get()), gp.geom.nranks,
                                                          block, d_counters ? d_counters : w->d_ctr.get(), st));
  for (uint32_t f = 0; d_frame_bgra && f < gp.nf; f++) {  // frame f into its own W x H x 4 bytes
    rpk::FrameGeom fg = gp.geom;
    fg.rank_words = block;
    RP_LAUNCH("frame assembly",
              rpk::launch_frame_assemble(fg, w->d_pack_recv.get() + gp.head + bgra_words(gp.t) * f, 1,
                                         reinterpret_cast<uint32_t*>(d_frame_bgra + 4ull * gp.geom.W * gp.geom.H * f), st));
  }
  if (d_frame_rgb)
    RP_LAUNCH("frame assembly", rpk::launch_frame_assemble(gp.geom, reinterpret_cast<const uint32_t*>(w->d_gather_rgb.get()), 6,
                                                           reinterpret_cast<uint32_t*>(d_frame_rgb), st));
  return RP_OK;
}

// A gather of nf frames' shards on the communicator's stream: stages (1) to (3).
int gather_frames(rp_comm* c, rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t nf, const double* d_shard_rgb,
                  uint8_t* d_frame_bgra, double* d_frame_rgb, uint64_t* d_counters, void* stream) {
  if (!w) w = &s->ws0;
  if (c->device != s->device) return fail(RP_EINVAL, "the communicator's device is not the scene's");
  GatherPlan gp;
  int rc = gather_plan(s, w, c->nranks, c->rank, p, gp, nf);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool bgra = d_frame_bgra != nullptr, rgb = d_frame_rgb != nullptr;
  DeviceGuard g(s->device);
  if ((rc = gather_stage(s, w, gp, d_shard_rgb, bgra, rgb, d_counters, st))) return rc;
  if ((rc = gather_collectives(c->comm.get(), w, gp, bgra, rgb, st))) return rc;
  if ((rc = gather_learn(s, w, gp, p, bgra, st))) return rc;
  return gather_assemble(s, w, gp, d_frame_bgra, d_frame_rgb, d_counters, st);
}

}  // namespace

extern "C" {

int rp_gather_stride(const rp_render_params* p, uint64_t* stride) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (!stride) return fail(RP_EINVAL, "stride is NULL");
  *stride = stage_slots(t);
  return RP_OK;
}

int rp_frame_assemble(const rp_render_params* p, const void* d_gathered, uint32_t words, void* d_frame, void* stream) {
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if (!d_gathered || !d_frame || words == 0) return fail(RP_EINVAL, "NULL buffer or zero words per slot");
  if (t.balanced) return fail(RP_EINVAL, "balanced frame: assemble with rp_frame_assemble_ws (the workspace holds the plan)");
  rpk::FrameGeom g{p->width, p->height, t.tw, t.th, t.tiles_x, t.shards, stage_slots(t), 0, nullptr};
  RP_LAUNCH("frame assembly", rpk::launch_frame_assemble(g, static_cast<const uint32_t*>(d_gathered), words,
                                                         static_cast<uint32_t*>(d_frame), stream));
  return RP_OK;
}

int rp_frame_assemble_ws(rp_scene* s, rp_workspace* w, const rp_render_params* p, const void* d_gathered,
                         uint32_t words, void* d_frame, void* stream) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  Tiling t;
  if ((rc = frame_tiling(p, t))) return rc;
  if (!d_gathered || !d_frame || words == 0) return fail(RP_EINVAL, "NULL buffer or zero words per slot");
  rpk::FrameGeom g{p->width, p->height, t.tw, t.th, t.tiles_x, t.shards, stage_slots(t), 0, nullptr};
  if (t.balanced) {
    if (!w->plan_matches(p, t)) return fail(RP_EINVAL, "no balanced plan for this frame in the workspace: render it first");
    g.tile_pos = w->d_plan.get() + t.n_tiles;
  }
  DeviceGuard dg(s->device);
  RP_LAUNCH("frame assembly", rpk::launch_frame_assemble(g, static_cast<const uint32_t*>(d_gathered), words,
                                                         static_cast<uint32_t*>(d_frame), stream));
  return RP_OK;
}

int rp_comm_unique_id(uint8_t id[RP_COMM_ID_BYTES]) {
  if (!id) return fail(RP_EINVAL, "id is NULL");
  ncclUniqueId u;
  RP_NCCL(ncclGetUniqueId(&u));
  std::memcpy(id, &u, sizeof u);
  return RP_OK;
}

int rp_comm_create(const uint8_t id[RP_COMM_ID_BYTES], int nranks, int rank, int device, rp_comm** out) {
  if (!out) return fail(RP_EINVAL, "out is NULL");
  *out = nullptr;
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(RP_EINVAL, "bad id / nranks / rank");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(RP_EINVAL, "device index out of range");
  DeviceGuard g(device);
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  Guarded<rp_comm> c(new rp_comm());
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  ncclComm_t comm = nullptr;
  ncclResult_t r = ncclCommInitRank(&comm, nranks, u, rank);
  if (r != ncclSuccess) return fail(RP_ERCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  c->comm = Comm(comm);
  *out = c.release();
  return RP_OK;
}

void rp_comm_destroy(rp_comm* c) { Guarded<rp_comm>{c}; }

int rp_comm_info(const rp_comm* c, int* nranks, int* rank, int* device) {
  if (!c) return fail(RP_EINVAL, "comm is NULL");
  if (nranks) *nranks = c->nranks;
  if (rank) *rank = c->rank;
  if (device) *device = c->device;
  return RP_OK;
}

int rp_frame_gather(rp_comm* c, rp_scene* s, rp_workspace* w, const rp_render_params* p, const double* d_shard_rgb,
                    uint8_t* d_frame_bgra, double* d_frame_rgb, uint64_t* d_counters, void* stream) {
  if (!c || !s || !d_shard_rgb) return fail(RP_EINVAL, "comm, scene and shard must be non-NULL");
  if (reinterpret_cast<uintptr_t>(d_frame_bgra) % 4 != 0) return fail(RP_EINVAL, "d_frame_bgra must be 4-byte aligned");
  return gather_frames(c, s, w, p, 1, d_shard_rgb, d_frame_bgra, d_frame_rgb, d_counters, stream);
}

int rp_frames_gather(rp_comm* c, rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t n_frames,
                     const double* d_shard_rgb, uint8_t* d_frames_bgra, uint64_t* d_counters, void* stream) {
  if (!c || !s || !d_shard_rgb) return fail(RP_EINVAL, "comm, scene and shards must be non-NULL");
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return fail(RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES");
  if (reinterpret_cast<uintptr_t>(d_frames_bgra) % 4 != 0) return fail(RP_EINVAL, "d_frames_bgra must be 4-byte aligned");
  return gather_frames(c, s, w, p, n_frames, d_shard_rgb, d_frames_bgra, nullptr, d_counters, stream);
}

int rp_frames_block_words(const rp_render_params* p, uint32_t n_frames, uint64_t* words) {
  if (!words) return fail(RP_EINVAL, "words is NULL");
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return fail(RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES");
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  *words = pack_words(t, true, n_frames);
  return RP_OK;
}

// rp_frames_gather's stage (1) and its stages (3a, 3) around the caller's collective: the workspace's own send / receive
// buffers are the ones rp_frames_gather uses, copied from / to the caller's.
int rp_frames_pack(rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t n_frames, const double* d_shard_rgb,
                   const uint64_t* d_counters, uint32_t* d_send, void* stream) {
  if (!s || !d_shard_rgb || !d_send || !p) return fail(RP_EINVAL, "scene, params, shards and send buffer must be non-NULL");
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return fail(RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES");
  if (!w) w = &s->ws0;
  GatherPlan gp;
  int rc = gather_plan(s, w, p->num_shards ? (int)p->num_shards : 1, (int)p->shard, p, gp, n_frames);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard g(s->device);
  if ((rc = gather_stage(s, w, gp, d_shard_rgb, true, false, d_counters, st))) return rc;
  RP_HIP(hipMemcpyAsync(d_send, w->d_pack_send.get(), sizeof(uint32_t) * pack_words(gp.t, true, n_frames),
                        hipMemcpyDeviceToDevice, st));
  return RP_OK;
}

int rp_frames_unpack(rp_scene* s, rp_workspace* w, const rp_render_params* p, uint32_t n_frames, const uint32_t* d_recv,
                     uint8_t* d_frames_bgra, uint64_t* d_counters, void* stream) {
  if (!s || !d_recv || !d_frames_bgra || !p) return fail(RP_EINVAL, "scene, params and buffers must be non-NULL");
  if (n_frames == 0 || n_frames > RP_MAX_FRAMES) return fail(RP_EINVAL, "n_frames must be 1..RP_MAX_FRAMES");
  if (reinterpret_cast<uintptr_t>(d_frames_bgra) % 4 != 0) return fail(RP_EINVAL, "d_frames_bgra must be 4-byte aligned");
  if (!w) w = &s->ws0;
  GatherPlan gp;
  int rc = gather_plan(s, w, p->num_shards ? (int)p->num_shards : 1, (int)p->shard, p, gp, n_frames);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  DeviceGuard g(s->device);
  RP_HIP(hipMemcpyAsync(w->d_pack_recv.get(), d_recv, sizeof(uint32_t) * pack_words(gp.t, true, n_frames) * gp.geom.nranks,
                        hipMemcpyDeviceToDevice, st));
  if ((rc = gather_learn(s, w, gp, p, true, st))) return rc;
  return gather_assemble(s, w, gp, d_frames_bgra, nullptr, d_counters, st);
}

int rp_render_gather(rp_comm* c, rp_scene* s, rp_workspace* w, const rp_camera* cam, const rp_render_params* p,
                     uint8_t* d_frame_bgra, double* d_frame_rgb, uint64_t* d_counters, void* stream) {
  if (!c || !s) return fail(RP_EINVAL, "comm and scene must be non-NULL");
  if (!w) w = &s->ws0;
  Tiling t;
  int rc = frame_tiling(p, t);
  if (rc) return rc;
  if ((int)t.shards != c->nranks || (int)t.shard != c->rank)
    return fail(RP_EINVAL, "params.shard / num_shards must be the communicator's rank / size");
  if (3 * stage_slots(t) > w->d_gs_rgb.capacity())
    return fail(RP_EINVAL, "workspace not reserved for this frame's gather: call rp_workspace_reserve");
  if ((rc = render_shard(s, w, cam, p, w->d_gs_rgb.get(), nullptr, d_counters, stream))) return rc;
  return rp_frame_gather(c, s, w, p, w->d_gs_rgb.get(), d_frame_bgra, d_frame_rgb, d_counters, stream);
}

void rp_multi_destroy(rp_multi* m) { delete m; }

int rp_multi_create(const rp_scene_desc* desc, const int* devices, int n, const rp_scene_options* opt, rp_multi** out) {
  if (!out) return fail(RP_EINVAL, "out is NULL");
  *out = nullptr;
  if (!devices || n < 1) return fail(RP_EINVAL, "devices must list >= 1 device");
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (devices[a] == devices[b]) return fail(RP_EINVAL, "devices must be distinct");
  std::unique_ptr<rp_multi> m(new rp_multi());  // every return below releases what the ranks hold by then
  for (int k = 0; k < n; k++) {
    m->ranks.emplace_back(new rp_multi::Rank());
    m->ranks[k]->device = devices[k];
    rp_scene* s = nullptr;
    int rc = scene_create(desc, devices[k], opt, &s);
    if (rc) return rc;
    m->ranks[k]->scene.reset(s);
  }
  std::vector<ncclComm_t> comms(n, nullptr);
  ncclResult_t r = ncclCommInitAll(comms.data(), n, devices);
  if (r != ncclSuccess) return fail(RP_ERCCL, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
  for (int k = 0; k < n; k++) m->ranks[k]->comm = Comm(comms[k]);
  for (int k = 0; k < n; k++) {
    DeviceGuard g(devices[k]);
    if (hipStreamCreateWithFlags(m->ranks[k]->stream.put(), hipStreamNonBlocking) != hipSuccess ||
        !m->ranks[k]->d_ctr.alloc(rpk::CTR_N))
      return fail(RP_EHIP, "stream / counter allocation");
  }
  *out = m.release();
  return RP_OK;
}

int rp_render_multi(rp_multi* m, const rp_camera* cam, const rp_render_params* p_in, double* out_rgb, uint8_t* out_bgra,
                    rp_stats* stats) {
  if (!m || !cam || !p_in) return fail(RP_EINVAL, "multi, camera and params must be non-NULL");
  const int n = (int)m->ranks.size();
  const bool bgra = out_bgra != nullptr, rgb = out_rgb != nullptr;
  std::vector<rp_render_params> ps(n, *p_in);
  std::vector<GatherPlan> plans(n);
  for (int k = 0; k < n; k++) {
    ps[k].shard = (uint32_t)k;
    ps[k].num_shards = (uint32_t)n;
    rp_scene* s = m->ranks[k]->scene.get();
    int rc = ws_reserve(s, &s->ws0, &ps[k], true);
    if (rc) return rc;
  }
  rp_multi::Rank& r0 = *m->ranks[0];
  const uint64_t frame_px = (uint64_t)p_in->width * p_in->height;
  {
    DeviceGuard g(r0.device);
    if (!r0.d_frame_rgb.reserve(3 * frame_px) || !r0.d_frame_bgra.reserve(frame_px)) return fail(RP_ENOMEM, "hipMalloc frame");
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < n; k++) {  // every device renders its shard into its staging buffer
    rp_multi::Rank& r = *m->ranks[k];
    rp_scene* s = r.scene.get();
    double* d_shard = s->ws0.d_gs_rgb.get();
    int rc = render_shard(s, &s->ws0, cam, &ps[k], d_shard, nullptr, r.d_ctr.get(), r.stream.get());
    if (rc) return rc;
    if ((rc = gather_plan(s, &s->ws0, n, k, &ps[k], plans[k]))) return rc;
    if ((rc = gather_stage(s, &s->ws0, plans[k], d_shard, bgra, rgb, r.d_ctr.get(), r.stream.get()))) return rc;
  }
  // one thread drives every device: the collectives of all ranks form one group
  RP_NCCL(ncclGroupStart());
  for (int k = 0; k < n; k++) {
    rp_multi::Rank& r = *m->ranks[k];
    DeviceGuard g(r.device);
    int rc = gather_collectives(r.comm.get(), &r.scene->ws0, plans[k], bgra, rgb, r.stream.get());
    if (rc) {
      (void)ncclGroupEnd();
      return rc;
    }
  }
  RP_NCCL(ncclGroupEnd());
  for (int k = 0; k < n; k++) {
    rp_multi::Rank& r = *m->ranks[k];
    int rc = gather_learn(r.scene.get(), &r.scene->ws0, plans[k], &ps[k], bgra, r.stream.get());
    if (rc) return rc;
  }
  int rc = gather_assemble(r0.scene.get(), &r0.scene->ws0, plans[0], bgra ? reinterpret_cast<uint8_t*>(r0.d_frame_bgra.get()) : nullptr,
                           rgb ? r0.d_frame_rgb.get() : nullptr, r0.d_ctr.get(), r0.stream.get());
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    DeviceGuard g(m->ranks[k]->device);
    hipError_t e = hipStreamSynchronize(m->ranks[k]->stream.get());
    if (e != hipSuccess) return fail(RP_EHIP, std::string("render: ") + hipGetErrorString(e));
  }
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  DeviceGuard g(r0.device);
  uint64_t ctr[rpk::CTR_N];
  RP_HIP(hipMemcpy(ctr, r0.d_ctr.get(), sizeof ctr, hipMemcpyDeviceToHost));
  // status bits OR-ed over the devices (gather_assemble)
  if (ctr[rpk::CTR_STATUS] & rpk::STATUS_STACK_OVERFLOW) return fail(RP_EINTERNAL, "traversal stack overflow");
  if (ctr[rpk::CTR_STATUS] & rpk::STATUS_PLAN_MISMATCH) return fail(RP_EINTERNAL, "devices made different tile plans");
  if (ctr[rpk::CTR_STATUS]) return fail(RP_EINTERNAL, "render kernel reported status " + std::to_string(ctr[rpk::CTR_STATUS]));
  if (rgb) RP_HIP(hipMemcpy(out_rgb, r0.d_frame_rgb.get(), sizeof(double) * 3 * frame_px, hipMemcpyDeviceToHost));
  if (bgra) RP_HIP(hipMemcpy(out_bgra, r0.d_frame_bgra.get(), 4 * frame_px, hipMemcpyDeviceToHost));
  if (stats) {
    stats->rays = ctr[rpk::CTR_RAYS];
    stats->samples = ctr[rpk::CTR_SAMPLES];
    stats->pixels = ctr[rpk::CTR_PIXELS];
    stats->seconds = secs;
  }
  return RP_OK;
}

}  // extern "C"
