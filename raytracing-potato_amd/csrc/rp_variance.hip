// rp_variance.hip -- the per-pixel variance pass (include/rp.h rp_render_variance_device_ws): the
// variance of every pixel's mean, estimated from the spread of the batch sums a multi-batch render leaves in its
// workspace (rp_workspace::d_partial, 3 f64 per unit at slot * nbatch + b; reduce_batches_kernel reads them once for the
// frame and nothing reads them again).  No ray is traced.  The arithmetic is rp_variance.h's, shared with the CPU loop
// behind rph_batch_variance; this file is the kernel, its launch and the C-ABI.
//
// A translation unit of its own, linked into librp.so and librp_diag.so and, like rp_aov.hip and rp_denoise.hip, not
// part of the rp_build_id hash: it runs after the render and decides no ray of it.
//
// Kernel: one lane per shard slot (the render's compact shard order, rp_units.h slot_pixel's decode); a lane reads its
// pixel's 3 B sums -- 24 B consecutive bytes -- twice (the second pass hits the cache) and writes 3 doubles.  Slots of
// edge tiles outside the frame are not written.  No allocation, no synchronisation, one launch on the caller's stream.
#include "rp_pass.h"  // first: the HIP runtime defines the qualifiers the shared headers use

#include "rp_units.h"
#include "rp_variance.h"

#pragma clang fp contract(off)

namespace rpv {

constexpr int VAR_BLOCK = 256;

struct VarArgs {
  rpp::ShardView v;
  uint32_t spp, sps, nbatch;
  const double* partial;     // 3 per unit, unit = slot * nbatch + b
  double* var;               // 3 per slot
};

__global__ void __launch_bounds__(VAR_BLOCK) variance_kernel(const VarArgs A) {
  const uint64_t slot = (uint64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (slot >= A.v.n_slots) return;
  uint32_t pi, pj;
  if (!rpk::slot_pixel(A.v, slot, pi, pj)) return;
  const double* S = A.partial + 3 * slot * A.nbatch;
#pragma unroll
  for (uint32_t c = 0; c < 3; c++) A.var[3 * slot + c] = batch_variance(S + c, 3, A.nbatch, A.spp, A.sps);
}

}  // namespace rpv

extern "C" {

int rp_render_variance_device_ws(rp_scene* s, rp_workspace* w, const rp_render_params* p, double* d_shard_var,
                                 void* stream) {
  int rc = use_ws(s, w);
  if (rc) return rc;
  if (!d_shard_var) return fail(RP_EINVAL, "d_shard_var is NULL");
  Tiling t;
  rpv::VarArgs a;
  if ((rc = rpp::shard_view(w, p, t, a.v))) return rc;
  if (t.nbatch < 2)
    return fail(RP_EINVAL, "the variance needs at least two sample batches per pixel (spp > samples_per_stream)");
  const uint64_t units = t.n_slots * t.nbatch;
  if (3 * units > w->d_partial.capacity() || units > w->d_partial_hits.capacity())
    return fail(RP_EINVAL, "the workspace holds no batch sums of this shape: reserve it (rp_workspace_reserve) and "
                           "render the frame first");
  if (t.n_slots == 0) return RP_OK;
  a.spp = p->spp, a.sps = t.sps, a.nbatch = t.nbatch;
  a.partial = w->d_partial.get();
  a.var = d_shard_var;
  DeviceGuard g(s->device);
  const uint64_t grid = (t.n_slots + rpv::VAR_BLOCK - 1) / rpv::VAR_BLOCK;  // n_slots < 2^32: < 2^24 blocks
  hipLaunchKernelGGL(rpv::variance_kernel, dim3((unsigned)grid), dim3(rpv::VAR_BLOCK), 0, (hipStream_t)stream, a);
  RP_HIP(hipGetLastError());
  return RP_OK;
}

}  // extern "C"
