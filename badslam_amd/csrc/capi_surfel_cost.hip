// capi_surfel_cost.hip -- the value of the BA objective per surfel through the C boundary (bahip_evaluate_surfel_costs): one sweep
// (kernels_surfel_cost.hip) that resolves every surfel's sums itself; under keyframe sharding the sweep stages integer words in slices of
// surfels, each slice summed over the ranks and resolved on the device.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kDefaultSliceSurfels = 65536;   // 65 536 x kCostWords x 8 bytes = 15.7 MB of staged words per exchange
SurfelCostShape g_shape{kSurfelCostDefaultWaves, 0};   // workgroups 0: kSurfelCostWorkgroupsPerUnit per compute unit
int g_slice_surfels = kDefaultSliceSurfels;
int g_tile_order = 1;
const char* const kOptInRefused = "bahip_evaluate_surfel_costs: the LDS of more than 4 wavefronts per workgroup was refused (hipFuncSetAttribute)";

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kSurfelCostWorkgroupsPerUnit * units;
}

int zero_fill(bahip_context* ctx, const SurfelCostPlanes& out, size_t n) {
  if (n == 0) return 0;
  for (double* plane : {out.depth, out.descriptor_1, out.descriptor_2})
    if (plane) HIP_TRY(hipMemsetAsync(plane, 0, sizeof(double) * n, ctx->stream));
  for (uint32_t* plane : {out.depth_residuals, out.descriptor_pairs})
    if (plane) HIP_TRY(hipMemsetAsync(plane, 0, sizeof(uint32_t) * n, ctx->stream));
  return 0;
}
}  // namespace

extern "C" {
int bahip_evaluate_surfel_costs(bahip_context* ctx, int use_depth, int use_desc, const bahip_surfels* surfels, const bahip_surfel_costs* out) {
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(surfels != nullptr && out != nullptr, "bahip_evaluate_surfel_costs: no surfels or no output planes");
  const SurfelCostPlanes planes{out->depth, out->descriptor_1, out->descriptor_2, out->depth_residuals, out->descriptor_pairs};
  const SurfelsView v = make_view(surfels);
  const uint32_t N = v.size;
  const int K = ctx->num_kfs;
  if (K == 0 || (!use_depth && !use_desc)) return zero_fill(ctx, planes, N);
  if (N == 0) return 0;   // (the slices of a keyframe partition derive from N: no rank exchanges anything)
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  const uint32_t* sched = g_tile_order ? tile_order_for(ctx, N) : nullptr;
  const SurfelCostShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups()};
  hipError_t e = hipSuccess;
  if (!kf_sharded(ctx)) {
    // unsharded, or a surfel shard: a surfel's cost needs its own rows and the bound keyframes only -- nothing to exchange
    launch_surfel_cost(ctx->stream, use_depth != 0, use_desc != 0, ctx->in, ctx->dev_kfs, K, 0, 1, v, 0, N, sched, shape, planes, nullptr, 0, &e);
    if (e != hipSuccess) return fail(kOptInRefused, __FILE__, __LINE__, e);
    CHECK_LAUNCH();
    return 0;
  }
  const uint32_t slice = std::min((uint32_t)g_slice_surfels, (N + 63u) / 64u * 64u);
  if (ctx->dev_surfel_cost_rows.reserve((size_t)kCostWords * slice, 0, "the surfel cost rows")) return 1;
  long long* rows = ctx->dev_surfel_cost_rows;
  for (uint32_t begin = 0; begin < N; begin += slice) {
    const uint32_t count = std::min(slice, N - begin);
    launch_surfel_cost(ctx->stream, use_depth != 0, use_desc != 0, ctx->in, ctx->dev_kfs, K, ctx->kf_rank, ctx->kf_world, v, begin, begin + count,
                       sched, shape, planes, rows, count, &e);
    if (e != hipSuccess) return fail(kOptInRefused, __FILE__, __LINE__, e);
    CHECK_LAUNCH();
    if (reduce_over_ranks(ctx, rows, (size_t)kCostWords * count, BAHIP_SUM_I64))
      return fail(("surfel cost evaluation: the sum of the surfel cost rows over the ranks failed (" + g_last_error + ")").c_str(), __FILE__, __LINE__);
    launch_surfel_cost_resolve(ctx->stream, rows, count, begin, count, planes);
    CHECK_LAUNCH();
  }
  return 0;
}

int bahip_debug_set_surfel_cost_shape(int waves, int workgroups, int slice_surfels, int tile_order) {
  if (waves < 0 || waves > kSurfelCostMaxWaves || workgroups < 0 || slice_surfels < 0 || slice_surfels % 64 != 0 || tile_order < -1 || tile_order > 1)
    return fail("bahip_debug_set_surfel_cost_shape: waves 0 .. 8, workgroups >= 0, slice_surfels >= 0 and a multiple of 64, tile_order -1 .. 1",
                __FILE__, __LINE__, hipSuccess);
  g_shape.waves = waves ? waves : kSurfelCostDefaultWaves;
  g_shape.workgroups = workgroups;
  g_slice_surfels = slice_surfels ? slice_surfels : kDefaultSliceSurfels;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  return 0;
}
}  // extern "C"
