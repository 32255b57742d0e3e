// capi_redundancy.hip -- keyframe redundancy through the C boundary (bahip_keyframe_observer_histogram): clear and sweep of
// kernels_redundancy.hip on the caller's rows; under surfel sharding with a transport the sweep fills compact words the context owns,
// which are summed over the ranks as int64 and then written into the caller's rows.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kStageClear = 1, kStageTraversal = 2, kStageAttribution = 4, kStageAll = 7;
RedundancyShape g_shape{kRedundancyDefaultWaves, 0, kRedundancyDefaultListCapacity};   // workgroups 0: kRedundancyWorkgroupsPerUnit per compute unit
int g_tile_order = 1;
int g_stages = kStageAll;   // what a call launches (scripts/keyframe_redundancy_eval.py times the stages by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kRedundancyWorkgroupsPerUnit * units;
}
}  // namespace

extern "C" {
int bahip_keyframe_observer_histogram(bahip_context* ctx, const bahip_surfels* surfels, int bins, uint32_t* hist, int pitch_words) {
  // every refusal comes before the first launch
  REQUIRE(ctx != nullptr && surfels != nullptr && hist != nullptr, "bahip_keyframe_observer_histogram: no context, no surfels or no hist");
  REQUIRE(bins >= 1 && bins <= kRedundancyMaxBins, "bahip_keyframe_observer_histogram: bins outside 1 .. 64");
  REQUIRE(pitch_words >= bins, "bahip_keyframe_observer_histogram: pitch_words is smaller than bins");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_keyframe_observer_histogram: no surfel data");
  const int K = ctx->num_kfs;
  if (K == 0) return 0;
  if (observed_structure_by_table(ctx)) {   // (capi_tile_masks.hip)
    REQUIRE(K < 65536, "bahip_keyframe_observer_histogram: more than 65 535 bound keyframes for the tile mask table");
    return tile_mask_histogram(ctx, surfels, bins, hist, pitch_words);
  }
  ctx->tile_mask_valid = false;   // (this call builds no table)
  if (ctx->redundancy_census.reserve(3, 0, "the keyframe redundancy census")) return 1;
  const bool exchange = is_sharded(ctx);   // (an empty surfel shard must still join the exchange of the others)
  const size_t words = (size_t)K * (size_t)bins;
  uint32_t* rows = hist;
  uint32_t pitch = (uint32_t)pitch_words;
  long long* wide = nullptr;
  if (exchange) {
    // [words int64 | words uint32]
    if (ctx->redundancy_stage.reserve(words + (words + 1) / 2, 0, "the keyframe redundancy words of a shard")) return 1;
    wide = ctx->redundancy_stage;
    rows = reinterpret_cast<uint32_t*>(wide + words);
    pitch = (uint32_t)bins;
  }
  Intrinsics in = ctx->in;
  in.fast_math = 0;   // (read by dispatchers only; this unit has one flavour)
  const SurfelsView v = make_view(surfels);
  HIP_TRY(hipMemsetAsync(ctx->redundancy_census, 0, 3 * sizeof(unsigned long long), ctx->stream));
  if (g_stages & kStageClear) {
    launch_redundancy_clear(ctx->stream, rows, K, bins, pitch);
    CHECK_LAUNCH();
  }
  if ((g_stages & kStageTraversal) && v.size > 0) {
    const uint32_t* sched = g_tile_order ? tile_order_for(ctx, v.size) : nullptr;
    const RedundancyShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups(), g_shape.list_capacity};
    launch_redundancy_sweep(ctx->stream, in, ctx->dev_kfs, K, v, sched, shape, (g_stages & kStageAttribution) != 0, bins, rows, pitch,
                            ctx->redundancy_census);
    CHECK_LAUNCH();
  }
  if (exchange) {
    launch_redundancy_widen(ctx->stream, rows, (uint32_t)words, wide);
    CHECK_LAUNCH();
    if (reduce_over_ranks(ctx, wide, words, BAHIP_SUM_I64))
      return fail(("keyframe redundancy: the sum of the table over the ranks failed (" + g_last_error + ")").c_str(), __FILE__, __LINE__);
    launch_redundancy_narrow(ctx->stream, wide, K, bins, hist, (uint32_t)pitch_words);
    CHECK_LAUNCH();
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_set_redundancy_shape(int waves, int workgroups, int list_capacity, int tile_order) {
  if (waves < 0 || waves > kRedundancyMaxWaves || workgroups < 0 || list_capacity < 0 || list_capacity > kRedundancyMaxListCapacity ||
      tile_order < -1 || tile_order > 1)
    return fail("bahip_debug_set_redundancy_shape: waves 0 .. 8, workgroups >= 0, list_capacity 0 .. 448, tile_order -1 .. 1", __FILE__, __LINE__,
                hipSuccess);
  g_shape.waves = waves ? waves : kRedundancyDefaultWaves;
  g_shape.workgroups = workgroups;
  g_shape.list_capacity = list_capacity ? list_capacity : kRedundancyDefaultListCapacity;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  return 0;
}

int bahip_debug_set_redundancy_stages(int stages) {
  if (stages < 0 || stages > kStageAll) return fail("bahip_debug_set_redundancy_stages: stages 0 .. 7", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}

int bahip_debug_redundancy_census(bahip_context* ctx, uint64_t out[3]) {
  REQUIRE(ctx != nullptr && out != nullptr, "bahip_debug_redundancy_census: no context or no output");
  out[0] = out[1] = out[2] = 0;
  if (!ctx->redundancy_census.get()) return 0;   // no call yet
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the census words are 64 bits");
  HIP_TRY(hipMemcpyAsync(out, ctx->redundancy_census, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // extern "C"
