// capi_covisibility.hip -- observed co-visibility through the C boundary (bahip_observed_covisibility): clear, sweep and mirror of
// kernels_covisibility.hip on the caller's rows; under surfel sharding with a transport the sweep fills compact words the context owns,
// which are summed over the ranks as int64 and then written into the caller's rows.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kStageClear = 1, kStageTraversal = 2, kStagePairs = 4, kStageAll = 7;
CovisShape g_shape{kCovisDefaultWaves, 0, kCovisDefaultListCapacity};   // workgroups 0: kCovisWorkgroupsPerUnit per compute unit
int g_tile_order = 1;
int g_stages = kStageAll;   // what a call launches (scripts/covisibility_eval.py times the stages by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kCovisWorkgroupsPerUnit * units;
}
}  // namespace

extern "C" {
int bahip_observed_covisibility(bahip_context* ctx, const bahip_surfels* surfels, uint32_t* counts, int pitch_words) {
  // every refusal comes before the first launch
  REQUIRE(ctx != nullptr && surfels != nullptr && counts != nullptr, "bahip_observed_covisibility: no context, no surfels or no counts");
  const int K = ctx->num_kfs;
  REQUIRE(pitch_words >= K, "bahip_observed_covisibility: pitch_words is smaller than the number of bound keyframes");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  REQUIRE(K < 65536, "bahip_observed_covisibility: more than 65 535 bound keyframes");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_observed_covisibility: no surfel data");
  if (K == 0) return 0;
  if (observed_structure_by_table(ctx)) return tile_mask_covisibility(ctx, surfels, counts, pitch_words);   // (capi_tile_masks.hip)
  ctx->tile_mask_valid = false;   // (this call builds no table)
  if (ctx->covis_census.reserve(3, 0, "the co-visibility census")) return 1;
  const bool exchange = is_sharded(ctx);   // (an empty surfel shard must still join the exchange of the others)
  const size_t words = (size_t)K * (size_t)K;
  uint32_t* rows = counts;
  uint32_t pitch = (uint32_t)pitch_words;
  long long* wide = nullptr;
  if (exchange) {
    // [words int64 | words uint32]
    if (ctx->covis_stage.reserve(words + (words + 1) / 2, 0, "the co-visibility words of a shard")) return 1;
    wide = ctx->covis_stage;
    rows = reinterpret_cast<uint32_t*>(wide + words);
    pitch = (uint32_t)K;
  }
  Intrinsics in = ctx->in;
  in.fast_math = 0;   // (read by dispatchers only; this unit has one flavour)
  const SurfelsView v = make_view(surfels);
  HIP_TRY(hipMemsetAsync(ctx->covis_census, 0, 3 * sizeof(unsigned long long), ctx->stream));
  if (g_stages & kStageClear) {
    launch_covisibility_clear(ctx->stream, rows, K, pitch);
    CHECK_LAUNCH();
  }
  if ((g_stages & kStageTraversal) && v.size > 0) {
    const uint32_t* sched = g_tile_order ? tile_order_for(ctx, v.size) : nullptr;
    const CovisShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups(), g_shape.list_capacity};
    launch_covisibility_sweep(ctx->stream, in, ctx->dev_kfs, K, v, sched, shape, (g_stages & kStagePairs) != 0, rows, pitch, ctx->covis_census);
    CHECK_LAUNCH();
    if (g_stages & kStagePairs) {   // the sweep sums the lower triangle
      launch_covisibility_mirror(ctx->stream, rows, K, pitch);
      CHECK_LAUNCH();
    }
  }
  if (exchange) {
    launch_covisibility_widen(ctx->stream, rows, K, wide);
    CHECK_LAUNCH();
    if (reduce_over_ranks(ctx, wide, words, BAHIP_SUM_I64))
      return fail(("observed co-visibility: the sum of the counts over the ranks failed (" + g_last_error + ")").c_str(), __FILE__, __LINE__);
    launch_covisibility_narrow(ctx->stream, wide, K, counts, (uint32_t)pitch_words);
    CHECK_LAUNCH();
  }
  return 0;
}

int bahip_debug_set_covisibility_shape(int waves, int workgroups, int list_capacity, int tile_order) {
  if (waves < 0 || waves > kCovisMaxWaves || workgroups < 0 || list_capacity < 0 || list_capacity > kCovisMaxListCapacity || tile_order < -1 ||
      tile_order > 1)
    return fail("bahip_debug_set_covisibility_shape: waves 0 .. 8, workgroups >= 0, list_capacity 0 .. 512, tile_order -1 .. 1", __FILE__, __LINE__,
                hipSuccess);
  g_shape.waves = waves ? waves : kCovisDefaultWaves;
  g_shape.workgroups = workgroups;
  g_shape.list_capacity = list_capacity ? list_capacity : kCovisDefaultListCapacity;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  return 0;
}

int bahip_debug_set_covisibility_stages(int stages) {
  if (stages < 0 || stages > kStageAll) return fail("bahip_debug_set_covisibility_stages: stages 0 .. 7", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}

int bahip_debug_covisibility_census(bahip_context* ctx, uint64_t out[3]) {
  REQUIRE(ctx != nullptr && out != nullptr, "bahip_debug_covisibility_census: no context or no output");
  out[0] = out[1] = out[2] = 0;
  if (!ctx->covis_census.get()) return 0;   // no call yet
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the census words are 64 bits");
  HIP_TRY(hipMemcpyAsync(out, ctx->covis_census, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // extern "C"
