// capi_observations.hip -- observation lists through the C boundary (bahip_surfel_observations): the count sweep of
// kernels_observations.hip into counts the context owns, the 64-bit total read back, the exclusive scan into the caller's surfel_first
// and, when the caller's planes hold the pairs, the fill sweep.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kStageCount = 1, kStageScan = 2, kStageFill = 4, kStageAll = 7;
constexpr uint64_t kDefaultPairLimit = 0xffffffffull;   // surfel_first holds 32-bit words
// the default fill ("Observation lists": which form won on the bench scene); the other stays behind the hook
constexpr bool kDefaultStaged = true;
ObsShape g_shape{kObsDefaultWaves, 0, kDefaultStaged ? kObsDefaultStageEntries : 0};   // workgroups 0: kObsWorkgroupsPerUnit per compute unit
int g_tile_order = 1;
int g_stages = kStageAll;   // what a call launches (scripts/surfel_observations_eval.py times the stages by difference)
uint64_t g_pair_limit = kDefaultPairLimit;

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kObsWorkgroupsPerUnit * units;
}
}  // namespace

extern "C" {
int bahip_surfel_observations(bahip_context* ctx, const bahip_surfels* surfels, const bahip_observations* out, uint64_t* pairs) {
  // every refusal comes before the first launch
  REQUIRE(ctx != nullptr && surfels != nullptr && out != nullptr && pairs != nullptr,
          "bahip_surfel_observations: no context, no surfels, no output or no pair count");
  REQUIRE(out->surfel_first != nullptr, "bahip_surfel_observations: no surfel_first");
  REQUIRE(out->keyframes != nullptr || (out->depth_raw == nullptr && out->descriptor_raw == nullptr),
          "bahip_surfel_observations: a payload plane (depth_raw, descriptor_raw) without keyframes");
  const int K = ctx->num_kfs;
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  REQUIRE(K < 65536, "bahip_surfel_observations: more than 65 535 bound keyframes");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_surfel_observations: no surfel data");
  const SurfelsView v = make_view(surfels);
  const size_t words = (size_t)v.size + 1;
  REQUIRE(words <= (size_t)0x7fffffff, "bahip_surfel_observations: too many surfels for the scan");
  if (K == 0 || v.size == 0) {
    HIP_TRY(hipMemsetAsync(out->surfel_first, 0, words * sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *pairs = 0;
    return 0;
  }
  if (observed_structure_by_table(ctx)) return tile_mask_observations(ctx, surfels, out, g_pair_limit, pairs);   // (capi_tile_masks.hip)
  ctx->tile_mask_valid = false;   // (this call builds no table)
  if (ctx->obs_counts.reserve(words, words / 8, "the observation counts")) return 1;
  if (ctx->obs_total.reserve(1, 0, "the observation total")) return 1;
  if (ctx->obs_scan_temp.reserve(scan_temp_bytes(words), 0, "the scan of the observation counts")) return 1;
  Intrinsics in = ctx->in;
  in.fast_math = 0;   // (read by dispatchers only; this unit has one flavour)
  const uint32_t* sched = g_tile_order ? tile_order_for(ctx, v.size) : nullptr;
  const ObsShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups(), g_shape.stage_entries};
  uint64_t P = 0;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the total is 64 bits");
  if (g_stages & kStageCount) {
    HIP_TRY(hipMemsetAsync(ctx->obs_total, 0, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->obs_counts + v.size, 0, sizeof(uint32_t), ctx->stream));   // the last input of the scan
    launch_observations_count(ctx->stream, in, ctx->dev_kfs, K, v, sched, shape, ctx->obs_counts, ctx->obs_total);
    CHECK_LAUNCH();
    HIP_TRY(hipMemcpyAsync(&P, ctx->obs_total, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (P > g_pair_limit) {
    char text[160];
    snprintf(text, sizeof(text), "bahip_surfel_observations: %llu pairs are more than the pair limit of %llu", (unsigned long long)P,
             (unsigned long long)g_pair_limit);
    return fail(text, __FILE__, __LINE__);
  }
  if ((g_stages & kStageScan) && (g_stages & kStageCount)) {
    HIP_TRY(scan_u32_exclusive(ctx->stream, ctx->obs_scan_temp, ctx->obs_scan_temp.size(), ctx->obs_counts, out->surfel_first, (int)words));
    if ((g_stages & kStageFill) && out->keyframes != nullptr && P <= out->capacity && P > 0) {
      const ObsPlanes planes{out->keyframes, out->depth_raw, out->descriptor_raw};
      launch_observations_fill(ctx->stream, in, ctx->dev_kfs, K, v, sched, shape, out->surfel_first, planes);
      CHECK_LAUNCH();
    }
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *pairs = P;
  return 0;
}

int bahip_debug_set_observations_shape(int waves, int workgroups, int stage_entries, int tile_order, uint64_t pair_limit) {
  if (waves < 0 || waves > kObsMaxWaves || workgroups < 0 || stage_entries < -2 || stage_entries > kObsMaxStageEntries || tile_order < -1 ||
      tile_order > 1)
    return fail("bahip_debug_set_observations_shape: waves 0 .. 8, workgroups >= 0, stage_entries -2 .. 4096, tile_order -1 .. 1", __FILE__, __LINE__,
                hipSuccess);
  g_shape.waves = waves ? waves : kObsDefaultWaves;
  g_shape.workgroups = workgroups;
  if (stage_entries == 0) g_shape.stage_entries = kDefaultStaged ? kObsDefaultStageEntries : 0;
  else if (stage_entries == -1) g_shape.stage_entries = 0;
  else if (stage_entries == -2) g_shape.stage_entries = kObsDefaultStageEntries;
  else g_shape.stage_entries = stage_entries;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  g_pair_limit = pair_limit ? std::min(pair_limit, kDefaultPairLimit) : kDefaultPairLimit;
  return 0;
}

int bahip_debug_set_observations_stages(int stages) {
  if (stages != 0 && stages != kStageCount && stages != (kStageCount | kStageScan) && stages != kStageAll)
    return fail("bahip_debug_set_observations_stages: stages 0, 1, 3 or 7 (the scan needs the count, the fill needs both)", __FILE__, __LINE__,
                hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}
}  // extern "C"
