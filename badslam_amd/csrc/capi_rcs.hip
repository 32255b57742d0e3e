// capi_rcs.hip -- the reduced camera system through the C boundary (bahip_reduced_camera_system): the pose sums of every bound keyframe
// by the pose sweep (kernels_pose.hip: launch_pose_accumulate, exact flavour), the surfel stage of kernels_rcs.hip, the sum of all the
// integer words over the ranks of a surfel partition, and the resolution into the caller's planes.  The sums live in one block that
// exists for the call only.
#include <algorithm>

#include "capi_internal.h"
#include "rcs_launch.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
RcsShape g_shape{kRcsDefaultWaves, 0, kRcsDefaultListCapacity};   // workgroups 0: kRcsWorkgroupsPerUnit per compute unit
int g_tile_order = 1;
constexpr int kStagePose = 1, kStageFactor = 2, kStagePairs = 4, kStageResolve = 8, kStageAll = 15;
int g_stages = kStageAll;   // what a call launches (scripts/reduced_camera_system_eval.py times the stages by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kRcsWorkgroupsPerUnit * units;
}
}  // namespace

extern "C" {
int bahip_reduced_camera_system(bahip_context* ctx, int use_depth, int use_desc, int marginalise, const bahip_surfels* surfels, double* S,
                                size_t pitch_doubles, double* g, double* A_diag, double* b, bahip_rcs_stats* stats) {
  // every refusal comes before the first launch
  REQUIRE(ctx != nullptr && surfels != nullptr && S != nullptr && g != nullptr, "bahip_reduced_camera_system: no context, no surfels, no S or no g");
  const int K = ctx->num_kfs;
  REQUIRE(K > 0, "bahip_reduced_camera_system: no keyframe is bound");
  REQUIRE(use_depth || use_desc, "bahip_reduced_camera_system: at least one residual type must be enabled");
  REQUIRE(pitch_doubles >= 6 * (size_t)K, "bahip_reduced_camera_system: pitch_doubles is smaller than six times the number of bound keyframes");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(!kf_sharded(ctx), "bahip_reduced_camera_system is not available under keyframe sharding (a rank lacks the other ranks' pairs): use surfel sharding");
  REQUIRE(K < 65536, "bahip_reduced_camera_system: more than 65 535 bound keyframes");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_reduced_camera_system: no surfel data");

  // [Hb K x kHbStride | census | blocks | v]
  const size_t hb_words = (size_t)K * kHbStride;
  const size_t block_words = marginalise ? rcs_block_index((size_t)K, 0) * kRcsBlockWords : 0, v_words = marginalise ? (size_t)K * kRcsVWords : 0;
  const size_t words = hb_words + kRcsCensusWords + block_words + v_words;
  DeviceBuffer<long long> sums;
  DeviceBuffer<PoseWork> work;
  if (sums.reserve(words, 0, "the sums of the reduced camera system")) return 1;
  if (work.reserve(pose_work_records((size_t)K), 0, "the work items of the reduced camera system")) return 1;
  HbFixed* Hb = sums;
  long long* census = sums + hb_words;
  long long* blocks = marginalise ? census + kRcsCensusWords : nullptr;
  long long* v = marginalise ? blocks + block_words : nullptr;

  Intrinsics in = ctx->in;
  in.fast_math = 0;   // the exact flavour of the pose sweep; the surfel stage has one flavour
  const SurfelsView view = make_view(surfels);
  HIP_TRY(hipMemsetAsync(sums, 0, words * sizeof(long long), ctx->stream));
  if (view.size > 0) {
    launch_rcs_work(ctx->stream, ctx->dev_kfs, K, work);
    CHECK_LAUNCH();
    if (ensure_tile_bounds(ctx, view.size)) return 1;
    if (g_stages & kStagePose) {
      launch_pose_accumulate(ctx->stream, use_depth != 0, use_desc != 0, in, ctx->dev_kfs, work, K, view, Hb, ctx->dev_tile_bounds,
                             /*stored_bounds*/ false, /*num_listed*/ 0, ctx->dev_tile_counters, &ctx->pose_parity);
      CHECK_LAUNCH();
    }
    if (marginalise && (g_stages & kStageFactor)) {
      const uint32_t* sched = g_tile_order ? tile_order_for(ctx, view.size) : nullptr;
      const RcsShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups(), g_shape.list_capacity};
      if (!launch_rcs_sweep(ctx->stream, use_depth != 0, use_desc != 0, in, ctx->dev_kfs, K, view, sched, shape, (g_stages & kStagePairs) != 0, blocks, v, census)) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return fail("bahip_reduced_camera_system: the launch shape does not fit the LDS of a workgroup", __FILE__, __LINE__);
      }
      CHECK_LAUNCH();
    }
  }
  if (is_sharded(ctx) && reduce_over_ranks(ctx, sums, words, BAHIP_SUM_I64)) {   // (an empty surfel shard joins the exchange of the others)
    const std::string why = "reduced camera system: the sum of the limbs over the ranks failed (" + g_last_error + ")";
    hipStreamSynchronize(ctx->stream);   // the block dies with this call
    return fail(why.c_str(), __FILE__, __LINE__);
  }
  if (g_stages & kStageResolve) {
    launch_rcs_resolve(ctx->stream, K, Hb, blocks, v, S, pitch_doubles, g, A_diag, b, census);
    CHECK_LAUNCH();
  }
  long long host_census[kRcsCensusWords];
  HIP_TRY(hipMemcpyAsync(host_census, census, sizeof(host_census), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (stats) {
    stats->list_entries = (uint64_t)host_census[kRcsEntries];
    stats->pairs_visited = (uint64_t)host_census[kRcsPairs];
    stats->atomics_issued = (uint64_t)host_census[kRcsAtomics];
    stats->degenerate_surfels = (uint64_t)host_census[kRcsDegenerate];
    stats->overflow_tiles = (uint64_t)host_census[kRcsOverflowTiles];
    stats->invalid = host_census[kRcsInvalid] != 0 ? 1u : 0u;
  }
  return 0;
}

int bahip_debug_set_rcs_shape(int waves, int workgroups, int list_capacity, int tile_order) {
  const int w = waves ? waves : kRcsDefaultWaves, c = list_capacity ? list_capacity : kRcsDefaultListCapacity;
  if (waves < 0 || waves > kRcsMaxWaves || workgroups < 0 || list_capacity < 0 || list_capacity > kRcsMaxListCapacity || tile_order < -1 || tile_order > 1 ||
      (size_t)w * (size_t)c * rcs_entry_bytes(true) > kRcsMaxLdsBytes)
    return fail("bahip_debug_set_rcs_shape: waves 0 .. 4, workgroups >= 0, list_capacity 0 .. 32, tile_order -1 .. 1, waves x list_capacity x 4 620 bytes <= 160 KB",
                __FILE__, __LINE__, hipSuccess);
  g_shape.waves = w;
  g_shape.workgroups = workgroups;
  g_shape.list_capacity = c;
  g_tile_order = tile_order < 0 ? 1 : tile_order;
  return 0;
}

int bahip_debug_set_rcs_stages(int stages) {
  if (stages < 0 || stages > kStageAll) return fail("bahip_debug_set_rcs_stages: stages 0 .. 15", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}

int bahip_debug_set_rcs_list_capacity(int list_capacity) {
  return bahip_debug_set_rcs_shape(g_shape.waves, g_shape.workgroups, list_capacity, g_tile_order);
}
}  // extern "C"
