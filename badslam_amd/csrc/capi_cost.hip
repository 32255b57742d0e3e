// capi_cost.hip -- the value of the BA objective through the C boundary (bahip_evaluate_cost, bahip_evaluate_frame_cost): one sweep
// (kernels_cost.hip), the integer rows summed over the ranks, the limbs resolved to binary64 on the device.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
CostShape g_cost_shape{8, 0, kCostMaxSlice};   // workgroups 0: two per compute unit
int g_cost_tile_order = 1;

int cost_workgroups() {
  if (g_cost_shape.workgroups > 0) return g_cost_shape.workgroups;
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return 2 * units;
}

// One sweep of `num` frames of the table `frames`, the rows summed over the ranks when `exchange`, resolved on the device
// (exact_sum.h: exact_value): out[0 .. num) per frame, out[num] the total from the summed limbs.
int cost_eval(bahip_context* ctx, bool use_depth, bool use_desc, const KfEntry* frames, int num, bool owned_only, bool exchange,
              const bahip_surfels* surfels, std::vector<bahip_cost>* out) {
  static_assert(sizeof(bahip_cost) == 5 * sizeof(long long), "bahip_cost is resolved into 5 words");
  const size_t row_words = (size_t)num * kCostWords, words = row_words + kCostWords + 5 * ((size_t)num + 1);
  if (ctx->dev_cost.reserve(words, 0, "the cost rows")) return 1;
  long long* rows = ctx->dev_cost;
  long long* total = rows + row_words;
  bahip_cost* resolved = reinterpret_cast<bahip_cost*>(total + kCostWords);
  HIP_TRY(hipMemsetAsync(rows, 0, sizeof(long long) * (row_words + kCostWords), ctx->stream));
  const SurfelsView v = make_view(surfels);
  const uint32_t* sched = g_cost_tile_order ? tile_order_for(ctx, v.size) : nullptr;
  const CostShape shape{g_cost_shape.waves, cost_workgroups(), g_cost_shape.slice};
  // (an empty shard launches nothing but still takes part in the exchange)
  launch_cost(ctx->stream, use_depth, use_desc, ctx->in, frames, num, owned_only ? ctx->kf_rank : 0, owned_only ? ctx->kf_world : 1, v, sched,
              shape, rows);
  CHECK_LAUNCH();
  if (exchange && reduce_over_ranks(ctx, rows, row_words, BAHIP_SUM_I64))
    return fail(("cost evaluation: the sum of the cost rows over the ranks failed (" + g_last_error + ")").c_str(), __FILE__, __LINE__);
  launch_cost_resolve(ctx->stream, rows, num, total, resolved);
  CHECK_LAUNCH();
  out->resize((size_t)num + 1);
  HIP_TRY(hipMemcpyAsync(out->data(), resolved, sizeof(bahip_cost) * ((size_t)num + 1), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}
}  // namespace

extern "C" {
int bahip_evaluate_cost(bahip_context* ctx, int use_depth, int use_desc, const bahip_surfels* surfels, bahip_cost* total,
                        bahip_cost* per_keyframe) {
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(surfels != nullptr, "bahip_evaluate_cost: no surfels");
  const int K = ctx->num_kfs;
  if (total) *total = bahip_cost{};
  if (per_keyframe) std::fill(per_keyframe, per_keyframe + K, bahip_cost{});
  // (the same on every rank; an empty surfel shard must still join the exchange of the others)
  if (K == 0 || (!use_depth && !use_desc)) return 0;
  if (surfels->surfels_size == 0 && !is_sharded(ctx)) return 0;
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  std::vector<bahip_cost> out;
  if (cost_eval(ctx, use_depth != 0, use_desc != 0, ctx->dev_kfs, K, /*owned_only*/ true, /*exchange*/ true, surfels, &out)) return 1;
  if (per_keyframe) std::copy(out.begin(), out.begin() + K, per_keyframe);
  if (total) *total = out[K];
  return 0;
}

int bahip_evaluate_frame_cost(bahip_context* ctx, int use_depth, int use_desc, const bahip_frame* frame, const float frame_T_global[12],
                              const bahip_surfels* surfels, bahip_cost* out) {
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(frame != nullptr && frame_T_global != nullptr && surfels != nullptr && out != nullptr, "bahip_evaluate_frame_cost: bad arguments");
  *out = bahip_cost{};
  // keyframe sharding: every rank holds all surfels, one frame's sums are complete on each (no exchange); surfel sharding: an empty
  // shard still joins the exchange of the others
  const bool exchange = !kf_sharded(ctx);
  if (!use_depth && !use_desc) return 0;
  if (surfels->surfels_size == 0 && !(exchange && is_sharded(ctx))) return 0;
  KfEntry e;
  if (make_entry(ctx, *frame, 0, &e)) return 1;
  memcpy(e.pose.F, frame_T_global, 12 * sizeof(float));
  HIP_TRY(hipMemcpyAsync(ctx->dev_frame1, &e, sizeof(e), hipMemcpyHostToDevice, ctx->stream));
  std::vector<bahip_cost> res;
  if (cost_eval(ctx, use_depth != 0, use_desc != 0, ctx->dev_frame1, 1, /*owned_only*/ false, exchange, surfels, &res)) return 1;
  *out = res[0];
  return 0;
}

int bahip_debug_set_cost_shape(int waves, int workgroups, int slice, int tile_order) {
  if (waves < 0 || waves > kCostMaxWaves || workgroups < 0 || slice < 0 || slice > kCostMaxSlice || tile_order < -1 || tile_order > 1)
    return fail("bahip_debug_set_cost_shape: waves 0 .. 8, workgroups >= 0, slice 0 .. 256, tile_order -1 .. 1", __FILE__, __LINE__, hipSuccess);
  g_cost_shape.waves = waves ? waves : 8;
  g_cost_shape.workgroups = workgroups;
  g_cost_shape.slice = slice ? slice : kCostMaxSlice;
  g_cost_tile_order = tile_order < 0 ? 1 : tile_order;
  return 0;
}
}  // extern "C"
