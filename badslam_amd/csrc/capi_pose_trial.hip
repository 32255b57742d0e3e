// capi_pose_trial.hip -- the pose phase of the alternating scheme under step control through the C boundary
// (bahip_estimate_keyframe_poses_controlled).  Kernels: kernels_pose_trial.hip.  Per round: the fused sweep, the exchange of the normal
// equations and the cost rows over the ranks (one buffer of int64), the controlled solve, and one read-back of four control words.
#include <cmath>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

extern "C" {
int bahip_estimate_keyframe_poses_controlled(bahip_context* ctx, int use_depth, int use_desc, const bahip_pose_step_control* control,
                                             const bahip_surfels* surfels, int update_activation, float* lambda_inout, float* global_T_frame_out,
                                             int* iterations_done, int* converged, int* moved, int* trials_out, int* rejected_out,
                                             bahip_cost* cost_before_out, bahip_cost* cost_after_out, int* rounds_out, int* num_converged_out) {
  REQUIRE(ctx && control && surfels && lambda_inout, "bahip_estimate_keyframe_poses_controlled: NULL argument");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(use_depth || use_desc, "at least one residual type must be enabled");
  REQUIRE(!kf_sharded(ctx), "bahip_estimate_keyframe_poses_controlled is not available under keyframe sharding: use surfel sharding, or "
                            "bahip_estimate_keyframe_poses without step control");
  REQUIRE(control->max_trials >= 1, "bahip_estimate_keyframe_poses_controlled: max_trials must be >= 1");
  REQUIRE(std::isfinite(control->lambda_up) && control->lambda_up >= 1.f, "bahip_estimate_keyframe_poses_controlled: lambda_up must be >= 1");
  REQUIRE(control->lambda_down > 0.f && control->lambda_down <= 1.f, "bahip_estimate_keyframe_poses_controlled: lambda_down must be in (0, 1]");
  REQUIRE(control->lambda_min >= 0.f && std::isfinite(control->lambda_max) && control->lambda_min <= control->lambda_max,
          "bahip_estimate_keyframe_poses_controlled: 0 <= lambda_min <= lambda_max (finite)");
  const int K = ctx->num_kfs;
  for (int k = 0; k < K; ++k)
    REQUIRE(std::isfinite(lambda_inout[k]) && lambda_inout[k] >= 0.f, "bahip_estimate_keyframe_poses_controlled: every damping factor must be finite and >= 0");
  if (rounds_out) *rounds_out = 0;
  if (num_converged_out) *num_converged_out = 0;
  if (K == 0) return 0;
  if (ensure_work(ctx, K)) return 1;
  const SurfelsView s = make_view(surfels);
  if (ensure_tile_bounds(ctx, s.size)) return 1;
  hipStream_t st = ctx->stream;

  // the buffer, in int64 words: [Hb | cost rows] (exchanged), records, lambdas, two lists, control words
  const size_t sum_words = (size_t)K * (kHbStride + kCostWords), record_words = (size_t)K * (sizeof(PoseTrialRecord) / 8);
  const size_t lambda_words = ((size_t)K + 1) / 2, list_words = (size_t)K, ctl_words = kPoseTrialWords / 2;
  if (ctx->pose_trial.reserve(sum_words + record_words + lambda_words + list_words + ctl_words, 0,
                  "the records of a controlled pose phase")) return 1;
  HbFixed* Hb = ctx->pose_trial;
  long long* cost_rows = Hb + (size_t)K * kHbStride;
  PoseTrialRecord* records = reinterpret_cast<PoseTrialRecord*>(ctx->pose_trial + sum_words);
  float* lambdas = reinterpret_cast<float*>(ctx->pose_trial + sum_words + record_words);
  int* lists = reinterpret_cast<int*>(ctx->pose_trial + sum_words + record_words + lambda_words);
  int* ctl = lists + 2 * (size_t)K;
  HIP_TRY(hipMemsetAsync(ctx->pose_trial, 0, sizeof(long long) * (sum_words + record_words + lambda_words + list_words + ctl_words), st));
  HIP_TRY(hipMemcpyAsync(lambdas, lambda_inout, sizeof(float) * K, hipMemcpyHostToDevice, st));
  launch_pose_init_from_keyframes(st, ctx->dev_kfs, K, ctx->dev_work, Hb, ctx->pinned_work);
  CHECK_LAUNCH();

  const uint32_t* sched = tile_order_for(ctx, s.size);
  // every item ends: at most BAHIP_MAX_POSE_ITERATIONS accepted steps, fewer than max_trials rejected candidates in front of each
  const long long max_rounds = 2 + (long long)(BAHIP_MAX_POSE_ITERATIONS + 1) * control->max_trials;
  int rounds = 0, iterating = K;
  for (long long round = 0; iterating > 0; ++round) {
    if (round >= max_rounds) return fail("bahip_estimate_keyframe_poses_controlled: the rounds did not end", __FILE__, __LINE__);
    const int* listed = round == 0 ? nullptr : lists + (size_t)((round - 1) & 1) * K;
    timer_begin(ctx, 2, round == 0, iterating);   // (the stage timers of the plain phase: 2 = the sweep, 3 = the solve)
    const int e = launch_pose_trial_sweep(st, use_depth != 0, use_desc != 0, ctx->in, ctx->dev_kfs, ctx->dev_work, K, listed, iterating, s, Hb, cost_rows,
                                          ctx->dev_tile_bounds, /*stored_bounds*/ round > 0, sched);
    timer_end(ctx, 2);
    if (e) return fail("the fused sweep of the controlled pose phase", __FILE__, __LINE__, (hipError_t)e);
    CHECK_LAUNCH();
    // integer sums over the ranks: every rank resolves the same cost bits and the same H, b, hence takes the same decisions
    if (reduce_over_ranks(ctx, ctx->pose_trial, sum_words, BAHIP_SUM_I64)) return 1;
    HIP_TRY(hipMemsetAsync(ctl + (round & 1), 0, sizeof(int), st));
    timer_begin(ctx, 3, round == 0);
    launch_pose_trial_solve(st, ctx->dev_work, K, records, Hb, cost_rows, ctx->dev_kfs, *control, update_activation ? 1 : 0, (int)std::min<long long>(round, 1 << 30),
                            lambdas, ctl, lists + (size_t)(round & 1) * K);
    timer_end(ctx, 3);
    CHECK_LAUNCH();
    HIP_TRY(hipMemcpyAsync(ctx->pinned_i, ctl, sizeof(int) * kPoseTrialWords, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->pinned_i[kPoseTrialInvalid])
      return fail("pose normal equations: a tile total was not finite or reached 2^52 (hb_split), or a sum left the fixed-point range; the "
                  "surfels or images hold non-finite values", __FILE__, __LINE__);
    iterating = ctx->pinned_i[round & 1];
    ++rounds;
  }

  std::vector<PoseWork> work((size_t)K);
  std::vector<PoseTrialRecord> recs((size_t)K);
  HIP_TRY(hipMemcpyAsync(work.data(), ctx->dev_work, sizeof(PoseWork) * K, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(recs.data(), records, sizeof(PoseTrialRecord) * K, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  int counted = 0;
  for (int k = 0; k < K; ++k) {
    const bool inactive = recs[k].evaluated == 0;   // (the device table's activation as the phase found it)
    const PoseWork& w = work[k];
    if (!inactive && w.iterations > 0) fill_pose(&ctx->host_kfs[k], w.T);
    if (!inactive) lambda_inout[k] = recs[k].lambda;
    if (global_T_frame_out) memcpy(global_T_frame_out + 7 * k, ctx->host_kfs[k].global_T_frame, 7 * sizeof(float));
    if (iterations_done) iterations_done[k] = w.iterations;
    if (converged) converged[k] = inactive ? 1 : w.converged;
    if (moved) moved[k] = update_activation ? w.moved : 0;
    if (trials_out) trials_out[k] = inactive ? 0 : recs[k].trials;
    if (rejected_out) rejected_out[k] = inactive ? 0 : recs[k].rejected;
    if (cost_before_out) cost_before_out[k] = inactive ? bahip_cost{} : recs[k].cost_before;
    if (cost_after_out) cost_after_out[k] = inactive ? bahip_cost{} : recs[k].cost;
    if (inactive || (update_activation && !w.moved)) ++counted;
  }
  if (update_activation && num_converged_out) *num_converged_out = counted;
  if (rounds_out) *rounds_out = rounds;
  return 0;
}
}  // extern "C"
