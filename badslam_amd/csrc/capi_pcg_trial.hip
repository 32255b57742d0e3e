// capi_pcg_trial.hip -- step control for the PCG scheme through the C boundary: the damping factor of the context and the controlled
// outer iteration (snapshot, damped iteration, cost, keep or undo).  Kernels: kernels_pcg_trial.hip.
#include <cmath>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
// the scalar a step is judged by: depth + descriptor_1 + descriptor_2 of the total, in that order, in binary64
double objective(const bahip_cost& c) { return (c.depth + c.descriptor_1) + c.descriptor_2; }

// What a trial may overwrite, host side: the poses of the keyframe table and the intrinsics of the context.
struct HostState {
  std::vector<KfEntry> kfs;
  bahip_camera color_cam, depth_cam;
  bahip_depth_params dp;
  Intrinsics in;
};
}  // namespace

extern "C" {
int bahip_context_set_pcg_damping(bahip_context* ctx, float lambda) {
  REQUIRE(ctx != nullptr, "bahip_context_set_pcg_damping: NULL context");
  REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "bahip_context_set_pcg_damping: the damping factor must be finite and >= 0");
  ctx->pcg_damping = lambda;
  return 0;
}
float bahip_context_get_pcg_damping(bahip_context* ctx) { return ctx ? ctx->pcg_damping : -1.f; }

int bahip_pcg_iteration_controlled(bahip_context* ctx, const bahip_pcg_options* opt, const bahip_pcg_step_control* control, int windowed,
                                   int update_normals, const bahip_surfels* surfels, float* lambda_inout, bahip_camera* out_color_camera,
                                   bahip_camera* out_depth_camera, float* out_a, int* inner_steps_out, int* num_converged_out,
                                   int have_cost_before, bahip_cost* cost_before, bahip_cost* cost_after, int* trials_out,
                                   int* accepted_out) {
  REQUIRE(ctx && opt && control && surfels && lambda_inout && out_color_camera && out_depth_camera && out_a && cost_before && cost_after,
          "bahip_pcg_iteration_controlled: NULL argument");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(!kf_sharded(ctx), "bahip_pcg_iteration_controlled is not available under keyframe sharding: use surfel sharding, or "
                            "bahip_pcg_iteration without step control");
  REQUIRE(control->max_trials >= 1, "bahip_pcg_iteration_controlled: max_trials must be >= 1");
  REQUIRE(std::isfinite(control->lambda_up) && control->lambda_up >= 1.f, "bahip_pcg_iteration_controlled: lambda_up must be >= 1");
  REQUIRE(control->lambda_down > 0.f && control->lambda_down <= 1.f, "bahip_pcg_iteration_controlled: lambda_down must be in (0, 1]");
  REQUIRE(control->lambda_min >= 0.f && std::isfinite(control->lambda_max) && control->lambda_min <= control->lambda_max,
          "bahip_pcg_iteration_controlled: 0 <= lambda_min <= lambda_max (finite)");
  REQUIRE(std::isfinite(*lambda_inout) && *lambda_inout >= 0.f, "bahip_pcg_iteration_controlled: the damping factor must be finite and >= 0");
  const int use_depth = opt->use_depth_residuals, use_desc = opt->use_descriptor_residuals;
  const int K = ctx->num_kfs;
  hipStream_t st = ctx->stream;
  if (trials_out) *trials_out = 0;
  if (accepted_out) *accepted_out = 0;
  if (inner_steps_out) *inner_steps_out = 0;
  if (num_converged_out) *num_converged_out = 0;

  // 1. the cost of the state as it is (or the caller's, from the previous call's cost_after on the same state)
  if (!have_cost_before && bahip_evaluate_cost(ctx, use_depth, use_desc, surfels, cost_before, nullptr)) return 1;
  *cost_after = *cost_before;
  const double before = objective(*cost_before);

  // 2. the snapshot: what the iteration (and the normals update inside the trial) may write
  const SurfelsView sv = make_view(surfels);
  const uint32_t all_tiles = (sv.size + 63u) / 64u;
  PcgTrialShape shape{};
  if (opt->optimize_geometry || update_normals) {
    shape.rows_mask = (1u << kSurfelX) | (1u << kSurfelY) | (1u << kSurfelZ) | (1u << kSurfelNormal);
    if (use_desc) shape.rows_mask |= (1u << kSurfelDescriptor1) | (1u << kSurfelDescriptor2);
    shape.rows_saved = (uint32_t)__builtin_popcount(shape.rows_mask);
    shape.num_tiles = all_tiles;
  }
  if (opt->optimize_poses) { shape.kf_table = reinterpret_cast<uint32_t*>(ctx->dev_kfs.get()); shape.kf_words = (uint32_t)(sizeof(KfEntry) / 4 * (size_t)K); }
  static_assert(sizeof(KfEntry) % 4 == 0, "the keyframe table is saved word by word");
  if (opt->optimize_depth_intrinsics) {
    shape.cfactor = reinterpret_cast<uint32_t*>(ctx->dp.cfactor);
    shape.cf_pitch_bytes = ctx->dp.cfactor_pitch_bytes;
    shape.cf_width = (uint32_t)ctx->in.cf_width; shape.cf_height = (uint32_t)ctx->in.cf_height;
  }
  // the buffer: [tile count | tile list (all_tiles words)] then the snapshot.  Under a window only the tiles with an active surfel are
  // saved (the list the windowed sweeps build: nothing else is written)
  const size_t list_words = 1 + (size_t)all_tiles;
  const bool listed = windowed && shape.num_tiles > 0;
  auto reserve = [&]() -> int {
    return ctx->pcg_trial.reserve(list_words + pcg_trial_snapshot_words(shape), 1024, "the snapshot of a PCG trial step");
  };
  auto list_tiles = [&]() -> int {
    HIP_TRY(hipMemsetAsync(ctx->pcg_trial, 0, sizeof(uint32_t), st));
    launch_pcg_window_tiles(st, sv, ctx->pcg_trial + 1, ctx->pcg_trial);
    CHECK_LAUNCH();
    HIP_TRY(hipMemcpyAsync(ctx->pinned_i, ctx->pcg_trial, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    shape.num_tiles = std::min((uint32_t)ctx->pinned_i[0], all_tiles);
    return 0;
  };
  if (listed) {
    shape.num_tiles = 0;
    if (reserve() || list_tiles()) return 1;
    if (list_words + pcg_trial_snapshot_words(shape) > ctx->pcg_trial.size() && (reserve() || list_tiles())) return 1;   // (growing drops the list)
    shape.tile_list = ctx->pcg_trial + 1;
  } else if (reserve()) {
    return 1;
  }
  uint32_t* const snap = ctx->pcg_trial + list_words;
  launch_pcg_trial_snapshot(st, sv, shape, snap);
  CHECK_LAUNCH();
  HostState saved{ctx->host_kfs, ctx->color_cam, ctx->depth_cam, ctx->dp, ctx->in};
  auto restore = [&]() -> int {
    launch_pcg_trial_restore(st, sv, shape, snap);
    CHECK_LAUNCH();
    ctx->host_kfs = saved.kfs;
    ctx->color_cam = saved.color_cam; ctx->depth_cam = saved.depth_cam; ctx->dp = saved.dp; ctx->in = saved.in;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  };

  // 3. / 4. trial steps
  const float damping_of_context = ctx->pcg_damping;
  float lambda = *lambda_inout;
  int inner_total = 0, rc = 0;
  bool accepted = false;
  for (int trial = 1; trial <= control->max_trials && !accepted; ++trial) {
    if (trials_out) *trials_out = trial;
    ctx->pcg_damping = lambda;
    int inner = 0, converged = 0;
    if (update_normals) rc = bahip_update_surfel_normals(ctx, surfels);
    if (!rc) rc = windowed ? bahip_pcg_iteration_windowed(ctx, opt, surfels, out_color_camera, out_depth_camera, out_a, &inner, &converged)
                           : bahip_pcg_iteration(ctx, opt, surfels, out_color_camera, out_depth_camera, out_a, &inner, &converged);
    ctx->pcg_damping = damping_of_context;
    inner_total += inner;
    if (num_converged_out) *num_converged_out = converged;
    if (!rc && (opt->optimize_depth_intrinsics || opt->optimize_color_intrinsics)) {
      // the iteration reports the new intrinsics; the cost has to be taken with them
      bahip_depth_params dp = ctx->dp;
      dp.a = *out_a;
      const bahip_camera color = *out_color_camera, depth = *out_depth_camera;
      rc = bahip_set_intrinsics(ctx, &color, &depth, &dp);
    }
    bahip_cost after{};
    if (!rc) rc = bahip_evaluate_cost(ctx, use_depth, use_desc, surfels, &after, nullptr);
    if (rc) {   // a failed trial leaves the state of before the call (the error text is the failing call's)
      const std::string text = g_last_error;
      (void)restore();
      g_last_error = text;
      return 1;
    }
    const double value = objective(after);
    if (std::isfinite(value) && value < before) {
      accepted = true;
      *cost_after = after;
      lambda = std::max(lambda * control->lambda_down, control->lambda_min);
    } else {
      if (restore()) return 1;
      lambda = std::min(lambda * control->lambda_up, control->lambda_max);
    }
  }
  if (!accepted) { *out_color_camera = ctx->color_cam; *out_depth_camera = ctx->depth_cam; *out_a = ctx->dp.a; }
  *lambda_inout = lambda;
  if (inner_steps_out) *inner_steps_out = inner_total;
  if (accepted_out) *accepted_out = accepted ? 1 : 0;
  return 0;
}
}  // extern "C"
