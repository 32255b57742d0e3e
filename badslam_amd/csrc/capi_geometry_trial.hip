// capi_geometry_trial.hip -- the geometry phase of the alternating scheme under step control through the C boundary
// (bahip_optimize_geometry_iteration_controlled).  Kernels: kernels_geometry_trial.hip.  Composed from sweeps the library has: phases 1
// and 2 of the three-phase geometry step (kernels_surfel.hip) for normals, flags and the per-surfel sums, and the per-surfel cost sweep
// (bahip_evaluate_surfel_costs) before the trials and once per trial; per trial one solve launch, one decide launch and one read-back of
// the count of surfels still open.
#include <cmath>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The buffer of a controlled step carved up (sizes in 8-byte words; the stride is a multiple of 64 surfels).
struct TrialLayout {
  float* position;   // the class partials of the position pass
  GeometryTrialState state;
  SurfelCostPlanes c0, c1;
  uint32_t* partials;
  uint32_t* ctl;
};
size_t trial_words(size_t stride, int classes, int sums) {
  const size_t blocks = (stride + kGeometryTrialBlock - 1) / kGeometryTrialBlock;
  return (size_t)classes * sums * stride / 2 + kGeometryTrialWords * stride / 2 + 2 * (4 * stride) + 2 * (stride / 8) + 2 * blocks + kGeometryTrialCtlWords / 2;
}
TrialLayout carve(double* base, size_t stride, int classes, int sums) {
  TrialLayout L{};
  double* p = base;
  L.position = reinterpret_cast<float*>(p);
  p += (size_t)classes * sums * stride / 2;
  L.state.saved = reinterpret_cast<uint32_t*>(p);
  p += kGeometryTrialWords * stride / 2;
  for (SurfelCostPlanes* c : {&L.c0, &L.c1}) {
    c->depth = p; c->descriptor_1 = p + stride; c->descriptor_2 = p + 2 * stride;
    c->depth_residuals = reinterpret_cast<uint32_t*>(p + 3 * stride);
    c->descriptor_pairs = c->depth_residuals + stride;
    p += 4 * stride;
  }
  L.state.open = reinterpret_cast<uint8_t*>(p);
  p += stride / 8;
  L.state.outcome = reinterpret_cast<uint8_t*>(p);
  p += stride / 8;
  L.state.stride = (uint32_t)stride;
  L.partials = reinterpret_cast<uint32_t*>(p);
  p += 2 * ((stride + kGeometryTrialBlock - 1) / kGeometryTrialBlock);
  L.ctl = reinterpret_cast<uint32_t*>(p);
  return L;
}

// Phases 1 and 2 of the three-phase geometry step (capi_ba.hip: geometry_keyframe_sharded, which is left as it is): flags and normals of
// the plain step, and per class the sums of the position pass in `position` (cleared first: the phases leave tiles without a live surfel
// unwritten).  Keyframe sharding: that step's two exchanges; otherwise this rank owns every class and nothing is exchanged.
int geometry_normals_and_sums(bahip_context* ctx, bool use_depth, bool use_desc, const SurfelsView& v, long long activate_count, float* position,
                              ClassPartials* cpp_out) {
  const int classes = ctx->sum_classes, nn = geometry_normals_sums(activate_count >= 0), np = geometry_position_sums(use_desc);
  const size_t stride = ((size_t)v.size + 63) & ~(size_t)63;
  const size_t normals_floats = (size_t)classes * nn * stride, position_floats = (size_t)classes * np * stride;
  if (ctx->kf_partials.reserve(normals_floats, 0, "the class partials of the normals pass")) return 1;
  const uint32_t owned = owned_classes(ctx, classes);
  const ClassPartials cpn{ctx->kf_partials, (uint32_t)stride, owned}, cpp{position, (uint32_t)stride, owned};
  *cpp_out = cpp;
  HIP_TRY(hipMemsetAsync(cpn.data, 0, sizeof(float) * normals_floats, ctx->stream));
  HIP_TRY(hipMemsetAsync(cpp.data, 0, sizeof(float) * position_floats, ctx->stream));
  launch_geometry_phase(ctx->stream, 1, use_depth, use_desc, ctx->in, ctx->dev_kfs, ctx->num_kfs, v, activate_count, cpn, cpp);
  CHECK_LAUNCH();
  if (kf_sharded(ctx) && reduce_over_ranks(ctx, cpn.data, normals_floats / 2, BAHIP_SUM_I64)) return 1;
  launch_geometry_phase(ctx->stream, 2, use_depth, use_desc, ctx->in, ctx->dev_kfs, ctx->num_kfs, v, activate_count, cpn, cpp);
  CHECK_LAUNCH();
  if (kf_sharded(ctx) && reduce_over_ranks(ctx, cpp.data, position_floats / 2, BAHIP_SUM_I64)) return 1;
  return 0;
}
}  // namespace

extern "C" {
int bahip_optimize_geometry_iteration_controlled(bahip_context* ctx, int use_depth, int use_desc, const bahip_geometry_step_control* control,
                                                 const bahip_surfels* surfels, long long activation_surfels_size, uint8_t* outcome,
                                                 bahip_geometry_step_stats* stats) {
  REQUIRE(ctx && control && surfels, "bahip_optimize_geometry_iteration_controlled: NULL argument");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(use_depth || use_desc, "at least one residual type must be enabled");
  REQUIRE(surfels->active != nullptr, "geometry optimisation needs the active-surfel buffer");
  REQUIRE(activation_surfels_size >= -1 && activation_surfels_size <= (long long)surfels->surfels_size,
          "bahip_optimize_geometry_iteration_controlled: activation range exceeds surfels_size");
  REQUIRE(std::isfinite(control->lambda_initial) && control->lambda_initial >= 0.f,
          "bahip_optimize_geometry_iteration_controlled: lambda_initial must be finite and >= 0");
  REQUIRE(std::isfinite(control->lambda_up) && control->lambda_up > 1.f, "bahip_optimize_geometry_iteration_controlled: lambda_up must be finite and > 1");
  REQUIRE(std::isfinite(control->lambda_min) && control->lambda_min > 0.f && std::isfinite(control->lambda_max) && control->lambda_min <= control->lambda_max,
          "bahip_optimize_geometry_iteration_controlled: 0 < lambda_min <= lambda_max (finite)");
  REQUIRE(control->max_trials >= 1 && control->max_trials <= 254, "bahip_optimize_geometry_iteration_controlled: max_trials must be 1 .. 254");
  REQUIRE(!kf_sharded(ctx) || is_sharded(ctx), "keyframe sharding needs an all-reduce hook or an RCCL communicator");
  if (stats) *stats = bahip_geometry_step_stats{};
  const SurfelsView v = make_view(surfels);
  const uint32_t N = v.size;
  if (N == 0) return 0;
  ctx->lifecycle_bounds_tiles = 0;   // positions change: a batch's tile bounds end here
  hipStream_t st = ctx->stream;
  const bool timing = ctx->geometry_trial_timing != 0;
  double t_last = 0;
  if (timing) {
    for (double& ms : ctx->geometry_trial_ms) ms = 0;
    HIP_TRY(hipStreamSynchronize(st));
    t_last = now_ms();
  }
  auto lap = [&](int part) -> int {   // (timing only) waits for the stream and books the time since the last lap
    if (!timing) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    const double t = now_ms();
    ctx->geometry_trial_ms[part] += t - t_last;
    t_last = t;
    return 0;
  };

  const int classes = ctx->sum_classes, sums = geometry_position_sums(use_desc != 0);
  const size_t stride = ((size_t)N + 63) & ~(size_t)63;
  ctx->geometry_trial_sums = 0;
  if (ctx->geometry_trial.reserve(trial_words(stride, classes, sums), 0, "the state of a controlled geometry step")) return 1;
  const TrialLayout L = carve(ctx->geometry_trial, stride, classes, sums);

  // 1. normals, activation and sums
  ClassPartials cpp;
  if (geometry_normals_and_sums(ctx, use_depth != 0, use_desc != 0, v, activation_surfels_size, L.position, &cpp)) return 1;
  ctx->geometry_trial_sums = sums; ctx->geometry_trial_classes = classes; ctx->geometry_trial_size = N; ctx->geometry_trial_stride = (uint32_t)stride;
  if (lap(0)) return 1;

  // 2. the cost before
  const bahip_surfel_costs before{L.c0.depth, L.c0.descriptor_1, L.c0.descriptor_2, L.c0.depth_residuals, L.c0.descriptor_pairs};
  const bahip_surfel_costs after{L.c1.depth, L.c1.descriptor_1, L.c1.descriptor_2, L.c1.depth_residuals, L.c1.descriptor_pairs};
  if (bahip_evaluate_surfel_costs(ctx, use_depth, use_desc, surfels, &before)) return 1;
  if (lap(1)) return 1;

  // 3. the snapshot
  HIP_TRY(hipMemsetAsync(L.ctl, 0, sizeof(uint32_t) * kGeometryTrialCtlWords, st));
  launch_geometry_trial_snapshot(st, v, L.state);
  CHECK_LAUNCH();

  // an error from here on leaves the words of before the call (the error text is the failing call's)
  auto undo = [&]() -> int {
    const std::string text = g_last_error;
    launch_geometry_trial_restore(st, v, L.state);
    (void)hipStreamSynchronize(st);
    g_last_error = text;
    return 1;
  };

  // 4. - 7. the trials
  float lambda = control->lambda_initial;
  int trials = 0;
  uint32_t* const words = reinterpret_cast<uint32_t*>(ctx->pinned_i.get());
  static_assert(kGeometryTrialCtlWords <= 16, "the control words are read back through the 16 words of pinned_i");
  for (int t = 0; t < control->max_trials; ++t) {
    launch_geometry_trial_solve(st, v, cpp, classes, use_desc != 0, lambda, t, L.state);
    if (hipGetLastError() != hipSuccess) { fail("the trial solve of the controlled geometry step", __FILE__, __LINE__); return undo(); }
    if (lap(2)) return undo();
    if (bahip_evaluate_surfel_costs(ctx, use_depth, use_desc, surfels, &after)) return undo();
    if (lap(1)) return undo();
    launch_geometry_trial_decide(st, v, L.c0, L.c1, control->guard_pairs != 0, t, L.state, L.partials, L.ctl);
    if (hipGetLastError() != hipSuccess) { fail("the decision of the controlled geometry step", __FILE__, __LINE__); return undo(); }
    if (lap(2)) return undo();
    if (hipMemcpyAsync(words, L.ctl, sizeof(uint32_t) * kGeometryTrialCtlWords, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      fail("the read-back of the controlled geometry step", __FILE__, __LINE__);
      return undo();
    }
    if (lap(3)) return undo();
    ++trials;
    if (words[kGeometryTrialCtlOpen] == 0) break;
    lambda = std::min(std::max(lambda * control->lambda_up, control->lambda_min), control->lambda_max);
  }
  launch_geometry_trial_finish(st, N, L.state, outcome);
  CHECK_LAUNCH();
  if (lap(2)) return 1;
  if (stats) {
    stats->candidates = words[kGeometryTrialCtlCandidates];
    stats->accepted = words[kGeometryTrialCtlAccepted];
    stats->restored = words[kGeometryTrialCtlOpen];
    stats->rejected_cost = words[kGeometryTrialCtlRejectedCost];
    stats->rejected_pairs = words[kGeometryTrialCtlRejectedPairs];
    stats->trials = trials;
  }
  return 0;
}

int bahip_debug_read_geometry_sums(bahip_context* ctx, float* host_out) {
  REQUIRE(ctx && host_out, "bahip_debug_read_geometry_sums: NULL argument");
  REQUIRE(ctx->geometry_trial_sums > 0, "bahip_debug_read_geometry_sums: no controlled geometry step has run on this context");
  const int sums = ctx->geometry_trial_sums, classes = ctx->geometry_trial_classes;
  const size_t stride = ctx->geometry_trial_stride, N = ctx->geometry_trial_size;
  std::vector<float> partials((size_t)classes * sums * stride);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(partials.data(), ctx->geometry_trial.get(), sizeof(float) * partials.size(), hipMemcpyDeviceToHost));
  for (int q = 0; q < sums; ++q)
    for (size_t i = 0; i < N; ++i) {
      // the order of kSumsConsume (kernels_surfel.hip: tile_sums), one rounding per add
      volatile float t = partials[(size_t)(0 * sums + q) * stride + i] + partials[(size_t)(1 * sums + q) * stride + i];
      for (int c = 2; c < classes; ++c) t = t + partials[(size_t)(c * sums + q) * stride + i];
      host_out[(size_t)q * N + i] = t;
    }
  return 0;
}

int bahip_debug_geometry_trial_timing(bahip_context* ctx, int enable, double out[4]) {
  REQUIRE(ctx != nullptr, "bahip_debug_geometry_trial_timing: NULL context");
  if (out) memcpy(out, ctx->geometry_trial_ms, sizeof(ctx->geometry_trial_ms));
  ctx->geometry_trial_timing = enable ? 1 : 0;
  return 0;
}
}  // extern "C"
