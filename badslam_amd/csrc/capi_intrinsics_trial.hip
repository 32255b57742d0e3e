// capi_intrinsics_trial.hip -- the intrinsics step of the alternating scheme under step control through the C boundary
// (bahip_optimize_intrinsics_controlled; definition: include/badslam_hip.h).  Kernels: kernels_intrinsics_trial.hip.  The sweep is the plain
// step's (capi_solvers.hip: intrinsics_accumulate); per trial one damped Schur complement from its sums, the host solves, one
// back-substitution from the saved cfactor plane and one evaluation of the objective (bahip_evaluate_cost).
#include <cmath>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the scalar a step is judged by: depth + descriptor_1 + descriptor_2 of the total, in that order, in binary64
double objective(const bahip_cost& c) { return (c.depth + c.descriptor_1) + c.descriptor_2; }

// the ladder of damping factors, in binary32: 0, lambda_first, lambda_first * lambda_up, ... capped at lambda_max
float ladder_up(const bahip_intrinsics_step_control& c, float l) { return l == 0.f ? c.lambda_first : std::min(l * c.lambda_up, c.lambda_max); }
float ladder_down(const bahip_intrinsics_step_control& c, float l) {
  const float t = l / c.lambda_up;
  return t < c.lambda_first ? 0.f : t;
}

// What a trial overwrites on the host: the intrinsics of the context.
struct HostState {
  bahip_camera color_cam, depth_cam;
  bahip_depth_params dp;
  Intrinsics in;
};

// The host part of the damped step from the 34 read-back sums g (the 20 of the depth system with the Schur complement added): the
// plain step's two systems (capi_solvers.hip) with every diagonal entry M_ii replaced by M_ii + (double)lambda * M_ii after the prior
// on a has been added, its solves and its update formulas on the intrinsics `at`.  lambda = 0: the plain step's bits.
void solve_damped(const float* g, const HostState& at, bool depth, bool color, float lambda, float x1[5], float xc[4],
                  bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a) {
  if (depth) {
    double M[25], rhs[5], x[5];
    int q = 0;
    for (int row = 0; row < 5; ++row)
      for (int col = row; col < 5; ++col) { M[row * 5 + col] = g[q]; M[col * 5 + row] = g[q]; ++q; }
    for (int c = 0; c < 5; ++c) rhs[c] = g[15 + c];
    constexpr float kAPriorWeight = 10;   // the weak prior pulling a towards zero, added in binary32 like the reference
    M[24] = (double)((float)M[24] + kAPriorWeight * kAPriorWeight);
    rhs[4] = (double)((float)rhs[4] + kAPriorWeight * kAPriorWeight * at.dp.a);
    for (int i = 0; i < 5; ++i) M[i * 5 + i] = M[i * 5 + i] + (double)lambda * M[i * 5 + i];
    ldlt_solve_sym<5>(M, rhs, x);
    for (int c = 0; c < 5; ++c) x1[c] = (float)x[c];
    const float new_fx = 1.0f / (at.in.fx_inv - x1[0]);
    const float new_fy = 1.0f / (at.in.fy_inv - x1[1]);
    out_depth_camera->fx = new_fx;
    out_depth_camera->fy = new_fy;
    out_depth_camera->cx = -(new_fx * (at.in.cx_inv - x1[2])) + 0.5f;
    out_depth_camera->cy = -(new_fy * (at.in.cy_inv - x1[3])) + 0.5f;
    *out_a = at.dp.a - x1[4];
  }
  if (color) {
    double M[16], rhs[4], x[4];
    int q = 20;
    for (int row = 0; row < 4; ++row)
      for (int col = row; col < 4; ++col) { M[row * 4 + col] = g[q]; M[col * 4 + row] = g[q]; ++q; }
    for (int c = 0; c < 4; ++c) rhs[c] = g[30 + c];
    for (int i = 0; i < 4; ++i) M[i * 4 + i] = M[i * 4 + i] + (double)lambda * M[i * 4 + i];
    ldlt_solve_sym<4>(M, rhs, x);
    for (int c = 0; c < 4; ++c) xc[c] = (float)x[c];
    out_color_camera->fx = at.color_cam.fx - xc[0];
    out_color_camera->fy = at.color_cam.fy - xc[1];
    out_color_camera->cx = at.color_cam.cx - xc[2];
    out_color_camera->cy = at.color_cam.cy - xc[3];
  }
}

int check_control(const bahip_intrinsics_step_control* c) {
  REQUIRE(std::isfinite(c->lambda_first) && c->lambda_first > 0.f, "bahip_intrinsics_step_control: lambda_first must be finite and > 0");
  REQUIRE(std::isfinite(c->lambda_up) && c->lambda_up > 1.f, "bahip_intrinsics_step_control: lambda_up must be finite and > 1");
  REQUIRE(std::isfinite(c->lambda_max) && c->lambda_first <= c->lambda_max, "bahip_intrinsics_step_control: lambda_first <= lambda_max (finite)");
  REQUIRE(c->max_trials >= 1, "bahip_intrinsics_step_control: max_trials must be >= 1");
  return 0;
}
}  // namespace

extern "C" {
int bahip_optimize_intrinsics_controlled(bahip_context* ctx, int optimize_depth, int optimize_color, int use_depth, int use_desc,
                                         const bahip_intrinsics_step_control* control, const bahip_surfels* surfels, float* lambda_inout,
                                         bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a, int have_cost_before,
                                         bahip_cost* cost_before, bahip_cost* cost_after, int* trials_out, int* accepted_out,
                                         float* lambda_accepted_out) {
  REQUIRE(ctx && control && surfels && lambda_inout && out_color_camera && out_depth_camera && out_a && cost_before && cost_after,
          "bahip_optimize_intrinsics_controlled: NULL argument");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(optimize_depth || optimize_color, "at least one of depth / colour intrinsics must be optimised");
  if (check_control(control)) return 1;
  REQUIRE(std::isfinite(*lambda_inout) && *lambda_inout >= 0.f, "bahip_optimize_intrinsics_controlled: the damping factor must be finite and >= 0");
  if (trials_out) *trials_out = 0;
  if (accepted_out) *accepted_out = 0;
  if (lambda_accepted_out) *lambda_accepted_out = 0.f;
  hipStream_t st = ctx->stream;
  const bool timing = ctx->intrinsics_trial_timing != 0;
  double t_last = 0;
  if (timing) {
    for (double& ms : ctx->intrinsics_trial_ms) ms = 0;
    HIP_TRY(hipStreamSynchronize(st));
    t_last = now_ms();
  }
  auto lap = [&](int part) {   // (timing only) books the host time since the last lap; the caller has waited for the stream where it matters
    if (!timing) return;
    const double t = now_ms();
    ctx->intrinsics_trial_ms[part] += t - t_last;
    t_last = t;
  };

  // 1. the cost of the state as it is (or the caller's, from the previous call's cost_after on the same state)
  if (!have_cost_before && bahip_evaluate_cost(ctx, use_depth, use_desc, surfels, cost_before, nullptr)) return 1;
  *cost_after = *cost_before;
  const double before = objective(*cost_before);
  lap(1);
  *out_color_camera = ctx->color_cam; *out_depth_camera = ctx->depth_cam; *out_a = ctx->dp.a;
  if (ctx->num_kfs == 0) return 0;   // nothing to sweep: no trial

  // 2. the plain step's sweep, once; its binary64 sums stay in the context's scratch
  IntrinsicsSweep sweep;
  if (intrinsics_accumulate(ctx, optimize_depth, optimize_color, surfels, out_color_camera, out_depth_camera, out_a, &sweep)) return 1;
  if (!sweep.swept) return 0;
  timer_end(ctx, 4);
  const int S = sweep.S;
  if (timing) HIP_TRY(hipStreamSynchronize(st));
  lap(0);

  // 3. the snapshot: the cfactor plane (its cf_width x cf_height words, rows packed) and the context's intrinsics
  const int cw = ctx->in.cf_width, ch = ctx->in.cf_height;
  const uint32_t saved_pitch = (uint32_t)(sizeof(float) * (size_t)cw);
  if (optimize_depth) {
    if (ctx->intrinsics_trial.reserve((size_t)S, 0, "the saved cfactor plane of a controlled intrinsics step")) return 1;
    launch_intrinsics_trial_plane_copy(st, cw, ch, ctx->dp.cfactor, ctx->dp.cfactor_pitch_bytes, ctx->intrinsics_trial, saved_pitch);
    CHECK_LAUNCH();
  }
  const HostState saved{ctx->color_cam, ctx->depth_cam, ctx->dp, ctx->in};
  auto restore = [&]() -> int {
    ctx->color_cam = saved.color_cam; ctx->depth_cam = saved.depth_cam; ctx->dp = saved.dp; ctx->in = saved.in;
    if (optimize_depth) {
      launch_intrinsics_trial_plane_copy(st, cw, ch, ctx->intrinsics_trial, saved_pitch, ctx->dp.cfactor, ctx->dp.cfactor_pitch_bytes);
      CHECK_LAUNCH();
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  };
  // an error from here on leaves the words of before the call (the error text is the failing call's)
  auto undo = [&]() -> int {
    const std::string text = g_last_error;
    (void)restore();
    g_last_error = text;
    return 1;
  };

  // 4. - 6. the trials
  float lambda = *lambda_inout;
  bool booked = false;
  for (int trial = 1; trial <= control->max_trials; ++trial) {
    if (trials_out) *trials_out = trial;
    launch_intrinsics_trial_schur(st, optimize_depth != 0, S, lambda, sweep.glob_d, sweep.cells_d, sweep.glob, sweep.cells, sweep.partials);
    if (hipGetLastError() != hipSuccess) { fail("the damped Schur complement of the controlled intrinsics step", __FILE__, __LINE__); return undo(); }
    if (hipMemcpyAsync(ctx->pinned_f, sweep.glob, 34 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) {
      fail("the read-back of the controlled intrinsics step", __FILE__, __LINE__);
      return undo();
    }
    lap(2);
    if (hipStreamSynchronize(st) != hipSuccess) { fail("the read-back of the controlled intrinsics step", __FILE__, __LINE__); return undo(); }
    lap(3);
    if (!booked) { intrinsics_accumulate_done(ctx, sweep); booked = true; }
    float x1[5] = {0, 0, 0, 0, 0}, xc[4] = {0, 0, 0, 0};
    bahip_camera color = saved.color_cam, depth = saved.depth_cam;
    bahip_depth_params dp = saved.dp;
    solve_damped(ctx->pinned_f, saved, optimize_depth != 0, optimize_color != 0, lambda, x1, xc, &color, &depth, &dp.a);
    if (optimize_depth) {
      memcpy(ctx->pinned_f + 40, x1, sizeof(x1));
      if (hipMemcpyAsync(sweep.glob + 40, ctx->pinned_f + 40, sizeof(x1), hipMemcpyHostToDevice, st) != hipSuccess) {
        fail("the upload of the controlled intrinsics step", __FILE__, __LINE__);
        return undo();
      }
      launch_intrinsics_trial_backsub(st, cw, S, sweep.cells, sweep.glob + 40, ctx->intrinsics_trial, saved_pitch, ctx->dp.cfactor,
                                      ctx->dp.cfactor_pitch_bytes);
      if (hipGetLastError() != hipSuccess) { fail("the back-substitution of the controlled intrinsics step", __FILE__, __LINE__); return undo(); }
    }
    if (bahip_set_intrinsics(ctx, &color, &depth, &dp)) return undo();
    if (timing && hipStreamSynchronize(st) != hipSuccess) { fail("the controlled intrinsics step", __FILE__, __LINE__); return undo(); }
    lap(2);
    bahip_cost after{};
    if (bahip_evaluate_cost(ctx, use_depth, use_desc, surfels, &after, nullptr)) return undo();
    lap(1);
    const double value = objective(after);
    if (std::isfinite(value) && value < before) {
      *cost_after = after;
      *out_color_camera = color; *out_depth_camera = depth; *out_a = dp.a;
      *lambda_inout = ladder_down(*control, lambda);
      if (lambda_accepted_out) *lambda_accepted_out = lambda;
      if (accepted_out) *accepted_out = 1;
      return 0;
    }
    if (restore()) return 1;
    lap(2);
    if (trial == control->max_trials || lambda >= control->lambda_max) break;   // (a rejection at lambda_max ends the ladder)
    lambda = ladder_up(*control, lambda);
  }
  // 7. no accepted trial: the state of before the call
  *lambda_inout = ladder_up(*control, lambda);
  return 0;
}

int bahip_debug_intrinsics_solve_damped(bahip_context* ctx, int optimize_depth, int optimize_color, float lambda, float x1_out[5], float xc_out[4],
                                        float* cells_after_out) {
  REQUIRE(ctx && x1_out && xc_out, "bahip_debug_intrinsics_solve_damped: NULL argument");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(ctx->intr_sums_cells >= 0 && ctx->intr_scratch, "bahip_debug_intrinsics_solve_damped: no intrinsics step has left its sums");
  REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "bahip_debug_intrinsics_solve_damped: the damping factor must be finite and >= 0");
  const int S = ctx->intr_sums_cells;
  // the layout of capi_solvers.hip: glob_d[64] | cells_d[8 capacity] | glob_f[64] | cells_f[8 capacity] | Schur partials
  double* glob_d = static_cast<double*>(ctx->intr_scratch.get());
  double* cells_d = glob_d + 64;
  float* glob = reinterpret_cast<float*>(cells_d + 8 * (size_t)ctx->intr_capacity);
  float* cells = glob + 64;
  float* partials = cells + 8 * (size_t)ctx->intr_capacity;
  launch_intrinsics_trial_schur(ctx->stream, optimize_depth != 0, S, lambda, glob_d, cells_d, glob, cells, partials);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(ctx->pinned_f, glob, 34 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const HostState at{ctx->color_cam, ctx->depth_cam, ctx->dp, ctx->in};
  bahip_camera color = at.color_cam, depth = at.depth_cam;
  float a = at.dp.a;
  for (int c = 0; c < 5; ++c) x1_out[c] = 0.f;
  for (int c = 0; c < 4; ++c) xc_out[c] = 0.f;
  solve_damped(ctx->pinned_f, at, optimize_depth != 0, optimize_color != 0, lambda, x1_out, xc_out, &color, &depth, &a);
  if (cells_after_out) {
    REQUIRE(optimize_depth, "bahip_debug_intrinsics_solve_damped: the cells table exists with the depth intrinsics only");
    HIP_TRY(hipMemcpy(cells_after_out, cells, sizeof(float) * 8 * (size_t)S, hipMemcpyDeviceToHost));
  }
  return 0;
}

int bahip_debug_intrinsics_trial_timing(bahip_context* ctx, int enable, double out[4]) {
  REQUIRE(ctx != nullptr, "bahip_debug_intrinsics_trial_timing: NULL context");
  if (out) memcpy(out, ctx->intrinsics_trial_ms, sizeof(ctx->intrinsics_trial_ms));
  ctx->intrinsics_trial_timing = enable ? 1 : 0;
  return 0;
}
}  // extern "C"
