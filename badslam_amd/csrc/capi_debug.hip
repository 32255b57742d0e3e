// capi_debug.hip -- test hooks and experiment switches of the C boundary (bahip_debug_*).
#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

static const char* const kHookScratch = "the scratch of a test hook";

extern "C" {
int bahip_debug_live_allocations(long long* count_out, long long* bytes_out) {
  if (count_out) *count_out = g_live_allocations.load();
  if (bytes_out) *bytes_out = g_live_bytes.load();
  return 0;
}

// ---- test hook ------------------------------------------------------------------------------------------------------
int bahip_debug_evaluate_pairs(bahip_context* ctx, const bahip_frame* frame, const float frame_T_global[12],
                               const bahip_surfels* surfels, const uint32_t* surfel_indices_host, int count, float* out_host) {
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  if (count <= 0) return 0;
  KfEntry e;
  if (make_entry(ctx, *frame, 0, &e)) return 1;
  memcpy(e.pose.F, frame_T_global, 12 * sizeof(float));
  DeviceBuffer<uint32_t> idx; DeviceBuffer<float> out;
  if (idx.reserve(count, 0, kHookScratch) || out.reserve(40 * (size_t)count, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemcpy(idx, surfel_indices_host, sizeof(uint32_t) * count, hipMemcpyHostToDevice));
  launch_evaluate_pairs(ctx->stream, ctx->in, e, make_view(surfels), idx, count, out);
  CHECK_LAUNCH();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out_host, out, sizeof(float) * 40 * count, hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_exact_sum(bahip_context* ctx, const float* values_host, size_t count, int mode, double* out_host) {
  REQUIRE(out_host != nullptr && (values_host != nullptr || count == 0) && (mode == 0 || mode == 1), "bahip_debug_exact_sum: bad arguments");
  DeviceBuffer<float> values; DeviceBuffer<ExactCell> cells; DeviceBuffer<double> out;
  if (values.reserve(count ? count : 1, 0, kHookScratch) || cells.reserve(pcg_exact_cells(0), 0, kHookScratch) || out.reserve(1, 0, kHookScratch)) return 1;
  if (count) HIP_TRY(hipMemcpy(values, values_host, sizeof(float) * count, hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(cells, 0, sizeof(ExactCell) * pcg_exact_cells(0), ctx->stream));
  launch_exact_sum_debug(ctx->stream, pcg_exact_view(cells, 0), values, count, mode, out);
  CHECK_LAUNCH();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out_host, out, sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_read_pcg_vector(bahip_context* ctx, int which, size_t offset, size_t count, float* out_host) {
  REQUIRE(ctx->pcg_buf != nullptr, "no PCG iteration has run on this context");
  REQUIRE(which >= 0 && which < 5 && offset + count <= ctx->pcg_capacity, "PCG vector range out of bounds");
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out_host, ctx->pcg_buf + (size_t)which * ctx->pcg_capacity + offset, sizeof(float) * count, hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_read_keyframe_activations(bahip_context* ctx, int* activation_out, int num_keyframes) {
  REQUIRE(num_keyframes == ctx->num_kfs && (activation_out != nullptr || num_keyframes == 0),
          "bahip_debug_read_keyframe_activations: one entry per bound keyframe");
  if (num_keyframes == 0) return 0;
  // the DEVICE table: the activation field of the host-side copy is "as bound" (capi_ba.hip: bahip_propagate_covisible_activation)
  std::vector<KfEntry> table((size_t)num_keyframes);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(table.data(), ctx->dev_kfs, sizeof(KfEntry) * table.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < num_keyframes; ++k) activation_out[k] = table[k].activation;
  return 0;
}

int bahip_debug_set_pose_lds_items(int items) {
  if (items < 0) return fail("bahip_debug_set_pose_lds_items: items must be >= 0", __FILE__, __LINE__, hipSuccess);
  set_pose_lds_items(items);
  return 0;
}
int bahip_debug_set_pose_lds_shape(int waves, int parts_shift) {
  if (waves < 0 || waves > 16 || parts_shift < -1 || parts_shift > 3) return fail("bahip_debug_set_pose_lds_shape: waves 0 .. 16, parts_shift -1 .. 3", __FILE__, __LINE__, hipSuccess);
  set_pose_lds_waves(waves);
  set_pose_lds_parts_shift(parts_shift);
  set_pose_trial_shape(waves, parts_shift);   // the fused sweep of the controlled phase has the persistent form only
  return 0;
}
int bahip_debug_set_intrinsics_reduce_form(int form) {
  if (form < -1 || form > 1) return fail("bahip_debug_set_intrinsics_reduce_form: 0, 1 or -1 (the default)", __FILE__, __LINE__, hipSuccess);
  set_intrinsics_reduce_form(form);
  return 0;
}

int bahip_debug_set_fused_iteration_begin(int enabled) {
  g_fused_iteration_begin = enabled ? 1 : 0;
  return 0;
}

int bahip_debug_set_pose_rounds_ahead(int rounds) {
  if (rounds < 0 || rounds > BAHIP_MAX_POSE_ITERATIONS) return fail("bahip_debug_set_pose_rounds_ahead: 0 .. BAHIP_MAX_POSE_ITERATIONS", __FILE__, __LINE__, hipSuccess);
  g_pose_rounds_ahead = rounds;
  return 0;
}
int bahip_debug_pose_form_launches(long long* global_form, long long* lds_form, int reset) {
  long long n[2];
  pose_form_launches(n, reset != 0);
  if (global_form) *global_form = n[0];
  if (lds_form) *lds_form = n[1];
  return 0;
}
int bahip_debug_pcg_step1_form_launches(long long* tile_form, long long* lds_form) {
  long long n[2];
  pcg_step1_form_launches(n);
  if (tile_form) *tile_form = n[0];
  if (lds_form) *lds_form = n[1];
  return 0;
}
int bahip_debug_pose_kernel_dispatches(long long* dispatches_out) {
  if (dispatches_out) *dispatches_out = pose_kernel_dispatches();
  return 0;
}
int bahip_debug_read_tile_schedule(bahip_context* ctx, uint32_t* padded_tiles_out, uint32_t* words_out, size_t max_words) {
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *padded_tiles_out = ctx->tile_order_tiles;
  if (ctx->tile_order_tiles == 0 || words_out == nullptr) return 0;
  const size_t words = std::min(max_words, tile_schedule_words(ctx->tile_order_tiles));
  HIP_TRY(hipMemcpy(words_out, ctx->dev_tile_order, sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_set_tile_order(int enabled) {
  g_tile_order_enabled = enabled ? 1 : 0;
  return 0;
}

int bahip_debug_set_append_groups(int groups) {
  REQUIRE(groups >= 0, "bahip_debug_set_append_groups: groups must be >= 0");
  set_append_groups_limit(groups);
  return 0;
}

int bahip_debug_set_pose_form(int form) {
  REQUIRE(form == 0 || form == 1 || form == 2, "pose form must be 0 (automatic), 1 (one tile per wavefront, global atomics) or 2 (persistent, LDS table)");
  set_pose_form(form);
  return 0;
}

int bahip_debug_set_launch_shapes(int tile_waves, int pose_parts) {
  REQUIRE(tile_waves == 0 || tile_waves == 1 || tile_waves == 4 || tile_waves == 5 || tile_waves == 6,
          "tile_waves must be 0 (automatic), 1, 4, 5 (the geometry step's hybrid shape) or 6 (its fused route)");
  REQUIRE(pose_parts == 0 || pose_parts == 1 || pose_parts == 2 || pose_parts == 4 || pose_parts == 8, "pose_parts must be 0, 1, 2, 4 or 8");
  set_tile_waves(tile_waves);
  set_pose_parts(pose_parts);
  return 0;
}

int bahip_debug_geometry_hybrid_launches(long long* launches_out) { if (launches_out) *launches_out = geometry_hybrid_launches(); return 0; }

int bahip_debug_set_geometry_fused(int threshold, int window) {
  REQUIRE(threshold >= 0 && threshold <= 65, "bahip_debug_set_geometry_fused: threshold must be 0 (default) or 1 .. 65");
  REQUIRE(window >= 0 && window <= 65536, "bahip_debug_set_geometry_fused: window must be 0 (default) or 1 .. 65536 tiles");
  set_geometry_fused(threshold, window);
  return 0;
}

int bahip_debug_geometry_fused_stats(bahip_context* ctx, long long out[4]) {
  REQUIRE(ctx != nullptr && out != nullptr, "bahip_debug_geometry_fused_stats: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  const size_t tiles = ctx->fused_launch_tiles;
  if (tiles == 0) return 0;
  std::vector<unsigned long long> deferred(tiles);
  std::vector<uint8_t> route(tiles);
  HIP_TRY(hipMemcpyAsync(deferred.data(), ctx->dev_fused_deferred, sizeof(unsigned long long) * tiles, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(route.data(), ctx->dev_fused_route, tiles, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t t = 0; t < tiles; ++t) {
    const int taken = route[t];
    REQUIRE(taken <= 2 && (taken == 2) == (deferred[t] != 0), "bahip_debug_geometry_fused_stats: a tile's route and its deferred lanes disagree");
    out[taken] += 1;
    out[3] += __builtin_popcountll(deferred[t]);
  }
  return 0;
}

int bahip_debug_jacobian(bahip_context* ctx, int kind, const float* in, int n_in, float* out, int n_out) {
  REQUIRE(kind >= 0 && kind <= 4 && n_in > 0 && n_in <= 16 && n_out > 0 && n_out <= 8, "bahip_debug_jacobian: bad arguments");
  DeviceBuffer<float> d_in, d_out;
  if (d_in.reserve(16, 0, kHookScratch) || d_out.reserve(8, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemcpyAsync(d_in, in, n_in * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  launch_jacobian_debug(ctx->stream, kind, d_in, d_out);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(out, d_out, n_out * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_read_pattern(bahip_context* ctx, size_t bytes, int pattern, int repeats) {
  REQUIRE(bytes >= 4096 && (pattern == 0 || pattern == 1) && repeats >= 1, "bahip_debug_read_pattern: bad arguments");
  DeviceBuffer<void> buf;   // (bytes + 4: the last word takes the result)
  if (buf.reserve(bytes + 4, 0, kHookScratch)) return 1;
  uint32_t* words = static_cast<uint32_t*>(buf.get());
  HIP_TRY(hipMemsetAsync(words, 0, bytes + 4, ctx->stream));
  for (int r = 0; r < repeats; ++r) {
    launch_read_pattern(ctx->stream, words, bytes / 4, pattern, words + bytes / 4);
    CHECK_LAUNCH();
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_exact_math(bahip_context* ctx, int kind, const float* in, float* out, size_t n) {
  REQUIRE(kind >= 0 && kind <= 5, "bahip_debug_exact_math: kind must be 0 (reciprocal), 1 (square root), 2 (sin), 3 (cos), 4 (atan) or 5 (exp)");
  if (n == 0) return 0;
  DeviceBuffer<float> d_in, d_out;
  if (d_in.reserve(n, 0, kHookScratch) || d_out.reserve(n, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemcpyAsync(d_in, in, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  launch_exact_math_debug(ctx->stream, kind, d_in, d_out, n);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_pose_limbs(bahip_context* ctx, const float* values_host, size_t count, long long* out_host) {
  if (count == 0) return 0;
  DeviceBuffer<float> in; DeviceBuffer<long long> out;
  if (in.reserve(count, 0, kHookScratch) || out.reserve(3 * count, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemcpy(in, values_host, sizeof(float) * count, hipMemcpyHostToDevice));
  launch_pose_limbs_debug(ctx->stream, in, out, count);
  CHECK_LAUNCH();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(out_host, out, sizeof(long long) * 3 * count, hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_pose_step(bahip_context* ctx, const float* H21_b6, const float* global_T_frame, float* out_25) {
  DeviceBuffer<float> d_in, d_out;
  if (d_in.reserve(34, 0, kHookScratch) || d_out.reserve(25, 0, kHookScratch)) return 1;
  float in[34];
  memcpy(in, H21_b6, 27 * sizeof(float));
  memcpy(in + 27, global_T_frame, 7 * sizeof(float));
  HIP_TRY(hipMemcpyAsync(d_in, in, sizeof(in), hipMemcpyHostToDevice, ctx->stream));
  launch_pose_step_debug(ctx->stream, d_in, d_out);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(out_25, d_out, 25 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_pose_step_damped(bahip_context* ctx, const float* H21_b6, const float* global_T_frame, float lambda, float* out_25) {
  DeviceBuffer<float> d_in, d_out;
  if (d_in.reserve(35, 0, kHookScratch) || d_out.reserve(25, 0, kHookScratch)) return 1;
  float in[35];
  memcpy(in, H21_b6, 27 * sizeof(float));
  memcpy(in + 27, global_T_frame, 7 * sizeof(float));
  in[34] = lambda;
  HIP_TRY(hipMemcpyAsync(d_in, in, sizeof(in), hipMemcpyHostToDevice, ctx->stream));
  launch_pose_step_damped_debug(ctx->stream, d_in, d_out);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(out_25, d_out, 25 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_wave_reduce(bahip_context* ctx, const float* in_64x28, float* out_80) {
  DeviceBuffer<float> d_in, d_out;
  if (d_in.reserve(64 * 28, 0, kHookScratch) || d_out.reserve(80, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemcpyAsync(d_in, in_64x28, 64 * 28 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemsetAsync(d_out, 0xff, 80 * sizeof(float), ctx->stream));
  launch_wave_reduce_debug(ctx->stream, d_in, d_out);
  CHECK_LAUNCH();
  HIP_TRY(hipMemcpyAsync(out_80, d_out, 80 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bahip_debug_count_pairs(bahip_context* ctx, const bahip_surfels* surfels, uint64_t* counts_out) {
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  DeviceBuffer<unsigned long long> d;
  if (d.reserve(4, 0, kHookScratch)) return 1;
  HIP_TRY(hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), ctx->stream));
  launch_count_pairs(ctx->stream, ctx->in, ctx->dev_kfs, ctx->num_kfs, make_view(surfels), d);
  CHECK_LAUNCH();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(counts_out, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_tile_cull(bahip_context* ctx, const bahip_surfels* surfels, float* bounds_out, uint64_t* masks_out) {
  if (ctx == nullptr || surfels == nullptr || masks_out == nullptr) return fail("bahip_debug_tile_cull: NULL argument", __FILE__, __LINE__, hipSuccess);
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(ctx->num_kfs > 0 && ctx->dev_kfs != nullptr, "bahip_debug_tile_cull: no keyframes bound (bahip_set_keyframes)");
  const SurfelsView view = make_view(surfels);
  const size_t tiles = ((size_t)view.size + 63u) / 64u;
  if (tiles == 0) return 0;
  REQUIRE(view.data != nullptr, "bahip_debug_tile_cull: surfels without a buffer");
  const size_t words = ((size_t)ctx->num_kfs + 63u) / 64u;
  DeviceBuffer<float> d_bounds; DeviceBuffer<unsigned long long> d_masks;
  if (d_bounds.reserve(4 * tiles, 0, kHookScratch) || d_masks.reserve(tiles * words, 0, kHookScratch)) return 1;
  launch_tile_cull_probe(ctx->stream, ctx->in, ctx->dev_kfs, ctx->num_kfs, view, d_bounds, d_masks);
  CHECK_LAUNCH();
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (bounds_out) HIP_TRY(hipMemcpy(bounds_out, d_bounds, sizeof(float) * 4 * tiles, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(masks_out, d_masks, sizeof(unsigned long long) * tiles * words, hipMemcpyDeviceToHost));
  return 0;
}

int bahip_debug_set_intrinsics_bin_capacity(bahip_context* ctx, int records_per_block) {
  ctx->intr_bin_forced = records_per_block;
  return 0;
}
int bahip_debug_set_intrinsics_slices(bahip_context* ctx, int slices) {
  ctx->intr_slices_forced = slices > 0 ? std::min(slices, kIntrMaxSlices) : 0;
  return 0;
}
int bahip_debug_read_intrinsics_sums(bahip_context* ctx, float out[34], float* cells_out) {
  REQUIRE(out != nullptr, "bahip_debug_read_intrinsics_sums: NULL argument");
  REQUIRE(ctx->intr_sums_cells >= 0 && ctx->intr_scratch, "bahip_debug_read_intrinsics_sums: no intrinsics step has left its sums");
  // the binary64 accumulators after the exchange (capi_solvers.hip: glob_d, cells_d), rounded like intrinsics_finish_kernel /
  // intrinsics_schur_kernel round them (round to nearest even)
  const size_t cells = 8 * (size_t)ctx->intr_sums_cells;
  std::vector<double> host(64 + (cells_out ? cells : 0));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(host.data(), ctx->intr_scratch, sizeof(double) * host.size(), hipMemcpyDeviceToHost));
  for (int q = 0; q < 34; ++q) out[q] = (float)host[q];
  if (cells_out)
    for (size_t e = 0; e < cells; ++e) cells_out[e] = (float)host[64 + e];
  return 0;
}

int bahip_debug_intrinsics_bin_stats(bahip_context* ctx, uint32_t* capacity_out, uint32_t* most_out, uint64_t* total_out) {
  uint32_t most = 0; uint64_t total = 0;
  for (size_t b = 0; b < (size_t)ctx->intr_bin_count * (size_t)std::max(ctx->intr_bin_rows, 0) && ctx->intr_bin_counts_host; ++b) {
    most = std::max(most, ctx->intr_bin_counts_host[b]); total += ctx->intr_bin_counts_host[b];
  }
  if (capacity_out) *capacity_out = ctx->intr_bin_capacity;
  if (most_out) *most_out = most;
  if (total_out) *total_out = total;
  return 0;
}

}  // extern "C"
