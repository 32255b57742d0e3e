// capi_residual_image.hip -- a frame's depth and descriptor residuals per pixel through the C boundary (bahip_frame_residual_image):
// clear, sweep and resolve of kernels_residual_image.hip on the caller's key and pair-count planes, or on planes the context owns when
// the caller passes NULL for them.  Exchanges nothing under either sharding.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr int kStageClear = 1, kStageSweep = 2, kStageResolve = 4, kStageAll = 7;
ResidualImageShape g_shape{kResidualImageDefaultWaves, 0};   // workgroups 0: kResidualImageWorkgroupsPerUnit per compute unit
int g_stages = kStageAll;   // the kernels a call launches (scripts/residual_image_eval.py times them by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kResidualImageWorkgroupsPerUnit * units;
}
}  // namespace

extern "C" {
int bahip_frame_residual_image(bahip_context* ctx, const bahip_frame* frame, const float frame_T_global[12], const bahip_surfels* surfels,
                               const bahip_residual_image_options* options, const bahip_residual_image_out* out) {
  // every refusal comes before the first launch (make_entry may pack the frame's planes on the stream)
  REQUIRE(ctx != nullptr && frame != nullptr && frame_T_global != nullptr && surfels != nullptr && options != nullptr && out != nullptr,
          "bahip_frame_residual_image: bad arguments");
  REQUIRE(options->select == BAHIP_RESIDUAL_BEST || options->select == BAHIP_RESIDUAL_WORST, "bahip_frame_residual_image: select is 0 (best) or 1 (worst)");
  REQUIRE((unsigned long long)options->index_base + surfels->surfels_size < 0xFFFFFFFFull,
          "bahip_frame_residual_image: index_base + surfels_size reaches 0xFFFFFFFF, the index of an empty pixel");
  REQUIRE(ctx->have_intrinsics, "bahip_set_intrinsics not called");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_frame_residual_image: no surfel data");
  const uint32_t pixels = (uint32_t)ctx->in.width * (uint32_t)ctx->in.height;
  if (!out->key && ctx->residual_keys.reserve(pixels, 0, "the residual image's key plane")) return 1;
  if (!out->pairs && ctx->residual_counts.reserve(pixels, 0, "the residual image's pair counts")) return 1;
  KfEntry e;
  if (make_entry(ctx, *frame, 0, &e)) return 1;
  ResidualFrame rf;
  memcpy(rf.F, frame_T_global, 12 * sizeof(float));
  rf.geom = e.geom;
  rf.lumafp = e.lumafp;
  Intrinsics in = ctx->in;
  in.fast_math = 0;   // (read by dispatchers only; this unit has one flavour)
  unsigned long long* keys = out->key ? reinterpret_cast<unsigned long long*>(out->key) : ctx->residual_keys.get();
  uint32_t* counts = out->pairs ? out->pairs : ctx->residual_counts.get();
  const SurfelsView v = make_view(surfels);
  if (g_stages & kStageClear) {
    launch_residual_image_clear(ctx->stream, keys, counts, pixels);
    CHECK_LAUNCH();
  }
  if ((g_stages & kStageSweep) && v.size > 0) {
    const ResidualImageShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups()};
    launch_residual_image_sweep(ctx->stream, in, rf, v, options->select, options->index_base, shape, keys, counts);
    CHECK_LAUNCH();
  }
  const ResidualImagePlanes planes{out->index, out->depth_residual, out->inv_stddev, out->desc_residual, out->color_valid};
  if ((g_stages & kStageResolve) && (planes.index || planes.depth_residual || planes.inv_stddev || planes.desc_residual || planes.color_valid)) {
    launch_residual_image_resolve(ctx->stream, in, rf, v, options->index_base, keys, pixels, planes);
    CHECK_LAUNCH();
  }
  return 0;
}

int bahip_debug_set_residual_image_shape(int waves, int workgroups) {
  if (waves < 0 || waves > kResidualImageMaxWaves || workgroups < 0)
    return fail("bahip_debug_set_residual_image_shape: waves 0 .. 8, workgroups >= 0", __FILE__, __LINE__, hipSuccess);
  g_shape.waves = waves ? waves : kResidualImageDefaultWaves;
  g_shape.workgroups = workgroups;
  return 0;
}

int bahip_debug_set_residual_image_stages(int stages) {
  if (stages < 0 || stages > kStageAll) return fail("bahip_debug_set_residual_image_stages: stages 0 .. 7", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}
}  // extern "C"
