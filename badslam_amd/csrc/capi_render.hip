// capi_render.hip -- the surfel map rendered into a camera view through the C boundary (bahip_render_surfels): clear, splat and resolve of
// kernels_render.hip on a key plane the context owns.  Needs no bound keyframe and no bahip_set_intrinsics; exchanges nothing under
// either sharding.
#include <algorithm>

#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

namespace {
constexpr long long kMaxPixels = 1ll << 26;
constexpr int kStageClear = 1, kStageSplat = 2, kStageResolve = 4, kStageAll = 7;
RenderShape g_shape{kRenderDefaultWaves, 0};   // workgroups 0: kRenderWorkgroupsPerUnit per compute unit
int g_stages = kStageAll;                      // the kernels a call launches (scripts/render_eval.py times them by difference)

int default_workgroups() {
  static int units = 0;
  if (units == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    units = cus;
  }
  return kRenderWorkgroupsPerUnit * units;
}

// the checks every entry point shares; fills the view, the parameters and the surfel view
int prepare(const bahip_surfels* surfels, const bahip_camera* view, const float* frame_T_global, const bahip_render_options* options,
            Intrinsics* in, RenderParams* rp, SurfelsView* v) {
  REQUIRE(surfels != nullptr && view != nullptr && frame_T_global != nullptr && options != nullptr, "bahip_render_surfels: bad arguments");
  REQUIRE(view->width >= 1 && view->height >= 1, "bahip_render_surfels: the view needs width >= 1 and height >= 1");
  REQUIRE((long long)view->width * view->height <= kMaxPixels, "bahip_render_surfels: the view has more than 2^26 pixels");
  REQUIRE(options->mode == BAHIP_RENDER_POINT || options->mode == BAHIP_RENDER_DISC, "bahip_render_surfels: mode is 0 (point) or 1 (disc)");
  REQUIRE(options->max_radius_px >= 0 && options->max_radius_px <= kRenderMaxRadiusPx, "bahip_render_surfels: max_radius_px outside 0 .. 16");
  REQUIRE(options->radius_factor > 0.f, "bahip_render_surfels: radius_factor is not > 0");
  REQUIRE(!(options->min_depth > options->max_depth), "bahip_render_surfels: min_depth > max_depth");
  REQUIRE((unsigned long long)options->index_base + surfels->surfels_size < 0xFFFFFFFFull,
          "bahip_render_surfels: index_base + surfels_size reaches 0xFFFFFFFF, the index of an empty pixel");
  REQUIRE(surfels->surfels_size == 0 || surfels->data != nullptr, "bahip_render_surfels: no surfel data");
  *in = make_intrinsics(*view, *view, bahip_depth_params{});
  memcpy(rp->F, frame_T_global, 12 * sizeof(float));
  rp->mode = options->mode;
  rp->max_radius_px = options->max_radius_px;
  rp->cull_backfaces = options->cull_backfaces ? 1 : 0;
  rp->radius_factor = options->radius_factor;
  rp->min_depth = options->min_depth;
  rp->max_depth = options->max_depth;
  rp->max_focal = std::max(view->fx, view->fy);
  rp->index_base = options->index_base;
  *v = make_view(surfels);
  return 0;
}
}  // namespace

extern "C" {
int bahip_render_surfels(bahip_context* ctx, const bahip_surfels* surfels, const bahip_camera* view, const float frame_T_global[12],
                         const bahip_render_options* options, const bahip_render_out* out) {
  REQUIRE(out != nullptr, "bahip_render_surfels: no output planes");
  Intrinsics in;
  RenderParams rp;
  SurfelsView v;
  if (prepare(surfels, view, frame_T_global, options, &in, &rp, &v)) return 1;
  REQUIRE(out->color == nullptr || (reinterpret_cast<uintptr_t>(out->color) & 3u) == 0, "bahip_render_surfels: the colour plane is not aligned to 4 bytes");
  const uint32_t pixels = (uint32_t)view->width * (uint32_t)view->height;
  if (ctx->render_keys.reserve(pixels, 0, "the render key plane")) return 1;
  unsigned long long* keys = ctx->render_keys;
  if (g_stages & kStageClear) {
    launch_render_clear(ctx->stream, keys, pixels);
    CHECK_LAUNCH();
  }
  if ((g_stages & kStageSplat) && v.size > 0) {
    const RenderShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups()};
    launch_render_splat(ctx->stream, in, rp, v, shape, keys, nullptr);
    CHECK_LAUNCH();
  }
  if (g_stages & kStageResolve) {
    const RenderPlanes planes{reinterpret_cast<unsigned long long*>(out->key), out->depth, out->index, out->normal,
                              reinterpret_cast<uint32_t*>(out->color)};
    launch_render_resolve(ctx->stream, rp, v, keys, pixels, planes);
    CHECK_LAUNCH();
  }
  return 0;
}

int bahip_debug_set_render_shape(int waves, int workgroups) {
  if (waves < 0 || waves > kRenderMaxWaves || workgroups < 0)
    return fail("bahip_debug_set_render_shape: waves 0 .. 8, workgroups >= 0", __FILE__, __LINE__, hipSuccess);
  g_shape.waves = waves ? waves : kRenderDefaultWaves;
  g_shape.workgroups = workgroups;
  return 0;
}

int bahip_debug_set_render_stages(int stages) {
  if (stages < 0 || stages > kStageAll) return fail("bahip_debug_set_render_stages: stages 0 .. 7", __FILE__, __LINE__, hipSuccess);
  g_stages = stages ? stages : kStageAll;
  return 0;
}

int bahip_debug_render_census(bahip_context* ctx, const bahip_surfels* surfels, const bahip_camera* view, const float frame_T_global[12],
                              const bahip_render_options* options, unsigned long long counts_out[3]) {
  REQUIRE(counts_out != nullptr, "bahip_debug_render_census: no output");
  Intrinsics in;
  RenderParams rp;
  SurfelsView v;
  if (prepare(surfels, view, frame_T_global, options, &in, &rp, &v)) return 1;
  const uint32_t pixels = (uint32_t)view->width * (uint32_t)view->height;
  if (ctx->render_keys.reserve(pixels, 0, "the render key plane") || ctx->render_counters.reserve(2, 0, "the render counters")) return 1;
  unsigned long long* keys = ctx->render_keys;
  HIP_TRY(hipMemsetAsync(ctx->render_counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
  launch_render_clear(ctx->stream, keys, pixels);
  CHECK_LAUNCH();
  if (v.size > 0) {
    const RenderShape shape{g_shape.waves, g_shape.workgroups > 0 ? g_shape.workgroups : default_workgroups()};
    launch_render_splat(ctx->stream, in, rp, v, shape, keys, ctx->render_counters);
    CHECK_LAUNCH();
  }
  std::vector<unsigned long long> host(pixels);
  HIP_TRY(hipMemcpyAsync(counts_out, ctx->render_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(host.data(), keys, sizeof(unsigned long long) * pixels, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  counts_out[2] = (unsigned long long)std::count_if(host.begin(), host.end(), [](unsigned long long k) { return k != ~0ull; });
  return 0;
}
}  // extern "C"
