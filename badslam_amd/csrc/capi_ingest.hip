// capi_ingest.hip -- a frame brought to the BA's pyramid level through the C boundary: the three kernels of kernels_ingest.hip behind
// bahip_median_filter_and_densify, bahip_downscale_depth_median and bahip_downscale_rgb_half.  Each call checks its shapes, launches
// one kernel on the context's stream and returns; a refused call launches nothing.  No context state, no allocation.
#include "capi_internal.h"

using namespace bahip;
using namespace bahip_capi;

extern "C" {
int bahip_median_filter_and_densify(bahip_context* ctx, const uint16_t* in_depth, uint32_t in_pitch, uint16_t* out_depth, uint32_t out_pitch,
                                    int width, int height) {
  REQUIRE(ctx != nullptr && in_depth != nullptr && out_depth != nullptr, "bahip_median_filter_and_densify: bad arguments");
  REQUIRE(in_depth != out_depth, "bahip_median_filter_and_densify cannot run in place");
  REQUIRE(width >= 1 && height >= 1 && width <= 65535 && height <= 65535, "bahip_median_filter_and_densify: width and height must be in 1 .. 65535");
  REQUIRE(in_pitch >= 2u * (uint32_t)width && out_pitch >= 2u * (uint32_t)width && in_pitch % 2u == 0 && out_pitch % 2u == 0,
          "bahip_median_filter_and_densify: a pitch is shorter than a row or odd");
  launch_median_densify(ctx->stream, in_depth, in_pitch, out_depth, out_pitch, width, height);
  CHECK_LAUNCH();
  return 0;
}

int bahip_downscale_depth_median(bahip_context* ctx, const uint16_t* in_depth, uint32_t in_pitch, int in_width, int in_height,
                                 uint16_t* out_depth, uint32_t out_pitch, int out_width, int out_height) {
  REQUIRE(ctx != nullptr && in_depth != nullptr && out_depth != nullptr, "bahip_downscale_depth_median: bad arguments");
  REQUIRE(in_depth != out_depth, "bahip_downscale_depth_median cannot run in place");
  REQUIRE(in_width >= 1 && in_height >= 1 && in_width <= 65535 && in_height <= 65535,
          "bahip_downscale_depth_median: the input's width and height must be in 1 .. 65535");
  REQUIRE(out_width >= 1 && out_width <= in_width && out_height >= 1 && out_height <= in_height,
          "bahip_downscale_depth_median: the output must be at least 1 x 1 and no larger than the input");
  // ceil(W / ow) bounds every block's width: (W (x + 1)) / ow - (W x) / ow <= ceil(W / ow)
  REQUIRE((in_width + out_width - 1) / out_width <= kIngestMaxBlock && (in_height + out_height - 1) / out_height <= kIngestMaxBlock,
          "bahip_downscale_depth_median: a block would be more than 9 pixels on a side (81 values is what a binary32 sum holds exactly)");
  REQUIRE(in_pitch >= 2u * (uint32_t)in_width && out_pitch >= 2u * (uint32_t)out_width && in_pitch % 2u == 0 && out_pitch % 2u == 0,
          "bahip_downscale_depth_median: a pitch is shorter than a row or odd");
  launch_downscale_depth_median(ctx->stream, in_depth, in_pitch, in_width, in_height, out_depth, out_pitch, out_width, out_height);
  CHECK_LAUNCH();
  return 0;
}

int bahip_downscale_rgb_half(bahip_context* ctx, const uint8_t* rgb_in, uint32_t in_pitch, int width, int height, int levels,
                             uint8_t* rgb_out, uint32_t out_pitch) {
  REQUIRE(ctx != nullptr && rgb_in != nullptr && rgb_out != nullptr, "bahip_downscale_rgb_half: bad arguments");
  REQUIRE(rgb_in != rgb_out, "bahip_downscale_rgb_half cannot run in place");
  REQUIRE(levels >= 1 && levels <= kIngestMaxLevels, "bahip_downscale_rgb_half: levels must be in 1 .. 3");
  REQUIRE(width >= 1 && height >= 1 && width <= 65535 && height <= 65535, "bahip_downscale_rgb_half: width and height must be in 1 .. 65535");
  REQUIRE(width % (1 << levels) == 0 && height % (1 << levels) == 0, "bahip_downscale_rgb_half: width and height must be divisible by 2^levels");
  REQUIRE(in_pitch >= 3u * (uint32_t)width && out_pitch >= 3u * (uint32_t)(width >> levels), "bahip_downscale_rgb_half: a pitch is shorter than a row");
  REQUIRE(launch_downscale_rgb_half(ctx->stream, rgb_in, in_pitch, width, height, levels, rgb_out, out_pitch) == 0,
          "bahip_downscale_rgb_half: levels must be in 1 .. 3");
  CHECK_LAUNCH();
  return 0;
}
}  // extern "C"
