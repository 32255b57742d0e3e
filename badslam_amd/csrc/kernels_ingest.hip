// kernels_ingest.hip -- what a video frame goes through before the brightness / bilateral / normals / radii chain when the BA runs at a
// pyramid level (BadSlam::PreprocessFrame, B/bad_slam.cc:657-689; DESIGN.md section 3, "Frame ingestion at a pyramid level").  The
// reference runs these three steps on the CPU; they are pure integer image rules, so the kernels give its results bit for bit.
//
// The median rule both depth kernels share, for a set of n >= 1 non-zero u16 values, sorted ascending s[0 .. n-1]:
//   n odd:  s[n/2];
//   n even: low = s[n/2 - 1], high = s[n/2], average = float(sum) / float(n) (binary32, correctly rounded; sum < 2^24 is exact);
//           low if |average - low| < |average - high| (strictly), else high.
//
// median_densify_kernel (B/preprocessing.cc:40-85, one iteration): the set is the non-zero values of the 3x3 window clipped to the image;
//   with n < 2 the output is the input pixel.  Nine registers go through a fixed compare-exchange network with zeros mapped to 0x10000
//   (above every value), so the n values end up first; s[n/2] and s[n/2 - 1] are picked by compares against constants, never by an index.
// downscale_depth_median_kernel (L/image.h:1003-1053 with value_to_ignore = 0): the set is the non-zero values of the block
//   [(W x) / ow, (W (x + 1)) / ow) x [(H y) / oh, (H (y + 1)) / oh); n = 0 gives 0.  At most 9 x 9 values (the boundary refuses more):
//   one pass counts and sums, 16 passes find s[n/2] bit by bit (the smallest v with #{values <= v} > n/2), one more pass finds
//   s[n/2 - 1] (the largest value below s[n/2] if n/2 values are below it, else s[n/2] itself).  The block is re-read from L1.
// downscale_rgb_half_kernel<levels> (L/image.h:929-948 applied `levels` times, as L/image_pyramid.h does): per channel
//   a / 4 + b / 4 + c / 4 + d / 4 with every quotient truncated; the levels fold in registers by recursion on a constant.
//
// One lane per output pixel, no private array, no LDS, no atomic.  The unit exists once, built with -ffp-contract=off, and a context set
// to the fast flavour still launches it.
#include "ba_device.h"
#include "ba_launch.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
constexpr int kIngestBlockX = 64, kIngestBlockY = 4;   // a wavefront per row segment, as in kernels_preprocess.hip
constexpr uint32_t kIngestAbsent = 0x10000u;   // a zero (or a pixel outside the image) in the 3x3 network: sorts behind every value

__device__ __forceinline__ const uint16_t* ingest_row(const uint16_t* base, uint32_t pitch, int y) {
  return reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(base) + (size_t)y * pitch);
}

__device__ __forceinline__ void ingest_cx(uint32_t& a, uint32_t& b) {
  const uint32_t lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

// the even-count choice between the two middle values
__device__ __forceinline__ uint32_t ingest_closer_to_average(uint32_t low, uint32_t high, uint32_t sum, uint32_t n) {
  const float average = (float)sum / (float)n;
  return (fabsf(average - (float)low) < fabsf(average - (float)high)) ? low : high;
}
}  // namespace

__global__ void __launch_bounds__(kIngestBlockX * kIngestBlockY)
median_densify_kernel(const uint16_t* __restrict__ in, uint32_t in_pitch, uint16_t* __restrict__ out, uint32_t out_pitch, int width, int height) {
  const int x = blockIdx.x * kIngestBlockX + threadIdx.x, y = blockIdx.y * kIngestBlockY + threadIdx.y;
  if (x >= width || y >= height) return;
  // the window with clamped addresses; what lies outside the image counts as absent
  const int xm = max(x - 1, 0), xp = min(x + 1, width - 1), ym = max(y - 1, 0), yp = min(y + 1, height - 1);
  const bool has_xm = x > 0, has_xp = x + 1 < width, has_ym = y > 0, has_yp = y + 1 < height;
  const uint16_t *r0 = ingest_row(in, in_pitch, ym), *r1 = ingest_row(in, in_pitch, y), *r2 = ingest_row(in, in_pitch, yp);
  const uint32_t centre = r1[x];
  uint32_t v0 = (has_ym && has_xm) ? r0[xm] : 0u, v1 = has_ym ? r0[x] : 0u, v2 = (has_ym && has_xp) ? r0[xp] : 0u;
  uint32_t v3 = has_xm ? r1[xm] : 0u, v4 = centre, v5 = has_xp ? r1[xp] : 0u;
  uint32_t v6 = (has_yp && has_xm) ? r2[xm] : 0u, v7 = has_yp ? r2[x] : 0u, v8 = (has_yp && has_xp) ? r2[xp] : 0u;
  const uint32_t sum = v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7 + v8;
  const uint32_t n = (v0 != 0u) + (v1 != 0u) + (v2 != 0u) + (v3 != 0u) + (v4 != 0u) + (v5 != 0u) + (v6 != 0u) + (v7 != 0u) + (v8 != 0u);
  v0 = v0 ? v0 : kIngestAbsent; v1 = v1 ? v1 : kIngestAbsent; v2 = v2 ? v2 : kIngestAbsent;
  v3 = v3 ? v3 : kIngestAbsent; v4 = v4 ? v4 : kIngestAbsent; v5 = v5 ? v5 : kIngestAbsent;
  v6 = v6 ? v6 : kIngestAbsent; v7 = v7 ? v7 : kIngestAbsent; v8 = v8 ? v8 : kIngestAbsent;
  // a 25-exchange sorting network on nine values (ascending)
  ingest_cx(v0, v1); ingest_cx(v3, v4); ingest_cx(v6, v7);
  ingest_cx(v1, v2); ingest_cx(v4, v5); ingest_cx(v7, v8);
  ingest_cx(v0, v1); ingest_cx(v3, v4); ingest_cx(v6, v7);
  ingest_cx(v0, v3); ingest_cx(v3, v6); ingest_cx(v0, v3);
  ingest_cx(v1, v4); ingest_cx(v4, v7); ingest_cx(v1, v4);
  ingest_cx(v2, v5); ingest_cx(v5, v8); ingest_cx(v2, v5);
  ingest_cx(v1, v3); ingest_cx(v5, v7); ingest_cx(v2, v6);
  ingest_cx(v4, v6); ingest_cx(v2, v4); ingest_cx(v2, v3);
  ingest_cx(v5, v6);
  // s[n/2] and s[n/2 - 1] for n = 2 .. 9: n/2 = 1 .. 4
  const uint32_t half = n >> 1;
  const uint32_t high = half == 1u ? v1 : half == 2u ? v2 : half == 3u ? v3 : v4;
  const uint32_t low = half == 1u ? v0 : half == 2u ? v1 : half == 3u ? v2 : v3;
  uint32_t result = centre;
  if (n >= 2u) result = (n & 1u) ? high : ingest_closer_to_average(low, high, sum, n);
  reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(out) + (size_t)y * out_pitch)[x] = (uint16_t)result;
}

__global__ void __launch_bounds__(kIngestBlockX * kIngestBlockY)
downscale_depth_median_kernel(const uint16_t* __restrict__ in, uint32_t in_pitch, uint32_t in_width, uint32_t in_height,
                              uint16_t* __restrict__ out, uint32_t out_pitch, uint32_t out_width, uint32_t out_height) {
  const uint32_t x = blockIdx.x * kIngestBlockX + threadIdx.x, y = blockIdx.y * kIngestBlockY + threadIdx.y;
  if (x >= out_width || y >= out_height) return;
  // in_width, out_width <= 65535: the products stay below 2^32
  const uint32_t x0 = (in_width * x) / out_width, x1 = (in_width * (x + 1u)) / out_width;
  const uint32_t y0 = (in_height * y) / out_height, y1 = (in_height * (y + 1u)) / out_height;
  uint32_t n = 0, sum = 0;
  for (uint32_t yy = y0; yy < y1; ++yy) {
    const uint16_t* row = ingest_row(in, in_pitch, (int)yy);
    for (uint32_t xx = x0; xx < x1; ++xx) {
      const uint32_t v = row[xx];
      n += v != 0u;
      sum += v;
    }
  }
  uint32_t result = 0;
  if (n > 0u) {
    // s[n/2]: the smallest value with more than n/2 values <= it, built from the top bit down
    const uint32_t half = n >> 1;
    uint32_t high = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t candidate = high | ((1u << bit) - 1u);
      uint32_t count = 0;
      for (uint32_t yy = y0; yy < y1; ++yy) {
        const uint16_t* row = ingest_row(in, in_pitch, (int)yy);
        for (uint32_t xx = x0; xx < x1; ++xx) {
          const uint32_t v = row[xx];
          count += (v != 0u) && (v <= candidate);
        }
      }
      if (count <= half) high |= 1u << bit;
    }
    result = high;
    if ((n & 1u) == 0u) {
      // s[n/2 - 1]: n/2 values lie below s[n/2] exactly when it differs from s[n/2]; then it is the largest of them
      uint32_t below = 0, largest_below = 0;
      for (uint32_t yy = y0; yy < y1; ++yy) {
        const uint16_t* row = ingest_row(in, in_pitch, (int)yy);
        for (uint32_t xx = x0; xx < x1; ++xx) {
          const uint32_t v = row[xx];
          const bool is_below = (v != 0u) && (v < high);
          below += is_below;
          largest_below = is_below ? max(largest_below, v) : largest_below;
        }
      }
      const uint32_t low = below == half ? largest_below : high;
      result = ingest_closer_to_average(low, high, sum, n);
    }
  }
  reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(out) + (size_t)y * out_pitch)[x] = (uint16_t)result;
}

namespace {
struct IngestRgb {
  uint32_t r, g, b;
};

// the pixel (x, y) of the image halved kLevels times, from the full-size image
template <int kLevels>
__device__ __forceinline__ IngestRgb ingest_halved_pixel(const uint8_t* __restrict__ in, uint32_t pitch, uint32_t x, uint32_t y) {
  if constexpr (kLevels == 0) {
    const uint8_t* p = in + (size_t)y * pitch + 3u * (size_t)x;
    return IngestRgb{p[0], p[1], p[2]};
  } else {
    const IngestRgb a = ingest_halved_pixel<kLevels - 1>(in, pitch, 2u * x, 2u * y);
    const IngestRgb b = ingest_halved_pixel<kLevels - 1>(in, pitch, 2u * x + 1u, 2u * y);
    const IngestRgb c = ingest_halved_pixel<kLevels - 1>(in, pitch, 2u * x, 2u * y + 1u);
    const IngestRgb d = ingest_halved_pixel<kLevels - 1>(in, pitch, 2u * x + 1u, 2u * y + 1u);
    return IngestRgb{(a.r >> 2) + (b.r >> 2) + (c.r >> 2) + (d.r >> 2), (a.g >> 2) + (b.g >> 2) + (c.g >> 2) + (d.g >> 2),
                     (a.b >> 2) + (b.b >> 2) + (c.b >> 2) + (d.b >> 2)};
  }
}
}  // namespace

template <int kLevels>
__global__ void __launch_bounds__(kIngestBlockX * kIngestBlockY)
downscale_rgb_half_kernel(const uint8_t* __restrict__ in, uint32_t in_pitch, uint8_t* __restrict__ out, uint32_t out_pitch, uint32_t out_width,
                          uint32_t out_height) {
  const uint32_t x = blockIdx.x * kIngestBlockX + threadIdx.x, y = blockIdx.y * kIngestBlockY + threadIdx.y;
  if (x >= out_width || y >= out_height) return;
  const IngestRgb v = ingest_halved_pixel<kLevels>(in, in_pitch, x, y);
  uint8_t* p = out + (size_t)y * out_pitch + 3u * (size_t)x;
  p[0] = (uint8_t)v.r;
  p[1] = (uint8_t)v.g;
  p[2] = (uint8_t)v.b;
}

namespace {
dim3 ingest_grid(int w, int h) { return dim3((w + kIngestBlockX - 1) / kIngestBlockX, (h + kIngestBlockY - 1) / kIngestBlockY); }
}  // namespace

void launch_median_densify(hipStream_t stream, const uint16_t* in, uint32_t in_pitch, uint16_t* out, uint32_t out_pitch, int w, int h) {
  hipLaunchKernelGGL(median_densify_kernel, ingest_grid(w, h), dim3(kIngestBlockX, kIngestBlockY), 0, stream, in, in_pitch, out, out_pitch, w, h);
}

void launch_downscale_depth_median(hipStream_t stream, const uint16_t* in, uint32_t in_pitch, int in_w, int in_h, uint16_t* out,
                                   uint32_t out_pitch, int out_w, int out_h) {
  hipLaunchKernelGGL(downscale_depth_median_kernel, ingest_grid(out_w, out_h), dim3(kIngestBlockX, kIngestBlockY), 0, stream, in, in_pitch,
                     (uint32_t)in_w, (uint32_t)in_h, out, out_pitch, (uint32_t)out_w, (uint32_t)out_h);
}

int launch_downscale_rgb_half(hipStream_t stream, const uint8_t* in, uint32_t in_pitch, int w, int h, int levels, uint8_t* out,
                              uint32_t out_pitch) {
  const int ow = w >> levels, oh = h >> levels;
  const dim3 grid = ingest_grid(ow, oh), block(kIngestBlockX, kIngestBlockY);
  if (levels == 1) hipLaunchKernelGGL(downscale_rgb_half_kernel<1>, grid, block, 0, stream, in, in_pitch, out, out_pitch, (uint32_t)ow, (uint32_t)oh);
  else if (levels == 2) hipLaunchKernelGGL(downscale_rgb_half_kernel<2>, grid, block, 0, stream, in, in_pitch, out, out_pitch, (uint32_t)ow, (uint32_t)oh);
  else if (levels == 3) hipLaunchKernelGGL(downscale_rgb_half_kernel<3>, grid, block, 0, stream, in, in_pitch, out, out_pitch, (uint32_t)ow, (uint32_t)oh);
  else return 1;
  return 0;
}

}  // namespace bahip
#endif
