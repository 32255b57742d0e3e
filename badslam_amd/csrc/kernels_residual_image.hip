// kernels_residual_image.hip -- the bundle-adjustment objective in image space: per pixel of a frame's depth image the surfel the BA
// associates with it and that pair's depth and descriptor residuals (bahip_frame_residual_image, capi_residual_image.hip; DESIGN.md
// section 3, "Residual images").  A rendered view (kernels_render.hip) is not this image: the renderer picks the nearest surfel by its own
// footprint rule, this unit uses the association rule of ba_device.h -- depth gate, normal tests, the cfactor-calibrated depth.
//
// DEFINITION.  For every surfel i < size the pair (i, frame) goes through the production chain, the device functions of
// evaluate_pairs_kernel (kernels_pose.hip) and cost_pairs (cost_device.h) in their order: project_surfel, load_pixel_words,
// associate_from_words<false>, assoc_inv_std, assoc_unproject.  Activation flags are ignored; a NaN position never associates.  An
// associated pair has its pixel (px, py) and raw = inv_std * dot3(nl, u - local).  With m = bits(raw) & 0x7fffffff its key is
//   BEST   (m << 32) | (index_base + i)                    WORST  ((0x7fffffff - m) << 32) | (index_base + i)
// and a pixel's value is the MINIMUM key over its pairs, all ones when it has none: the smallest |raw| under BEST, the largest under
// WORST (a NaN residual counts as the largest magnitude under both), equal magnitudes to the lower index.  A minimum and a count do not
// depend on the order of arrival, the launch shape or the surfel order.
//
// Three kernels: clear (keys to all ones, pair counts to zero), sweep (64-surfel tiles, one wavefront per tile, a lane per surfel; the
// tile is culled against the one frame with the bounding sphere of wave_cull.h; on associated lanes one 64-bit atomic minimum and one
// 32-bit atomic add, agent scope, relaxed, no value returned; no descriptor gathers), resolve (one thread per pixel: the winner's pair
// evaluated again -- the same operations on the same operands, so raw has the key's magnitude bits -- the descriptors only when a plane
// asks for them, then the planes).
//
// The unit exists once, built with -ffp-contract=off, and a context set to the fast flavour still launches it: the image is the EXACT
// flavour's association and residuals under either flavour of the sweeps.
#include "ba_device.h"
#include "ba_launch.h"
#include "wave_cull.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
constexpr unsigned long long kResidualEmptyKey = ~0ull;

// the pair (surfel, frame) as evaluate_pairs_kernel evaluates it: associated?, and then the pixel and the two depth words
struct ResidualPair {
  int px, py;
  float pxx, pxy;
  float raw, inv_std;
};
__device__ __forceinline__ bool residual_pair(const Intrinsics& in, const ResidualFrame& frame, Vec3 gp, Vec3 gn, bool in_range, ResidualPair* out) {
  const float* F = frame.F;
  const Projected p = project_surfel(in, F, gp);
  const PixelWords pix = load_pixel_words(in, frame.geom, p);
  Assoc r;
  const bool visible = in_range && associate_from_words<false>(in, F, gn, p, pix, &r, nullptr);
  gathers_arrived(pix);
  if (!visible) return false;
  const float inv_std = assoc_inv_std(in, r);
  const Vec3 u = assoc_unproject(r);
  out->px = r.px; out->py = r.py; out->pxx = r.pxx; out->pxy = r.pxy;
  out->inv_std = inv_std;
  out->raw = inv_std * dot3(r.nl, u - r.local);
  return true;
}
__device__ __forceinline__ unsigned long long residual_key(int select, float raw, uint32_t index) {
  const uint32_t m = __float_as_uint(raw) & 0x7fffffffu;
  return ((unsigned long long)(select ? 0x7fffffffu - m : m) << 32) | (unsigned long long)index;
}
}  // namespace

__global__ void __launch_bounds__(256) residual_image_clear_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts, uint32_t pixels) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  keys[p] = kResidualEmptyKey;
  counts[p] = 0u;
}

// Wavefront w of workgroup b takes the 64-surfel tiles b * waves + w, + gridDim.x * waves, ...
__global__ void __launch_bounds__(64 * kResidualImageMaxWaves)
residual_image_sweep_kernel(Intrinsics in, ResidualFrame frame, SurfelsView s, uint32_t num_tiles, int select, uint32_t index_base,
                            unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t waves = blockDim.x >> 6;
  for (uint32_t tile = blockIdx.x * waves + (threadIdx.x >> 6); tile < num_tiles; tile += gridDim.x * waves) {
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    const WaveBounds wb = wave_bounds(t.gp, t.in_range && (t.gp.x == t.gp.x));
    if (!sphere_may_project(in, frame.F, wb)) continue;   // wave-uniform: a frame that sees a tenth of the cloud gathers for a tenth
    ResidualPair r;
    if (!residual_pair(in, frame, t.gp, t.gn, t.in_range, &r)) continue;
    // (px, py) lies in the image: project_surfel's `ok` is a precondition of association
    const size_t p = (size_t)r.py * (size_t)in.width + (size_t)r.px;
    __hip_atomic_fetch_min(keys + p, residual_key(select, r.raw, index_base + t.i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(counts + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool kDescriptors>
__global__ void __launch_bounds__(256)
residual_image_resolve_kernel(Intrinsics in, ResidualFrame frame, SurfelsView s, uint32_t index_base, const unsigned long long* __restrict__ keys,
                              uint32_t pixels, ResidualImagePlanes out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  const unsigned long long key = keys[p];
  const uint32_t i = (uint32_t)key - index_base;
  uint32_t index = kInvalidIndex;
  float raw = 0.f, inv_std = 0.f, r1 = 0.f, r2 = 0.f;
  uint8_t color_valid = 0;
  if (key != kResidualEmptyKey && i < s.size) {
    const Vec3 gp = surfel_position(s, i);
    const Vec3 gn = surfel_normal(s, i);
    ResidualPair r;
    if (residual_pair(in, frame, gp, gn, true, &r)) {
      index = (uint32_t)key;
      raw = r.raw;
      inv_std = r.inv_std;
      if (kDescriptors) {
        float cx, cy;
        if (depth_to_color_pixel(in, r.pxx, r.pxy, &cx, &cy)) {
          color_valid = 1;
          DescEval e;
          eval_descriptor<true>(in, frame.lumafp, frame.F, gp, gn, s.row(kSurfelRadiusSquared)[i], cx, cy, s.row(kSurfelDescriptor1)[i],
                                s.row(kSurfelDescriptor2)[i], &e);
          r1 = e.r1;
          r2 = e.r2;
        }
      }
    }
  }
  if (out.index) out.index[p] = index;
  if (out.depth_residual) out.depth_residual[p] = raw;
  if (out.inv_stddev) out.inv_stddev[p] = inv_std;
  if (kDescriptors) {
    if (out.color_valid) out.color_valid[p] = color_valid;
    if (out.desc_residual) {
      out.desc_residual[2 * (size_t)p] = r1;
      out.desc_residual[2 * (size_t)p + 1] = r2;
    }
  }
}

void launch_residual_image_clear(hipStream_t stream, unsigned long long* keys, uint32_t* counts, uint32_t pixels) {
  hipLaunchKernelGGL(residual_image_clear_kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, keys, counts, pixels);
}

void launch_residual_image_sweep(hipStream_t stream, const Intrinsics& in, const ResidualFrame& frame, const SurfelsView& s, int select,
                                 uint32_t index_base, const ResidualImageShape& shape, unsigned long long* keys, uint32_t* counts) {
  if (s.size == 0) return;
  const uint32_t tiles = (s.size + 63u) / 64u;
  const uint32_t waves = (uint32_t)shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (tiles + waves - 1) / waves));
  hipLaunchKernelGGL(residual_image_sweep_kernel, dim3(grid), dim3(64 * waves), 0, stream, in, frame, s, tiles, select, index_base, keys, counts);
}

void launch_residual_image_resolve(hipStream_t stream, const Intrinsics& in, const ResidualFrame& frame, const SurfelsView& s, uint32_t index_base,
                                   const unsigned long long* keys, uint32_t pixels, const ResidualImagePlanes& out) {
  auto kernel = (out.desc_residual || out.color_valid) ? residual_image_resolve_kernel<true> : residual_image_resolve_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, in, frame, s, index_base, keys, pixels, out);
}

}  // namespace bahip
#endif
