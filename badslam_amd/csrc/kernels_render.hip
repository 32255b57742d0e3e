// kernels_render.hip -- the surfel map seen from a camera: per pixel the nearest surfel's depth, index, normal and colour
// (bahip_render_surfels, capi_render.hip; DESIGN.md section 3, "Rendered views of the map").  The reference looks at its map through an
// OpenGL window; this is the map as numbers.
//
// DEFINITION (binary32 throughout, in the order written, nothing contracted).  Per surfel i with a finite position:
//   local = F p (project_surfel's chain), nl = R n (rotate34 of surfel_normal), skipped unless local.z > 0;
//   nd = mad(nl.y, local.y, mad(nl.x, local.x, nl.z * local.z)) (depth_sigma_factor's nesting: the z term innermost), skipped unless
//   nd < 0 under culling; inv_z, pxx, pxy as project_surfel leaves them, skipped unless |pxx| < 1e6 and |pxy| < 1e6;
//   px = (int)floorf(pxx), py = (int)floorf(pxy).
// Point mode: the one candidate pixel (px, py) if it lies in the image, t = local.z.  Disc mode (r^2 finite and > 0):
//   rs2 = (radius_factor * radius_factor) * r^2, rs = sqrt_exact(rs2), hf = (max(fx, fy) * rs) * inv_z,
//   h = min(max_radius_px, (int)hf + 1) (max_radius_px when hf is not below it), candidates [px - h, px + h] x [py - h, py + h] clipped
//   to the image; per candidate (x, y): d = (mad(fx_inv, x, cx_inv), mad(fy_inv, y, cy_inv), 1), den = mad(nl.y, d.y, mad(nl.x, d.x,
//   nl.z)), rejected unless den < 0; t = nd / den (IEEE); q = (t d.x - local.x, t d.y - local.y, t - local.z), rejected unless
//   sqlen3(q) <= rs2.  Without culling the two sign tests are dropped and t > 0 is required instead.
// A candidate with min_depth <= t <= max_depth contributes the key (bits(t) << 32) | (index_base + i); a pixel's value is the MINIMUM
// key over all candidates (t > 0: the bit pattern orders as the value; equal depths go to the lower index), all ones when it has none.
// A minimum does not depend on the order of arrival, the launch shape or the surfel order within equal keys.
//
// Three kernels: clear (the key plane to all ones), splat (one lane per surfel, 64-bit unsigned atomic minimum at agent scope on the
// dense width x height plane, no value returned), resolve (one thread per pixel: the planes from the winning key; the winner's normal
// is rotated again, the same operations on the same operands).  A plain load of the key before the atomic, skipping the atomic when the
// candidate's key is not below it (safe: keys only fall during the splat), was built and measured slower on the bench scene's view --
// DESIGN.md has the figures -- and is not kept.
//
// The unit exists once, built with -ffp-contract=off, and a context set to the fast flavour still launches it: a rendered view is the
// same image under either flavour of the sweeps.  (rcp_exact / sqrt_exact are then their exact forms.)
#include "ba_device.h"
#include "ba_launch.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
constexpr unsigned long long kRenderEmptyKey = ~0ull;

__device__ __forceinline__ bool render_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// What a surfel leaves of the per-surfel part of the definition: its candidate box (empty when the surfel is skipped) and what the
// per-candidate test needs.
struct RenderFootprint {
  int x0, x1, y0, y1;
  Vec3 local, nl;
  float nd, rs2;
};

template <bool kDisc>
__device__ __forceinline__ RenderFootprint render_footprint(const Intrinsics& in, const RenderParams& rp, const SurfelsView& s, uint32_t i,
                                                            bool in_range, Vec3 gp, Vec3 gn) {
  RenderFootprint f;
  f.x0 = f.y0 = 0;
  f.x1 = f.y1 = -1;
  const Projected p = project_surfel(in, rp.F, gp);
  f.local = p.local;
  f.nl = rotate34(rp.F, gn);
  f.nd = mad(f.nl.y, p.local.y, mad(f.nl.x, p.local.x, f.nl.z * p.local.z));
  f.rs2 = 0.f;
  bool ok = in_range && render_finite(gp.x) && render_finite(gp.y) && render_finite(gp.z) && (p.local.z > 0.f);
  if (rp.cull_backfaces) ok = ok && (f.nd < 0.f);
  ok = ok && (fabsf(p.pxx) < 1e6f) && (fabsf(p.pxy) < 1e6f);
  int h = 0;
  if (kDisc) {
    const float radius_sq = s.row(kSurfelRadiusSquared)[in_range ? i : 0];
    ok = ok && render_finite(radius_sq) && (radius_sq > 0.f);
    f.rs2 = (rp.radius_factor * rp.radius_factor) * radius_sq;
    const float rs = sqrt_exact(f.rs2);
    const float hf = (rp.max_focal * rs) * p.inv_z;
    h = rp.max_radius_px;
    if (ok && hf < (float)rp.max_radius_px) h = min(rp.max_radius_px, (int)hf + 1);
  }
  if (!ok) return f;
  const int px = (int)floorf(p.pxx), py = (int)floorf(p.pxy);
  f.x0 = max(px - h, 0);
  f.x1 = min(px + h, in.width - 1);
  f.y0 = max(py - h, 0);
  f.y1 = min(py + h, in.height - 1);
  return f;
}
}  // namespace

__global__ void __launch_bounds__(256) render_clear_kernel(unsigned long long* __restrict__ keys, uint32_t pixels) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < pixels) keys[p] = kRenderEmptyKey;
}

// Wavefront w of workgroup b takes the 64-surfel tiles b * waves + w, + gridDim.x * waves, ...; each lane walks its own surfel's box.
// kCount (the census of scripts/render_eval.py): counters[0] += candidate tests, [1] += candidates with a key = atomics issued.
template <bool kDisc, bool kCount>
__global__ void __launch_bounds__(64 * kRenderMaxWaves)
render_splat_kernel(Intrinsics in, RenderParams rp, SurfelsView s, uint32_t num_tiles, unsigned long long* __restrict__ keys,
                    unsigned long long* __restrict__ counters) {
  const int lane = threadIdx.x & 63;
  const uint32_t waves = blockDim.x >> 6;
  unsigned long long tests = 0, keyed = 0;
  for (uint32_t tile = blockIdx.x * waves + (threadIdx.x >> 6); tile < num_tiles; tile += gridDim.x * waves) {
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    const RenderFootprint f = render_footprint<kDisc>(in, rp, s, t.i, t.in_range, t.gp, t.gn);
    const unsigned long long low = (unsigned long long)(rp.index_base + t.i);
    for (int y = f.y0; y <= f.y1; ++y) {
      const float dy = mad(in.fy_inv, (float)y, in.cy_inv);
      unsigned long long* row = keys + (size_t)y * (size_t)in.width;
      for (int x = f.x0; x <= f.x1; ++x) {
        if (kCount) ++tests;
        float depth = f.local.z;
        if (kDisc) {
          const float dx = mad(in.fx_inv, (float)x, in.cx_inv);
          const float den = mad(f.nl.y, dy, mad(f.nl.x, dx, f.nl.z));
          if (rp.cull_backfaces && !(den < 0.f)) continue;
          depth = f.nd / den;
          if (!rp.cull_backfaces && !(depth > 0.f)) continue;
          const Vec3 q = mk3(depth * dx - f.local.x, depth * dy - f.local.y, depth - f.local.z);
          if (!(sqlen3(q) <= f.rs2)) continue;
        }
        if (!(depth >= rp.min_depth && depth <= rp.max_depth)) continue;
        if (kCount) ++keyed;
        const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | low;
        __hip_atomic_fetch_min(row + x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (kCount) {
    if (tests) atomicAdd(counters, tests);
    if (keyed) atomicAdd(counters + 1, keyed);
  }
}

__global__ void __launch_bounds__(256)
render_resolve_kernel(RenderParams rp, SurfelsView s, const unsigned long long* __restrict__ keys, uint32_t pixels, RenderPlanes out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  const unsigned long long key = keys[p];
  const uint32_t i = (uint32_t)key - rp.index_base;
  float depth = 0.f;
  uint32_t index = kInvalidIndex, color = 0;
  Vec3 nl = mk3(0.f, 0.f, 0.f);
  if (key != kRenderEmptyKey && i < s.size) {
    depth = __uint_as_float((uint32_t)(key >> 32));
    index = (uint32_t)key;
    nl = rotate34(rp.F, surfel_normal(s, i));
    color = reinterpret_cast<const uint32_t*>(s.row(kSurfelColor))[i];
  }
  if (out.key) out.key[p] = key;
  if (out.depth) out.depth[p] = depth;
  if (out.index) out.index[p] = index;
  if (out.normal) {
    out.normal[3 * (size_t)p] = nl.x;
    out.normal[3 * (size_t)p + 1] = nl.y;
    out.normal[3 * (size_t)p + 2] = nl.z;
  }
  if (out.color) out.color[p] = color;
}

void launch_render_clear(hipStream_t stream, unsigned long long* keys, uint32_t pixels) {
  hipLaunchKernelGGL(render_clear_kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, keys, pixels);
}

void launch_render_splat(hipStream_t stream, const Intrinsics& view, const RenderParams& rp, const SurfelsView& s, const RenderShape& shape,
                         unsigned long long* keys, unsigned long long* counters) {
  if (s.size == 0) return;
  const uint32_t tiles = (s.size + 63u) / 64u;
  const uint32_t waves = (uint32_t)shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (tiles + waves - 1) / waves));
  const bool disc = rp.mode == 1;
  auto kernel = counters ? (disc ? render_splat_kernel<true, true> : render_splat_kernel<false, true>)
                         : (disc ? render_splat_kernel<true, false> : render_splat_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), 0, stream, view, rp, s, tiles, keys, counters);
}

void launch_render_resolve(hipStream_t stream, const RenderParams& rp, const SurfelsView& s, const unsigned long long* keys, uint32_t pixels,
                           const RenderPlanes& out) {
  hipLaunchKernelGGL(render_resolve_kernel, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, rp, s, keys, pixels, out);
}

}  // namespace bahip
#endif
