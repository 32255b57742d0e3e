// kernels_cull_probe.hip -- the tile cull of wave_cull.h as the device compiles it, made visible (bahip_debug_tile_cull,
// capi_debug.hip; DESIGN.md section 3, "Wavefront-level culling").  Per 64-entry tile of the surfel buffer, in buffer order: the
// bounding sphere wave_bounds gives the entries whose x is not NaN, and per bound keyframe k the decision
// sphere_may_project(depth intrinsics, kfs[k].pose.F, sphere) as bit k % 64 of word k / 64 of the tile's mask row.  Activation flags of
// surfels and keyframes are not looked at.
//
// One wavefront per tile, a lane per entry for the sphere and a lane per keyframe for the decisions (the candidate item of
// sphere_may_project_item, as the sweeps test it), 64 keyframes per ballot.  Compiled in both arithmetic flavours like the sweeps: the
// exact unit with -ffp-contract=off and the correctly rounded square root, the fast unit with contraction at the compiler's discretion
// and the approximate one.  tests/tile_cull.py restates both functions in numpy; tests/test_gpu_tile_cull.py holds this unit to it.
#include "ba_device.h"
#include "ba_launch.h"
#include "wave_cull.h"

BAHIP_FLAVOURED_BEGIN

__global__ void __launch_bounds__(64)
tile_cull_probe_kernel(Intrinsics in, const KfEntry* __restrict__ kfs, int num_kfs, SurfelsView s, uint32_t tiles, float* __restrict__ bounds,
                       unsigned long long* __restrict__ masks) {
  const uint32_t tile = blockIdx.x;
  if (tile >= tiles) return;   // wave-uniform
  const int lane = threadIdx.x;
  const uint32_t i = tile * 64u + lane;
  const bool in_range = i < s.size;
  const Vec3 gp = surfel_position(s, in_range ? i : 0);
  const WaveBounds wb = wave_bounds(gp, in_range && (gp.x == gp.x));
  if (bounds && lane == 0) {
    bounds[4 * (size_t)tile + 0] = wb.cx;
    bounds[4 * (size_t)tile + 1] = wb.cy;
    bounds[4 * (size_t)tile + 2] = wb.cz;
    bounds[4 * (size_t)tile + 3] = wb.r;
  }
  const uint32_t words = ((uint32_t)num_kfs + 63u) / 64u;
  for (uint32_t w = 0; w < words; ++w) {
    const int k = (int)(w * 64u) + lane;
    const bool may = (k < num_kfs) && sphere_may_project_item(in, kfs[k].pose.F, wb);
    const unsigned long long m = __ballot(may);
    if (lane == 0) masks[(size_t)tile * words + w] = m;
  }
}

void launch_tile_cull_probe(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, float* bounds,
                            unsigned long long* masks) {
  const uint32_t tiles = (s.size + 63u) / 64u;
  if (tiles == 0 || num_kfs <= 0) return;
  hipLaunchKernelGGL(tile_cull_probe_kernel, dim3(tiles), dim3(64), 0, stream, in, kfs, num_kfs, s, tiles, bounds, masks);
}

BAHIP_FLAVOURED_END

#ifndef BAHIP_FAST_MATH
namespace bahip {
void launch_tile_cull_probe(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, float* bounds,
                            unsigned long long* masks) {
  BAHIP_PICK(in, launch_tile_cull_probe(stream, in, kfs, num_kfs, s, bounds, masks));
}
}  // namespace bahip
#endif
