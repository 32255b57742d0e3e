// cost_device.h -- the terms of the bundle-adjustment objective and the resolution of a keyframe's cost row, shared between the cost
// sweep (kernels_cost.hip) and the fused sweep of the pose phase under step control (kernels_pose_trial.hip): one spelling, so that
// both produce the same binary32 terms and the same resolved binary64 sums.
#pragma once

#include "ba_device.h"
#include "ba_launch.h"
#include "exact_sum.h"

BAHIP_FLAVOURED_BEGIN

// B/robust_weighting.cuh: TukeyResidual / HuberResidual, the cost and not the weight; spelled as oracle_internal.h spells them
// (tukey_residual, huber_residual) so that the exact flavour has the oracle's bits.
__device__ __forceinline__ float tukey_cost(float r, float k) {
  if (fabsf(r) < k) { const float q = r * (1.f / k); const float t = 1.f - q * q; return (1 / 6.f) * k * k * (1 - t * t * t); }
  return (1 / 6.f) * k * k;
}
__device__ __forceinline__ float huber_cost(float r, float k) {
  const float a = fabsf(r);
  return (a < k) ? (0.5f * r * r) : (k * (a - 0.5f * k));
}
// B/cost_function.cuh:95-98, 183-185
__device__ __forceinline__ float weighted_depth_cost(float r) { return 1.f * tukey_cost(r, 1.f * 10.f); }
__device__ __forceinline__ float weighted_descriptor_cost(float r) { return 1.f * 1e-2f * huber_cost(r, 10.f); }

// row += v exactly, in workgroup memory (limbs [0, kExactLimbs) of the row); a non-finite v sets the row's flag word instead
__device__ __forceinline__ void cost_lds_add(long long* limbs, long long* flag, float v) {
  const ExactSplit s = exact_split(v);
  if (s.limb >= 0) {
    __hip_atomic_fetch_add(&limbs[s.limb], s.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (s.hi) __hip_atomic_fetch_add(&limbs[s.limb + 1], s.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else if (s.limb == -2) {
    *flag = 1;   // (every writer stores the same value)
  }
}

BAHIP_FLAVOURED_END

namespace bahip {
// ---- resolution of the summed rows (after the exchange over the ranks): exact_value of exact_sum.h --------------------------------
// A cell with its carries propagated: limbs 0 .. 7 in [0, 2^32), limb 8 holds the rest (signed); the same value.  Summed over K rows
// such limbs stay far from the int64 range for any K < 2^31 (a row itself takes < 2^30 pairs: two addends below 2^32 per pair and limb).
__device__ __forceinline__ void cost_normalise(const long long* in, long long (&out)[kExactLimbs]) {
  long long carry = 0;
#pragma unroll
  for (int j = 0; j < kExactLimbs - 1; ++j) {
    const long long t = in[j] + carry;
    out[j] = t & 0xffffffffll;
    carry = t >> 32;   // arithmetic shift: floor
  }
  out[kExactLimbs - 1] = in[kExactLimbs - 1] + carry;
}
__device__ __forceinline__ bahip_cost cost_resolve(const long long (&cells)[3][kExactLimbs], long long depth_count, long long pair_count, bool bad) {
  const double nan = __builtin_nan("");
  bahip_cost c;
  c.depth = bad ? nan : exact_value(cells[0]);
  c.descriptor_1 = bad ? nan : exact_value(cells[1]);
  c.descriptor_2 = bad ? nan : exact_value(cells[2]);
  c.depth_residuals = (uint64_t)depth_count;
  c.descriptor_pairs = (uint64_t)pair_count;
  return c;
}
}  // namespace bahip
