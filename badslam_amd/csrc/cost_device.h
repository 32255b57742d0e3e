// cost_device.h -- what the sweeps that evaluate the bundle-adjustment objective share: the terms, the traversal of one tile against
// a keyframe range (cost_pairs: the cost sweep of kernels_cost.hip and the per-surfel sweep of kernels_surfel_cost.hip are this
// traversal with two sinks), the row sink (CostRowSink: the cost sweep's, and what the fused sweep of the pose phase under step
// control, kernels_pose_trial.hip, adds its terms through) and the resolution of a summed row.  One spelling, so that all of them
// produce the same binary32 terms and the same resolved binary64 sums.
#pragma once

#include "ba_device.h"
#include "ba_launch.h"
#include "exact_sum.h"
#include "wave_cull.h"

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

// Where the terms of a (tile, keyframe) pair go in the sweeps that keep one row per keyframe: row `item` of the workgroup's table in
// LDS ([items][kCostWords]: three exact cells, two counts, a flag), which all lanes and all wavefronts of the workgroup add to with
// atomics.  The sink of cost_pairs in the cost sweep, and what the fused sweep of the controlled pose phase adds its terms through.
template <bool kUseDepth>
struct CostRowSink {
  long long* table;
  __device__ __forceinline__ long long* pair(int item) const { return table + (size_t)item * kCostWords; }
  __device__ __forceinline__ void depth(long long* row, float raw) { cost_lds_add(row, row + kCostFlagWord, weighted_depth_cost(raw)); }
  __device__ __forceinline__ void descriptors(long long* row, float raw1, float raw2) {
    cost_lds_add(row + kExactLimbs, row + kCostFlagWord, weighted_descriptor_cost(raw1));
    cost_lds_add(row + 2 * kExactLimbs, row + kCostFlagWord, weighted_descriptor_cost(raw2));
  }
  // every lane of the wavefront: the lanes with an association, and whether this one added descriptor terms
  __device__ __forceinline__ void end(long long* row, unsigned long long associated, bool has_desc) {
    const unsigned long long with_desc = __builtin_amdgcn_ballot_w64(has_desc);
    if ((threadIdx.x & 63) == 0) {
      if (kUseDepth) __hip_atomic_fetch_add(&row[kCostDepthCountWord], (long long)__popcll(associated), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (with_desc) __hip_atomic_fetch_add(&row[kCostPairCountWord], (long long)__popcll(with_desc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
};

// The terms of one 64-surfel tile against the keyframes [kf_begin, kf_begin + kf_count) this rank holds: the pose sweep's traversal
// without Jacobians -- the frustum cull of wave_cull.h, every gather of a pair in flight before the first wait, the production
// association rule of ba_device.h.  For every pair with an associated lane the sink says where the pair's terms go (pair(item)) and gets, on
// the lanes concerned, depth(where, raw) and descriptors(where, raw1, raw2) (only where the colour pixel is valid), then
// end(where, associated, has_desc) on every lane.
template <bool kUseDepth, bool kUseDesc, typename Sink>
__device__ __forceinline__ void cost_pairs(const Intrinsics& in, const KfEntry* __restrict__ frames, int kf_begin, int kf_count, uint32_t owner_mask,
                                           uint32_t owner_rank, const TileSurfel& t, Sink& sink) {
  const WaveBounds wb = wave_bounds(t.gp, t.in_range && (t.gp.x == t.gp.x));
  for_each_candidate(
      kf_count,
      [&](int item) {
        const int k = kf_begin + item;
        if (((uint32_t)k & owner_mask) != owner_rank) return false;   // keyframe sharding: another rank holds its images
        float f[12];
        load_candidate(frames[k].pose.F, nullptr, f, nullptr);
        return sphere_may_project(in, f, wb);
      },
      [&](int item) {
        // (asked first: behind the ballot even an EMPTY pair() cost the descriptor-only per-surfel sweep of the fast flavour a spilled
        // register at its 72; here the cost sweep's code is what it was and nothing spills)
        const auto where = sink.pair(item);
        const KfEntry& kf = frames[kf_begin + item];
        const float* F = kf.pose.F;
        // every gather of the pair goes out before the first one is waited for (ba_device.h: project_surfel)
        const Projected p = project_surfel(in, F, t.gp);
        const PixelWords pix = load_pixel_words(in, kf.geom, p);
        DescWords dw;
        if (kUseDesc) dw = load_descriptor_words(in, kf.lumafp, F, t.tp, p);
        Assoc r;
        const bool visible = t.in_range && associate_from_words<false>(in, F, t.gn, p, pix, &r, nullptr);
        if (kUseDesc) gathers_arrived(pix, dw);
        else gathers_arrived(pix);
        const unsigned long long associated = __builtin_amdgcn_ballot_w64(visible);
        if (associated == 0ull) return;
        bool has_desc = false;
        if (visible) {
          if (kUseDepth) {
            const float inv_std = assoc_inv_std(in, r);
            const Vec3 u = assoc_unproject(r);
            sink.depth(where, inv_std * dot3(r.nl, u - r.local));
          }
          if (kUseDesc && dw.color_ok) {
            DescEval e;
            eval_descriptor_from_words(in, kf.lumafp, dw, t.d1, t.d2, &e);
            sink.descriptors(where, e.r1, e.r2);
            has_desc = true;
          }
        }
        sink.end(where, associated, has_desc);
      });
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
