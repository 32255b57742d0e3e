// kernels_cost.hip -- the value of the bundle-adjustment objective: the robust depth cost plus the robust descriptor cost over every
// associated (surfel, keyframe) pair, per keyframe.
//
// The reference evaluates it on the host only (and, behind a debug switch, as a side sum of its pose kernel: B/kernel_opt_pose.cu:
// 373-380); the oracle's orc_evaluate_cost is the same sum over all pairs.  Here it is the pose sweep's traversal without Jacobians:
// 64-surfel tiles, the frustum cull of wave_cull.h, association and residuals from ba_device.h, the heavy-first run order of the sweeps.
//
// DEFINITION.  Per keyframe three sums -- depth terms 1 * Tukey cost (k = 10), and the two descriptor terms 1e-2 *
// Huber cost (k = 10) of the pairs whose colour pixel is valid -- each the EXACT sum of its binary32 terms rounded once to binary64
// (exact_sum.h), and two counts.  The workgroup keeps a table of ExactCells and counts of its keyframes in LDS (one global row per
// keyframe would take every workgroup's atomics: MI355X_MICROARCH.md "Global float atomics") and adds the non-zero words to the
// output once.  Integer sums: any launch shape, tile order, surfel order or sharding gives the same words.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "exact_sum.h"
#include "wave_cull.h"

namespace bahip {
static_assert(kCostCellWords == kExactLimbs, "a cost row holds three ExactCells");
#ifndef BAHIP_COST_WAVES_ATTR
#define BAHIP_COST_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(4)))   // at most 128 VGPRs: 4 wavefronts per SIMD
#endif
}  // namespace bahip

BAHIP_FLAVOURED_BEGIN

// One 64-surfel tile against the keyframes [kf_begin, kf_begin + kf_count) this rank holds.
template <bool kUseDepth, bool kUseDesc>
__device__ __forceinline__ void cost_tile(const Intrinsics& in, const KfEntry* __restrict__ frames, int kf_begin, int kf_count,
                                          uint32_t owner_mask, uint32_t owner_rank, const SurfelsView& s, uint32_t tile, long long* table) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = tile * 64u + lane;
  const bool in_range = i < s.size;
  const uint32_t ii = in_range ? i : 0;
  const Vec3 gp = surfel_position(s, ii);
  const Vec3 gn = surfel_normal(s, ii);
  float radius_sq = 0, d1 = 0, d2 = 0;
  if (kUseDesc) {
    radius_sq = s.row(kSurfelRadiusSquared)[ii];
    d1 = s.row(kSurfelDescriptor1)[ii];
    d2 = s.row(kSurfelDescriptor2)[ii];
  }
  const TangentPoints tp = surfel_tangent_points(gp, gn, radius_sq);
  const WaveBounds wb = wave_bounds(gp, in_range && (gp.x == gp.x));
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
        const KfEntry& kf = frames[kf_begin + item];
        const float* F = kf.pose.F;
        // every gather of the pair goes out before the first one is waited for (ba_device.h: project_surfel)
        const Projected p = project_surfel(in, F, gp);
        const PixelWords pix = load_pixel_words(in, kf.geom, p);
        DescWords dw;
        if (kUseDesc) dw = load_descriptor_words(in, kf.lumafp, F, tp, p);
        Assoc r;
        const bool visible = in_range && associate_from_words<false>(in, F, gn, p, pix, &r, nullptr);
        if (kUseDesc) gathers_arrived(pix, dw);
        else gathers_arrived(pix);
        const unsigned long long associated = __builtin_amdgcn_ballot_w64(visible);
        if (associated == 0ull) return;
        long long* row = table + (size_t)item * kCostWords;
        long long* flag = row + kCostFlagWord;
        bool has_desc = false;
        if (visible) {
          if (kUseDepth) {
            const float inv_std = assoc_inv_std(in, r);
            const Vec3 u = assoc_unproject(r);
            const float raw = inv_std * dot3(r.nl, u - r.local);
            cost_lds_add(row, flag, weighted_depth_cost(raw));
          }
          if (kUseDesc && dw.color_ok) {
            DescEval e;
            eval_descriptor_from_words(in, kf.lumafp, dw, d1, d2, &e);
            cost_lds_add(row + kExactLimbs, flag, weighted_descriptor_cost(e.r1));
            cost_lds_add(row + 2 * kExactLimbs, flag, weighted_descriptor_cost(e.r2));
            has_desc = true;
          }
        }
        const unsigned long long with_desc = __builtin_amdgcn_ballot_w64(has_desc);
        if (lane == 0) {
          if (kUseDepth) __hip_atomic_fetch_add(&row[kCostDepthCountWord], (long long)__popcll(associated), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (with_desc) __hip_atomic_fetch_add(&row[kCostPairCountWord], (long long)__popcll(with_desc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      });
}

// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile).
template <bool kUseDepth, bool kUseDesc>
__global__ void __launch_bounds__(64 * kCostMaxWaves) BAHIP_COST_WAVES_ATTR
cost_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int kf_begin, int kf_count, uint32_t owner_mask, uint32_t owner_rank,
            SurfelsView s, uint32_t tiles, uint32_t padded_tiles, const uint32_t* __restrict__ sched, long long* __restrict__ out) {
  extern __shared__ long long cost_table[];   // [kf_count][kCostWords]
  const int words = kf_count * kCostWords;
  for (int w = threadIdx.x; w < words; w += blockDim.x) cost_table[w] = 0;
  __syncthreads();
  const uint32_t waves = blockDim.x >> 6;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + (threadIdx.x >> 6); pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    cost_tile<kUseDepth, kUseDesc>(in, frames, kf_begin, kf_count, owner_mask, owner_rank, s, tile, cost_table);
  }
  __syncthreads();
  long long* dst = out + (size_t)kf_begin * kCostWords;
  for (int w = threadIdx.x; w < words; w += blockDim.x) {
    const long long v = cost_table[w];
    if (v) __hip_atomic_fetch_add(&dst[w], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

void launch_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                 int kf_world, const SurfelsView& s, const uint32_t* sched, const CostShape& shape, long long* out) {
  const uint32_t tiles = (s.size + 63u) / 64u;
  if (tiles == 0 || num_kfs == 0) return;
  const uint32_t padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(padded, sched);
  const int waves = shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + waves - 1) / waves));
  const uint32_t mask = (uint32_t)(kf_world - 1), rank = (uint32_t)kf_rank;
  for (int begin = 0; begin < num_kfs; begin += shape.slice) {
    const int count = std::min(shape.slice, num_kfs - begin);
    const size_t lds = sizeof(long long) * kCostWords * (size_t)count;
    auto kernel = use_depth ? (use_desc ? cost_kernel<true, true> : cost_kernel<true, false>) : cost_kernel<false, true>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, stream, in, frames, begin, count, mask, rank, s, tiles, padded, sched, out);
  }
}

BAHIP_FLAVOURED_END

#ifndef BAHIP_FAST_MATH
namespace bahip {
// ---- resolution of the summed rows (after the exchange over the ranks): compiled once, exact_value of exact_sum.h ---------------
// One thread per row: the keyframe's costs, and its normalised limbs, counts and flag added into `total` (kCostWords, zeroed).
__global__ void cost_resolve_rows_kernel(const long long* __restrict__ rows, int num, long long* __restrict__ total, bahip_cost* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= num) return;
  const long long* row = rows + (size_t)k * kCostWords;
  long long cells[3][kExactLimbs];
#pragma unroll
  for (int c = 0; c < 3; ++c) cost_normalise(row + c * kExactLimbs, cells[c]);
  const bool bad = row[kCostFlagWord] != 0;
  out[k] = cost_resolve(cells, row[kCostDepthCountWord], row[kCostPairCountWord], bad);
  auto add = [&](int w, long long v) { if (v) atomicAdd(reinterpret_cast<unsigned long long*>(total + w), (unsigned long long)v); };
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) add(c * kExactLimbs + j, cells[c][j]);
  add(kCostDepthCountWord, row[kCostDepthCountWord]);
  add(kCostPairCountWord, row[kCostPairCountWord]);
  add(kCostFlagWord, bad ? 1 : 0);
}
// The total, from the summed limbs (not from the rounded per-row values): out[num].
__global__ void cost_resolve_total_kernel(const long long* __restrict__ total, int num, bahip_cost* __restrict__ out) {
  if (threadIdx.x != 0) return;
  long long cells[3][kExactLimbs];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) cells[c][j] = total[c * kExactLimbs + j];
  out[num] = cost_resolve(cells, total[kCostDepthCountWord], total[kCostPairCountWord], total[kCostFlagWord] != 0);
}
void launch_cost_resolve(hipStream_t stream, const long long* rows, int num, long long* total, bahip_cost* out) {
  if (num <= 0) return;
  hipLaunchKernelGGL(cost_resolve_rows_kernel, dim3((num + 255) / 256), dim3(256), 0, stream, rows, num, total, out);
  hipLaunchKernelGGL(cost_resolve_total_kernel, dim3(1), dim3(64), 0, stream, total, num, out);
}

void launch_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                 int kf_world, const SurfelsView& s, const uint32_t* sched, const CostShape& shape, long long* out) {
  BAHIP_PICK(in, launch_cost(stream, use_depth, use_desc, in, frames, num_kfs, kf_rank, kf_world, s, sched, shape, out));
}
}  // namespace bahip
#endif
