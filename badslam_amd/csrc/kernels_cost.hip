// kernels_cost.hip -- the value of the bundle-adjustment objective: the robust depth cost plus the robust descriptor cost over every
// associated (surfel, keyframe) pair, per keyframe.
//
// The reference evaluates it on the host only (and, behind a debug switch, as a side sum of its pose kernel: B/kernel_opt_pose.cu:
// 373-380); the oracle's orc_evaluate_cost is the same sum over all pairs.  Here it is the pose sweep's traversal without Jacobians:
// 64-surfel tiles, the frustum cull of wave_cull.h, association and residuals from ba_device.h, the heavy-first run order of the sweeps.
// The traversal of a tile (cost_pairs) and the sink that adds into a keyframe's row (CostRowSink) are in cost_device.h; this unit
// holds the kernel that deals the tiles and keeps the table, its launcher, and the resolution kernels.
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
    // the tile's terms into the rows of the table (cost_device.h: cost_pairs, CostRowSink)
    CostRowSink<kUseDepth> sink{cost_table};
    cost_pairs<kUseDepth, kUseDesc>(in, frames, kf_begin, kf_count, owner_mask, owner_rank, load_tile_surfel<kUseDesc>(s, tile, threadIdx.x & 63), sink);
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
