// kernels_surfel_cost.hip -- the value of the bundle-adjustment objective per SURFEL: for every surfel the robust depth cost and the two
// robust descriptor costs over every bound keyframe it is associated with, and the two counts ("The objective per
// surfel").  With the poses frozen -- the geometry phase of the alternating scheme -- a surfel's cost depends on that surfel only.
//
// A tile's pairs are walked by cost_pairs (cost_device.h), as the cost sweep's are; this unit holds the sink, the
// tile's epilogue, the kernel and its launcher.  Where the cost sweep adds every term with an LDS atomic into one row per keyframe
// that all 64 lanes (and all wavefronts of the workgroup) contend for (CostRowSink), here each lane owns the three exact
// accumulators of its own surfel -- 3 x kExactLimbs columns of the wavefront's [limb][64] block in LDS (exact_sum.h: exact_lds_add's
// layout; the limb index is data dependent, so registers cannot hold them), plain read-modify-write, no atomic anywhere.  The counts
// and the non-finite flag are registers.  Integer limbs: keyframe order, launch shape, tile order and sharding cannot move a bit.
//
// After a tile's keyframes the lane reads its 27 limbs back, leaves zeros for the next tile, and either
//   resolves them (exact_value) and stores the five values itself -- unsharded and surfel-sharded calls: no limb reaches global memory --, or
//   stores them with the counts and the flag as kCostWords int64 into staging planes ([word][slice], coalesced) that are summed over
//   the ranks of a keyframe partition and resolved by surfel_cost_resolve_kernel.
// Each lane is the only writer of its surfel's entries; every entry [0, surfels_size) of the swept range is written, a surfel without
// a term gets +0.0, +0.0, +0.0, 0, 0.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "exact_sum.h"
#include "wave_cull.h"

namespace bahip {
// Wavefronts per SIMD the register allocation must allow: what the cost sweep of the same residual selection reaches in this
// flavour (tests/test_cpu_surfel_cost_kernel_resources.py compares the listings) -- 4 (at most 128 VGPRs) with both residual types, 7
// (at most 72) with depth alone; with descriptors alone the per-lane read-modify-write leaves the allocator two registers above
// the cost sweep's 72 in the fast flavour unless it is told.
#ifdef BAHIP_FAST_MATH
constexpr int kSurfelCostDescOnlyWaves = 7;
#else
constexpr int kSurfelCostDescOnlyWaves = 6;
#endif
constexpr int surfel_cost_waves_per_simd(bool use_depth, bool use_desc) { return use_depth ? (use_desc ? 4 : 7) : kSurfelCostDescOnlyWaves; }
static_assert(kSurfelCostLdsPerWave == 3 * kExactLimbs * 64 * (int)sizeof(long long), "three ExactCells per lane");
}  // namespace bahip

BAHIP_FLAVOURED_BEGIN

// cell += v exactly, in the lane's own column of the [kExactLimbs][64] block `cell` (a wave-uniform address); a non-finite v raises the
// lane's flag instead
__device__ __forceinline__ void surfel_cost_add(long long* cell, int lane, float v, bool* bad) {
  const ExactSplit s = exact_split(v);
  if (s.limb >= 0) {
    cell[s.limb * 64 + lane] += s.lo;
    if (s.hi) cell[(s.limb + 1) * 64 + lane] += s.hi;
  } else if (s.limb == -2) {
    *bad = true;
  }
}

// The sink of cost_pairs (cost_device.h) per lane: the terms into the lane's own columns of `acc` (3 x [kExactLimbs][64] words, a
// wave-uniform address), the counts and the non-finite flag in registers.
struct SurfelCostLaneSink {
  long long* acc;
  int lane;
  uint32_t &depth_count, &pair_count;
  bool& bad;
  struct Here {};   // (the lane's own columns, whatever the keyframe)
  __device__ __forceinline__ Here pair(int /*k*/) const { return {}; }
  __device__ __forceinline__ void depth(Here, float raw) {
    surfel_cost_add(acc, lane, weighted_depth_cost(raw), &bad);
    ++depth_count;
  }
  __device__ __forceinline__ void descriptors(Here, float raw1, float raw2) {
    surfel_cost_add(acc + kExactLimbs * 64, lane, weighted_descriptor_cost(raw1), &bad);
    surfel_cost_add(acc + 2 * kExactLimbs * 64, lane, weighted_descriptor_cost(raw2), &bad);
    ++pair_count;
  }
  __device__ __forceinline__ void end(Here, unsigned long long /*associated*/, bool /*has_desc*/) {}
};

// One 64-surfel tile against the keyframes this rank holds.  `acc`: the wavefront's 3 x [kExactLimbs][64] words, zero on entry and on
// return.  rows != NULL: the row epilogue (keyframe sharding), into the staging planes of the slice that begins at surfel `slice_begin`
// (a branch in the epilogue, not a second instantiation: two copies of the candidate loop in one kernel double what the compiler hoists
// out of the position loop -- the descriptor-only kernel of the fast flavour then needed scratch at its 72 registers).
template <bool kUseDepth, bool kUseDesc>
__device__ __forceinline__ void surfel_cost_tile(const Intrinsics& in, const KfEntry* __restrict__ frames, int num_kfs, uint32_t owner_mask,
                                                 uint32_t owner_rank, const SurfelsView& s, uint32_t tile, long long* acc,
                                                 const SurfelCostPlanes& out, long long* __restrict__ rows, uint32_t slice_begin,
                                                 uint32_t row_stride) {
  const int lane = threadIdx.x & 63;
  const TileSurfel t = load_tile_surfel<kUseDesc>(s, tile, lane);
  const uint32_t i = t.i;
  const bool in_range = t.in_range;
  uint32_t depth_count = 0, pair_count = 0;
  bool bad = false;
  SurfelCostLaneSink sink{acc, lane, depth_count, pair_count, bad};
  cost_pairs<kUseDepth, kUseDesc>(in, frames, 0, num_kfs, owner_mask, owner_rank, t, sink);
  // One cell after the other (a loop that is not unrolled: nine limbs in registers at a time, one copy of exact_value, so that the
  // epilogue does not set the kernel's register count): the lane's limbs back into registers, zeros left behind for the next tile
  // (its own columns: no barrier), then resolved and stored, or staged.
  long long* row = rows ? rows + (in_range ? i - slice_begin : 0u) : nullptr;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    long long cell[kExactLimbs];
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) {
      long long* word = acc + (c * kExactLimbs + j) * 64 + lane;
      cell[j] = *word;
      *word = 0;
    }
    if (!in_range) continue;
    if (row) {
#pragma unroll
      for (int j = 0; j < kExactLimbs; ++j) row[(size_t)(c * kExactLimbs + j) * row_stride] = cell[j];
    } else {
      double* plane = c == 0 ? out.depth : (c == 1 ? out.descriptor_1 : out.descriptor_2);
      if (plane) plane[i] = bad ? __builtin_nan("") : exact_value(cell);
    }
  }
  if (!in_range) return;
  if (row) {
    row[(size_t)kCostDepthCountWord * row_stride] = depth_count;
    row[(size_t)kCostPairCountWord * row_stride] = pair_count;
    row[(size_t)kCostFlagWord * row_stride] = bad ? 1 : 0;
  } else {
    if (out.depth_residuals) out.depth_residuals[i] = depth_count;
    if (out.descriptor_pairs) out.descriptor_pairs[i] = pair_count;
  }
}

// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile) and, of those, the tiles
// [tile_begin, tile_end).  rows != NULL: the row epilogue.
template <bool kUseDepth, bool kUseDesc>
__global__ void __launch_bounds__(64 * kSurfelCostMaxWaves) __attribute__((amdgpu_waves_per_eu(surfel_cost_waves_per_simd(kUseDepth, kUseDesc))))
surfel_cost_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank, SurfelsView s,
                   uint32_t tile_begin, uint32_t tile_end, uint32_t padded_tiles, const uint32_t* __restrict__ sched, SurfelCostPlanes out,
                   long long* __restrict__ rows, uint32_t row_stride) {
  extern __shared__ long long surfel_cost_acc[];   // [waves][3][kExactLimbs][64]
  constexpr int kWaveWords = kSurfelCostLdsPerWave / (int)sizeof(long long);
  long long* acc = surfel_cost_acc + (threadIdx.x >> 6) * kWaveWords;
  for (int w = threadIdx.x & 63; w < kWaveWords; w += 64) acc[w] = 0;   // the wavefront's own block: no barrier
  const uint32_t waves = blockDim.x >> 6;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + (threadIdx.x >> 6); pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile < tile_begin || tile >= tile_end) continue;
    surfel_cost_tile<kUseDepth, kUseDesc>(in, frames, num_kfs, owner_mask, owner_rank, s, tile, acc, out, rows, tile_begin * 64u, row_stride);
  }
}

void launch_surfel_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                        int kf_world, const SurfelsView& s, uint32_t surfel_begin, uint32_t surfel_end, const uint32_t* sched,
                        const SurfelCostShape& shape, const SurfelCostPlanes& out, long long* rows, uint32_t row_stride, hipError_t* error) {
  *error = hipSuccess;
  surfel_end = std::min(surfel_end, s.size);
  if (surfel_begin >= surfel_end || num_kfs == 0) return;
  const uint32_t tile_begin = surfel_begin / 64u, tile_end = (surfel_end + 63u) / 64u;
  const uint32_t padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(padded, sched);
  const int waves = shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + waves - 1) / waves));
  const size_t lds = (size_t)kSurfelCostLdsPerWave * waves;
  auto kernel = use_depth ? (use_desc ? surfel_cost_kernel<true, true> : surfel_cost_kernel<true, false>) : surfel_cost_kernel<false, true>;
  static bool opted_in[3] = {false, false, false};   // per kernel of this flavour
  const int variant = use_depth ? (use_desc ? 0 : 1) : 2;
  if (lds > 64 * 1024 && !opted_in[variant]) {   // dynamic LDS beyond 64 KB needs the opt-in: once per kernel, not per launch
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             kSurfelCostLdsPerWave * kSurfelCostMaxWaves);
    if (e != hipSuccess) { *error = e; return; }
    opted_in[variant] = true;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, stream, in, frames, num_kfs, (uint32_t)(kf_world - 1), (uint32_t)kf_rank, s,
                     tile_begin, tile_end, padded, sched, out, rows, row_stride);
}

BAHIP_FLAVOURED_END

#ifndef BAHIP_FAST_MATH
namespace bahip {
// ---- resolution of the staged words (after the exchange over the ranks): compiled once, exact_value of exact_sum.h ---------------
// One thread per surfel of the slice: plane w of the staging buffer holds word w of every surfel (kCostWords planes of `stride` words).
__global__ void surfel_cost_resolve_kernel(const long long* __restrict__ rows, uint32_t stride, uint32_t begin, uint32_t count, SurfelCostPlanes out) {
  const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
  if (local >= count) return;
  const long long* row = rows + local;
  long long cells[3][kExactLimbs];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    long long summed[kExactLimbs];
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) summed[j] = row[(size_t)(c * kExactLimbs + j) * stride];
    cost_normalise(summed, cells[c]);
  }
  const bahip_cost c = cost_resolve(cells, row[(size_t)kCostDepthCountWord * stride], row[(size_t)kCostPairCountWord * stride],
                                    row[(size_t)kCostFlagWord * stride] != 0);
  const uint32_t i = begin + local;
  if (out.depth) out.depth[i] = c.depth;
  if (out.descriptor_1) out.descriptor_1[i] = c.descriptor_1;
  if (out.descriptor_2) out.descriptor_2[i] = c.descriptor_2;
  if (out.depth_residuals) out.depth_residuals[i] = (uint32_t)c.depth_residuals;
  if (out.descriptor_pairs) out.descriptor_pairs[i] = (uint32_t)c.descriptor_pairs;
}
void launch_surfel_cost_resolve(hipStream_t stream, const long long* rows, uint32_t stride, uint32_t begin, uint32_t count, const SurfelCostPlanes& out) {
  if (count == 0) return;
  hipLaunchKernelGGL(surfel_cost_resolve_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, rows, stride, begin, count, out);
}

void launch_surfel_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                        int kf_world, const SurfelsView& s, uint32_t surfel_begin, uint32_t surfel_end, const uint32_t* sched,
                        const SurfelCostShape& shape, const SurfelCostPlanes& out, long long* rows, uint32_t row_stride, hipError_t* error) {
  BAHIP_PICK(in, launch_surfel_cost(stream, use_depth, use_desc, in, frames, num_kfs, kf_rank, kf_world, s, surfel_begin, surfel_end, sched, shape, out,
                                    rows, row_stride, error));
}
}  // namespace bahip
#endif
