// kernels_observations.hip -- observation lists: the keyframes paired with each surfel, in compressed rows, with each pair's raw
// residuals (bahip_surfel_observations, capi_observations.hip; DESIGN.md section 3, "Observation lists").
//
// DEFINITION.  A[k][s] = 1 when the pair (surfel s, keyframe k) is in the pair population of the cost sweep with the depth term on
// (cost_device.h: cost_pairs<true, false>: the production association rule, a finite position, activation flags ignored) -- the matrix
// of kernels_covisibility.hip.  The table is A by surfel: first[s + 1] - first[s] keyframes per surfel, their bound-order indices
// ascending in keyframes[first[s] ..), and entry for entry the raw depth residual (what cost_pairs hands sink.depth) and the two raw
// descriptor residuals (0x7fc00000 twice where the pair's colour pixel is not valid).
//
// COUNT.  The co-visibility sweep's traversal as it is (one wavefront per 64-surfel tile, heavy-first run order, persistent
// workgroups); the sink's end adds (associated >> lane) & 1 to the lane's counter.  One coalesced store of the 64 counts per tile; the
// 64-bit total by one wave reduction and one atomic per wavefront at the end of the launch.  The caller scans the counts.
//
// FILL.  The same traversal: a lane starts at first[s] and advances by one per associated keyframe; k ascends by construction of
// for_each_candidate, so there is no atomic and no sort.  Two forms:
//   direct  each lane stores into its own list: the 64 lanes of one store instruction write into up to 64 different rows.
//   staged  the 64 lists of a tile are ONE contiguous range [first[64 t], first[64 t + 64]) of every plane.  The wavefront assembles
//           the first `stage_entries` entries of that range -- the window -- in LDS and writes them with coalesced stores after the
//           tile's keyframes; an entry whose position in the range lies beyond the window is stored at once, as in the direct form.
//           One traversal per tile whatever its size, so the walk is exact for any K (a tile's pairs are bounded by 64 K only).
//           The first version walked a larger tile in passes, one traversal per window: on the bench scene (1 117 pairs per tile
//           on average) it lost to this one at every window tried ("Observation lists").
// Either form writes position p of a lane's list only while p is below the end of that list (first[s + 1]): a table that does not
// belong to this state cannot make a store leave the planes.
//
// The unit exists once, built with -ffp-contract=off: a context set to the fast flavour launches the same code, and the table holds the
// exact flavour's association and residual bits.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "wave_cull.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
constexpr uint32_t kObsNaNWord = 0x7fc00000u;

struct ObsCountSink {
  int lane;
  uint32_t count;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float) {}
  __device__ __forceinline__ void descriptors(int, float, float) {}
  __device__ __forceinline__ void end(int, unsigned long long associated, bool) { count += (uint32_t)((associated >> lane) & 1ull); }
};

// direct: pos and limit are positions in the planes (the lane's list is [first[s], first[s + 1]))
template <bool kDesc>
struct ObsDirectSink {
  uint16_t* __restrict__ kf_plane;
  float* __restrict__ depth_plane;   // NULL: not asked for (wave-uniform)
  float* __restrict__ desc_plane;
  uint32_t pos, limit;
  int lane;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float raw) {
    if (depth_plane && pos < limit) depth_plane[pos] = raw;
  }
  __device__ __forceinline__ void descriptors(int, float r1, float r2) {
    if (kDesc && pos < limit) {
      desc_plane[2 * (size_t)pos] = r1;
      desc_plane[2 * (size_t)pos + 1] = r2;
    }
  }
  __device__ __forceinline__ void end(int item, unsigned long long associated, bool has_desc) {
    if (!((associated >> lane) & 1ull)) return;
    if (pos < limit) {
      kf_plane[pos] = (uint16_t)item;
      if (kDesc && !has_desc) {
        desc_plane[2 * (size_t)pos] = __uint_as_float(kObsNaNWord);
        desc_plane[2 * (size_t)pos + 1] = __uint_as_float(kObsNaNWord);
      }
    }
    ++pos;
  }
};

// staged: pos and limit are positions in the tile's range, which begins at entry `base` of the planes; the first `window` entries of
// the range are held in the wavefront's LDS, the entries beyond go to the planes at once
template <bool kDesc>
struct ObsStagedSink {
  uint16_t* kf_lds;
  float* depth_lds;   // NULL: not asked for (wave-uniform)
  float* desc_lds;
  uint16_t* __restrict__ kf_plane;
  float* __restrict__ depth_plane;
  float* __restrict__ desc_plane;
  size_t base;
  uint32_t pos, limit, window;
  int lane;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float raw) {
    if (!depth_lds || pos >= limit) return;
    if (pos < window) depth_lds[pos] = raw;
    else depth_plane[base + pos] = raw;
  }
  __device__ __forceinline__ void pair_of_words(float r1, float r2) {
    if (pos < window) {
      desc_lds[2 * pos] = r1;
      desc_lds[2 * pos + 1] = r2;
    } else {
      desc_plane[2 * (base + pos)] = r1;
      desc_plane[2 * (base + pos) + 1] = r2;
    }
  }
  __device__ __forceinline__ void descriptors(int, float r1, float r2) {
    if (kDesc && pos < limit) pair_of_words(r1, r2);
  }
  __device__ __forceinline__ void end(int item, unsigned long long associated, bool has_desc) {
    if (!((associated >> lane) & 1ull)) return;
    if (pos < limit) {
      if (pos < window) kf_lds[pos] = (uint16_t)item;
      else kf_plane[base + pos] = (uint16_t)item;
      if (kDesc && !has_desc) pair_of_words(__uint_as_float(kObsNaNWord), __uint_as_float(kObsNaNWord));
    }
    ++pos;
  }
};

__device__ __forceinline__ unsigned long long obs_wave_sum(unsigned long long v) {
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step, 64);
  return v;
}
}  // namespace

// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile).
__global__ void __launch_bounds__(64 * kObsMaxWaves)
observations_count_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                          const uint32_t* __restrict__ sched, uint32_t* __restrict__ counts, unsigned long long* __restrict__ total) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long mine = 0;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    ObsCountSink sink{lane, 0u};
    exact::cost_pairs<true, false>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
    if (t.in_range) counts[t.i] = sink.count;
    mine += sink.count;
  }
  const unsigned long long sum = obs_wave_sum(mine);
  if (lane == 0 && sum) __hip_atomic_fetch_add(total, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kDesc>
__global__ void __launch_bounds__(64 * kObsMaxWaves)
observations_fill_direct_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                                const uint32_t* __restrict__ sched, const uint32_t* __restrict__ first, ObsPlanes planes) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<kDesc>(s, tile, lane);
    ObsDirectSink<kDesc> sink{planes.keyframes, planes.depth_raw, planes.descriptor_raw, 0u, 0u, lane};
    if (t.in_range) {
      sink.pos = first[t.i];
      sink.limit = first[t.i + 1];
    }
    exact::cost_pairs<true, kDesc>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
  }
}

// LDS: [waves][2 * window] descriptor words (kDesc), [waves][window] depth words (when asked for), [waves][window] keyframe indices
template <bool kDesc>
__global__ void __launch_bounds__(64 * kObsMaxWaves)
observations_fill_staged_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                                const uint32_t* __restrict__ sched, const uint32_t* __restrict__ first, ObsPlanes planes, uint32_t window) {
  extern __shared__ float obs_lds[];
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  float* cursor = obs_lds;
  float* desc_lds = nullptr;
  float* depth_lds = nullptr;
  if (kDesc) {
    desc_lds = cursor + (size_t)wave * 2u * window;
    cursor += (size_t)waves * 2u * window;
  }
  if (planes.depth_raw) {
    depth_lds = cursor + (size_t)wave * window;
    cursor += (size_t)waves * window;
  }
  uint16_t* kf_lds = reinterpret_cast<uint16_t*>(cursor) + (size_t)wave * window;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const uint32_t base = first[tile * 64u];
    const uint32_t entries = first[min(tile * 64u + 64u, s.size)] - base;   // of the tile (wave-uniform)
    if (entries == 0u) continue;
    const TileSurfel t = load_tile_surfel<kDesc>(s, tile, lane);
    const uint32_t my_first = t.in_range ? first[t.i] - base : 0u, my_limit = t.in_range ? first[t.i + 1] - base : 0u;
    ObsStagedSink<kDesc> sink{kf_lds, depth_lds, desc_lds, planes.keyframes, planes.depth_raw, planes.descriptor_raw, (size_t)base, my_first, my_limit,
                              window, lane};
    exact::cost_pairs<true, kDesc>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
    __builtin_amdgcn_wave_barrier();
    const uint32_t n = min(window, entries);
    for (uint32_t i = lane; i < n; i += 64u) planes.keyframes[(size_t)base + i] = kf_lds[i];
    if (depth_lds)
      for (uint32_t i = lane; i < n; i += 64u) planes.depth_raw[(size_t)base + i] = depth_lds[i];
    if (kDesc)
      for (uint32_t i = lane; i < 2u * n; i += 64u) planes.descriptor_raw[2 * (size_t)base + i] = desc_lds[i];
    __builtin_amdgcn_wave_barrier();
  }
}

namespace {
struct ObsGrid {
  uint32_t tiles, padded, waves, grid;
};
ObsGrid obs_grid(const SurfelsView& s, const uint32_t* sched, const ObsShape& shape) {
  ObsGrid g;
  g.tiles = (s.size + 63u) / 64u;
  g.padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(g.padded, sched);
  g.waves = (uint32_t)shape.waves;
  g.grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + g.waves - 1) / g.waves));
  return g;
}
}  // namespace

void launch_observations_count(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                               const uint32_t* sched, const ObsShape& shape, uint32_t* counts, unsigned long long* total) {
  if (s.size == 0 || num_kfs <= 0) return;
  const ObsGrid g = obs_grid(s, sched, shape);
  hipLaunchKernelGGL(observations_count_kernel, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, s, g.tiles, g.padded, sched, counts,
                     total);
}

void launch_observations_fill(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                              const uint32_t* sched, const ObsShape& shape, const uint32_t* first, const ObsPlanes& planes) {
  if (s.size == 0 || num_kfs <= 0 || !planes.keyframes) return;
  const ObsGrid g = obs_grid(s, sched, shape);
  const bool desc = planes.descriptor_raw != nullptr;
  if (shape.stage_entries <= 0) {
    if (desc)
      hipLaunchKernelGGL(observations_fill_direct_kernel<true>, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, s, g.tiles, g.padded,
                         sched, first, planes);
    else
      hipLaunchKernelGGL(observations_fill_direct_kernel<false>, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, s, g.tiles, g.padded,
                         sched, first, planes);
    return;
  }
  // the window that fits: waves x window x entry bytes within kObsMaxLdsBytes (a smaller window means more passes, the same words)
  const size_t entry = obs_entry_bytes(planes);
  const uint32_t window = (uint32_t)std::max<size_t>(1, std::min<size_t>((size_t)shape.stage_entries, (size_t)kObsMaxLdsBytes / (g.waves * entry)));
  // the keyframe indices come last and are two bytes wide: the block is rounded up to whole words
  const size_t lds = ((size_t)g.waves * window * entry + 3u) & ~(size_t)3u;
  if (desc)
    hipLaunchKernelGGL(observations_fill_staged_kernel<true>, dim3(g.grid), dim3(64 * g.waves), lds, stream, in, frames, num_kfs, s, g.tiles, g.padded,
                       sched, first, planes, window);
  else
    hipLaunchKernelGGL(observations_fill_staged_kernel<false>, dim3(g.grid), dim3(64 * g.waves), lds, stream, in, frames, num_kfs, s, g.tiles, g.padded,
                       sched, first, planes, window);
}

}  // namespace bahip
#endif
