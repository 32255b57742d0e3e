// kernels_covisibility.hip -- observed co-visibility: for every pair (i, j) of bound keyframes the number of surfels that the BA's own
// association rule pairs with both (bahip_observed_covisibility, capi_covisibility.hip; DESIGN.md section 3, "Observed co-visibility").
//
// DEFINITION.  A[k][s] = 1 when the pair (surfel s, keyframe k) is in the pair population of the cost sweep with the depth term on
// (cost_device.h: cost_pairs<true, false>: the production association rule, a finite position, activation flags ignored), else 0.
// counts[i][j] = sum over s of A[i][s] * A[j][s]: the matrix A A^T, both triangles, the diagonal a keyframe's own pair count.  A sum of
// integers: launch shape, tile order, surfel order and the order in which atomics arrive cannot move a word.
//
// The traversal is the cost sweep's (cost_pairs, heavy-first run order, one wavefront per 64-surfel tile); the sink ignores the terms
// and keeps, per keyframe with a non-zero ballot, the entry (k, mask) -- 64 rows of one column of A -- in the wavefront's list in LDS, k
// ascending by construction.  After the tile's keyframes the lanes share the c (c + 1) / 2 pairs a <= b of the list: popcount(mask_a &
// mask_b), added with a 32-bit atomic add that returns nothing to counts[k_b][k_a] -- the LOWER triangle only (k_b >= k_a), the lanes of
// one instruction running along a row.  The matrix is symmetric, and the pair stage runs at the rate of the scattered 4-byte add:
// measured on the bench scene, 25 adds per nanosecond whether both triangles are summed (20.0 M adds, 0.78 ms) or one (10.4 M adds,
// 0.42 ms) -- so one triangle is summed and a last launch copies it into the upper one.  At most one atomic per (tile, i <= j), never
// one per (surfel, i, j); a pair whose masks do not meet adds nothing.
//
// OVERFLOW.  The list holds `capacity` entries; a tile's entries are bounded by K only.  The tile is then walked in passes: pass p keeps
// the entries p * capacity .. (p + 1) * capacity - 1 (counted in the order the traversal meets them, which is the same in every pass:
// same surfels, same poses) and, for every LATER entry, adds its pairs with the whole list as it is met; after the traversal the
// pairs within the list.  Every pair a <= b is produced exactly once -- within the list of pass a / capacity when b is in the same
// pass, else as a cross pair of that pass -- so the words are those of an unbounded list.  A tile with c entries is traversed
// ceil(c / capacity) times; nothing leaves the chip but the atomics.
//
// The unit exists once, built with -ffp-contract=off: a context set to the fast flavour launches the same code, and the matrix is the
// exact flavour's association.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "wave_cull.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
__device__ __forceinline__ void covis_add(uint32_t* __restrict__ counts, uint32_t pitch, uint32_t row, uint32_t col, uint32_t v) {
  __hip_atomic_fetch_add(counts + (size_t)row * pitch + col, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sink of cost_pairs: the wavefront's list (`masks`, `ks`: wave-uniform LDS addresses), the entries of earlier passes skipped, the
// entries beyond the list paired with it at once.  seen, skip and atomics are wave-uniform.
struct CovisListSink {
  unsigned long long* masks;
  uint32_t* ks;
  uint32_t* __restrict__ counts;
  uint32_t pitch;
  int capacity, lane;
  bool pair_stage;
  int skip, seen;
  unsigned long long atomics;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float) {}
  __device__ __forceinline__ void descriptors(int, float, float) {}
  // every lane of the wavefront, only for a keyframe with an associated lane
  __device__ __forceinline__ void end(int item, unsigned long long associated, bool /*has_desc*/) {
    const int n = seen++;
    if (n < skip) return;
    const int slot = n - skip;
    if (slot < capacity) {
      if (lane == 0) { masks[slot] = associated; ks[slot] = (uint32_t)item; }
      return;
    }
    if (!pair_stage) return;
    // beyond the list, which is full: this entry against every entry of it (all of them earlier keyframes)
    __builtin_amdgcn_wave_barrier();
    for (int a = lane; a < capacity; a += 64) {
      const uint32_t v = (uint32_t)__popcll(masks[a] & associated);
      if (v) covis_add(counts, pitch, (uint32_t)item, ks[a], v);   // (item is the later keyframe: the lower triangle)
      atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(v != 0u));
    }
  }
};

// the pairs a <= b within the first c entries of the list, shared by the lanes; returns the atomics issued (wave-uniform)
__device__ __forceinline__ unsigned long long covis_list_pairs(const unsigned long long* masks, const uint32_t* ks, int c, int lane,
                                                               uint32_t* __restrict__ counts, uint32_t pitch) {
  unsigned long long atomics = 0;
  const int pairs = c * (c + 1) / 2;   // c <= kCovisMaxListCapacity: 8 * pairs + 1 < 2^24, exact in binary32
  for (int base = 0; base < pairs; base += 64) {
    const int p = base + lane;
    bool added = false;
    if (p < pairs) {
      // p = b (b + 1) / 2 + a with a <= b: b from the square root, put right by one step either way
      int b = (int)((sqrtf((float)(8 * p + 1)) - 1.f) * 0.5f);
      if (b * (b + 1) / 2 > p) --b;
      else if ((b + 1) * (b + 2) / 2 <= p) ++b;
      const int a = p - b * (b + 1) / 2;
      const uint32_t v = (uint32_t)__popcll(masks[a] & masks[b]);
      if (v) covis_add(counts, pitch, ks[b], ks[a], v);   // consecutive lanes: consecutive a of one row b
      added = v != 0u;
    }
    atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(added));
  }
  return atomics;
}
}  // namespace

// counts[i][j] = 0 for i, j < num_kfs; the words [num_kfs, pitch) of a row are not touched
__global__ void __launch_bounds__(256) covisibility_clear_kernel(uint32_t* __restrict__ counts, uint32_t num_kfs, uint32_t pitch) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_kfs * num_kfs) return;
  counts[(size_t)(w / num_kfs) * pitch + w % num_kfs] = 0u;
}

// counts[i][j] = counts[j][i] for i < j < num_kfs: the upper triangle from the lower one the sweep summed
__global__ void __launch_bounds__(256) covisibility_mirror_kernel(uint32_t* __restrict__ counts, uint32_t num_kfs, uint32_t pitch) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_kfs * num_kfs) return;
  const uint32_t i = w / num_kfs, j = w % num_kfs;
  if (i < j) counts[(size_t)i * pitch + j] = counts[(size_t)j * pitch + i];
}

// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile).  census: NULL, or three words --
// (tile, keyframe) entries with a non-zero mask, atomic adds issued into counts, tiles that needed more than one pass.
__global__ void __launch_bounds__(64 * kCovisMaxWaves)
covisibility_sweep_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                          const uint32_t* __restrict__ sched, int capacity, int pair_stage, uint32_t* __restrict__ counts, uint32_t pitch,
                          unsigned long long* __restrict__ census) {
  extern __shared__ unsigned long long covis_lds[];   // [waves][capacity] masks, then [waves][capacity] keyframe indices
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long* masks = covis_lds + (size_t)wave * capacity;
  uint32_t* ks = reinterpret_cast<uint32_t*>(covis_lds + (size_t)waves * capacity) + (size_t)wave * capacity;
  unsigned long long entries = 0, atomics = 0, overflowed = 0;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    CovisListSink sink{masks, ks, counts, pitch, capacity, lane, pair_stage != 0, 0, 0, 0ull};
#pragma unroll 1
    for (;;) {   // the passes of the tile (one, unless its entries outnumber the list)
      sink.seen = 0;
      exact::cost_pairs<true, false>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
      __builtin_amdgcn_wave_barrier();
      const int listed = min(sink.seen - sink.skip, capacity);
      if (pair_stage && listed > 0) sink.atomics += covis_list_pairs(masks, ks, listed, lane, counts, pitch);
      __builtin_amdgcn_wave_barrier();
      if (sink.skip == 0) {
        entries += (unsigned long long)sink.seen;
        if (sink.seen > capacity) ++overflowed;
      }
      if (!pair_stage || sink.seen - sink.skip <= capacity) break;
      sink.skip += capacity;
    }
    atomics += sink.atomics;
  }
  if (census && lane == 0) {
    if (entries) __hip_atomic_fetch_add(census + 0, entries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (atomics) __hip_atomic_fetch_add(census + 1, atomics, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (overflowed) __hip_atomic_fetch_add(census + 2, overflowed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the compact num_kfs x num_kfs words of a shard as int64, for the sum over the ranks, and back into the caller's pitched rows
__global__ void __launch_bounds__(256) covisibility_widen_kernel(const uint32_t* __restrict__ compact, uint32_t words, long long* __restrict__ wide) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < words) wide[w] = (long long)compact[w];
}
__global__ void __launch_bounds__(256) covisibility_narrow_kernel(const long long* __restrict__ wide, uint32_t num_kfs, uint32_t* __restrict__ counts,
                                                                  uint32_t pitch) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_kfs * num_kfs) return;
  counts[(size_t)(w / num_kfs) * pitch + w % num_kfs] = (uint32_t)wide[w];
}

void launch_covisibility_clear(hipStream_t stream, uint32_t* counts, int num_kfs, uint32_t pitch) {
  if (num_kfs <= 0) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)num_kfs;
  hipLaunchKernelGGL(covisibility_clear_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, counts, (uint32_t)num_kfs, pitch);
}

void launch_covisibility_sweep(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                               const uint32_t* sched, const CovisShape& shape, bool pair_stage, uint32_t* counts, uint32_t pitch,
                               unsigned long long* census) {
  const uint32_t tiles = (s.size + 63u) / 64u;
  if (tiles == 0 || num_kfs <= 0) return;
  const uint32_t padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(padded, sched);
  const uint32_t waves = (uint32_t)shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + waves - 1) / waves));
  const size_t lds = (size_t)waves * (size_t)shape.list_capacity * kCovisEntryBytes;   // at most 48 KB: no opt-in
  hipLaunchKernelGGL(covisibility_sweep_kernel, dim3(grid), dim3(64 * waves), lds, stream, in, frames, num_kfs, s, tiles, padded, sched,
                     shape.list_capacity, pair_stage ? 1 : 0, counts, pitch, census);
}

void launch_covisibility_mirror(hipStream_t stream, uint32_t* counts, int num_kfs, uint32_t pitch) {
  if (num_kfs <= 1) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)num_kfs;
  hipLaunchKernelGGL(covisibility_mirror_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, counts, (uint32_t)num_kfs, pitch);
}

void launch_covisibility_widen(hipStream_t stream, const uint32_t* compact, int num_kfs, long long* wide) {
  if (num_kfs <= 0) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)num_kfs;
  hipLaunchKernelGGL(covisibility_widen_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, compact, words, wide);
}

void launch_covisibility_narrow(hipStream_t stream, const long long* wide, int num_kfs, uint32_t* counts, uint32_t pitch) {
  if (num_kfs <= 0) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)num_kfs;
  hipLaunchKernelGGL(covisibility_narrow_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, wide, (uint32_t)num_kfs, counts, pitch);
}

}  // namespace bahip
#endif
