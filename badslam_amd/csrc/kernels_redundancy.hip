// kernels_redundancy.hip -- keyframe redundancy: per bound keyframe, its surfels by the number of OTHER keyframes that observe them
// (bahip_keyframe_observer_histogram, capi_redundancy.hip; DESIGN.md section 3, "Keyframe redundancy").
//
// DEFINITION.  A[k][s] = 1 when the pair (surfel s, keyframe k) is in the pair population of the cost sweep with the depth term on
// (cost_device.h: cost_pairs<true, false>: the production association rule, a finite position, activation flags ignored), else 0 -- the
// matrix of kernels_covisibility.hip.  c_s = sum over k of A[k][s]; a surfel with A[k][s] = 1 has o = c_s - 1 other observers.
// hist[k][j] = the number of s with A[k][s] = 1 and min(o, bins - 1) = j.  Sums of integers: launch shape, tile order, surfel order,
// list capacity and the order in which atomics arrive cannot move a word.
//
// The traversal is the cost sweep's (cost_pairs, heavy-first run order, one wavefront per 64-surfel tile).  The sink ignores the terms;
// per keyframe with a non-zero ballot every lane adds its own bit of the ballot to its count c -- whatever becomes of the list -- and
// the entry (k, mask) goes into the wavefront's list in LDS while there is room.  After the tile's keyframes a lane with c > 0 knows
// its bin, min(c - 1, bins - 1).  The bins PRESENT in the tile (at most 64, usually a handful) are put into LDS as (bin, ballot of its
// lanes), and the lanes share the cells (entry e, present bin i), i running fastest: popcount(mask_e & binmask_i), added with a 32-bit
// atomic add that returns nothing to hist[k_e][bin_i] where it is not zero -- the lanes of one instruction run along one row of the
// table, then the next.  At most one atomic per (entry, bin present in the entry's mask), never one per (surfel, keyframe).
//
// OVERFLOW.  The list holds `capacity` entries; a tile's entries are bounded by K only.  A tile with more is traversed a second time,
// the bins now known: the entries beyond the list (counted in the order the traversal meets them, which is the same both times: same
// surfels, same poses) are attributed as they are met, lane i taking present bin i.  Nothing is spilled, and the words are those of an
// unbounded list.  A tile that fits is traversed once.
//
// The unit exists once, built with -ffp-contract=off: a context set to the fast flavour launches the same code, and the table is the
// exact flavour's association.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "wave_cull.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
__device__ __forceinline__ void redundancy_add(uint32_t* __restrict__ hist, uint32_t pitch, uint32_t row, uint32_t bin, uint32_t v) {
  __hip_atomic_fetch_add(hist + (size_t)row * pitch + bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sink of cost_pairs.  First traversal: the lane's count and the wavefront's list (`masks`, `ks`: wave-uniform LDS addresses).
// Second traversal (`second`): the entries beyond the list against the `present` bins parked in LDS (`binmasks`, `binvals`).  seen,
// second, present and atomics are wave-uniform.
struct RedundancySink {
  unsigned long long* masks;
  uint32_t* ks;
  const unsigned long long* binmasks;
  const uint32_t* binvals;
  uint32_t* __restrict__ hist;
  uint32_t pitch;
  int capacity, lane;
  bool second;
  int present, seen;
  uint32_t count;
  unsigned long long atomics;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float) {}
  __device__ __forceinline__ void descriptors(int, float, float) {}
  // every lane of the wavefront, only for a keyframe with an associated lane
  __device__ __forceinline__ void end(int item, unsigned long long associated, bool /*has_desc*/) {
    const int n = seen++;
    if (!second) {
      count += (uint32_t)((associated >> lane) & 1ull);   // (the list plays no part in the count)
      if (n < capacity && lane == 0) { masks[n] = associated; ks[n] = (uint32_t)item; }
      return;
    }
    if (n < capacity) return;
    // beyond the list: this entry against every present bin, lane i taking bin i (present <= 64)
    uint32_t v = 0u;
    if (lane < present) {
      v = (uint32_t)__popcll(associated & binmasks[lane]);
      if (v) redundancy_add(hist, pitch, (uint32_t)item, binvals[lane], v);
    }
    atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(v != 0u));
  }
};
}  // namespace

// hist[k][j] = 0 for k < num_kfs, j < bins; the words [bins, pitch) of a row are not touched
__global__ void __launch_bounds__(256) redundancy_clear_kernel(uint32_t* __restrict__ hist, uint32_t num_kfs, uint32_t bins, uint32_t pitch) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_kfs * bins) return;
  hist[(size_t)(w / bins) * pitch + w % bins] = 0u;
}

// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile).  census: NULL, or three words --
// (tile, keyframe) entries with a non-zero mask, atomic adds issued into hist, tiles traversed a second time.
__global__ void __launch_bounds__(64 * kRedundancyMaxWaves)
redundancy_sweep_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                        const uint32_t* __restrict__ sched, int capacity, int attribute, uint32_t bins, uint32_t* __restrict__ hist, uint32_t pitch,
                        unsigned long long* __restrict__ census) {
  // [waves][capacity] masks, [waves][64] bin masks, then [waves][capacity] keyframe indices, [waves][64] bins
  extern __shared__ unsigned long long redundancy_lds[];
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long* masks = redundancy_lds + (size_t)wave * capacity;
  unsigned long long* binmasks = redundancy_lds + (size_t)waves * capacity + (size_t)wave * 64u;
  uint32_t* words = reinterpret_cast<uint32_t*>(redundancy_lds + (size_t)waves * ((size_t)capacity + 64u));
  uint32_t* ks = words + (size_t)wave * capacity;
  uint32_t* binvals = words + (size_t)waves * capacity + (size_t)wave * 64u;
  unsigned long long entries = 0, atomics = 0, overflowed = 0;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    RedundancySink sink{masks, ks, binmasks, binvals, hist, pitch, capacity, lane, false, 0, 0, 0u, 0ull};
    exact::cost_pairs<true, false>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
    __builtin_amdgcn_wave_barrier();
    entries += (unsigned long long)sink.seen;
    if (sink.seen > capacity) ++overflowed;
    if (!attribute || sink.seen == 0) continue;
    // the bins present in the tile, in the order of their first lanes
    const bool counted = sink.count > 0u;
    const uint32_t bin = min(sink.count - 1u, bins - 1u);   // (of a counted lane)
    unsigned long long remaining = __builtin_amdgcn_ballot_w64(counted);
    int present = 0;
    while (remaining) {
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)remaining) - 1);
      const unsigned long long m = __builtin_amdgcn_ballot_w64(counted && bin == b);
      if (lane == 0) { binmasks[present] = m; binvals[present] = b; }
      ++present;
      remaining &= ~m;
    }
    __builtin_amdgcn_wave_barrier();
    // the cells (entry, present bin) of the list, shared by the lanes: consecutive lanes, consecutive bins of one row
    const uint32_t cells = (uint32_t)min(sink.seen, capacity) * (uint32_t)present;
    for (uint32_t base = 0; base < cells; base += 64u) {
      const uint32_t cell = base + (uint32_t)lane;
      uint32_t v = 0u;
      if (cell < cells) {
        const uint32_t e = cell / (uint32_t)present, i = cell - e * (uint32_t)present;
        v = (uint32_t)__popcll(masks[e] & binmasks[i]);
        if (v) redundancy_add(hist, pitch, ks[e], binvals[i], v);
      }
      atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(v != 0u));
    }
    if (sink.seen > capacity) {   // the entries beyond the list: a second traversal, the bins known
      sink.second = true;
      sink.present = present;
      sink.seen = 0;
      exact::cost_pairs<true, false>(in, frames, 0, num_kfs, 0u, 0u, t, sink);
      atomics += sink.atomics;
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (census && lane == 0) {
    if (entries) __hip_atomic_fetch_add(census + 0, entries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (atomics) __hip_atomic_fetch_add(census + 1, atomics, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (overflowed) __hip_atomic_fetch_add(census + 2, overflowed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the compact num_kfs x bins words of a shard as int64, for the sum over the ranks, and back into the caller's pitched rows
__global__ void __launch_bounds__(256) redundancy_widen_kernel(const uint32_t* __restrict__ compact, uint32_t words, long long* __restrict__ wide) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < words) wide[w] = (long long)compact[w];
}
__global__ void __launch_bounds__(256) redundancy_narrow_kernel(const long long* __restrict__ wide, uint32_t num_kfs, uint32_t bins,
                                                                uint32_t* __restrict__ hist, uint32_t pitch) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_kfs * bins) return;
  hist[(size_t)(w / bins) * pitch + w % bins] = (uint32_t)wide[w];
}

void launch_redundancy_clear(hipStream_t stream, uint32_t* hist, int num_kfs, int bins, uint32_t pitch) {
  if (num_kfs <= 0 || bins <= 0) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)bins;
  hipLaunchKernelGGL(redundancy_clear_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, hist, (uint32_t)num_kfs, (uint32_t)bins, pitch);
}

void launch_redundancy_sweep(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                             const uint32_t* sched, const RedundancyShape& shape, bool attribute, int bins, uint32_t* hist, uint32_t pitch,
                             unsigned long long* census) {
  const uint32_t tiles = (s.size + 63u) / 64u;
  if (tiles == 0 || num_kfs <= 0 || bins <= 0) return;
  const uint32_t padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(padded, sched);
  const uint32_t waves = (uint32_t)shape.waves;
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + waves - 1) / waves));
  const size_t lds = (size_t)waves * ((size_t)shape.list_capacity + 64u) * kRedundancyEntryBytes;   // at most 48 KB: no opt-in
  hipLaunchKernelGGL(redundancy_sweep_kernel, dim3(grid), dim3(64 * waves), lds, stream, in, frames, num_kfs, s, tiles, padded, sched,
                     shape.list_capacity, attribute ? 1 : 0, (uint32_t)bins, hist, pitch, census);
}

void launch_redundancy_widen(hipStream_t stream, const uint32_t* compact, uint32_t words, long long* wide) {
  if (words == 0u) return;
  hipLaunchKernelGGL(redundancy_widen_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, compact, words, wide);
}

void launch_redundancy_narrow(hipStream_t stream, const long long* wide, int num_kfs, int bins, uint32_t* hist, uint32_t pitch) {
  if (num_kfs <= 0 || bins <= 0) return;
  const uint32_t words = (uint32_t)num_kfs * (uint32_t)bins;
  hipLaunchKernelGGL(redundancy_narrow_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream, wide, (uint32_t)num_kfs, (uint32_t)bins, hist, pitch);
}

}  // namespace bahip
#endif
