// kernels_tile_masks.hip -- the tile mask table: the observed structure of the BA in the form a keyframe partition can exchange, and
// the three reductions of it (capi_tile_masks.hip; DESIGN.md section 3, "The tile mask table").
//
// DEFINITION.  A[k][s] = 1 when the pair (surfel s, keyframe k) is in the pair population of the cost sweep with the depth term on
// (cost_device.h: cost_pairs<true, false>: the production association rule, a finite position, activation flags ignored) -- the matrix
// of kernels_covisibility.hip.  T = ceil(N / 64) tiles.  An entry (t, k, m) exists iff m != 0, where bit i of m is A[k][64 t + i].
// tile_first (T + 1 words) delimits the entries of a tile, which are contiguous and ascending in k; entry_keyframe and entry_mask hold
// them.  Integers only: launch shape, tile order, arithmetic flavour and the order anything arrives in cannot move a word.
//
// BUILDING IT.  Two traversals of the cost sweep's (one wavefront per 64-surfel tile, heavy-first run order, persistent workgroups),
// over the keyframes this rank owns (k & owner_mask == owner_rank; owner_mask 0: all of them):
//   count   the tile's entries, into counts[t] and into this rank's 16-bit field of a zero-filled plane of T x ceil(world / 4) int64
//           words -- what the ranks sum; one rank writes a field, so the sum cannot carry;
//   offsets per tile, from the summed plane, the entries of all ranks and of the ranks below this one; the caller scans the former
//           into tile_first;
//   fill    the same traversal writes (k, mask) at tile_first[t] + the lower ranks' entries of t + the running index, into zero-filled
//           planes: the rank-major layout.  pack / unpack move a slice of it through int64 words (a mask is one word, keyframe
//           indices go four to a word) for the sum over the ranks, which is a union because every entry has one writer;
//   merge   per tile the ranks' ascending runs become one ascending run: one lane per entry places itself by counting the tile's
//           smaller keyframes, in chunks of 64 entries.  A tile holds at most K entries.
// No workgroup waits for another; every loop is bounded by K or by the tile's entry count.
//
// THE REDUCTIONS read the merged table from global memory, the tiles t with t % world == rank:
//   co-visibility  per tile the pairs a <= b of its entries: popcount(mask_a & mask_b), at most one 32-bit atomic add per pair into the
//                  lower triangle (row = the later keyframe: the lanes of one instruction run along one row);
//   redundancy     per lane c = the entries holding its bit; the bins present in the tile as (bin, ballot) in LDS; the cells (entry,
//                  present bin): popcount(mask & binmask), at most one atomic per cell -- kernels_redundancy.hip's attribution;
//   observations   per lane the same c is the length of its list; the keyframes plane is the entries holding the lane's bit, in
//                  order; the payload planes need the images: a third traversal over this rank's keyframes, in which a cursor
//                  through the tile's entries, ascending in k like the traversal, gives each lane the position of (s, k) in its list.
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
constexpr uint32_t kTileMaskNaNWord = 0x7fc00000u;

__device__ __forceinline__ void tile_mask_add(uint32_t* __restrict__ word, uint32_t v) {
  __hip_atomic_fetch_add(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void tile_mask_add64(unsigned long long* __restrict__ word, unsigned long long v) {
  __hip_atomic_fetch_add(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long tile_mask_wave_sum(unsigned long long v) {
#pragma unroll
  for (int step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step, 64);
  return v;
}

struct TileMaskCountSink {
  uint32_t seen;   // wave-uniform
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float) {}
  __device__ __forceinline__ void descriptors(int, float, float) {}
  // every lane of the wavefront, only for a keyframe with an associated lane
  __device__ __forceinline__ void end(int, unsigned long long, bool) { ++seen; }
};

// entry `seen` of this rank's run of the tile goes to position base + seen while it is below `limit` (the count the table was laid
// out for): a table that does not belong to this state cannot make a store leave the planes
struct TileMaskFillSink {
  uint32_t* __restrict__ keyframes;
  unsigned long long* __restrict__ masks;
  uint32_t base, limit, seen;   // wave-uniform
  int lane;
  __device__ __forceinline__ int pair(int item) const { return item; }
  __device__ __forceinline__ void depth(int, float) {}
  __device__ __forceinline__ void descriptors(int, float, float) {}
  __device__ __forceinline__ void end(int item, unsigned long long associated, bool) {
    if (seen < limit && lane == 0) {
      keyframes[base + seen] = (uint32_t)item;
      masks[base + seen] = associated;
    }
    ++seen;
  }
};

// The payload of the observation lists.  cursor walks the tile's merged entries [0, entries) ascending in k, as the traversal meets
// the keyframes; pos is the lane's position in its own list: the entries before the cursor that hold its bit.  A lane writes position
// p only while first + p is below the end of its list.
template <bool kDesc>
struct TileMaskPayloadSink {
  const uint32_t* __restrict__ entry_kf;            // the tile's entries
  const unsigned long long* __restrict__ entry_mask;
  float* __restrict__ depth_plane;                  // NULL: not asked for (wave-uniform)
  float* __restrict__ desc_plane;
  uint32_t entries, cursor;                         // wave-uniform
  uint32_t first, limit, pos;
  int lane;
  uint32_t words;                                   // payload words this lane wrote
  __device__ __forceinline__ int pair(int item) {
    while (cursor < entries && entry_kf[cursor] < (uint32_t)item) {
      pos += (uint32_t)((entry_mask[cursor] >> lane) & 1ull);
      ++cursor;
    }
    return item;
  }
  __device__ __forceinline__ void depth(int, float raw) {
    if (depth_plane && first + pos < limit) {
      depth_plane[first + pos] = raw;
      ++words;
    }
  }
  __device__ __forceinline__ void pair_of_words(float r1, float r2) {
    desc_plane[2 * (size_t)(first + pos)] = r1;
    desc_plane[2 * (size_t)(first + pos) + 1] = r2;
    words += 2u;
  }
  __device__ __forceinline__ void descriptors(int, float r1, float r2) {
    if (kDesc && first + pos < limit) pair_of_words(r1, r2);
  }
  __device__ __forceinline__ void end(int, unsigned long long associated, bool has_desc) {
    if (kDesc && !has_desc && ((associated >> lane) & 1ull) && first + pos < limit)
      pair_of_words(__uint_as_float(kTileMaskNaNWord), __uint_as_float(kTileMaskNaNWord));
  }
};
}  // namespace

// ---- building the table ---------------------------------------------------------------------------------------------------------------
// Persistent workgroups of `blockDim.x / 64` wavefronts; wavefront w of workgroup b takes the run-order positions b * waves + w,
// + gridDim.x * waves, ... (heavy tiles first when `sched` is given: wave_cull.h, scheduled_tile).  counts (tiles words) and plane
// (tiles x plane_words int64) are zero before the launch; *listed (zero) += the entries this rank counted.
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_count_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank, SurfelsView s,
                       uint32_t tiles, uint32_t padded_tiles, const uint32_t* __restrict__ sched, uint32_t* __restrict__ counts,
                       long long* __restrict__ plane, uint32_t plane_words, unsigned long long* __restrict__ listed) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long mine = 0;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    TileMaskCountSink sink{0u};
    exact::cost_pairs<true, false>(in, frames, 0, num_kfs, owner_mask, owner_rank, t, sink);
    if (lane == 0 && sink.seen) {
      counts[tile] = sink.seen;
      plane[(size_t)tile * plane_words + (owner_rank >> 2)] = (long long)sink.seen << (16u * (owner_rank & 3u));
    }
    mine += sink.seen;
  }
  if (lane == 0 && mine) tile_mask_add64(listed, mine);
}

// totals[t] = the entries of tile t over all ranks (totals[tiles] = 0: the last input of the scan), rank_offset[t] = those of the ranks
// below `rank`, from the summed plane
__global__ void __launch_bounds__(256)
tile_mask_offsets_kernel(const long long* __restrict__ plane, uint32_t plane_words, uint32_t tiles, uint32_t rank, uint32_t world,
                         uint32_t* __restrict__ totals, uint32_t* __restrict__ rank_offset) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > tiles) return;
  if (t == tiles) {
    totals[t] = 0u;
    return;
  }
  uint32_t total = 0u, below = 0u;
  for (uint32_t r = 0; r < world; ++r) {
    const uint32_t field = (uint32_t)((unsigned long long)plane[(size_t)t * plane_words + (r >> 2)] >> (16u * (r & 3u))) & 0xffffu;
    total += field;
    if (r < rank) below += field;
  }
  totals[t] = total;
  rank_offset[t] = below;
}

// keyframes and masks (`entries` each) are zero before the launch
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_fill_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank, SurfelsView s,
                      uint32_t tiles, uint32_t padded_tiles, const uint32_t* __restrict__ sched, const uint32_t* __restrict__ counts,
                      const uint32_t* __restrict__ tile_first, const uint32_t* __restrict__ rank_offset, uint32_t entries,
                      uint32_t* __restrict__ keyframes, unsigned long long* __restrict__ masks) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const uint32_t mine = counts[tile];
    if (mine == 0u) continue;
    const uint32_t base = tile_first[tile] + rank_offset[tile];
    if (base > entries || mine > entries - base) continue;   // (not this state's table)
    const TileSurfel t = load_tile_surfel<false>(s, tile, lane);
    TileMaskFillSink sink{keyframes, masks, base, mine, 0u, lane};
    exact::cost_pairs<true, false>(in, frames, 0, num_kfs, owner_mask, owner_rank, t, sink);
  }
}

// A slice [begin, begin + count) of the rank-major planes as int64 words: `count` masks, then ceil(count / 4) words of four keyframe
// indices each (K < 65 536) -- and back.
__global__ void __launch_bounds__(256)
tile_mask_pack_kernel(const uint32_t* __restrict__ keyframes, const unsigned long long* __restrict__ masks, uint32_t begin, uint32_t count,
                      long long* __restrict__ stage) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) stage[i] = (long long)masks[begin + i];
  if (i < (count + 3u) / 4u) {
    unsigned long long word = 0ull;
    for (uint32_t q = 0; q < 4u; ++q)
      if (4u * i + q < count) word |= (unsigned long long)(keyframes[begin + 4u * i + q] & 0xffffu) << (16u * q);
    stage[count + i] = (long long)word;
  }
}
__global__ void __launch_bounds__(256)
tile_mask_unpack_kernel(const long long* __restrict__ stage, uint32_t begin, uint32_t count, uint32_t* __restrict__ keyframes,
                        unsigned long long* __restrict__ masks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  masks[begin + i] = (unsigned long long)stage[i];
  keyframes[begin + i] = (uint32_t)((unsigned long long)stage[count + (i >> 2)] >> (16u * (i & 3u))) & 0xffffu;
}

// rank-major -> ascending in k, per tile: wavefront w of workgroup b takes the tiles b * waves + w, + gridDim.x * waves, ...
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_merge_kernel(const uint32_t* __restrict__ tile_first, uint32_t tiles, uint32_t entries, const uint32_t* __restrict__ in_kf,
                       const unsigned long long* __restrict__ in_mask, uint32_t* __restrict__ out_kf, unsigned long long* __restrict__ out_mask) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t tile = blockIdx.x * waves + wave; tile < tiles; tile += gridDim.x * waves) {
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    if (end <= base || end > entries) continue;
    const uint32_t n = end - base;
    for (uint32_t chunk = 0; chunk < n; chunk += 64u) {
      const uint32_t e = chunk + lane;
      const bool live = e < n;
      const uint32_t k = live ? in_kf[base + e] : 0u;
      uint32_t place = 0u;
      for (uint32_t j = 0; j < n; ++j) place += in_kf[base + j] < k ? 1u : 0u;   // (wave-uniform loads)
      if (live) {   // (distinct keyframes: place < n)
        out_kf[base + place] = k;
        out_mask[base + place] = in_mask[base + e];
      }
    }
  }
}

// ---- the reductions -------------------------------------------------------------------------------------------------------------------
// The tiles t with (t % world) == rank.  counts[i][j] += surfels shared by the entries' keyframes, i >= j; *adds += atomics issued.
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_covisibility_kernel(const uint32_t* __restrict__ tile_first, uint32_t tiles, uint32_t entries, const uint32_t* __restrict__ entry_kf,
                              const unsigned long long* __restrict__ entry_mask, uint32_t rank, uint32_t world, uint32_t num_kfs,
                              uint32_t* __restrict__ counts, uint32_t pitch, unsigned long long* __restrict__ adds) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long atomics = 0;
  for (uint32_t slot = blockIdx.x * waves + wave; (size_t)slot * world + rank < tiles; slot += gridDim.x * waves) {
    const uint32_t tile = slot * world + rank;
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    if (end <= base || end > entries) continue;
    const uint32_t n = end - base;
    for (uint32_t b = 0; b < n; ++b) {   // the later keyframe of the pair: a row of the lower triangle
      const uint32_t kb = entry_kf[base + b];
      const unsigned long long mb = entry_mask[base + b];
      for (uint32_t chunk = 0; chunk <= b; chunk += 64u) {
        const uint32_t a = chunk + lane;
        uint32_t v = 0u;
        if (a <= b) {
          const uint32_t ka = entry_kf[base + a];
          v = (uint32_t)__popcll(entry_mask[base + a] & mb);
          if (v && ka < num_kfs && kb < num_kfs) tile_mask_add(counts + (size_t)kb * pitch + ka, v);
          else v = 0u;
        }
        atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(v != 0u));
      }
    }
  }
  if (lane == 0 && atomics) tile_mask_add64(adds, atomics);
}

// The number of the tile's entries that hold the lane's bit (wave-uniform loads of the masks).
__device__ __forceinline__ uint32_t tile_mask_lane_count(const unsigned long long* __restrict__ masks, uint32_t n, uint32_t lane) {
  uint32_t c = 0u;
  for (uint32_t e = 0; e < n; ++e) c += (uint32_t)((masks[e] >> lane) & 1ull);
  return c;
}

// hist[k][min(o, bins - 1)] += ...; LDS: [waves][64] bin masks, then [waves][64] bins
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_redundancy_kernel(const uint32_t* __restrict__ tile_first, uint32_t tiles, uint32_t entries, const uint32_t* __restrict__ entry_kf,
                            const unsigned long long* __restrict__ entry_mask, uint32_t rank, uint32_t world, uint32_t num_kfs, uint32_t bins,
                            uint32_t* __restrict__ hist, uint32_t pitch, unsigned long long* __restrict__ adds) {
  extern __shared__ unsigned long long tile_mask_lds[];
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long* binmasks = tile_mask_lds + (size_t)wave * 64u;
  uint32_t* binvals = reinterpret_cast<uint32_t*>(tile_mask_lds + (size_t)waves * 64u) + (size_t)wave * 64u;
  unsigned long long atomics = 0;
  for (uint32_t slot = blockIdx.x * waves + wave; (size_t)slot * world + rank < tiles; slot += gridDim.x * waves) {
    const uint32_t tile = slot * world + rank;
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    if (end <= base || end > entries) continue;
    const uint32_t n = end - base;
    const uint32_t count = tile_mask_lane_count(entry_mask + base, n, lane);
    // the bins present in the tile, in the order of their first lanes
    const bool counted = count > 0u;
    const uint32_t bin = min(count - 1u, bins - 1u);   // (of a counted lane)
    unsigned long long remaining = __builtin_amdgcn_ballot_w64(counted);
    uint32_t present = 0u;
    while (remaining) {
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)remaining) - 1);
      const unsigned long long m = __builtin_amdgcn_ballot_w64(counted && bin == b);
      if (lane == 0) { binmasks[present] = m; binvals[present] = b; }
      ++present;
      remaining &= ~m;
    }
    __builtin_amdgcn_wave_barrier();
    // the cells (entry, present bin), shared by the lanes: consecutive lanes, consecutive bins of one row
    const uint32_t cells = n * present;
    for (uint32_t first = 0; first < cells; first += 64u) {
      const uint32_t cell = first + lane;
      uint32_t v = 0u;
      if (cell < cells) {
        const uint32_t e = cell / present, i = cell - e * present;
        const uint32_t k = entry_kf[base + e];
        v = (uint32_t)__popcll(entry_mask[base + e] & binmasks[i]);
        if (v && k < num_kfs) tile_mask_add(hist + (size_t)k * pitch + binvals[i], v);
        else v = 0u;
      }
      atomics += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(v != 0u));
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0 && atomics) tile_mask_add64(adds, atomics);
}

// counts[s] = the entries that hold surfel s, for s < surfels (counts[surfels] is not written); *total (zeroed) += their sum
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_observation_counts_kernel(const uint32_t* __restrict__ tile_first, uint32_t tiles, uint32_t entries,
                                    const unsigned long long* __restrict__ entry_mask, uint32_t surfels, uint32_t* __restrict__ counts,
                                    unsigned long long* __restrict__ total) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long mine = 0;
  for (uint32_t tile = blockIdx.x * waves + wave; tile < tiles; tile += gridDim.x * waves) {
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    const uint32_t n = (end <= base || end > entries) ? 0u : end - base;
    const uint32_t count = tile_mask_lane_count(entry_mask + base, n, lane);
    const uint32_t i = tile * 64u + lane;
    if (i < surfels) {
      counts[i] = count;
      mine += count;
    }
  }
  const unsigned long long sum = tile_mask_wave_sum(mine);
  if (lane == 0 && sum) tile_mask_add64(total, sum);
}

// keyframes[first[s] ..) = the keyframes of the entries that hold surfel s, ascending; first: the exclusive scan of the counts
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_observation_keyframes_kernel(const uint32_t* __restrict__ tile_first, uint32_t tiles, uint32_t entries,
                                       const uint32_t* __restrict__ entry_kf, const unsigned long long* __restrict__ entry_mask, uint32_t surfels,
                                       const uint32_t* __restrict__ first, uint16_t* __restrict__ keyframes) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t tile = blockIdx.x * waves + wave; tile < tiles; tile += gridDim.x * waves) {
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    if (end <= base || end > entries) continue;
    const uint32_t i = tile * 64u + lane;
    uint32_t pos = 0u, limit = 0u;
    if (i < surfels) {
      pos = first[i];
      limit = first[i + 1];
    }
    for (uint32_t e = base; e < end; ++e) {   // (wave-uniform loads)
      if (((entry_mask[e] >> lane) & 1ull) && pos < limit) keyframes[pos++] = (uint16_t)entry_kf[e];
    }
  }
}

// the payload of this rank's keyframes into zero-filled planes; *words += the payload words written
template <bool kDesc>
__global__ void __launch_bounds__(64 * kTileMaskMaxWaves)
tile_mask_payload_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank, SurfelsView s,
                         uint32_t tiles, uint32_t padded_tiles, const uint32_t* __restrict__ sched, const uint32_t* __restrict__ tile_first,
                         uint32_t entries, const uint32_t* __restrict__ entry_kf, const unsigned long long* __restrict__ entry_mask,
                         const uint32_t* __restrict__ first, float* __restrict__ depth_plane, float* __restrict__ desc_plane,
                         unsigned long long* __restrict__ words) {
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long mine = 0;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const uint32_t base = tile_first[tile], end = tile_first[tile + 1];
    if (end <= base || end > entries) continue;
    const TileSurfel t = load_tile_surfel<kDesc>(s, tile, lane);
    TileMaskPayloadSink<kDesc> sink{entry_kf + base, entry_mask + base, depth_plane, desc_plane, end - base, 0u, 0u, 0u, 0u, lane, 0u};
    if (t.in_range) {
      sink.first = first[t.i];
      sink.limit = first[t.i + 1];
    }
    exact::cost_pairs<true, kDesc>(in, frames, 0, num_kfs, owner_mask, owner_rank, t, sink);
    mine += sink.words;
  }
  const unsigned long long sum = tile_mask_wave_sum(mine);
  if (lane == 0 && sum) tile_mask_add64(words, sum);
}

// 32-bit words [begin, begin + count) of a plane, two to an int64 word of the stage (the last may hold one) -- and back
__global__ void __launch_bounds__(256)
tile_mask_words_pack_kernel(const uint32_t* __restrict__ plane, size_t begin, uint32_t count, long long* __restrict__ stage) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (count + 1u) / 2u) return;
  unsigned long long word = plane[begin + 2u * (size_t)i];
  if (2u * i + 1u < count) word |= (unsigned long long)plane[begin + 2u * (size_t)i + 1u] << 32;
  stage[i] = (long long)word;
}
__global__ void __launch_bounds__(256)
tile_mask_words_unpack_kernel(const long long* __restrict__ stage, size_t begin, uint32_t count, uint32_t* __restrict__ plane) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  plane[begin + i] = (uint32_t)((unsigned long long)stage[i >> 1] >> (32u * (i & 1u)));
}

// census[0 .. 3) = (entries of the merged table, *adds, 0): what the census hooks of the direct routes report
__global__ void tile_mask_census_kernel(unsigned long long entries, const unsigned long long* __restrict__ adds, unsigned long long* __restrict__ census) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    census[0] = entries;
    census[1] = *adds;
    census[2] = 0ull;
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
namespace {
struct TileMaskGrid {
  uint32_t tiles, padded, waves, grid;
};
TileMaskGrid sweep_grid(const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape) {
  TileMaskGrid g;
  g.tiles = (s.size + 63u) / 64u;
  g.padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(g.padded, sched);
  g.waves = (uint32_t)shape.waves;
  g.grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + g.waves - 1) / g.waves));
  return g;
}
uint32_t table_grid(uint32_t tiles, const TileMaskShape& shape) {
  const uint32_t waves = (uint32_t)shape.waves;
  return std::max(1u, std::min((uint32_t)shape.workgroups, (tiles + waves - 1) / waves));
}
}  // namespace

void launch_tile_mask_count(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                            const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, uint32_t* counts, long long* plane,
                            uint32_t plane_words, unsigned long long* listed) {
  if (s.size == 0 || num_kfs <= 0) return;
  const TileMaskGrid g = sweep_grid(s, sched, shape);
  hipLaunchKernelGGL(tile_mask_count_kernel, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, owner_mask, owner_rank, s, g.tiles,
                     g.padded, sched, counts, plane, plane_words, listed);
}

void launch_tile_mask_offsets(hipStream_t stream, const long long* plane, uint32_t plane_words, uint32_t tiles, uint32_t rank, uint32_t world,
                              uint32_t* totals, uint32_t* rank_offset) {
  hipLaunchKernelGGL(tile_mask_offsets_kernel, dim3((tiles + 1u + 255u) / 256u), dim3(256), 0, stream, plane, plane_words, tiles, rank, world, totals,
                     rank_offset);
}

void launch_tile_mask_fill(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                           const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, const uint32_t* counts,
                           const uint32_t* tile_first, const uint32_t* rank_offset, uint32_t entries, uint32_t* keyframes,
                           unsigned long long* masks) {
  if (s.size == 0 || num_kfs <= 0 || entries == 0u) return;
  const TileMaskGrid g = sweep_grid(s, sched, shape);
  hipLaunchKernelGGL(tile_mask_fill_kernel, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, owner_mask, owner_rank, s, g.tiles,
                     g.padded, sched, counts, tile_first, rank_offset, entries, keyframes, masks);
}

void launch_tile_mask_pack(hipStream_t stream, const uint32_t* keyframes, const unsigned long long* masks, uint32_t begin, uint32_t count,
                           long long* stage) {
  if (count == 0u) return;
  hipLaunchKernelGGL(tile_mask_pack_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, keyframes, masks, begin, count, stage);
}
void launch_tile_mask_unpack(hipStream_t stream, const long long* stage, uint32_t begin, uint32_t count, uint32_t* keyframes,
                             unsigned long long* masks) {
  if (count == 0u) return;
  hipLaunchKernelGGL(tile_mask_unpack_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, stage, begin, count, keyframes, masks);
}

void launch_tile_mask_merge(hipStream_t stream, const TileMaskShape& shape, const uint32_t* tile_first, uint32_t tiles, uint32_t entries,
                            const uint32_t* in_kf, const unsigned long long* in_mask, uint32_t* out_kf, unsigned long long* out_mask) {
  if (tiles == 0u || entries == 0u) return;
  hipLaunchKernelGGL(tile_mask_merge_kernel, dim3(table_grid(tiles, shape)), dim3(64 * shape.waves), 0, stream, tile_first, tiles, entries, in_kf,
                     in_mask, out_kf, out_mask);
}

void launch_tile_mask_covisibility(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t rank, uint32_t world,
                                   int num_kfs, uint32_t* counts, uint32_t pitch, unsigned long long* adds) {
  if (table.tiles == 0u || table.entries == 0u || num_kfs <= 0) return;
  const uint32_t dealt = (table.tiles + world - 1u) / world;
  hipLaunchKernelGGL(tile_mask_covisibility_kernel, dim3(table_grid(dealt, shape)), dim3(64 * shape.waves), 0, stream, table.tile_first, table.tiles,
                     table.entries, table.keyframes, table.masks, rank, world, (uint32_t)num_kfs, counts, pitch, adds);
}

void launch_tile_mask_redundancy(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t rank, uint32_t world,
                                 int num_kfs, int bins, uint32_t* hist, uint32_t pitch, unsigned long long* adds) {
  if (table.tiles == 0u || table.entries == 0u || num_kfs <= 0 || bins <= 0) return;
  const uint32_t dealt = (table.tiles + world - 1u) / world;
  const size_t lds = (size_t)shape.waves * 64u * kTileMaskBinBytes;   // at most 6 KB
  hipLaunchKernelGGL(tile_mask_redundancy_kernel, dim3(table_grid(dealt, shape)), dim3(64 * shape.waves), lds, stream, table.tile_first, table.tiles,
                     table.entries, table.keyframes, table.masks, rank, world, (uint32_t)num_kfs, (uint32_t)bins, hist, pitch, adds);
}

void launch_tile_mask_observation_counts(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t surfels,
                                         uint32_t* counts, unsigned long long* total) {
  if (table.tiles == 0u) return;
  hipLaunchKernelGGL(tile_mask_observation_counts_kernel, dim3(table_grid(table.tiles, shape)), dim3(64 * shape.waves), 0, stream, table.tile_first,
                     table.tiles, table.entries, table.masks, surfels, counts, total);
}

void launch_tile_mask_observation_keyframes(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t surfels,
                                            const uint32_t* first, uint16_t* keyframes) {
  if (table.tiles == 0u || table.entries == 0u) return;
  hipLaunchKernelGGL(tile_mask_observation_keyframes_kernel, dim3(table_grid(table.tiles, shape)), dim3(64 * shape.waves), 0, stream,
                     table.tile_first, table.tiles, table.entries, table.keyframes, table.masks, surfels, first, keyframes);
}

void launch_tile_mask_payload(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                              const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, const TileMaskTable& table,
                              const uint32_t* first, float* depth_plane, float* desc_plane, unsigned long long* words) {
  if (s.size == 0 || num_kfs <= 0 || table.entries == 0u || (!depth_plane && !desc_plane)) return;
  const TileMaskGrid g = sweep_grid(s, sched, shape);
  if (desc_plane)
    hipLaunchKernelGGL(tile_mask_payload_kernel<true>, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, owner_mask, owner_rank, s,
                       g.tiles, g.padded, sched, table.tile_first, table.entries, table.keyframes, table.masks, first, depth_plane, desc_plane, words);
  else
    hipLaunchKernelGGL(tile_mask_payload_kernel<false>, dim3(g.grid), dim3(64 * g.waves), 0, stream, in, frames, num_kfs, owner_mask, owner_rank, s,
                       g.tiles, g.padded, sched, table.tile_first, table.entries, table.keyframes, table.masks, first, depth_plane, desc_plane, words);
}

void launch_tile_mask_words_pack(hipStream_t stream, const uint32_t* plane, size_t begin, uint32_t count, long long* stage) {
  if (count == 0u) return;
  hipLaunchKernelGGL(tile_mask_words_pack_kernel, dim3(((count + 1u) / 2u + 255u) / 256u), dim3(256), 0, stream, plane, begin, count, stage);
}
void launch_tile_mask_words_unpack(hipStream_t stream, const long long* stage, size_t begin, uint32_t count, uint32_t* plane) {
  if (count == 0u) return;
  hipLaunchKernelGGL(tile_mask_words_unpack_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, stage, begin, count, plane);
}

void launch_tile_mask_census(hipStream_t stream, unsigned long long entries, const unsigned long long* adds, unsigned long long* census) {
  hipLaunchKernelGGL(tile_mask_census_kernel, dim3(1), dim3(64), 0, stream, entries, adds, census);
}

}  // namespace bahip
#endif
