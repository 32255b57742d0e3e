// kernels_lifecycle_dealt.hip -- the surfel lifecycle dealt over the ranks of a surfel partition (bahip_context_set_lifecycle_dealing).
//
// Inside a whole-cloud phase of surfel sharding every rank holds the gathered cloud and every keyframe's images.  Creation and merging
// deal their up-front sweeps by keyframe with the keyframe-sharded kernels of kernels_lifecycle.hip; deletion + radius update is per
// surfel over ALL keyframes, so it is dealt by surfel instead: each rank sweeps its own chunks of the chunk-cyclic partition (chunk c of
// the gathered cloud belongs to rank c % world) with delete_update_kernel's arithmetic and writes, per surfel, the two words the decision
// leaves in the data rows -- x (the deleted marker or unchanged) and the squared radius (the new minimum or unchanged) -- as one 64-bit
// word of a zero-filled vector, and the number it newly deleted behind it.  That vector is summed over the ranks as int64 (every word has
// exactly one non-zero contributor, so the sum is that rank's bits) and delete_unpack_kernel writes the two rows on every rank.
// The accumulator rows delete_update_kernel fills (scratch by contract) are not written.
//
// The lifecycle exists in one (exact) flavour: this unit is built once, like kernels_lifecycle.hip.
#include <hip/hip_fp16.h>

#include "ba_device.h"
#include "ba_launch.h"

namespace bahip {

namespace {
constexpr int kDealBlock = 256;
inline unsigned blocks_for(uint32_t n) { return (n + kDealBlock - 1) / kDealBlock; }
}  // namespace

// thread t of the grid -> surfel t of this rank's chunks, in ascending order; index of that surfel in the gathered cloud.  chunk is a
// multiple of 64, so a wavefront sweeps 64 consecutive surfels of one chunk.
__device__ __forceinline__ uint32_t dealt_surfel(uint32_t t, uint32_t rank, uint32_t world, uint32_t chunk) {
  return ((t / chunk) * world + rank) * chunk + t % chunk;
}

// delete_update_kernel (kernels_lifecycle.hip, B/kernel_delete_surfels.cu:42-176) over this rank's chunks; packed[i] = (x, radius^2)
// as the decision leaves them; *deleted_count += the surfels this rank newly marked deleted.  packed and the count start zeroed.
__global__ void __launch_bounds__(kDealBlock)
delete_chunks_kernel(Intrinsics in, const KfEntry* __restrict__ kfs, int num_kfs, SurfelsView s, uint32_t own_count, uint32_t rank, uint32_t world,
                     uint32_t chunk, int min_observation_count, uint2* __restrict__ packed, uint32_t* __restrict__ deleted_count) {
  const uint32_t t = blockIdx.x * kDealBlock + threadIdx.x;
  bool newly_deleted = false;
  if (t < own_count) {
    const uint32_t i = dealt_surfel(t, rank, world, chunk);
    const Vec3 gp = surfel_position(s, i);
    const Vec3 gn = surfel_normal(s, i);
    float obs = 0, viol = 0, min_r = __builtin_huge_valf();
    for (int k = 0; k < num_kfs; ++k) {
      Assoc r;
      bool fsv = false;
      if (project_associate<true>(in, kfs[k].pose.F, kfs[k].geom, gp, gn, &r, &fsv)) {
        obs += 1.f;
        min_r = fminf(min_r, __half2float(__ushort_as_half(pitched_load(kfs[k].radius, kfs[k].radius_pitch, r.py, r.px))));
      } else if (fsv) {
        viol += 1.f;
      }
    }
    uint2 word = make_uint2(__float_as_uint(gp.x), __float_as_uint(s.row(kSurfelRadiusSquared)[i]));
    if (obs < (float)min_observation_count || viol > obs) {
      if (word.x != kDeletedSurfelBits) { word.x = kDeletedSurfelBits; newly_deleted = true; }
    } else {
      word.y = __float_as_uint(min_r);
    }
    packed[i] = word;
  }
  const unsigned long long m = __ballot(newly_deleted);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(deleted_count, (uint32_t)__popcll(m));
}

// every rank, after the sum over the ranks: the two rows the decision writes, for the whole cloud
__global__ void __launch_bounds__(kDealBlock)
delete_unpack_kernel(SurfelsView s, const uint2* __restrict__ packed) {
  const uint32_t i = blockIdx.x * kDealBlock + threadIdx.x;
  if (i >= s.size) return;
  const uint2 word = packed[i];
  s.row(kSurfelX)[i] = __uint_as_float(word.x);
  s.row(kSurfelRadiusSquared)[i] = __uint_as_float(word.y);
}

// ---- launches (ba_launch.h) ------------------------------------------------------------------------------------------------------------
uint32_t dealt_surfel_count(uint32_t total, uint32_t rank, uint32_t world, uint32_t chunk) {
  const uint64_t stride = (uint64_t)chunk * (uint64_t)world;
  const uint64_t full = total / stride, rest = total % stride;
  const uint64_t begin = (uint64_t)rank * chunk;
  const uint64_t tail = rest > begin ? (rest - begin < chunk ? rest - begin : chunk) : 0;
  return (uint32_t)(full * chunk + tail);
}
void launch_delete_chunks(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, uint32_t rank, uint32_t world,
                          uint32_t chunk, int min_obs, void* packed, uint32_t* deleted_count) {
  const uint32_t own = dealt_surfel_count(s.size, rank, world, chunk);
  if (own)
    hipLaunchKernelGGL(delete_chunks_kernel, dim3(blocks_for(own)), dim3(kDealBlock), 0, st, in, kfs, num_kfs, s, own, rank, world, chunk, min_obs,
                       static_cast<uint2*>(packed), deleted_count);
}
void launch_delete_unpack(hipStream_t st, const SurfelsView& s, const void* packed) {
  if (s.size) hipLaunchKernelGGL(delete_unpack_kernel, dim3(blocks_for(s.size)), dim3(kDealBlock), 0, st, s, static_cast<const uint2*>(packed));
}

}  // namespace bahip
