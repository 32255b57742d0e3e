// rcs_launch.h -- the reduced camera system (bahip_reduced_camera_system; kernels_rcs.hip, capi_rcs.hip; DESIGN.md section 3, "The
// reduced camera system"): what the device unit and its driver share.
#pragma once

#include "ba_device.h"
#include "ba_launch.h"

namespace bahip {

// The sums of a call, all 64-bit integers (what the ranks of a surfel partition sum): the fixed-point limb pairs of ba_device.h
// (HbFixed: limb 0 weighs 2^-32, limb 1 weighs 1) and the census.
//   blocks  [K (K + 1) / 2][36][2]   M_ba of the pair b >= a of bound keyframes at block b (b + 1) / 2 + a, word i * 6 + j (row i of
//                                    keyframe b, column j of keyframe a); of a diagonal block only the words i <= j are summed
//   v       [K][6][2]
//   census  [kRcsCensusWords]        list entries, pairs of entries visited (a <= b, masks that meet), limb adds issued, degenerate
//                                    surfels, tiles with more entries than the list holds, non-zero = a value the fixed point cannot hold
constexpr int kRcsBlockWords = 72, kRcsVWords = 12, kRcsCensusWords = 6;
constexpr int kRcsEntries = 0, kRcsPairs = 1, kRcsAtomics = 2, kRcsDegenerate = 3, kRcsOverflowTiles = 4, kRcsInvalid = 5;
__host__ __device__ constexpr size_t rcs_block_index(size_t b, size_t a) { return b * (b + 1) / 2 + a; }   // b >= a

// One wavefront per 64-surfel tile; a workgroup of `waves` wavefronts keeps, per wavefront, a list of `list_capacity` entries in LDS:
// the mask (8 bytes), the keyframe (4) and Y, 6 m words per lane (m = 3 with descriptors: 4 608 bytes, else 1 536).
constexpr int kRcsMaxWaves = 4, kRcsMaxListCapacity = 32;
constexpr int kRcsDefaultWaves = 1, kRcsWorkgroupsPerUnit = 8, kRcsDefaultListCapacity = 8;
constexpr size_t kRcsMaxLdsBytes = 160 * 1024;   // the LDS of a gfx950 compute unit (beyond 64 KB by opt-in)
__host__ __device__ constexpr size_t rcs_entry_bytes(bool use_desc) { return 12 + (use_desc ? 18 : 6) * 64 * sizeof(float); }
struct RcsShape {
  int waves, workgroups, list_capacity;
};
// work := the work items of a pose sweep (launch_pose_accumulate) over every bound keyframe at its current pose, whatever its
// activation: pose_work_records(num_kfs) records
void launch_rcs_work(hipStream_t stream, const KfEntry* frames, int num_kfs, PoseWork* work);
// blocks, v and census zeroed by the caller; false when the shape does not fit the LDS of a workgroup (nothing launched);
// pair_stage false: the factor traversal and the count of degenerate surfels only (timing)
bool launch_rcs_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs,
                      const SurfelsView& s, const uint32_t* sched, const RcsShape& shape, bool pair_stage, long long* blocks, long long* v,
                      long long* census);
// S (6K x 6K doubles, pitch in doubles), g (6K), A_diag (K x 36) and b (K x 6) from the summed limbs: S_kl = delta_kl A_k - M_kl and
// g_k = b_k - v_k in binary64; Hb = the K rows of the pose sums (kHbStride words each).  blocks == NULL: S = blockdiag(A), g = b.
// A NULL plane is skipped.  A sum beyond the fixed point's range raises census[kRcsInvalid].
void launch_rcs_resolve(hipStream_t stream, int num_kfs, const HbFixed* Hb, const long long* blocks, const long long* v, double* S, size_t pitch,
                        double* g, double* A_diag, double* b, long long* census);

}  // namespace bahip
