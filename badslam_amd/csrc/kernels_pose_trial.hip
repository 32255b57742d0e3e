// kernels_pose_trial.hip -- the pose phase of the alternating scheme under step control ("Step control of the
// pose phase"): per keyframe, a damped Gauss-Newton step is kept only if the keyframe's objective falls.
//
// Two kernels per round.  The FUSED SWEEP evaluates, for every work item still iterating and at the pose in its record (the accepted
// pose in round 0, the candidate afterwards), the normal equations AND the cost row: the pose sweep and the cost sweep walk the same
// tiles, cull against the same frusta and make the same gathers and the same association test, so one traversal yields both --
// H, b as the two-limb fixed point of the plain phase (pose_device.h: LdsSink), the cost as the row kernels_cost.hip keeps (three
// exact cells, two counts, a flag; cost_device.h).  The tile body is the plain sweeps' (pose_device.h: pose_tile); what this unit
// adds to it is the per-pair policy below, which puts the cost terms through the cost sweep's row sink (cost_device.h: CostRowSink).
// Persistent workgroups hold both tables of their items in LDS and add the non-zero words to global memory once.  The CONTROLLED SOLVE, one lane per item, resolves the row (exact_sum.h: exact_value),
// decides, keeps the accepted (H, b), pose and cost in the item's record, and derives the next candidate from the stored equations.
#include "ba_device.h"
#include "ba_launch.h"
#include "cost_device.h"
#include "exact_sum.h"
#include "pose_device.h"
#include "se3_device.h"
#include "wave_cull.h"
#include "wave_reduce.h"

namespace bahip {
#ifndef BAHIP_POSE_TRIAL_WAVES_ATTR
#define BAHIP_POSE_TRIAL_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(4)))   // at most 128 VGPRs: the 16 wavefronts of a workgroup on one compute unit
#endif
constexpr int kPoseTrialWaves = 16;
constexpr size_t kPoseTrialLdsLimit = 144 * 1024;   // of the 160 KB of a compute unit
constexpr size_t kPoseTrialItemBytes = sizeof(HbFixed) * kHbStride + sizeof(long long) * kCostWords;   // 688: 214 items per launch (the bench scene's 200 keyframes in one)
}  // namespace bahip

// ---- the fused sweep: compiled once per arithmetic flavour (ba_launch.h) -----------------------------------------------------------
BAHIP_FLAVOURED_BEGIN

// What the fused sweep does per pair besides H, b (pose_device.h: pose_tile's per-pair policy): the pair's three cost terms and two
// counts into the item's row of the workgroup's cost table, through the row sink of the cost sweep (cost_device.h).
template <bool kUseDepth>
struct TrialPairTerms {
  CostRowSink<kUseDepth> cost;
  long long* row;
  bool has_desc;
  // The frustum test derives four norms from the intrinsics (wave_cull.h: sphere_may_project).  Hoisted out of the loops they live in
  // vector registers across the candidate body -- the plain sweep has exactly its 128, this one carries the cost row besides and
  // spilled them.  Taken through an opaque scalar copy per test they are recomputed per chunk of 64 items (four square roots) instead.
  // The copy is an empty inline-asm statement: an optimisation barrier that emits no instruction (DESIGN.md section 3 names it as the
  // unit's exception to "plain C++ only", with the barrier of pose_tile's reduction).
  __device__ __forceinline__ Intrinsics cull_intrinsics(const Intrinsics& in) const {
    Intrinsics c = in;
    asm volatile("" : "+s"(c.fx), "+s"(c.fy), "+s"(c.cx), "+s"(c.cy));
    return c;
  }
  __device__ __forceinline__ void begin(int item) { row = cost.pair(item); has_desc = false; }
  __device__ __forceinline__ void depth(bool visible, float raw) { if (visible) cost.depth(row, raw); }   // (on a visible lane the selected value is the residual itself)
  __device__ __forceinline__ void descriptors(const DescEval& e) { cost.descriptors(row, e.r1, e.r2); has_desc = true; }
  __device__ __forceinline__ void end(unsigned long long associated) { cost.end(row, associated, has_desc); }
};

// Persistent workgroups of blockDim.x / 64 wavefronts; the units (run-order position x part; heavy tiles first when `sched` is
// given: wave_cull.h) are dealt to the wavefronts statically, as the cost sweep and the short later rounds of the plain sweep deal
// them.  LDS: [num_items][kHbStride] limbs of H, b, then [num_items][kCostWords] words of the cost rows.
template <bool kUseDepth, bool kUseDesc>
__global__ void __launch_bounds__(64 * kPoseTrialWaves) BAHIP_POSE_TRIAL_WAVES_ATTR
pose_trial_sweep_kernel(Intrinsics in, const KfEntry* __restrict__ frames, const PoseWork* __restrict__ work, int num_work,
                        const int* __restrict__ listed, int item_begin, int num_items, SurfelsView s, HbFixed* __restrict__ Hb,
                        long long* __restrict__ cost_rows, WaveBounds* __restrict__ tile_bounds, int stored_bounds, int* __restrict__ invalid,
                        uint32_t tiles, uint32_t padded_tiles, const uint32_t* __restrict__ sched, uint32_t parts_shift) {
  extern __shared__ HbFixed trial_table[];
  long long* cost_table = trial_table + (size_t)num_items * kHbStride;
  const int lane = threadIdx.x & 63;
  const int words = num_items * (kHbStride + kCostWords);
  for (int e = threadIdx.x; e < words; e += blockDim.x) trial_table[e] = 0;
  __syncthreads();
  const int slot = wave_reduce28_slot(lane);
  const uint32_t table_address = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) HbFixed*)trial_table;   // LDS byte address
  LdsSink sink{table_address + (uint32_t)(slot > 0 ? slot : 0) * (uint32_t)(kHbLimbs * sizeof(HbFixed)), invalid, slot >= 0 && slot < 27, 0.f, -1};
  const uint32_t waves = blockDim.x >> 6;
  const uint32_t units = sched_positions(padded_tiles, sched) << parts_shift;
  for (uint32_t unit = blockIdx.x * waves + (threadIdx.x >> 6); unit < units; unit += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(unit >> parts_shift, padded_tiles, sched, &tile) || tile >= tiles) continue;
    // (the plain sweeps' tile: `listed` is non-NULL exactly when the bounds are stored -- round 0 has neither --, no tile census)
    pose_tile<kUseDepth, kUseDesc>(in, frames, work, listed, num_work, s, tile_bounds, stored_bounds, num_items, tile, 1 << parts_shift,
                                   (int)(unit & ((1u << parts_shift) - 1u)), sink, nullptr, item_begin, num_items,
                                   TrialPairTerms<kUseDepth>{{cost_table}, nullptr, false});
  }
  __syncthreads();
  for (int e = threadIdx.x; e < words; e += blockDim.x) {
    const long long v = trial_table[e];
    if (v == 0) continue;
    const bool is_cost = e >= num_items * kHbStride;
    const int local = is_cost ? e - num_items * kHbStride : e;
    const int stride = is_cost ? kCostWords : kHbStride;
    const int item = local / stride;
    const int w = listed ? listed[item_begin + item] : item_begin + item;
    long long* dst = (is_cost ? cost_rows : Hb) + (size_t)w * stride + (local - item * stride);
    __hip_atomic_fetch_add(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static int g_pose_trial_waves = 0, g_pose_trial_parts_shift = -1;
void set_pose_trial_shape(int waves, int parts_shift) {
  g_pose_trial_waves = (waves >= 1 && waves <= kPoseTrialWaves) ? waves : 0;
  g_pose_trial_parts_shift = (parts_shift >= 0 && parts_shift <= 3) ? parts_shift : -1;
}

int launch_pose_trial_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, const void* work,
                            int num_work, const int* listed, int num_items, const SurfelsView& s, HbFixed* Hb, long long* cost_rows,
                            void* tile_bounds, bool stored_bounds, const uint32_t* sched) {
  if (s.size == 0 || num_items == 0) return 0;
  auto kernel = use_depth ? (use_desc ? pose_trial_sweep_kernel<true, true> : pose_trial_sweep_kernel<true, false>) : pose_trial_sweep_kernel<false, true>;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  const uint32_t tiles = (s.size + 63u) / 64u, padded = pose_padded_tiles(s.size);
  // small grids (a shard of a multi-GPU run) last as long as their longest tile: the wavefronts share a tile's items there
  const uint32_t parts_shift = g_pose_trial_parts_shift >= 0 ? (uint32_t)g_pose_trial_parts_shift : padded >= 16384 ? 0u : padded >= 8192 ? 1u : 2u;
  const uint32_t waves = g_pose_trial_waves > 0 ? (uint32_t)g_pose_trial_waves : (uint32_t)kPoseTrialWaves;
  const uint32_t units = sched_positions(padded, sched) << parts_shift;
  const uint32_t grid = std::max(1u, std::min((uint32_t)cus, (units + waves - 1) / waves));
  const int per_launch = (int)(kPoseTrialLdsLimit / kPoseTrialItemBytes);
  const int slices = (num_items + per_launch - 1) / per_launch, per_slice = (num_items + slices - 1) / slices;
  const size_t lds = kPoseTrialItemBytes * (size_t)per_slice;
  static bool opted_in[3] = {false, false, false};   // per kernel of this flavour
  const int variant = use_depth ? (use_desc ? 0 : 1) : 2;
  if (lds > 64 * 1024 && !opted_in[variant]) {   // dynamic LDS beyond 64 KB needs the opt-in: once per kernel, not per launch
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPoseTrialLdsLimit);
    if (e != hipSuccess) return (int)e;
    opted_in[variant] = true;
  }
  for (int begin = 0; begin < num_items; begin += per_slice) {
    const int count = std::min(per_slice, num_items - begin);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), kPoseTrialItemBytes * (size_t)count, stream, in, frames, static_cast<const PoseWork*>(work),
                       num_work, listed, begin, count, s, Hb, cost_rows, static_cast<WaveBounds*>(tile_bounds), stored_bounds ? 1 : 0,
                       pose_invalid_word(Hb), tiles, padded, sched, parts_shift);
  }
  return 0;
}

BAHIP_FLAVOURED_END

// ---- what exists once (the exact unit): the controlled solve, the debug hook, the dispatchers --------------------------------------
#ifndef BAHIP_FAST_MATH
namespace bahip {

__device__ __forceinline__ double pose_trial_objective(const bahip_cost& c) { return (c.depth + c.descriptor_1) + c.descriptor_2; }

// One lane per work item still iterating.  `round` 0: the sums are those of the item's pose T -- they become its state, nothing is
// decided.  Later rounds: the sums are those of the candidate T' = T * exp(-x(lambda)); it is accepted iff its objective is finite
// and strictly below the stored one.  An item that goes on gets its next candidate from the STORED equations and the new lambda and
// is appended to `list_next`; an item that is done gets its pose written to the keyframe table (if it took a step at all) and the
// activation rule of the plain phase (pose_solve_kernel).  The sums of the round are cleared for the next one.
__global__ void pose_trial_solve_kernel(PoseWork* __restrict__ work, int num_work, PoseTrialRecord* __restrict__ records, HbFixed* __restrict__ Hb,
                                        long long* __restrict__ cost_rows, KfEntry* __restrict__ frames, bahip_pose_step_control control,
                                        int update_activation, int round, const float* __restrict__ lambda_in, int* __restrict__ ctl,
                                        int* __restrict__ list_next) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w == 0 && *pose_invalid_word(Hb) != 0) {   // raised by a sweep of this round, on this rank or another (pose_device.h)
    atomicOr(&ctl[kPoseTrialInvalid], 1);
    Hb[27 * kHbLimbs] = 0;
  }
  if (w >= num_work || work[w].done) return;
  PoseWork& pw = work[w];
  PoseTrialRecord& rec = records[w];
  HbFixed* fixed = Hb + (size_t)w * kHbStride;
  long long* row = cost_rows + (size_t)w * kCostWords;
  bool out_of_range = false;
#pragma unroll
  for (int c = 0; c < 27; ++c) {
    const HbFixed hi = fixed[c * kHbLimbs + 1];
    out_of_range = out_of_range || hi >= kHbSumLimit || hi <= -kHbSumLimit;
  }
  if (out_of_range) atomicOr(&ctl[kPoseTrialInvalid], 1);
  long long cells[3][kExactLimbs];
#pragma unroll
  for (int c = 0; c < 3; ++c) cost_normalise(row + c * kExactLimbs, cells[c]);
  const bahip_cost fresh = cost_resolve(cells, row[kCostDepthCountWord], row[kCostPairCountWord], row[kCostFlagWord] != 0);

  bool take, done = false;
  if (round == 0) {
    take = true;
    rec.lambda = lambda_in[w];
    rec.cost_before = fresh;
    rec.trials = 0; rec.rejected = 0; rec.consecutive_rejected = 0;
    rec.evaluated = 1;
  } else {
    const double f_new = pose_trial_objective(fresh), f_old = pose_trial_objective(rec.cost);
    take = f_new - f_new == 0.0 && f_new < f_old;   // finite and strictly lower
    rec.trials += 1;
  }
  if (take) {
    for (int c = 0; c < kHbStride; ++c) rec.Hb[c] = fixed[c];
    rec.cost = fresh;
    if (round > 0) {
      for (int c = 0; c < 7; ++c) pw.T[c] = rec.T_candidate[c];
      pw.iterations += 1;
      rec.lambda = fmaxf(rec.lambda * control.lambda_down, control.lambda_min);
      rec.consecutive_rejected = 0;
      if (rec.candidate_converged) { pw.converged = 1; done = true; }
      else if (pw.iterations >= BAHIP_MAX_POSE_ITERATIONS) done = true;
    }
  } else {
    rec.lambda = fminf(rec.lambda * control.lambda_up, control.lambda_max);
    rec.rejected += 1;
    rec.consecutive_rejected += 1;
    if (rec.consecutive_rejected >= control.max_trials) done = true;
  }
  for (int c = 0; c < kHbStride; ++c) fixed[c] = 0;
  for (int c = 0; c < kCostWords; ++c) row[c] = 0;

  if (!done) {
    // the stored totals rounded to binary32 first, as pose_solve_kernel rounds them: H and b are what the plain phase solves
    float hb[27], xf[6], next[7], inv[7];
#pragma unroll
    for (int c = 0; c < 27; ++c) hb[c] = (float)hb_value(rec.Hb[c * kHbLimbs], rec.Hb[c * kHbLimbs + 1]);
    pose_gn_step_damped(hb, pw.T, rec.lambda, xf, next);
    for (int c = 0; c < 7; ++c) rec.T_candidate[c] = next[c];
    se3_inverse(next, inv);
    se3_matrix3x4(inv, pw.F);
    rec.candidate_converged = is_scale1_pose_converged(xf) ? 1 : 0;
    const int slot = atomicAdd(&ctl[round & 1], 1);
    list_next[slot] = w;
    return;
  }
  pw.done = 1;
  pw.skip = 1;
  KfEntry& kf = frames[pw.kf_index];
  if (pw.iterations > 0) {   // (a keyframe without an accepted step keeps every word of its entry)
    float inv[7];
    se3_inverse(pw.T, inv);
    se3_matrix3x4(inv, pw.F);
    for (int c = 0; c < 7; ++c) kf.global_T_frame[c] = pw.T[c];
    for (int c = 0; c < 12; ++c) kf.pose.F[c] = pw.F[c];
    se3_rotation(pw.T, kf.pose.GR);
  }
  if (update_activation) {
    float inv0[7], diff[7], lg[6];
    se3_inverse(pw.T0, inv0);
    se3_mul(inv0, pw.T, diff);
    se3_log(diff, lg);
    const bool moved = !is_scale1_pose_converged(lg);
    kf.activation = moved ? BAHIP_KF_ACTIVE : BAHIP_KF_INACTIVE;
    pw.moved = moved ? 1 : 0;
  }
}

void launch_pose_trial_solve(hipStream_t stream, void* work, int num_work, PoseTrialRecord* records, HbFixed* Hb, long long* cost_rows, KfEntry* frames,
                             const bahip_pose_step_control& control, int update_activation, int round, const float* lambda_in, int* ctl,
                             int* list_next) {
  if (num_work == 0) return;
  hipLaunchKernelGGL(pose_trial_solve_kernel, dim3((num_work + 63) / 64), dim3(64), 0, stream, static_cast<PoseWork*>(work), num_work, records, Hb,
                     cost_rows, frames, control, update_activation, round, lambda_in, ctl, list_next);
}

// Test hook: pose_gn_step_damped on explicit inputs.  in = hb[27] | T[7] | lambda; out as pose_step_debug_kernel's.
__global__ void pose_step_damped_debug_kernel(const float* __restrict__ in, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  float hb[27], T[7], xf[6], next[7], inv[7], F[12];
  for (int c = 0; c < 27; ++c) hb[c] = in[c];
  for (int c = 0; c < 7; ++c) T[c] = in[27 + c];
  pose_gn_step_damped(hb, T, in[34], xf, next);
  se3_inverse(next, inv);
  se3_matrix3x4(inv, F);
  for (int c = 0; c < 6; ++c) out[c] = xf[c];
  for (int c = 0; c < 7; ++c) out[6 + c] = next[c];
  for (int c = 0; c < 12; ++c) out[13 + c] = F[c];
}
void launch_pose_step_damped_debug(hipStream_t stream, const float* in, float* out) {
  hipLaunchKernelGGL(pose_step_damped_debug_kernel, dim3(1), dim3(64), 0, stream, in, out);
}

int launch_pose_trial_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, const void* work,
                            int num_work, const int* listed, int num_items, const SurfelsView& s, HbFixed* Hb, long long* cost_rows,
                            void* tile_bounds, bool stored_bounds, const uint32_t* sched) {
  if (in.fast_math) return fast::launch_pose_trial_sweep(stream, use_depth, use_desc, in, frames, work, num_work, listed, num_items, s, Hb, cost_rows, tile_bounds, stored_bounds, sched);
  return exact::launch_pose_trial_sweep(stream, use_depth, use_desc, in, frames, work, num_work, listed, num_items, s, Hb, cost_rows, tile_bounds, stored_bounds, sched);
}
void set_pose_trial_shape(int waves, int parts_shift) { exact::set_pose_trial_shape(waves, parts_shift); fast::set_pose_trial_shape(waves, parts_shift); }

}  // namespace bahip
#endif   // !BAHIP_FAST_MATH
