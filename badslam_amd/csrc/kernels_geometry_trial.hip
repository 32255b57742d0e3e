// kernels_geometry_trial.hip -- step control for the geometry phase of the alternating scheme: the damped per-surfel solve from the
// class partials of the position pass, and the per-surfel decision from two planes of the per-surfel cost
// (bahip_optimize_geometry_iteration_controlled, capi_geometry_trial.hip).  The reference has no such mode.
//
// With the poses frozen a surfel's cost depends on that surfel alone, so every surfel is its own small problem: the call keeps or
// undoes each surfel's step by that surfel's cost, and a rejected surfel tries again under more damping while the accepted ones rest.
// The sweeps are the library's own (kernels_surfel.hip: phases 1 and 2 of the three-phase step; kernels_surfel_cost.hip); this unit holds
// the per-surfel arithmetic only: one thread per surfel, no keyframe is visited, no atomic, no LDS beyond the eight words of a count.
//
// DEFINITION of the damped solve.  tot[q] = (p0[q] + p1[q]) + p2[q] ... over the classes, the order of kSumsConsume (kernels_surfel.hip:
// tile_sums).  With a scalar lambda >= 0 (binary32, the same for every surfel of a trial) the diagonal is damped as ONE product and then
// ONE add: H_ii = (a_ii + 1e-6f) + lambda * a_ii for a0, a3 and a5, followed by the Cholesky solve of geometry_step word for word;
// depth-only: the gate stays H > 1e-6f and t = -b / (H + lambda * H).  lambda = 0 and finite sums: lambda * a = +-0 and x + (+-0) = x
// for the x met here (a + 1e-6f and H are not zero), so every expression has the bits of the plain step.  The unit exists once, built
// with -ffp-contract=off, and both arithmetic flavours of the sweeps launch it; the pragma below keeps a change of flags from fusing
// the product into the add.
#include "ba_device.h"
#include "ba_launch.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
constexpr int kTrialBlock = kGeometryTrialBlock;

__device__ __forceinline__ bool word_finite(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

// the count of the workgroup's threads with `flag` set, valid in thread 0; every thread of the workgroup must call
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t* lds /* kTrialBlock / 64 words */) {
  const uint32_t wave_total = (uint32_t)__popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  uint32_t total = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kTrialBlock / 64; ++w) total += lds[w];
  __syncthreads();   // the words are reused by the next call
  return total;
}
}  // namespace

// Saves the five words of every surfel and opens the live ones (active, position not NaN).
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_snapshot_kernel(SurfelsView s, GeometryTrialState st) {
  const uint32_t i = blockIdx.x * kTrialBlock + threadIdx.x;
  if (i >= s.size) return;
  const int rows[kGeometryTrialWords] = {kSurfelX, kSurfelY, kSurfelZ, kSurfelDescriptor1, kSurfelDescriptor2};
  uint32_t w[kGeometryTrialWords];
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) w[r] = reinterpret_cast<const uint32_t*>(s.row(rows[r]))[i];
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) st.saved[(size_t)r * st.stride + i] = w[r];
  const float x = __uint_as_float(w[0]);
  const bool live = (s.active[i] & kSurfelActiveFlag) != 0 && x == x;
  st.open[i] = live ? 1 : 0;
  st.outcome[i] = 0;
}

// The candidate of trial `trial` under damping `lambda` for every open surfel, from the saved words, the normal row and the exchanged
// class partials; written under the plain step's own write conditions.  Trial 0 closes the surfels whose candidate is their words.
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_solve_kernel(SurfelsView s, ClassPartials cpp, int classes, int use_desc, float lambda, int trial, GeometryTrialState st) {
  const uint32_t i = blockIdx.x * kTrialBlock + threadIdx.x;
  if (i >= s.size || !st.open[i]) return;
  const int count = use_desc ? 8 : 2;
  float tot[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (q >= count) { tot[q] = 0.f; continue; }
    float t = cpp.data[(size_t)(0 * count + q) * cpp.stride + i] + cpp.data[(size_t)(1 * count + q) * cpp.stride + i];
    for (int c = 2; c < classes; ++c) t += cpp.data[(size_t)(c * count + q) * cpp.stride + i];
    tot[q] = t;
  }
  uint32_t old[kGeometryTrialWords];
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) old[r] = st.saved[(size_t)r * st.stride + i];
  const Vec3 gp = mk3(__uint_as_float(old[0]), __uint_as_float(old[1]), __uint_as_float(old[2]));
  const Vec3 gn = surfel_normal(s, i);
  uint32_t cand[kGeometryTrialWords];
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) cand[r] = old[r];
  if (!use_desc) {
    const float H = tot[0], b = tot[1];
    if (H > 1e-6f) {
      const float damping = lambda * H;
      const float t = -1.f * b / (H + damping);
      const Vec3 np = gp + t * gn;
      cand[0] = __float_as_uint(np.x); cand[1] = __float_as_uint(np.y); cand[2] = __float_as_uint(np.z);
    }
  } else {
    const float d1 = __uint_as_float(old[3]), d2 = __uint_as_float(old[4]);
    const float a0 = tot[0], a1 = tot[1], a2 = tot[2], a3 = tot[3], a5 = tot[4], a6 = tot[5], a7 = tot[6], a8 = tot[7];
    const float t0 = lambda * a0, t3 = lambda * a3, t5 = lambda * a5;
    float H00 = (a0 + 1e-6f) + t0, H01 = a1, H02 = a2, H11 = (a3 + 1e-6f) + t3, H12 = 0.f, H22 = (a5 + 1e-6f) + t5;
    H00 = sqrtf(H00);
    H01 = H01 / H00;
    H11 = sqrtf(H11 - H01 * H01);
    H02 = H02 / H00;
    H12 = (H12 - H02 * H01) / H11;
    H22 = sqrtf(H22 - H02 * H02 - H12 * H12);
    const float y0 = a6 / H00;
    const float y1 = (a7 - H01 * y0) / H11;
    const float y2 = (a8 - H02 * y0 - H12 * y1) / H22;
    const float x2 = y2 / H22;
    const float x1 = (y1 - H12 * x2) / H11;
    const float x0 = (y0 - H02 * x2 - H01 * x1) / H00;
    if (x0 != 0) {
      const Vec3 np = gp - x0 * gn;
      cand[0] = __float_as_uint(np.x); cand[1] = __float_as_uint(np.y); cand[2] = __float_as_uint(np.z);
    }
    if (x1 != 0) cand[3] = __float_as_uint(fmaxf(-180.f, fminf(180.f, d1 - x1)));
    if (x2 != 0) cand[4] = __float_as_uint(fmaxf(-180.f, fminf(180.f, d2 - x2)));
  }
  bool moved = false;
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) moved = moved || cand[r] != old[r];
  if (trial == 0 && !moved) { st.open[i] = 0; return; }   // (its outcome is the snapshot's 0)
  const int rows[kGeometryTrialWords] = {kSurfelX, kSurfelY, kSurfelZ, kSurfelDescriptor1, kSurfelDescriptor2};
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r)
    if (cand[r] != old[r]) reinterpret_cast<uint32_t*>(s.row(rows[r]))[i] = cand[r];
}

// Keeps or undoes the candidate of every open surfel: c0 = the cost planes of the state before the trials, c1 = those of the candidate
// state.  partials[block] = {open surfels met, accepted, rejected by the pair guard alone, 0}.
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_decide_kernel(SurfelsView s, SurfelCostPlanes c0, SurfelCostPlanes c1, int guard_pairs, int trial, GeometryTrialState st,
                             uint32_t* __restrict__ partials) {
  __shared__ uint32_t lds[kTrialBlock / 64];
  const uint32_t i = blockIdx.x * kTrialBlock + threadIdx.x;
  const bool open = i < s.size && st.open[i] != 0;
  bool accepted = false, lost_pairs = false;
  if (open) {
    const int rows[kGeometryTrialWords] = {kSurfelX, kSurfelY, kSurfelZ, kSurfelDescriptor1, kSurfelDescriptor2};
    bool finite = true;
#pragma unroll
    for (int r = 0; r < kGeometryTrialWords; ++r) finite = finite && word_finite(reinterpret_cast<const uint32_t*>(s.row(rows[r]))[i]);
    if (finite) {   // (a NaN position would read as a deleted surfel of cost 0: its c1 is not looked at)
      const double f0 = (c0.depth[i] + c0.descriptor_1[i]) + c0.descriptor_2[i];
      const double f1 = (c1.depth[i] + c1.descriptor_1[i]) + c1.descriptor_2[i];
      const bool lower = isfinite(f1) && f1 < f0;
      const bool kept_pairs = c1.depth_residuals[i] >= c0.depth_residuals[i] && c1.descriptor_pairs[i] >= c0.descriptor_pairs[i];
      lost_pairs = lower && guard_pairs != 0 && !kept_pairs;
      accepted = lower && !lost_pairs;
    }
    if (accepted) {
      st.outcome[i] = (uint8_t)(1 + trial);
      st.open[i] = 0;
    } else {
#pragma unroll
      for (int r = 0; r < kGeometryTrialWords; ++r) reinterpret_cast<uint32_t*>(s.row(rows[r]))[i] = st.saved[(size_t)r * st.stride + i];
    }
  }
  const uint32_t n_open = block_count(open, lds), n_accepted = block_count(accepted, lds), n_lost = block_count(lost_pairs, lds);
  if (threadIdx.x == 0) {
    uint32_t* mine = partials + 4 * (size_t)blockIdx.x;
    mine[0] = n_open; mine[1] = n_accepted; mine[2] = n_lost; mine[3] = 0;
  }
}

// One workgroup: the partials of the decide launch -> the control words (kGeometryTrialCtl*).
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_count_kernel(const uint32_t* __restrict__ partials, uint32_t blocks, int trial, uint32_t* __restrict__ ctl) {
  __shared__ uint32_t lds[3][kTrialBlock];
  uint32_t sum[3] = {0, 0, 0};
  for (uint32_t b = threadIdx.x; b < blocks; b += kTrialBlock)
    for (int q = 0; q < 3; ++q) sum[q] += partials[4 * (size_t)b + q];
  for (int q = 0; q < 3; ++q) lds[q][threadIdx.x] = sum[q];
  __syncthreads();
  for (int half = kTrialBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half)
      for (int q = 0; q < 3; ++q) lds[q][threadIdx.x] += lds[q][threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t met = lds[0][0], accepted = lds[1][0], lost = lds[2][0];
    if (trial == 0) ctl[kGeometryTrialCtlCandidates] = met;
    ctl[kGeometryTrialCtlOpen] = met - accepted;
    ctl[kGeometryTrialCtlAccepted] += accepted;
    ctl[kGeometryTrialCtlRejectedPairs] += lost;
    ctl[kGeometryTrialCtlRejectedCost] += met - accepted - lost;
  }
}

// The end of the call: what is still open is restored (the decide launch wrote its words back) -> 255; `out` may be NULL.
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_finish_kernel(uint32_t size, GeometryTrialState st, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kTrialBlock + threadIdx.x;
  if (i >= size) return;
  out[i] = st.open[i] ? (uint8_t)255 : st.outcome[i];
}

// The saved words of every surfel back into the rows (an error inside the loop).
__global__ void __launch_bounds__(kTrialBlock)
geometry_trial_restore_kernel(SurfelsView s, GeometryTrialState st) {
  const uint32_t i = blockIdx.x * kTrialBlock + threadIdx.x;
  if (i >= s.size) return;
  const int rows[kGeometryTrialWords] = {kSurfelX, kSurfelY, kSurfelZ, kSurfelDescriptor1, kSurfelDescriptor2};
#pragma unroll
  for (int r = 0; r < kGeometryTrialWords; ++r) reinterpret_cast<uint32_t*>(s.row(rows[r]))[i] = st.saved[(size_t)r * st.stride + i];
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
static inline unsigned trial_blocks(uint32_t n) { return (n + kTrialBlock - 1) / kTrialBlock; }

void launch_geometry_trial_snapshot(hipStream_t st, const SurfelsView& s, const GeometryTrialState& state) {
  if (s.size == 0) return;
  hipLaunchKernelGGL(geometry_trial_snapshot_kernel, dim3(trial_blocks(s.size)), dim3(kTrialBlock), 0, st, s, state);
}
void launch_geometry_trial_solve(hipStream_t st, const SurfelsView& s, const ClassPartials& cpp, int classes, bool use_desc, float lambda, int trial,
                                 const GeometryTrialState& state) {
  if (s.size == 0) return;
  hipLaunchKernelGGL(geometry_trial_solve_kernel, dim3(trial_blocks(s.size)), dim3(kTrialBlock), 0, st, s, cpp, classes, use_desc ? 1 : 0, lambda, trial, state);
}
void launch_geometry_trial_decide(hipStream_t st, const SurfelsView& s, const SurfelCostPlanes& c0, const SurfelCostPlanes& c1, bool guard_pairs,
                                  int trial, const GeometryTrialState& state, uint32_t* partials, uint32_t* ctl) {
  if (s.size == 0) return;
  const unsigned blocks = trial_blocks(s.size);
  hipLaunchKernelGGL(geometry_trial_decide_kernel, dim3(blocks), dim3(kTrialBlock), 0, st, s, c0, c1, guard_pairs ? 1 : 0, trial, state, partials);
  hipLaunchKernelGGL(geometry_trial_count_kernel, dim3(1), dim3(kTrialBlock), 0, st, partials, blocks, trial, ctl);
}
void launch_geometry_trial_finish(hipStream_t st, uint32_t size, const GeometryTrialState& state, uint8_t* out) {
  if (size == 0 || out == nullptr) return;
  hipLaunchKernelGGL(geometry_trial_finish_kernel, dim3(trial_blocks(size)), dim3(kTrialBlock), 0, st, size, state, out);
}
void launch_geometry_trial_restore(hipStream_t st, const SurfelsView& s, const GeometryTrialState& state) {
  if (s.size == 0) return;
  hipLaunchKernelGGL(geometry_trial_restore_kernel, dim3(trial_blocks(s.size)), dim3(kTrialBlock), 0, st, s, state);
}

}  // namespace bahip
#endif
