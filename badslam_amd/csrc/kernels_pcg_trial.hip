// kernels_pcg_trial.hip -- step control for the PCG scheme: the damped per-unknown kernels, and the snapshot / restore pair that
// lets an outer iteration be undone (bahip_pcg_iteration_controlled, capi_pcg_trial.hip).  The reference has no such mode.
//
// DEFINITION of the damped system.  A damping factor lambda >= 0 (binary32, per context, default 0), scaled by
// the diagonal M the scheme assembles (Marquardt).  For unknown u, with e = kDiagEpsilon + prior_at(L, u) as in kernels_pcg.hip and
//     t = lambda * M[u]                                     (ONE binary32 product),
//   - the preconditioner's denominators are ((M[u] + kDiagEpsilon) + prior_at(L, u)) + t   (PCGInit2, PCGStep2),
//   - the diagonal term the matrix-free product adds is (e + t)                             (the epsilon terms of alpha_d in PCGInit2,
//     PCGStep3 and the stand-alone kernel; g + (e + t) * p in PCGStep2).
// The pair sweeps (PCGInit, PCGStep1) are the undamped ones.  Rows with M = 0 (the gauge, fixed poses, inactive surfels under a
// window) have t = 0: they stay untouched.  The fused iteration, the windowed one and the stage entry points launch these same
// kernels, so the three are one system.
// lambda = 0 and M finite: t = +0 (M >= 0: a sum of squares), and x + (+0) = x bit for bit for the x met here (denominators and e are
// >= 1e-8 > 0), so every expression has the bits of the undamped kernels.  Contraction: the per-unknown kernels exist once, built
// with -ffp-contract=off, and BOTH arithmetic flavours launch them (the flavours differ in the sweeps only) -- there is no fast
// build of e + t.  Were one made, fma(lambda, M, d) at lambda = 0 is still d, but at lambda > 0 it would skip the rounding of t
// that the definition asks for; the pragma below keeps that from happening by a change of flags.  With lambda == 0 the launchers
// run the undamped kernels of kernels_pcg.hip themselves (their code is pinned by tests/test_cpu_pcg_window_kernel_resources.py,
// which is why the damped ones are kernels of their own here and not a parameter there).
//
// SNAPSHOT / RESTORE.  What an outer iteration may write: surfel rows x, y, z (pcg_update_surfels_kernel), the packed normal row
// (normals_kernel, run inside the trial), the two descriptor rows with descriptor residuals; the keyframe table (poses); the cfactor
// plane.  (Intrinsics and `a` are host values of the context: capi_pcg_trial.hip keeps them.)  Layout of the snapshot, in words:
//   [ tile b: rows_saved x 64 words ] x num_tiles | keyframe table words | cfactor plane, dense
// One wavefront per 64-surfel tile -- tile b of the window's tile list, or tile b itself for the whole map --, lane l on word l of each
// row: 256 contiguous bytes per row and wavefront, vector loads and stores only, all loads of a tile in flight before its first store.
// Further wavefronts copy the two flat blocks, 64 words each.  Restore is the same kernel with source and destination swapped: the
// words come back, so a rejected step leaves every bit as it was (subtracting the update would not).  Bandwidth kernels: 6 rows x
// 3 M surfels = 72 MB each way; no time is promised (DESIGN.md section 3 says what was measured).  Budget: no scratch, <= 32 VGPRs
// (8 wavefronts per SIMD: the occupancy a copy wants to cover HBM latency).
#include "ba_device.h"
#include "ba_launch.h"
#include "exact_sum.h"
#include "pcg_device.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

// ---- the damped per-unknown kernels (kernels_pcg.hip: pcg_init2_kernel, pcg_step2_kernel, pcg_step3_kernel, pcg_eps_terms_kernel) ----
__global__ void __launch_bounds__(kPcgBlock)
pcg_damped_init2_kernel(PcgLayout L, PcgExact ex, float lambda, float a, const float* __restrict__ r_, const float* __restrict__ M_,
                        float* __restrict__ delta, float* __restrict__ g_, float* __restrict__ p_) {
  __shared__ BlockExact<2> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    g_[u] = 0;
    const float r_value = r_[u] + ((u == L.a_index) ? (-kAPriorWeight * kAPriorWeight * a) : 0);
    const float m = M_[u];
    const float t = lambda * m;
    const float p_value = r_value / (((m + kDiagEpsilon) + prior_at(L, u)) + t);
    p_[u] = p_value;
    delta[u] = 0;
    const float dot_term = r_value * p_value;
    const float eps_term = ((kDiagEpsilon + prior_at(L, u)) + t) * p_value * p_value;
    if (is_local(L, u)) {
      block_exact_add(acc, 0, dot_term, ex.invalid);
      block_exact_add(acc, 1, eps_term, ex.invalid);
    } else {
      exact_atomic_add(hot_cell(ex, kHotDotHead, replica), dot_term, ex.invalid);
      exact_atomic_add(hot_cell(ex, kHotEpsHead, replica), eps_term, ex.invalid);
    }
  }
  const int slots[2] = {kHotDotLocal, kHotEpsLocal};
  block_exact_flush(acc, ex, slots);
}

__global__ void __launch_bounds__(kPcgBlock)
pcg_damped_step2_kernel(PcgLayout L, PcgExact ex, float lambda, float* __restrict__ r_, const float* __restrict__ M_, float* __restrict__ delta,
                        float* __restrict__ g_, const float* __restrict__ p_, const float* alpha_n, const float* alpha_d, const PcgControl* ctl) {
  if (ctl->stop) return;
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  const float ad = *alpha_d;
  const float alpha = (ad >= 1e-35f) ? (*alpha_n / ad) : 0;
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    const float p_value = p_[u];
    delta[u] += alpha * p_value;
    const float m = M_[u];
    const float t = lambda * m;
    float r_value = r_[u];
    r_value -= alpha * (g_[u] + ((kDiagEpsilon + prior_at(L, u)) + t) * p_value);
    r_[u] = r_value;
    const float z_value = r_value / (((m + kDiagEpsilon) + prior_at(L, u)) + t);
    g_[u] = z_value;
    const float term = z_value * r_value;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotDotHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotDotLocal};
  block_exact_flush(acc, ex, slots);
}

__global__ void __launch_bounds__(kPcgBlock)
pcg_damped_step3_kernel(PcgLayout L, PcgExact ex, float lambda, const float* __restrict__ M_, const float* __restrict__ g_, float* __restrict__ p_,
                        const float* alpha_n, const float* beta_n, const PcgControl* ctl) {
  if (ctl->stop) return;
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  const float an = *alpha_n;
  const float beta = (an >= 1e-35f) ? (*beta_n / an) : 0;
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    const float pv = g_[u] + beta * p_[u];
    p_[u] = pv;
    const float t = lambda * M_[u];
    const float term = ((kDiagEpsilon + prior_at(L, u)) + t) * pv * pv;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotEpsHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotEpsLocal};
  block_exact_flush(acc, ex, slots);
}

__global__ void __launch_bounds__(kPcgBlock)
pcg_damped_eps_terms_kernel(PcgLayout L, PcgExact ex, float lambda, const float* __restrict__ M_, const float* __restrict__ p_) {
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    const float pv = p_[u];
    const float t = lambda * M_[u];
    const float term = ((kDiagEpsilon + prior_at(L, u)) + t) * pv * pv;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotEpsHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotEpsLocal};
  block_exact_flush(acc, ex, slots);
}

// ---- snapshot / restore ---------------------------------------------------------------------------------------------------------
constexpr int kTrialBlock = 64;
template <bool kRestore>
__device__ __forceinline__ void trial_move(uint32_t* live, uint32_t* saved) {
  if (kRestore) *live = *saved;
  else *saved = *live;
}
template <bool kRestore>
__global__ void __launch_bounds__(kTrialBlock) pcg_trial_copy_kernel(SurfelsView s, PcgTrialShape t, uint32_t* __restrict__ snap) {
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x < t.num_tiles) {
    const uint32_t tile = t.tile_list ? t.tile_list[blockIdx.x] : blockIdx.x;
    const uint32_t i = tile * 64u + lane;
    if (tile >= (s.size + 63u) / 64u || i >= s.size) return;   // (a tile past the cloud: nothing of it exists)
    uint32_t* slot = snap + (size_t)blockIdx.x * t.rows_saved * 64u + lane;
    uint32_t v[kPcgTrialMaxRows];
    int j = 0;
#pragma unroll
    for (int r = 0; r < kPcgTrialMaxRows; ++r) {   // every load of the tile, then every store
      if (!((t.rows_mask >> r) & 1u)) continue;
      v[r] = kRestore ? slot[(size_t)j * 64u] : reinterpret_cast<const uint32_t*>(s.row(r))[i];
      ++j;
    }
    j = 0;
#pragma unroll
    for (int r = 0; r < kPcgTrialMaxRows; ++r) {
      if (!((t.rows_mask >> r) & 1u)) continue;
      if (kRestore) reinterpret_cast<uint32_t*>(s.row(r))[i] = v[r];
      else slot[(size_t)j * 64u] = v[r];
      ++j;
    }
    return;
  }
  // the flat blocks behind the tiles: the keyframe table, then the cfactor plane (pitched where it lives, dense in the snapshot)
  const uint32_t f = (blockIdx.x - t.num_tiles) * 64u + lane;
  uint32_t* flat = snap + (size_t)t.num_tiles * t.rows_saved * 64u;
  if (f < t.kf_words) {
    trial_move<kRestore>(t.kf_table + f, flat + f);
  } else if (f - t.kf_words < t.cf_width * t.cf_height) {
    const uint32_t c = f - t.kf_words, y = c / t.cf_width, x = c - y * t.cf_width;
    trial_move<kRestore>(reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(t.cfactor) + (size_t)y * t.cf_pitch_bytes) + x, flat + f);
  }
}

size_t pcg_trial_snapshot_words(const PcgTrialShape& t) {
  return (size_t)t.num_tiles * t.rows_saved * 64u + t.kf_words + (size_t)t.cf_width * t.cf_height;
}
static unsigned trial_grid(const PcgTrialShape& t) {
  const size_t flat = (size_t)t.kf_words + (size_t)t.cf_width * t.cf_height;
  return (unsigned)(t.num_tiles + (flat + 63) / 64);
}
void launch_pcg_trial_snapshot(hipStream_t st, const SurfelsView& s, const PcgTrialShape& t, uint32_t* snap) {
  if (trial_grid(t)) hipLaunchKernelGGL(pcg_trial_copy_kernel<false>, dim3(trial_grid(t)), dim3(kTrialBlock), 0, st, s, t, snap);
}
void launch_pcg_trial_restore(hipStream_t st, const SurfelsView& s, const PcgTrialShape& t, uint32_t* snap) {
  if (trial_grid(t)) hipLaunchKernelGGL(pcg_trial_copy_kernel<true>, dim3(trial_grid(t)), dim3(kTrialBlock), 0, st, s, t, snap);
}

// ---- launchers of the per-unknown kernels under a damping factor (shapes of kernels_pcg.hip: a grid-stride loop over at most
// kPcgReduceBlocks workgroups) ----
static inline unsigned damped_grid(uint32_t n) {
  const unsigned blocks = (n + kPcgBlock - 1) / kPcgBlock;
  return blocks < kPcgReduceBlocks ? blocks : kPcgReduceBlocks;
}
void launch_pcg_damped_init2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, float a, const float* r, const float* M,
                             float* delta, float* g, float* p) {
  if (lambda == 0.f) return launch_pcg_init2(st, L, ex, a, r, M, delta, g, p);   // off: the undamped kernel itself
  if (L.unknown_count) hipLaunchKernelGGL(pcg_damped_init2_kernel, dim3(damped_grid(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, lambda, a, r, M, delta, g, p);
}
void launch_pcg_damped_eps_terms(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, const float* M, const float* p) {
  if (lambda == 0.f) return launch_pcg_eps_terms(st, L, ex, p);   // off: the undamped kernel itself
  if (L.unknown_count) hipLaunchKernelGGL(pcg_damped_eps_terms_kernel, dim3(damped_grid(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, lambda, M, p);
}
void launch_pcg_damped_step2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, float* r, const float* M, float* delta, float* g,
                             const float* p, const float* alpha_n, const float* alpha_d, const void* ctl) {
  if (lambda == 0.f) return launch_pcg_step2(st, L, ex, r, M, delta, g, p, alpha_n, alpha_d, ctl);   // off: the undamped kernel itself
  if (L.unknown_count) hipLaunchKernelGGL(pcg_damped_step2_kernel, dim3(damped_grid(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, lambda, r, M, delta, g, p,
                                          alpha_n, alpha_d, static_cast<const PcgControl*>(ctl));
}
void launch_pcg_damped_step3(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, const float* M, const float* g, float* p,
                             const float* alpha_n, const float* beta_n, const void* ctl) {
  if (lambda == 0.f) return launch_pcg_step3(st, L, ex, g, p, alpha_n, beta_n, ctl);   // off: the undamped kernel itself
  if (L.unknown_count) hipLaunchKernelGGL(pcg_damped_step3_kernel, dim3(damped_grid(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, lambda, M, g, p,
                                          alpha_n, beta_n, static_cast<const PcgControl*>(ctl));
}

}  // namespace bahip
#endif
