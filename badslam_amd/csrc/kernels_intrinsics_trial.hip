// kernels_intrinsics_trial.hip -- step control for the intrinsics step of the alternating scheme: the damped Schur complement over the
// sparse cells, the back-substitution from a saved cfactor plane into the live one, and the copy that saves / restores that plane
// (bahip_optimize_intrinsics_controlled, capi_intrinsics_trial.hip).  The reference has no such mode.
//
// The sweep of a controlled step is the plain step's (kernels_intrinsics.hip, which stays as it is); its binary64 sums stay in the
// context's scratch, and every trial forms its system from them again.  This unit holds the per-cell arithmetic only: one thread per
// sparse cell, no keyframe is visited, no atomic, no LDS.
//
// DEFINITION of the damped Schur complement.  Per cell the eight binary64 sums are rounded to binary32 (as intrinsics_schur_kernel
// rounds them) and D' = D + lambda * D is formed as ONE binary32 product and then ONE add.  Everything intrinsics_schur_kernel does
// with D is done with D': the test 1 / D' < 1e12, D'^-1 b2, D'^-1 B, the 20 terms -(B_r D'^-1) B_c and -(B_c (D'^-1 b2)), their xor
// butterfly over the 64 cells of a wavefront (wave_sum) and one partial per wavefront in that kernel's layout, which
// intrinsics_finish_kernel (reused) adds in wavefront order to the rounded global sums.  lambda = 0 and finite sums: lambda * D = +-0 and
// D + (+-0) = D, so every word has the bits of the plain step.  The unit exists once, built with -ffp-contract=off, and both arithmetic
// flavours of the sweep launch it; the pragma below keeps a change of flags from fusing the product into the add.
#include "ba_device.h"
#include "ba_launch.h"
#include "wave_reduce.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

// kernels_intrinsics.hip (exact unit): glob_f[q] = (float)glob_d[q] [+ the chain over the wavefronts' partials for q < 20]
__global__ void intrinsics_finish_kernel(int num_waves, const float* __restrict__ partials, const double* __restrict__ glob_d,
                                         float* __restrict__ glob_f);

namespace {
constexpr int kTrialBlock = kIntrinsicsTrialBlock;   // four wavefronts: the partial layout of intrinsics_schur_kernel
constexpr int kFinishThreads = 256;                  // the workgroup intrinsics_finish_kernel is written for
constexpr int kRows = 5;                             // fx_inv, fy_inv, cx_inv, cy_inv, a
constexpr int kRecord = 8;                           // B0..B4, D, b2, observation count
template <typename T>
__device__ __forceinline__ const T* pitched_src(const T* base, uint32_t pitch, int y, int x) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)y * pitch + (size_t)x * sizeof(T));
}
}  // namespace

// One thread per sparse cell.  cells[cell] = {D'^-1 B0..B4, D'^-1 b2 (NaN: the cell is left out), b2, observation count}; lanes past S
// contribute zeros to their wavefront's partial and write no cell.
__global__ void __launch_bounds__(kTrialBlock)
intrinsics_schur_damped_kernel(int S, float lambda, float* __restrict__ partials /* [wavefronts][20] */, const double* __restrict__ cells_d,
                               float* __restrict__ cells) {
  const int cell = blockIdx.x * kTrialBlock + threadIdx.x;
  float part[20];
#pragma unroll
  for (int q = 0; q < 20; ++q) part[q] = 0.f;
  if (cell < S) {
    const double2* in = reinterpret_cast<const double2*>(cells_d + (size_t)cell * kRecord);
    const double2 r0 = in[0], r1 = in[1], r2 = in[2], r3 = in[3];
    float Bc[kRows] = {(float)r0.x, (float)r0.y, (float)r1.x, (float)r1.y, (float)r2.x};
    const float D = (float)r2.y, b2 = (float)r3.x, obs = (float)r3.y;
    const float scaled = lambda * D;
    const float damped = D + scaled;
    const float D_inverse = 1.0f / damped;
    float D_inv_b2 = __builtin_nanf("");
    if (D_inverse < 1e12f) {
      D_inv_b2 = D_inverse * b2;
      int q = 0;
#pragma unroll
      for (int row = 0; row < kRows; ++row)
#pragma unroll
        for (int col = row; col < kRows; ++col) part[q++] = -1.f * (Bc[row] * D_inverse * Bc[col]);
#pragma unroll
      for (int c = 0; c < kRows; ++c) part[15 + c] = -1.f * (Bc[c] * D_inv_b2);
#pragma unroll
      for (int c = 0; c < kRows; ++c) Bc[c] = D_inverse * Bc[c];
    }
    float4* out = reinterpret_cast<float4*>(cells + (size_t)cell * kRecord);
    out[0] = make_float4(Bc[0], Bc[1], Bc[2], Bc[3]);
    out[1] = make_float4(Bc[4], D_inv_b2, b2, obs);
  }
  const int lane = threadIdx.x & 63;
  float mine = 0.f;
#pragma unroll
  for (int q = 0; q < 20; ++q) {
    const float v = wave_sum(part[q]);
    if (lane == q) mine = v;
  }
  const int wave = (blockIdx.x * kTrialBlock + threadIdx.x) >> 6;
  if (lane < 20) partials[(size_t)wave * 20 + lane] = mine;
}

// Back-substitution (intrinsics_solve_cells_kernel with a source plane): dst = src - (D'^-1 b2 - sum_c D'^-1 B_c x_c), zero where the
// cell has no observation.  Both planes pitched; the padding of dst is not written.
__global__ void __launch_bounds__(kTrialBlock)
intrinsics_backsub_kernel(int cf_width, int S, const float* __restrict__ cells, const float* __restrict__ x1 /* 5 */,
                          const float* __restrict__ src, uint32_t src_pitch, float* __restrict__ dst, uint32_t dst_pitch) {
  const int cell = blockIdx.x * kTrialBlock + threadIdx.x;
  if (cell >= S) return;
  const float4* rec = reinterpret_cast<const float4*>(cells + (size_t)cell * kRecord);
  const float4 lo = rec[0], hi = rec[1];
  const float Bc[kRows] = {lo.x, lo.y, lo.z, lo.w, hi.x};
  float offset = hi.y;
  if (offset != offset) {
    offset = 0;
  } else {
#pragma unroll
    for (int c = 0; c < kRows; ++c) offset -= Bc[c] * x1[c];
  }
  const int y = cell / cf_width, x = cell - y * cf_width;
  float value = *pitched_src(src, src_pitch, y, x) - offset;
  if (hi.w == 0.f) value = 0;
  *pitched_ptr(dst, dst_pitch, y, x) = value;
}

// dst(y, x) = src(y, x) for the width x height words of a plane, word for word; the padding of either plane is neither read nor written.
__global__ void __launch_bounds__(kTrialBlock)
intrinsics_plane_copy_kernel(int width, int S, const uint32_t* __restrict__ src, uint32_t src_pitch, uint32_t* __restrict__ dst,
                             uint32_t dst_pitch) {
  const int cell = blockIdx.x * kTrialBlock + threadIdx.x;
  if (cell >= S) return;
  const int y = cell / width, x = cell - y * width;
  *pitched_ptr(dst, dst_pitch, y, x) = *pitched_src(src, src_pitch, y, x);
}

void launch_intrinsics_trial_schur(hipStream_t st, bool schur, int S, float lambda, const double* glob_d, const double* cells_d, float* glob_f,
                                   float* cells_f, float* partials) {
  int waves = 0;
  if (schur) {
    const int blocks = (S + kTrialBlock - 1) / kTrialBlock;
    hipLaunchKernelGGL(intrinsics_schur_damped_kernel, dim3(blocks), dim3(kTrialBlock), 0, st, S, lambda, partials, cells_d, cells_f);
    waves = blocks * (kTrialBlock / 64);
  }
  hipLaunchKernelGGL(intrinsics_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, waves, (const float*)partials, glob_d, glob_f);
}
void launch_intrinsics_trial_backsub(hipStream_t st, int cf_width, int S, const float* cells_f, const float* x1, const float* src,
                                     uint32_t src_pitch, float* dst, uint32_t dst_pitch) {
  hipLaunchKernelGGL(intrinsics_backsub_kernel, dim3((S + kTrialBlock - 1) / kTrialBlock), dim3(kTrialBlock), 0, st, cf_width, S, cells_f, x1, src,
                     src_pitch, dst, dst_pitch);
}
void launch_intrinsics_trial_plane_copy(hipStream_t st, int width, int height, const float* src, uint32_t src_pitch, float* dst, uint32_t dst_pitch) {
  const int S = width * height;
  hipLaunchKernelGGL(intrinsics_plane_copy_kernel, dim3((S + kTrialBlock - 1) / kTrialBlock), dim3(kTrialBlock), 0, st, width, S,
                     reinterpret_cast<const uint32_t*>(src), src_pitch, reinterpret_cast<uint32_t*>(dst), dst_pitch);
}

}  // namespace bahip
#endif
