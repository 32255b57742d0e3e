// pose_device.h -- what the sweeps and the solve kernels of the pose phase share between kernels_pose.hip (the plain Gauss-Newton phase)
// and kernels_pose_trial.hip (the phase under step control): the accumulation chain of the normal equations, the LDS sink of the
// persistent form, the 6x6 solve and the convergence test.  Every function here is inlined into its callers.
#pragma once

#include "ba_device.h"
#include "ba_launch.h"
#include "se3_device.h"

namespace bahip {
constexpr int kPoseBlock = 64;    // one wavefront per workgroup: no LDS, no barriers, and finished waves free their slot at once
// Where a sweep reports a tile total it could not represent (hb_split): the low word of the unused 28th coefficient of work item
// 0's row -- inside the buffer the ranks of a sharded run exchange, so that after the exchange EVERY rank's solve launch sees the
// flag and every host fails the call alike (a flag in the rank's own counter record let the other ranks run on).
__host__ __device__ inline int* pose_invalid_word(HbFixed* Hb) { return reinterpret_cast<int*>(Hb + 27 * kHbLimbs); }
}  // namespace bahip

BAHIP_FLAVOURED_BEGIN

// acc += w * [upper(J J^T) | r J], as fused multiply-add chains (the oracle's orc_accumulate_pose_coeffs spells the same chain:
// the per-lane sums, the wave tree and the fixed-point totals are part of the numerical definition, ba_device.h: HbFixed).
// (Two entries per instruction with v_pk_fma_f32 -- entries (r, c) (r, c + 1) for even c, 45 VALU instructions fewer per pair,
// bit-identical -- was measured in round 3: the pose sweep got 3 % SLOWER.  gfx950 issues a plain wave64 binary32 instruction
// in about half the cycles of a packed one, so packing buys nothing here and costs register-pair alignment.)
__device__ __forceinline__ void accumulate_jtj(float (&acc)[28], const float (&J)[6], float wgt, float raw) {
  int q = 0;
#pragma unroll
  for (int row = 0; row < 6; ++row) {
    const float wj = wgt * J[row];
#pragma unroll
    for (int col = row; col < 6; ++col, ++q) acc[q] = __builtin_fmaf(wj, J[col], acc[q]);
  }
  const float wr = wgt * raw;
#pragma unroll
  for (int c = 0; c < 6; ++c) acc[21 + c] = __builtin_fmaf(wr, J[c], acc[21 + c]);
}

// LdsSink: where the 27 tile totals of a (tile, work item) pair go in the persistent forms -- the workgroup's own table of limb pairs
// in LDS, one row per work item; ds_add_u64 costs no memory round trip and does not take part in vmcnt, so the totals are added at
// once.  The workgroup flushes the table to Hb when it runs out of tiles (pose_accumulate_lds_kernel): per launch 256 workgroups x K
// x 27 x 2 global atomics instead of 2 per total of every (tile, work item) pair -- 25 M memory-side atomics and 97 MB of write
// traffic per launch at the bench size (profiles/r2_e).
struct LdsSink {
  uint32_t lane_offset;   // LDS byte address of this lane's coefficient in row 0 of the table [num_items][kHbCoefficients][kHbLimbs]
  int* invalid;
  bool holds_total;       // this lane holds one of the 27 tile totals
  float pending;
  int pending_item;       // wave-uniform
  // The totals are added right behind the reduction (add() flushes at once; BAHIP_LDS_DEFERRED restores the GlobalSink shape,
  // where they wait in `pending` for the next candidate).  History: the round-3 builds gave wrong sums for rows > 0 in the immediate
  // shape and the oracle's bits in the deferred one.  The round-4 bisect (profiles/r4_lds_anomaly_bisect.txt) reproduced that on the
  // old commits, showed that the sink and the LDS atomics were innocent -- a shadow table kept by global atomics held the same wrong
  // values, add() was called once per (tile, item): the values REACHING the sink were already wrong, i.e. code generation upstream
  // of it -- and that every build from commit b4280f8 on is right in both shapes.  The instruction at fault was not pinned down;
  // tests/test_gpu_scale_parity.py runs the sweep at 1 / 2 / 16 wavefronts x 1 / 37 / 292 items x parts x rounds-ahead against the
  // oracle so that a toolchain or source change that brings it back cannot pass.
  __device__ __forceinline__ void flush() {
    if (pending_item >= 0 && holds_total) {
      // magnitudes added or subtracted according to the total's sign (ba_device.h: hb_split_magnitudes): the same sums as the
      // signed limbs of hb_split, without its four exponent ranges and without the 64-bit negations
      const HbMagnitudes m = hb_split_magnitudes(pending);
      const uint32_t address = lane_offset + (uint32_t)pending_item * (uint32_t)(kHbStride * sizeof(HbFixed));
      auto* cell = reinterpret_cast<__attribute__((address_space(3))) HbFixed*>(address);
      const HbFixed lo = (HbFixed)(unsigned long long)m.lo, hi = (HbFixed)(((unsigned long long)m.hi_hi << 32) | m.hi_lo);
      if (m.valid) {
        if (m.negative) {
          if (lo) __hip_atomic_fetch_sub(cell, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (hi) __hip_atomic_fetch_sub(cell + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          if (lo) __hip_atomic_fetch_add(cell, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (hi) __hip_atomic_fetch_add(cell + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      } else {
        atomicOr(invalid, 1);
      }
    }
    pending_item = -1;
  }
  __device__ __forceinline__ void gathers_done() { flush(); }
  __device__ __forceinline__ void add(int item, int /*w*/, float total) {
    pending = total; pending_item = item;
#ifndef BAHIP_LDS_DEFERRED
    flush();
#endif
  }
  __device__ __forceinline__ void finish() { flush(); }
};

BAHIP_FLAVOURED_END

namespace bahip {

// B/convergence_analysis.h:43-51
__device__ __forceinline__ bool is_scale1_pose_converged(const float* x) {
  float sq = 0.f;
  for (int c = 0; c < 3; ++c) sq += x[c] * x[c];
  for (int c = 3; c < 6; ++c) { const float v = x[c] * 10.f; sq += v * v; }
  return sq < 1e-06f;
}

// LDLT with symmetric diagonal pivoting + pseudo-inverse rule on D, binary64 (what Eigen's
// H.cast<double>().selfadjointView<Upper>().ldlt().solve(b) does, B/direct_ba_alternating.cc:206).
// Every index below is a compile-time constant once the loops are unrolled -- the pivot search and the row / column / perm
// exchanges are selects over the candidates, not dynamically indexed accesses -- so the 36 + 6 + 6 binary64 values live in
// registers: with dynamic indices they lived in scratch memory and one step of 200 keyframes took 24 us, most of it the
// latency of dependent scratch accesses (round 4 trace, profiles/r4_emu8_timeline.txt).  Same operations on the same values in
// the same order as the loop form (which the oracle restates, oracle_pose.c), only where the values are kept differs.
template <int N>
__device__ __forceinline__ void ldlt_solve(double (&A)[N * N], const double (&b)[N], double (&x)[N]) {
  constexpr double kTiny = 2.2250738585072014e-308;
  int perm[N];
#pragma unroll
  for (int c = 0; c < N; ++c) perm[c] = c;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int piv = k;
    double best = fabs(A[k * N + k]);
#pragma unroll
    for (int c = k + 1; c < N; ++c) {
      const double v = fabs(A[c * N + c]);
      const bool better = v > best;
      best = better ? v : best;
      piv = better ? c : piv;
    }
#pragma unroll
    for (int c = k + 1; c < N; ++c) {
      const bool exchange = piv == c;   // true for at most one c: rows, then columns, then perm, as the loop form
#pragma unroll
      for (int j = 0; j < N; ++j) { const double t = A[k * N + j], u = A[c * N + j]; A[k * N + j] = exchange ? u : t; A[c * N + j] = exchange ? t : u; }
#pragma unroll
      for (int j = 0; j < N; ++j) { const double t = A[j * N + k], u = A[j * N + c]; A[j * N + k] = exchange ? u : t; A[j * N + c] = exchange ? t : u; }
      const int tp = perm[k], up = perm[c];
      perm[k] = exchange ? up : tp;
      perm[c] = exchange ? tp : up;
    }
    const double d = A[k * N + k];
    if (fabs(d) > kTiny) {
#pragma unroll
      for (int c = k + 1; c < N; ++c) A[c * N + k] /= d;
#pragma unroll
      for (int c = k + 1; c < N; ++c)
#pragma unroll
        for (int j = k + 1; j <= c; ++j) {
          A[c * N + j] -= A[c * N + k] * d * A[j * N + k];
          A[j * N + c] = A[c * N + j];
        }
    } else {
#pragma unroll
      for (int c = k + 1; c < N; ++c) A[c * N + k] = 0;
    }
  }
  double y[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    y[c] = b[0];
#pragma unroll
    for (int j = 1; j < N; ++j) y[c] = perm[c] == j ? b[j] : y[c];
  }
#pragma unroll
  for (int c = 0; c < N; ++c)
#pragma unroll
    for (int j = 0; j < c; ++j) y[c] -= A[c * N + j] * y[j];
#pragma unroll
  for (int c = 0; c < N; ++c) { const double d = A[c * N + c]; y[c] = (fabs(d) > kTiny) ? y[c] / d : 0.0; }
#pragma unroll
  for (int c = N - 1; c >= 0; --c)
#pragma unroll
    for (int j = c + 1; j < N; ++j) y[c] -= A[j * N + c] * y[j];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    x[j] = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) x[j] = perm[c] == j ? y[c] : x[j];
  }
}

// pose_gn_step of kernels_pose.hip under a Marquardt damping factor: diagonal entry i of the binary64 system is
// (double)H_ii + (double)lambda * (double)H_ii (the product of two binary32 values is exact in binary64), everything else -- the
// solve, x rounded to binary32, T_next = T * exp(-x) -- is that function's.  lambda = 0 gives its bits: H_ii + 0 * H_ii is H_ii.
__device__ __forceinline__ void pose_gn_step_damped(const float* hb, const float* T, float lambda, float* xf, float* T_next) {
  double A[36], b[6], x[6];
  int q = 0;
#pragma unroll
  for (int row = 0; row < 6; ++row)
#pragma unroll
    for (int col = row; col < 6; ++col) { const double v = (double)hb[q]; A[row * 6 + col] = v; A[col * 6 + row] = v; ++q; }
#pragma unroll
  for (int c = 0; c < 6; ++c) A[c * 6 + c] = A[c * 6 + c] + (double)lambda * A[c * 6 + c];
#pragma unroll
  for (int c = 0; c < 6; ++c) b[c] = (double)hb[21 + c];
  ldlt_solve<6>(A, b, x);
  float mx[6];
  for (int c = 0; c < 6; ++c) { xf[c] = (float)x[c]; mx[c] = -1.f * xf[c]; }
  float upd[7];
  se3_exp(mx, upd);
  se3_mul(T, upd, T_next);
}

}  // namespace bahip
