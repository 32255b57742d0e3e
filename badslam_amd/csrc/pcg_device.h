// pcg_device.h -- device code the PCG sweeps share: the whole-map sweeps of kernels_pcg.hip and the windowed ones of
// kernels_pcg_window.hip (the terms of one associated pair, its gathers and association, the exact accumulators' hot cells).
#pragma once
#include "ba_device.h"
#include "ba_launch.h"
#include "exact_sum.h"
#include "wave_cull.h"

namespace bahip {

constexpr int kPcgSweepBlock = 64; // surfel sweeps (init, step 1): one wavefront per workgroup, like kernels_surfel.hip
#define BAHIP_PCG_SWEEP_ATTR __attribute__((amdgpu_waves_per_eu(4)))   // 128-VGPR cap: 4 waves per SIMD
__device__ __forceinline__ uint32_t head_index(const PcgLayout& L, uint32_t u) { return u < L.head_lo ? u : L.head_lo + (u - L.head_hi); }
// Slot `slot`, replica `replica` of the replicated accumulators (kernels_pcg.hip: "the exact accumulators of one PCG solve").
__device__ __forceinline__ ExactCell* hot_cell(const PcgExact& ex, int slot, int replica) {
  return (slot < kHotExchanged1 ? ex.hot : ex.hot_tail - (size_t)kHotExchanged1 * kHotReplicas) + (size_t)slot * kHotReplicas + replica;
}

// The device-side inner-loop control block (kernels_pcg.hip: "inner-loop control on the device").
struct PcgControl {
  double prev_r_norm;
  int no_improvement;
  int stop;
  int steps;
  int pad;
};
static_assert(sizeof(PcgControl) == 24, "PcgControl lives behind the scalars of the PCG buffer");

// ---- what the per-unknown kernels share (kernels_pcg.hip and the damped ones of kernels_pcg_trial.hip) ----
constexpr int kPcgBlock = 256;     // per-unknown vector kernels
// The per-unknown kernels run a grid-stride loop over at most kPcgReduceBlocks workgroups: each ends in 9 atomics per sum.
constexpr unsigned kPcgReduceBlocks = 1024;
constexpr float kDiagEpsilon = 1e-8f;   // B/kernel_pcg.cu:44
constexpr float kAPriorWeight = 10.f;   // B/kernel_pcg.cu:48
__device__ __forceinline__ float prior_at(const PcgLayout& L, uint32_t u) {
  return (u == L.a_index) ? (kAPriorWeight * kAPriorWeight) : 0.f;
}
__device__ __forceinline__ bool is_local(const PcgLayout& L, uint32_t u) { return u >= L.head_lo && u < L.head_hi; }

// ---- exact dot products in the per-unknown kernels -----------------------------------------------------------------------------
// A thread's terms over the local (surfel) unknowns go into a private column of limbs in workgroup memory (the limb index is
// data dependent); terms of dense-head unknowns -- few -- go straight to the head's replicated slot with atomics.  At the end
// the workgroup folds its columns and adds 9 limbs per sum to one of the 64 replicas.
template <int kSets>
struct BlockExact {
  long long limbs[kSets][kExactLimbs][kPcgBlock];
};
template <int kSets>
__device__ __forceinline__ void block_exact_clear(BlockExact<kSets>& b) {
#pragma unroll
  for (int set = 0; set < kSets; ++set)
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) b.limbs[set][j][threadIdx.x] = 0;
}
template <int kSets>
__device__ __forceinline__ void block_exact_add(BlockExact<kSets>& b, int set, float v, unsigned* invalid) {
  exact_lds_add(&b.limbs[set][0][0], kPcgBlock, (int)threadIdx.x, v, invalid);
}
template <int kSets>
__device__ __forceinline__ void block_exact_flush(BlockExact<kSets>& b, const PcgExact& ex, const int (&slots)[kSets]) {
  __syncthreads();
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  const int part = threadIdx.x & 15;
  for (int row = threadIdx.x >> 4; row < kSets * kExactLimbs; row += kPcgBlock >> 4) {   // 16 threads fold one row of 256 columns
    const long long* line = &b.limbs[0][0][0] + (size_t)row * kPcgBlock;
    long long sum = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) sum += line[c * 16 + part];
    for (int off = 8; off; off >>= 1) sum += __shfl_xor(sum, off);
    if (part == 0 && sum != 0) limb_atomic_add(&hot_cell(ex, slots[row / kExactLimbs], replica)->limb[row % kExactLimbs], sum);
  }
}

}  // namespace bahip

BAHIP_FLAVOURED_BEGIN
// Terms of one associated pair (B/kernel_pcg.cu:213-303,334-395 and :663-748,786-905).
struct PairTerms {
  float raw, w, Jgeom;
  float Jpose[6];
  bool di_valid;
  float Jdi[5], Jcf;
  uint32_t cf_index;
  bool color_ok;
  float raw1, raw2, w1, w2, Jg1, Jg2;
  float Jp1[6], Jp2[6];
  float Jci1[4], Jci2[4];
};

template <bool kDepthIntr, bool kColorIntr>
__device__ __forceinline__ void eval_pair_terms(const PcgLayout& L, const Intrinsics& in, const KfEntry& kf, const Assoc& r,
                                                const PixelWords& pix, const DescWords& dw, Vec3 gn, float d1, float d2, PairTerms* t) {
  const float* F = kf.pose.F;
  const Vec3 rn = r.nl;
  const float nx = r.nx, ny = r.ny;   // the association computed them (ba_device.h: Assoc)
  t->di_valid = false;
  t->color_ok = false;
  // All Jacobians come from the jac_* functions of ba_device.h -- the ones the alternating sweeps use and the ones checked
  // against the golden vectors derived from the reference's own script (tests/golden/jacobians.json).
  if (L.use_depth) {
    const float inv_std = assoc_inv_std(in, r);
    const Vec3 u = assoc_unproject(r);
    t->raw = inv_std * dot3(rn, u - r.local);
    t->w = depth_residual_weight(t->raw);
    t->Jgeom = -inv_std;
    jac_depth_pose(rn, u, inv_std, t->Jpose);
    if (kDepthIntr) {
      // cfactor of the pixel's cell and the raw depth: the words the association already loaded (the geometry plane's low
      // half is the keyframe's depth image)
      const int sparse_px = r.px / in.cell, sparse_py = r.py / in.cell;
      const float cfactor = pix.cfactor;
      const float raw_inv_depth = 1.0f / (in.raw_to_float_depth * (uint16_t)(pix.geom & 0xffffu));
      const float exp_inv_depth = exp_det(-in.a * raw_inv_depth);
      const float corrected = cfactor * exp_inv_depth + raw_inv_depth;
      t->di_valid = !(fabsf(corrected) < 1e-4f);
      const float dot = dot3(mk3(nx, ny, 1), rn);
      float Jdi[6];   // fx_inv, fy_inv, cx_inv, cy_inv, a, cfactor (B/kernel_opt_intrinsics.cu:107-140 = B/kernel_pcg.cu:258-303)
      jac_depth_intrinsics(r.px, r.py, r.depth, inv_std, dot3(gn, mk3(F[0], F[1], F[2])), dot3(gn, mk3(F[4], F[5], F[6])), dot, cfactor,
                           raw_inv_depth, exp_inv_depth, corrected, Jdi);
#pragma unroll
      for (int c = 0; c < 5; ++c) t->Jdi[c] = Jdi[c];
      t->Jcf = Jdi[5];
      t->cf_index = L.depth_intr_start + 5 + sparse_px + sparse_py * in.cf_width;
    }
  }
  if (L.use_desc) {
    t->color_ok = dw.color_ok;
    if (t->color_ok) {
      DescEval e;
      eval_descriptor_from_words(in, kf.lumafp, dw, d1, d2, &e);
      t->raw1 = e.r1; t->raw2 = e.r2;
      t->w1 = descriptor_residual_weight(e.r1);
      t->w2 = descriptor_residual_weight(e.r2);
      t->Jg1 = jac_descriptor_surfel(rn, r.local, r.inv_z, e.gx1, e.gy1, in.cfx, in.cfy);
      t->Jg2 = jac_descriptor_surfel(rn, r.local, r.inv_z, e.gx2, e.gy2, in.cfx, in.cfy);
      jac_descriptor_pose(r.local, r.inv_z, e.gx1 * in.cfx, e.gy1 * in.cfy, t->Jp1);
      jac_descriptor_pose(r.local, r.inv_z, e.gx2 * in.cfx, e.gy2 * in.cfy, t->Jp2);
      if (kColorIntr) {
        jac_descriptor_color_intrinsics(e.gx1, e.gy1, nx, ny, t->Jci1);
        jac_descriptor_color_intrinsics(e.gx2, e.gy2, nx, ny, t->Jci2);
      }
    }
  }
}

// The gathers of one (surfel, keyframe) pair, all in flight before the first is waited for (ba_device.h: project_surfel), and
// the association on the loaded words.
struct PairGather {
  PixelWords pix;
  DescWords dw;
  Assoc a;
};
__device__ __forceinline__ bool gather_and_associate(const PcgLayout& L, const Intrinsics& in, const KfEntry& kf, Vec3 gp, Vec3 gn,
                                                     const TangentPoints& tp, bool in_range, PairGather* g) {
  const float* F = kf.pose.F;
  const Projected p = project_surfel(in, F, gp);
  g->pix = load_pixel_words(in, kf.geom, p);
  if (L.use_desc) g->dw = load_descriptor_words(in, kf.lumafp, F, tp, p);
  const bool visible = in_range && associate_from_words<false>(in, F, gn, p, g->pix, &g->a, nullptr);
  if (L.use_desc) gathers_arrived(g->pix, g->dw);
  else gathers_arrived(g->pix);
  return visible;
}

BAHIP_FLAVOURED_END
