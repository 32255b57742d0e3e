// pcg_device.h -- device code the PCG sweeps share: the whole-map sweeps of kernels_pcg.hip and the windowed ones of
// kernels_pcg_window.hip.  The terms of one associated pair, its gathers and association, the exact accumulators' hot cells, and the
// pair bodies themselves: PcgInitPairs (PCGInit: pending flush and candidate), PcgStep1Pairs (PCGStep1: candidate) and
// pcg_update_surfel.  A sweep kernel draws its tile, opens it, declares the state and calls these; what differs between the sweeps
// (which keyframes, which pose unknowns, which surfels) reaches the bodies as arguments, so a new parameter of a pair body is a
// parameter, not a copy.  tests/test_cpu_pcg_window_kernel_resources.py holds every sweep kernel to its instruction mix and resources.
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

// UpdateSurfelsFromPCGDelta for surfel i (B/kernel_pcg.cu:1306-1331): the body of pcg_update_surfels_kernel (kernels_pcg.hip) and of
// pcg_window_update_surfels_kernel (kernels_pcg_window.hip), which runs it on the active surfels only
__device__ __forceinline__ void pcg_update_surfel(const PcgLayout& L, const SurfelsView& s, const float* __restrict__ delta, uint32_t i) {
  const uint32_t gi = L.surfel_start + (uint32_t)L.geom_stride * i;
  const float t = delta[gi];
  if (t != 0) {
    const Vec3 np = surfel_position(s, i) + t * surfel_normal(s, i);
    s.row(kSurfelX)[i] = np.x; s.row(kSurfelY)[i] = np.y; s.row(kSurfelZ)[i] = np.z;
  }
  if (L.geom_stride == 3) {
    float a = s.row(kSurfelDescriptor1)[i]; a += delta[gi + 1];
    s.row(kSurfelDescriptor1)[i] = fmaxf(-180.f, fminf(180.f, a));
    float b = s.row(kSurfelDescriptor2)[i]; b += delta[gi + 2];
    s.row(kSurfelDescriptor2)[i] = fmaxf(-180.f, fminf(180.f, b));
  }
}

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

// ---- PCGInit: r -= J^T W F, M += diag(J^T W J) -- one candidate keyframe of one 64-surfel tile (B/kernel_pcg.cu:179-541) ----
// The ONE definition of the pair body of pcg_init_kernel (kernels_pcg.hip) and pcg_window_init_kernel (kernels_pcg_window.hip).  The
// state -- the surfel chains gr / gM and the pending totals -- stays in locals of the calling kernel, declared there in this order, and
// is reached through the references below (a struct that owns the state compiles to other code).  What differs per caller comes as
// two callables of candidate(): whether the keyframe's pose is an unknown (asked after the nobody-sees-it exit) and the head index of
// its first pose unknown (asked last, only for an unknown).
// The exact atomics of a candidate keyframe are issued one candidate late, behind the next candidate's gathers
// (exact_sum.h: exact_atomic_add_part_untracked): the (tile, keyframe) totals wait in pending_a / pending_b -- lanes
// 4 j .. 4 j + 3 hold total j of a 16-value halving butterfly: pending_a = 6 pose entries of r, 6 of M, the first 4 global
// intrinsics entries of r; pending_b (intrinsics only) = the other 5 of r and the 9 of M -- and the per-cell cfactor terms
// of a lane in pending_cf*.
template <bool kDepthIntr, bool kColorIntr>
struct PcgInitPairs {
  static constexpr bool kIntr = kDepthIntr || kColorIntr;
  const PcgLayout& L; const PcgExact& ex; const Intrinsics& in;
  const Vec3& gp; const Vec3& gn; const TangentPoints& tp; const float& d1; const float& d2;   // the lane's surfel
  const bool& in_range; const int& lane; const int& replica;
  float (&gr)[3]; float (&gM)[3];               // surfel entries
  float& pending_a; float& pending_b;
  bool& pending_any; bool& pending_pose;        // wave-uniform
  uint32_t& pending_base;                       // wave-uniform
  uint32_t& pending_cf;                         // per lane: head index of the cell
  float& pending_cf_r; float& pending_cf_M;
  static __device__ __forceinline__ bool intr_enabled(int q) { return q < 5 ? kDepthIntr : kColorIntr; }
  __device__ __forceinline__ void flush() const {
    if (pending_any) {
      const int j = lane >> 2, part = lane & 3;   // two of the four lanes that hold total j add its two parts
      if (part < 2) {
        if (j < 12) {
          if (pending_pose) exact_atomic_add_part_untracked(j < 6 ? &ex.head_a[pending_base + j] : &ex.head_b[pending_base + j - 6], pending_a, part, ex.invalid);
        } else if (kIntr && intr_enabled(j - 12)) {
          exact_atomic_add_part_untracked(hot_cell(ex, kHotA + (j - 12), replica), pending_a, part, ex.invalid);
        }
        if (kIntr) {
          if (j < 5) { if (intr_enabled(4 + j)) exact_atomic_add_part_untracked(hot_cell(ex, kHotA + 4 + j, replica), pending_b, part, ex.invalid); }
          else if (j < 14 && intr_enabled(j - 5)) exact_atomic_add_part_untracked(hot_cell(ex, kHotB + (j - 5), replica), pending_b, part, ex.invalid);
        }
      }
      pending_any = false;
    }
    if (kDepthIntr) {
      if (pending_cf != 0xffffffffu) {
#pragma unroll
        for (int part = 0; part < 2; ++part) {
          exact_atomic_add_part_untracked(&ex.head_a[pending_cf], pending_cf_r, part, ex.invalid);
          exact_atomic_add_part_untracked(&ex.head_b[pending_cf], pending_cf_M, part, ex.invalid);
        }
      }
      pending_cf = 0xffffffffu;
    }
  }
  template <typename PoseIsUnknown, typename PoseIndex>
  __device__ __forceinline__ void candidate(const KfEntry& kf, PoseIsUnknown pose_is_unknown, PoseIndex pose_index) const {
    PairGather pg;
    bool visible = gather_and_associate(L, in, kf, gp, gn, tp, in_range, &pg);
    flush();
    if (!__any(visible)) return;
    const bool pose_kf = pose_is_unknown();
    float pr[6] = {0, 0, 0, 0, 0, 0}, pM[6] = {0, 0, 0, 0, 0, 0};
    float ir[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, iM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // this keyframe's global intrinsics terms
    if (visible) {
      PairTerms t;
      eval_pair_terms<kDepthIntr, kColorIntr>(L, in, kf, pg.a, pg.pix, pg.dw, gn, d1, d2, &t);
      if (L.use_depth) {
        if (L.optimize_geometry) {
          gr[0] -= t.Jgeom * t.w * t.raw;
          gM[0] += t.Jgeom * t.w * t.Jgeom;
        }
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) { const float wj = t.w * t.Jpose[c]; pr[c] += -1 * wj * t.raw; pM[c] += t.Jpose[c] * wj; }
        }
        if (kDepthIntr) {
          if (!t.di_valid) visible = false;   // B/kernel_pcg.cu:272-274: also hides the descriptor part
          if (visible) {
#pragma unroll
            for (int c = 0; c < 5; ++c) { const float wj = t.w * t.Jdi[c]; ir[c] += -1 * wj * t.raw; iM[c] += t.Jdi[c] * wj; }
            const float wj = t.w * t.Jcf;
            pending_cf = head_index(L, t.cf_index);
            pending_cf_r = -1 * wj * t.raw;
            pending_cf_M = t.Jcf * wj;
          }
        }
      }
      if (L.use_desc && visible && t.color_ok) {
        if (L.optimize_geometry) {
          gr[0] -= t.Jg1 * t.w1 * t.raw1 + t.Jg2 * t.w2 * t.raw2;
          gM[0] += t.Jg1 * t.w1 * t.Jg1 + t.Jg2 * t.w2 * t.Jg2;
          gr[1] -= -1.f * t.w1 * t.raw1 + 0.f * t.w2 * t.raw2;
          gM[1] += -1.f * t.w1 * -1.f + 0.f * t.w2 * 0.f;
          gr[2] -= 0.f * t.w1 * t.raw1 + -1.f * t.w2 * t.raw2;
          gM[2] += 0.f * t.w1 * 0.f + -1.f * t.w2 * -1.f;
        }
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const float wj1 = t.w1 * t.Jp1[c], wj2 = t.w2 * t.Jp2[c];
            pr[c] += -1 * wj1 * t.raw1 + -1 * wj2 * t.raw2;
            pM[c] += t.Jp1[c] * wj1 + t.Jp2[c] * wj2;
          }
        }
        if (kColorIntr) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float wj1 = t.w1 * t.Jci1[c], wj2 = t.w2 * t.Jci2[c];
            ir[5 + c] += -1 * wj1 * t.raw1 + -1 * wj2 * t.raw2;
            iM[5 + c] += t.Jci1[c] * wj1 + t.Jci2[c] * wj2;
          }
        }
      }
    }
    if (pose_kf || kIntr) {
      // (tile, keyframe) totals with the halving butterfly of wave_reduce.h: lanes 4 j .. 4 j + 3 hold total j
      const float va[16] = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pM[0], pM[1], pM[2], pM[3], pM[4], pM[5], ir[0], ir[1], ir[2], ir[3]};
      pending_a = wave_reduce_small<16>(va, lane);
      if (kIntr) {
        const float vb[16] = {ir[4], ir[5], ir[6], ir[7], ir[8], iM[0], iM[1], iM[2], iM[3], iM[4], iM[5], iM[6], iM[7], iM[8], 0.f, 0.f};
        pending_b = wave_reduce_small<16>(vb, lane);
      }
      pending_any = true;
      pending_pose = pose_kf;
      pending_base = pose_kf ? pose_index() : 0u;   // pose unknowns come first: head index == unknown index
    }
  }
};

// ---- PCGStep1: g += J^T W J p, alpha_d += p^T J^T W J p -- one candidate keyframe of one 64-surfel tile (B/kernel_pcg.cu:646-1026) ----
// The ONE definition of the pair body of pcg_step1_tile (kernels_pcg.hip: pcg_step1_kernel, pcg_step1_lds_kernel) and
// pcg_window_step1_kernel (kernels_pcg_window.hip), in the form of PcgInitPairs: the chains gs and the pending totals stay in locals
// of the caller, declared there in this order (the lane's surfel is held by value: by reference one of the 64 sweep kernels came out
// one instruction longer).  candidate() asks its callables whether the keyframe's pose is an unknown and then, in any case, for the
// head index of its first pose unknown, and calls the caller's `flush` behind the candidate's gathers and loads of p.
// The flush itself stays with the callers: it is where they differ (the whole-map sweeps add through a sink, global or LDS; the
// windowed sweep adds to the accumulators directly), and written once over a sink it cost the windowed depth-intrinsics kernels two
// instructions and four whole-map kernels a wait.  The (tile, keyframe) totals it adds: 6 pose entries of g, the keyframe's share
// of alpha_d and (intrinsics) the 9 global intrinsics entries of g -- 8 or 16 values, one halving butterfly; the cfactor cell per lane.
template <bool kDepthIntr, bool kColorIntr>
struct PcgStep1Pairs {
  static constexpr bool kIntr = kDepthIntr || kColorIntr;
  const PcgLayout& L; const Intrinsics& in;
  const float* __restrict__ const& p_;
  const Vec3 gp; const Vec3 gn; const TangentPoints tp; const float d1; const float d2;   // the lane's surfel (copies, see above)
  const bool& in_range; const int& lane;
  const float (&ps)[3]; const float (&pdi)[5]; const float (&pci)[4];   // p: the surfel's entries, the global intrinsics entries
  float (&gs)[3];                               // surfel entries of g
  float& pending;
  bool& pending_any; bool& pending_pose;        // wave-uniform
  uint32_t& pending_base;                       // wave-uniform
  uint32_t& pending_cf;                         // per lane
  float& pending_cf_g;
  template <typename PoseIsUnknown, typename PoseIndex, typename Flush>
  __device__ __forceinline__ void candidate(const KfEntry& kf, PoseIsUnknown pose_is_unknown, PoseIndex pose_index, Flush flush) const {
    PairGather pg;
    const bool visible = gather_and_associate(L, in, kf, gp, gn, tp, in_range, &pg);
    const bool pose_kf = pose_is_unknown();
    const uint32_t base = pose_index();
    float pp[6] = {0, 0, 0, 0, 0, 0};
    if (pose_kf) for (int c = 0; c < 6; ++c) pp[c] = p_[base + c];   // (wave-uniform address: scalar loads)
    flush();
    if (!__any(visible)) return;
    float gpose[6] = {0, 0, 0, 0, 0, 0};
    float gi_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // this keyframe's terms of the global intrinsics entries
    float ad = 0.f;                                   // ... and of alpha_d
    if (visible) {
      PairTerms t;
      eval_pair_terms<kDepthIntr, kColorIntr>(L, in, kf, pg.a, pg.pix, pg.dw, gn, d1, d2, &t);
      if (L.use_depth) {
        float sum = 0;
        if (L.optimize_geometry) sum += t.Jgeom * ps[0];
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) sum += t.Jpose[c] * pp[c];
        }
        const bool di = kDepthIntr && t.di_valid;
        float pcf = 0.f;
        if (di) {
          sum += t.Jdi[2] * pdi[2];
          sum += t.Jdi[3] * pdi[3];
          sum += t.Jdi[0] * pdi[0];
          sum += t.Jdi[1] * pdi[1];
          sum += t.Jdi[4] * pdi[4];
          pcf = p_[t.cf_index];
          sum += t.Jcf * pcf;
        }
        ad += sum * t.w * sum;
        sum *= t.w;
        if (L.optimize_geometry) gs[0] += t.Jgeom * sum;
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) gpose[c] += t.Jpose[c] * sum;
        }
        if (di) {
#pragma unroll
          for (int c = 0; c < 5; ++c) gi_acc[c] += t.Jdi[c] * sum;
          pending_cf = head_index(L, t.cf_index);
          pending_cf_g = t.Jcf * sum;
        }
      }
      if (L.use_desc && t.color_ok) {
        float sum1 = 0, sum2 = 0;
        if (L.optimize_geometry) {
          sum1 += t.Jg1 * ps[0]; sum2 += t.Jg2 * ps[0];
          sum1 += -1.f * ps[1];
          sum2 += -1.f * ps[2];
        }
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) { sum1 += t.Jp1[c] * pp[c]; sum2 += t.Jp2[c] * pp[c]; }
        }
        if (kColorIntr) {
#pragma unroll
          for (int c = 0; c < 4; ++c) { sum1 += t.Jci1[c] * pci[c]; sum2 += t.Jci2[c] * pci[c]; }
        }
        ad += sum1 * t.w1 * sum1 + sum2 * t.w2 * sum2;
        sum1 *= t.w1; sum2 *= t.w2;
        if (L.optimize_geometry) {
          gs[0] += t.Jg1 * sum1 + t.Jg2 * sum2;
          gs[1] += -1.f * sum1 + 0.f * sum2;
          gs[2] += 0.f * sum1 + -1.f * sum2;
        }
        if (pose_kf) {
#pragma unroll
          for (int c = 0; c < 6; ++c) gpose[c] += t.Jp1[c] * sum1 + t.Jp2[c] * sum2;
        }
        if (kColorIntr) {
#pragma unroll
          for (int c = 0; c < 4; ++c) gi_acc[5 + c] += t.Jci1[c] * sum1 + t.Jci2[c] * sum2;
        }
      }
    }
    if (kIntr) {
      const float v[16] = {gpose[0], gpose[1], gpose[2], gpose[3], gpose[4], gpose[5], ad, gi_acc[0], gi_acc[1], gi_acc[2], gi_acc[3], gi_acc[4],
                           gi_acc[5], gi_acc[6], gi_acc[7], gi_acc[8]};
      pending = wave_reduce_small<16>(v, lane);   // lanes 4 j .. 4 j + 3 hold total j
    } else {
      const float v[8] = {gpose[0], gpose[1], gpose[2], gpose[3], gpose[4], gpose[5], ad, 0.f};
      pending = wave_reduce_small<8>(v, lane);    // lanes 8 j .. 8 j + 7 hold total j
    }
    pending_any = true;
    pending_pose = pose_kf;
    pending_base = pose_kf ? base : 0u;
  }
};

BAHIP_FLAVOURED_END
