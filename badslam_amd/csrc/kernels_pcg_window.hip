// kernels_pcg_window.hip -- the PCG sweeps (PCGInit, PCGStep1) over an active keyframe window: bahip_pcg_iteration_windowed.
//
// DEFINITION of the windowed system.  Inputs: the activation field of the bound keyframe table (as bahip_set_activation_window /
// bahip_apply_activation_window / bahip_propagate_covisible_activation leave it) and the surfels' kSurfelActiveFlag.
//   - Swept keyframes: those whose activation is not kInactive, in ascending bound order.  A kInactive keyframe is not read at all
//     (neither its images nor its pose).
//   - Pose unknowns: 6 per kActive keyframe, in bound order.  Gauge: if at least one keyframe is kCovisibleActive, no kActive pose is
//     held fixed (the fixed co-visible poses anchor the gauge); otherwise opt->gauge_keyframe (a bound index) if it is kActive, else
//     the first kActive keyframe.  kCovisibleActive keyframes contribute residuals with fixed poses.
//   - Surfel unknowns: the surfels with the active bit.  The layout stays geom_stride x surfels_size: an inactive surfel keeps all-zero
//     rows of r, M, g and p, and its pairs contribute nothing -- to surfel, pose or intrinsics rows, cfactor cells, or alpha_d.
//   - Unchanged bits: rows 0-7 of every inactive surfel (pcg_window_update_surfels_kernel skips them) and the pose of every keyframe
//     that is not a pose unknown (the host applies no update to it).
//   - Everything else is kernels_pcg.hip's definition: exact dense sums, the surfel block as one binary32 chain per entry over the
//     swept keyframes in order, the epsilon terms of alpha_d counted once per swept keyframe, the device-side stopping rule and the
//     sticky non-finite flag.  Every bound keyframe whose pose is not an unknown counts as converged.
// Consequences: with every keyframe kActive and every surfel active this is bahip_pcg_iteration's system with the same gauge; it is
// the stage-by-stage driver's (bahip_pcg_init / bahip_pcg_step1 once per swept keyframe, optimize_pose_of_keyframe = 0 for the
// co-visible ones) on a buffer of the active surfels alone, in the same order and the same 64-surfel tiles (the pose entries are
// exact sums of per-(tile, keyframe) binary32 halving trees: tiles of other composition give other terms); two keyframe groups that
// see disjoint surfels do not mix.
//
// Launch shape.  The grid runs over a compact list of the 64-surfel tiles that hold at least one active surfel
// (pcg_window_tiles_kernel, once per outer iteration); a lane's predicate is in_range && (active[i] & kSurfelActiveFlag).  The
// keyframe loop walks the device list of swept keyframes (bound index and pose-unknown index per entry) with the wave64 frustum cull
// of wave_cull.h and the gathers of gather_and_associate.  So the cost scales with the window, not with the map.  The per-unknown
// kernels (init2, step2, step3, control, resolve) are kernels_pcg.hip's: zero rows give exact zeros.
#include "pcg_device.h"

BAHIP_FLAVOURED_BEGIN

// ---- windowed PCGInit: r -= J^T W F, M += diag(J^T W J) over the swept keyframes (kernels_pcg.hip: pcg_init_kernel) ----
template <bool kDepthIntr, bool kColorIntr>
__global__ void __launch_bounds__(kPcgSweepBlock) BAHIP_PCG_SWEEP_ATTR
pcg_window_init_kernel(PcgLayout L, PcgExact ex, Intrinsics in, const KfEntry* __restrict__ kfs, PcgWindow w, SurfelsView s,
                       float* __restrict__ r_, float* __restrict__ M_) {
  const uint32_t tile = w.tiles[blockIdx.x];
  const uint32_t i = tile * kPcgSweepBlock + threadIdx.x;
  const uint32_t ii = i < s.size ? i : 0;
  const bool in_range = i < s.size && (s.active[ii] & kSurfelActiveFlag);
  const Vec3 gp = surfel_position(s, ii);
  const Vec3 gn = surfel_normal(s, ii);
  const float radius_sq = s.row(kSurfelRadiusSquared)[ii];
  const float d1 = s.row(kSurfelDescriptor1)[ii], d2 = s.row(kSurfelDescriptor2)[ii];
  const TangentPoints tp = surfel_tangent_points(gp, gn, radius_sq);
  const WaveBounds wb = wave_bounds(gp, in_range && (gp.x == gp.x));
  const int lane = threadIdx.x & 63;
  const int replica = (int)(tile & (kHotReplicas - 1));
  const uint32_t gi = L.optimize_geometry ? (L.surfel_start + (uint32_t)L.geom_stride * ii) : 0u;
  float gr[3] = {0, 0, 0}, gM[3] = {0, 0, 0};
  constexpr bool kIntr = kDepthIntr || kColorIntr;
  // the exact atomics of a candidate go out one candidate late, as in pcg_init_kernel (same lane layout of pending_a / pending_b)
  float pending_a = 0.f, pending_b = 0.f;
  bool pending_any = false, pending_pose = false;
  uint32_t pending_base = 0;
  uint32_t pending_cf = 0xffffffffu;
  float pending_cf_r = 0.f, pending_cf_M = 0.f;
  auto intr_enabled = [&](int q) { return q < 5 ? kDepthIntr : kColorIntr; };
  auto flush_pending = [&]() {
    if (pending_any) {
      const int j = lane >> 2, part = lane & 3;
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
  };
  const auto may_project = [&](int j) { return sphere_may_project_item(in, kfs[w.kf[j]].pose.F, wb); };
  const auto candidate = [&](int j) {
    const KfEntry& kf = kfs[w.kf[j]];
    PairGather pg;
    bool visible = gather_and_associate(L, in, kf, gp, gn, tp, in_range, &pg);
    flush_pending();
    if (!__any(visible)) return;
    const uint32_t base = w.pose_index[j];
    const bool pose_kf = L.optimize_poses && base != 0xffffffffu;
    float pr[6] = {0, 0, 0, 0, 0, 0}, pM[6] = {0, 0, 0, 0, 0, 0};
    float ir[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, iM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
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
          if (!t.di_valid) visible = false;
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
      const float va[16] = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pM[0], pM[1], pM[2], pM[3], pM[4], pM[5], ir[0], ir[1], ir[2], ir[3]};
      pending_a = wave_reduce_small<16>(va, lane);
      if (kIntr) {
        const float vb[16] = {ir[4], ir[5], ir[6], ir[7], ir[8], iM[0], iM[1], iM[2], iM[3], iM[4], iM[5], iM[6], iM[7], iM[8], 0.f, 0.f};
        pending_b = wave_reduce_small<16>(vb, lane);
      }
      pending_any = true;
      pending_pose = pose_kf;
      pending_base = pose_kf ? base : 0u;
    }
  };
  for_each_candidate(w.num_kfs, may_project, candidate);
  flush_pending();
  if (in_range && L.optimize_geometry) {
    r_[gi] = gr[0]; M_[gi] = gM[0];
    if (L.geom_stride == 3) { r_[gi + 1] = gr[1]; M_[gi + 1] = gM[1]; r_[gi + 2] = gr[2]; M_[gi + 2] = gM[2]; }
  }
}

// ---- windowed PCGStep1: g += J^T W J p, alpha_d += p^T J^T W J p over the swept keyframes (kernels_pcg.hip: pcg_step1_tile) ----
template <bool kDepthIntr, bool kColorIntr>
__global__ void __launch_bounds__(kPcgSweepBlock) BAHIP_PCG_SWEEP_ATTR
pcg_window_step1_kernel(PcgLayout L, PcgExact ex, Intrinsics in, const KfEntry* __restrict__ kfs, PcgWindow w, SurfelsView s,
                        const float* __restrict__ p_, float* __restrict__ g_, const PcgControl* ctl) {
  if (ctl->stop) return;
  const uint32_t tile = w.tiles[blockIdx.x];
  const int replica = (int)(tile & (kHotReplicas - 1));
  const uint32_t i = tile * kPcgSweepBlock + threadIdx.x;
  const uint32_t ii = i < s.size ? i : 0;
  const bool in_range = i < s.size && (s.active[ii] & kSurfelActiveFlag);
  const Vec3 gp = surfel_position(s, ii);
  const Vec3 gn = surfel_normal(s, ii);
  const float radius_sq = s.row(kSurfelRadiusSquared)[ii];
  const float d1 = s.row(kSurfelDescriptor1)[ii], d2 = s.row(kSurfelDescriptor2)[ii];
  const TangentPoints tp = surfel_tangent_points(gp, gn, radius_sq);
  const WaveBounds wb = wave_bounds(gp, in_range && (gp.x == gp.x));
  const int lane = threadIdx.x & 63;
  const uint32_t gi = L.optimize_geometry ? (L.surfel_start + (uint32_t)L.geom_stride * ii) : 0u;
  float ps[3] = {0, 0, 0};
  if (L.optimize_geometry) {
    ps[0] = p_[gi];
    if (L.geom_stride == 3) { ps[1] = p_[gi + 1]; ps[2] = p_[gi + 2]; }
  }
  float pdi[5] = {0, 0, 0, 0, 0}, pci[4] = {0, 0, 0, 0};
  if (kDepthIntr) for (int c = 0; c < 5; ++c) pdi[c] = p_[L.depth_intr_start + c];
  if (kColorIntr) for (int c = 0; c < 4; ++c) pci[c] = p_[L.color_intr_start + c];
  float gs[3] = {0, 0, 0};
  constexpr bool kIntr = kDepthIntr || kColorIntr;
  float pending = 0.f;
  bool pending_any = false, pending_pose = false;
  uint32_t pending_base = 0;
  uint32_t pending_cf = 0xffffffffu;
  float pending_cf_g = 0.f;
  auto flush_pending = [&]() {
    if (pending_any) {
      const int j = kIntr ? (lane >> 2) : (lane >> 3), part = kIntr ? (lane & 3) : (lane & 7);
      if (part < 2) {
        if (j < 6) { if (pending_pose) exact_atomic_add_part_untracked(&ex.head_a[pending_base + j], pending, part, ex.invalid); }
        else if (j == 6) exact_atomic_add_part_untracked(hot_cell(ex, kHotAlphaD, replica), pending, part, ex.invalid);
        else if (kIntr && j < 16 && ((j - 7) < 5 ? kDepthIntr : kColorIntr))
          exact_atomic_add_part_untracked(hot_cell(ex, kHotA + (j - 7), replica), pending, part, ex.invalid);
      }
      pending_any = false;
    }
    if (kDepthIntr) {
      if (pending_cf != 0xffffffffu) {
        exact_atomic_add_part_untracked(&ex.head_a[pending_cf], pending_cf_g, 0, ex.invalid);
        exact_atomic_add_part_untracked(&ex.head_a[pending_cf], pending_cf_g, 1, ex.invalid);
      }
      pending_cf = 0xffffffffu;
    }
  };
  const auto may_project = [&](int j) { return sphere_may_project_item(in, kfs[w.kf[j]].pose.F, wb); };
  const auto candidate = [&](int j) {
    const KfEntry& kf = kfs[w.kf[j]];
    PairGather pg;
    const bool visible = gather_and_associate(L, in, kf, gp, gn, tp, in_range, &pg);
    const uint32_t base = w.pose_index[j];
    const bool pose_kf = L.optimize_poses && base != 0xffffffffu;
    float pp[6] = {0, 0, 0, 0, 0, 0};
    if (pose_kf) for (int c = 0; c < 6; ++c) pp[c] = p_[base + c];
    flush_pending();
    if (!__any(visible)) return;
    float gpose[6] = {0, 0, 0, 0, 0, 0};
    float gi_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    float ad = 0.f;
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
        if (di) {
          sum += t.Jdi[2] * pdi[2];
          sum += t.Jdi[3] * pdi[3];
          sum += t.Jdi[0] * pdi[0];
          sum += t.Jdi[1] * pdi[1];
          sum += t.Jdi[4] * pdi[4];
          sum += t.Jcf * p_[t.cf_index];
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
      pending = wave_reduce_small<16>(v, lane);
    } else {
      const float v[8] = {gpose[0], gpose[1], gpose[2], gpose[3], gpose[4], gpose[5], ad, 0.f};
      pending = wave_reduce_small<8>(v, lane);
    }
    pending_any = true;
    pending_pose = pose_kf;
    pending_base = pose_kf ? base : 0u;
  };
  for_each_candidate(w.num_kfs, may_project, candidate);
  flush_pending();
  if (in_range && L.optimize_geometry) {
    g_[gi] = gs[0];
    if (L.geom_stride == 3) { g_[gi + 1] = gs[1]; g_[gi + 2] = gs[2]; }
  }
}

void launch_pcg_window_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                            const SurfelsView& s, float* r, float* M) {
  if (!w.num_tiles || !w.num_kfs) return;
  const dim3 grid(w.num_tiles), block(kPcgSweepBlock);
  const bool di = L.optimize_depth_intrinsics, ci = L.optimize_color_intrinsics;
  if (di && ci) hipLaunchKernelGGL((pcg_window_init_kernel<true, true>), grid, block, 0, st, L, ex, in, kfs, w, s, r, M);
  else if (di) hipLaunchKernelGGL((pcg_window_init_kernel<true, false>), grid, block, 0, st, L, ex, in, kfs, w, s, r, M);
  else if (ci) hipLaunchKernelGGL((pcg_window_init_kernel<false, true>), grid, block, 0, st, L, ex, in, kfs, w, s, r, M);
  else hipLaunchKernelGGL((pcg_window_init_kernel<false, false>), grid, block, 0, st, L, ex, in, kfs, w, s, r, M);
}
void launch_pcg_window_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                             const SurfelsView& s, const float* p, float* g, const void* ctl) {
  if (!w.num_tiles || !w.num_kfs) return;
  const PcgControl* stop = static_cast<const PcgControl*>(ctl);
  const dim3 grid(w.num_tiles), block(kPcgSweepBlock);
  const bool di = L.optimize_depth_intrinsics, ci = L.optimize_color_intrinsics;
  if (di && ci) hipLaunchKernelGGL((pcg_window_step1_kernel<true, true>), grid, block, 0, st, L, ex, in, kfs, w, s, p, g, stop);
  else if (di) hipLaunchKernelGGL((pcg_window_step1_kernel<true, false>), grid, block, 0, st, L, ex, in, kfs, w, s, p, g, stop);
  else if (ci) hipLaunchKernelGGL((pcg_window_step1_kernel<false, true>), grid, block, 0, st, L, ex, in, kfs, w, s, p, g, stop);
  else hipLaunchKernelGGL((pcg_window_step1_kernel<false, false>), grid, block, 0, st, L, ex, in, kfs, w, s, p, g, stop);
}
BAHIP_FLAVOURED_END

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
constexpr int kPcgWindowBlock = 256;
// The tile list: one thread per 64-surfel tile appends the tile if any of its surfels is active.  The list's order follows the
// atomics; nothing depends on it (the surfel chains are per surfel, the dense sums exact).
__global__ void __launch_bounds__(kPcgWindowBlock) pcg_window_tiles_kernel(SurfelsView s, uint32_t* __restrict__ tiles, uint32_t* __restrict__ count) {
  const uint32_t tile = blockIdx.x * kPcgWindowBlock + threadIdx.x;
  const uint32_t first = tile * kPcgSweepBlock;
  if (first >= s.size) return;
  const uint32_t end = min(first + (uint32_t)kPcgSweepBlock, s.size);
  bool any = false;
  for (uint32_t i = first; i < end && !any; ++i) any = (s.active[i] & kSurfelActiveFlag) != 0;
  if (any) tiles[atomicAdd(count, 1u)] = tile;
}
// UpdateSurfelsFromPCGDelta (kernels_pcg.hip: pcg_update_surfels_kernel) on the active surfels only: an inactive surfel's rows stay
// bit-identical (the unmasked kernel would clamp its descriptors and turn -0 into +0)
__global__ void __launch_bounds__(kPcgWindowBlock)
pcg_window_update_surfels_kernel(PcgLayout L, SurfelsView s, const float* __restrict__ delta) {
  const uint32_t i = blockIdx.x * kPcgWindowBlock + threadIdx.x;
  if (i >= s.size || !(s.active[i] & kSurfelActiveFlag)) return;
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
void launch_pcg_window_tiles(hipStream_t st, const SurfelsView& s, uint32_t* tiles, uint32_t* count) {
  const uint32_t n = (s.size + kPcgSweepBlock - 1) / kPcgSweepBlock;
  if (n) hipLaunchKernelGGL(pcg_window_tiles_kernel, dim3((n + kPcgWindowBlock - 1) / kPcgWindowBlock), dim3(kPcgWindowBlock), 0, st, s, tiles, count);
}
void launch_pcg_window_update_surfels(hipStream_t st, const PcgLayout& L, const SurfelsView& s, const float* delta) {
  if (s.size) hipLaunchKernelGGL(pcg_window_update_surfels_kernel, dim3((s.size + kPcgWindowBlock - 1) / kPcgWindowBlock), dim3(kPcgWindowBlock), 0, st, L, s, delta);
}
// dispatchers (ba_launch.h: "Two arithmetic flavours")
void launch_pcg_window_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                            const SurfelsView& s, float* r, float* M) {
  BAHIP_PICK(in, launch_pcg_window_init(st, L, ex, in, kfs, w, s, r, M));
}
void launch_pcg_window_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                             const SurfelsView& s, const float* p, float* g, const void* ctl) {
  BAHIP_PICK(in, launch_pcg_window_step1(st, L, ex, in, kfs, w, s, p, g, ctl));
}
}  // namespace bahip
#endif
