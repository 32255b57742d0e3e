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
//
// Where the code lives.  The pair bodies -- everything a candidate keyframe contributes, PCGInit's pending flush, the surfel update --
// are defined once, in pcg_device.h, for these sweeps and the whole-map ones of kernels_pcg.hip.  This unit holds what is the window's
// own: drawing a tile from the list, the active-flag predicate, the lookup of a swept keyframe and its pose unknown, the step-1
// flush on the accumulators, the stores, the tile-list kernel, the launchers and the dispatchers.
#include "pcg_device.h"

BAHIP_FLAVOURED_BEGIN

// ---- windowed PCGInit: r -= J^T W F, M += diag(J^T W J) over the swept keyframes (the pair body: pcg_device.h, PcgInitPairs) ----
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
  // the pending (tile, keyframe) totals: the state of PcgInitPairs (pcg_device.h), which holds the pair body
  float pending_a = 0.f, pending_b = 0.f;
  bool pending_any = false, pending_pose = false;
  uint32_t pending_base = 0;
  uint32_t pending_cf = 0xffffffffu;
  float pending_cf_r = 0.f, pending_cf_M = 0.f;
  const PcgInitPairs<kDepthIntr, kColorIntr> pairs{   // by name: a swap of two members of one type must not compile
      .L = L, .ex = ex, .in = in, .gp = gp, .gn = gn, .tp = tp, .d1 = d1, .d2 = d2, .in_range = in_range, .lane = lane, .replica = replica,
      .gr = gr, .gM = gM, .pending_a = pending_a, .pending_b = pending_b, .pending_any = pending_any, .pending_pose = pending_pose,
      .pending_base = pending_base, .pending_cf = pending_cf, .pending_cf_r = pending_cf_r, .pending_cf_M = pending_cf_M};
  const auto may_project = [&](int j) { return sphere_may_project_item(in, kfs[w.kf[j]].pose.F, wb); };
  const auto candidate = [&](int j) {
    uint32_t base = 0;   // loaded once, when the pair body asks whether the pose is an unknown
    pairs.candidate(kfs[w.kf[j]], [&] { base = w.pose_index[j]; return L.optimize_poses && base != 0xffffffffu; }, [&] { return base; });
  };
  for_each_candidate(w.num_kfs, may_project, candidate);
  pairs.flush();
  if (in_range && L.optimize_geometry) {
    r_[gi] = gr[0]; M_[gi] = gM[0];
    if (L.geom_stride == 3) { r_[gi + 1] = gr[1]; M_[gi + 1] = gM[1]; r_[gi + 2] = gr[2]; M_[gi + 2] = gM[2]; }
  }
}

// ---- windowed PCGStep1: g += J^T W J p, alpha_d += p^T J^T W J p over the swept keyframes (the pair body: pcg_device.h, PcgStep1Pairs) ----
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
  // the pending (tile, keyframe) totals: the state of PcgStep1Pairs (pcg_device.h), which holds the pair body
  float pending = 0.f;
  bool pending_any = false, pending_pose = false;
  uint32_t pending_base = 0;
  uint32_t pending_cf = 0xffffffffu;
  float pending_cf_g = 0.f;
  const PcgStep1Pairs<kDepthIntr, kColorIntr> pairs{   // by name, as for PcgInitPairs
      .L = L, .in = in, .p_ = p_, .gp = gp, .gn = gn, .tp = tp, .d1 = d1, .d2 = d2, .in_range = in_range, .lane = lane, .ps = ps, .pdi = pdi,
      .pci = pci, .gs = gs, .pending = pending, .pending_any = pending_any, .pending_pose = pending_pose, .pending_base = pending_base,
      .pending_cf = pending_cf, .pending_cf_g = pending_cf_g};
  constexpr bool kIntr = kDepthIntr || kColorIntr;
  auto flush_pending = [&]() {   // stays with the caller: pcg_device.h, PcgStep1Pairs
    if (pending_any) {
      const int j = kIntr ? (lane >> 2) : (lane >> 3), part = kIntr ? (lane & 3) : (lane & 7);   // the lanes that hold total j
      if (part < 2) {
        if (j < 6) { if (pending_pose) exact_atomic_add_part_untracked(&ex.head_a[pending_base + j], pending, part, ex.invalid); }
        else if (j == 6) exact_atomic_add_part_untracked(hot_cell(ex, kHotAlphaD, replica), pending, part, ex.invalid);
        else if (kIntr && j < 16 && ((j - 7) < 5 ? kDepthIntr : kColorIntr)) exact_atomic_add_part_untracked(hot_cell(ex, kHotA + (j - 7), replica), pending, part, ex.invalid);
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
    uint32_t base = 0;   // loaded once, when the pair body asks whether the pose is an unknown
    pairs.candidate(kfs[w.kf[j]], [&] { base = w.pose_index[j]; return L.optimize_poses && base != 0xffffffffu; }, [&] { return base; }, flush_pending);
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
  pcg_update_surfel(L, s, delta, i);
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
