// kernels_pcg.hip -- matrix-free preconditioned conjugate gradients on the full Gauss-Newton system.
//
// Reference (B/ = applications/badslam/src/badslam/): B/kernel_pcg.cu:179-1389 driven by
// B/direct_ba_pcg.cc:229-646.  Unknowns: [6 per non-gauge keyframe | 1 or 3 per surfel | 5 + S depth
// intrinsics | 4 colour intrinsics].  PCGInit and PCGStep1 are launched once per keyframe over all
// surfels there, with 12..46 serial block reductions per block and read-modify-write of the
// surfel entries per keyframe.
//
// Here both are single launches: a thread owns a surfel and sweeps the keyframes that survive the
// wave64 frustum test (wave_cull.h).  Surfel entries of r / M / g are accumulated in registers in
// keyframe order (identical to the reference's launch order) and written once.
//
// DEFINITION of the dense sums (round 3; restated by oracle_pcg.c).  Everything the reference merges with binary32
// atomics in arbitrary order (B/kernel_pcg.cu:98-154) is an EXACT sum here (exact_sum.h: 9 x int64 limbs, integer atomics),
// rounded once to binary64 and then to the PCGScalar:
//   - the 6 pose entries of a keyframe, the 5 + 4 global intrinsics entries and the pair part of alpha_d: per (64-surfel tile,
//     keyframe) the halving tree of wave_reduce.h over that keyframe's per-surfel terms, the (tile, keyframe) totals exact --
//     the intrinsics entries and alpha_d into one of 64 replicas, folded when resolved (exactness makes the replication free,
//     and 47 k tiles would otherwise serialise on one address).  Nothing is carried from one keyframe to the next, so one
//     sweep over all keyframes and one call per keyframe (the stage entry points of the C ABI) give the same sums;
//   - per-cell cfactor entries: per-pair terms, exact;
//   - dot products over the unknowns (alpha_n, beta_n, the epsilon terms of alpha_d): the binary32 products, exact.
// So the conjugate gradient is deterministic, bit-identical to the oracle (inner step count included), independent of the
// launch shape, and a surfel-sharded run -- limbs exchanged with an int64 all-reduce -- equals the unsharded one bit for bit.
//
// DEFINITION of the surfel block of r, M (PCGInit) and g (PCGStep1) over C keyframe classes (bahip_context_set_pcg_sum_classes: 1, 2,
// 4 or 8; keyframe k of the bound table belongs to class k % C): per surfel entry and class a binary32 chain over the class's keyframes
// in ascending order, p_c, and the entry is ((p0 + p1) + p2) + ... -- the combination rule of tile_sums in kernels_surfel.hip.  C = 1
// is the one chain over all keyframes, written by the sweep itself (the kernels without the class loop, kClassed off).  With C > 1 the
// sweeps (kClassed on) visit the classes a rank owns and store their chains to class partials ([class][entry][surfel], zero for the
// classes of other ranks); under keyframe sharding the ranks sum the partials as 64-bit integers (x + 0 keeps every bit) and
// pcg_class_combine_kernel adds them up as defined.  A single GPU with C > 1 takes the same route without the exchange.
#include "ba_device.h"
#include "ba_launch.h"
#include "exact_sum.h"
#include "wave_cull.h"
#include "pcg_device.h"

namespace bahip {


__device__ __forceinline__ uint32_t kf_pose_index(const PcgLayout& L, int k) {
  // B/direct_ba_pcg.cc:329-337
  if (L.single_keyframe >= 0) return L.single_pose_index;   // per-keyframe entry points (Route B): the caller names the index
  if (k == L.gauge) return 0xffffffffu;
  return (k < L.gauge) ? 6u * (uint32_t)k : 6u * (uint32_t)(k - 1);
}
__device__ __forceinline__ bool kf_pose_is_unknown(const PcgLayout& L, int k) {
  return L.optimize_poses && (L.single_keyframe >= 0 || k != L.gauge);
}
// Slot (0..8) of a global intrinsics unknown among the replicated accumulators, or -1.
__device__ __forceinline__ int intrinsics_slot(const PcgLayout& L, uint32_t u) {
  if (L.optimize_depth_intrinsics && u >= L.depth_intr_start && u < L.depth_intr_start + 5u) return (int)(u - L.depth_intr_start);
  if (L.optimize_color_intrinsics && u >= L.color_intr_start && u < L.color_intr_start + 4u) return 5 + (int)(u - L.color_intr_start);
  return -1;
}
// The classes of a kClassed sweep come as its last kernel argument; a sweep without the class loop has no such argument, so its code
// (kernel arguments included) is that of the one-class definition alone.
__device__ __forceinline__ PcgClasses pcg_classes_of() { return PcgClasses{}; }
__device__ __forceinline__ PcgClasses pcg_classes_of(const PcgClasses& c) { return c; }
// Plane q of class c's partials (kClassed sweeps: the entries of this rank's classes; pcg_class_combine_kernel: all of them).
__device__ __forceinline__ float* pcg_class_plane(const PcgClasses& pc, int c, int q) {
  return pc.cp.data + (size_t)(c * pc.entries + q) * pc.cp.stride;
}

// ---- the exact accumulators of one PCG solve ------------------------------------------------------------------------------
// One device allocation, laid out so that what a sharded run exchanges is contiguous:
//   [ replicated slots 0..19 | head A | head B | invalid flag | replicated slot 20 | replicated slots 21..22 ]
// exchange 1 (after a sweep) = slots 0..19 + head A (+ head B after PCGInit); exchange 2 (after a dot product) = the flag's cell +
// slot 20.  The sticky flag travels with exchange 2, which precedes every evaluation of the stopping rule: once any rank has
// added a non-finite term, every rank's flag is non-zero (the integer sum counts the ranks that raised it) from the next control
// step on, all ranks stop after the same inner step and all fail the call alike (round 4 kept the flag behind the block: a
// rank that saw a NaN stopped three steps later, its peers went on, and the collective sequence diverged -- a hang).
// Slots 21 / 22 hold the dense head's share of the dot products: the head is replicated over the ranks, so every rank adds the
// same terms there and they are NOT exchanged.
// One wavefront folds the 64 replicas of slot a (and of slot b if b >= 0) into the exact binary64 value; optionally clears them.
__device__ __forceinline__ double fold_hot(const PcgExact& ex, int a, int b, bool clear) {
  const int lane = threadIdx.x & 63;
  long long l[kExactLimbs];
  ExactCell* ca = hot_cell(ex, a, lane);
  ExactCell* cb = b >= 0 ? hot_cell(ex, b, lane) : nullptr;
#pragma unroll
  for (int j = 0; j < kExactLimbs; ++j) {
    l[j] = ca->limb[j] + (cb ? cb->limb[j] : 0ll);
    if (clear) { ca->limb[j] = 0; if (cb) cb->limb[j] = 0; }
  }
#pragma unroll
  for (int j = 0; j < kExactLimbs; ++j)
    for (int off = 32; off; off >>= 1) l[j] += __shfl_xor(l[j], off);
  return exact_value(l);
}

}  // namespace bahip

// ---- the sweeps (PCGInit, PCGStep1): compiled once per arithmetic flavour (ba_launch.h) ----
BAHIP_FLAVOURED_BEGIN
// ---- PCGInit: r -= J^T W F, M += diag(J^T W J)  (B/kernel_pcg.cu:179-541) -----------------------------
// kClassed: the surfel entries over the keyframe classes of `classes_arg` (one PcgClasses, see "DEFINITION of the surfel block"),
// of which the sweep visits the owned ones and stores their chains to the partials (r_ / M_ are not written); !kClassed: one class,
// every keyframe, the chains written to r_ / M_ -- the kernel as it is without the class loop (no further argument).
template <bool kDepthIntr, bool kColorIntr, bool kClassed, typename... Classes>
__global__ void __launch_bounds__(kPcgSweepBlock) BAHIP_PCG_SWEEP_ATTR
pcg_init_kernel(PcgLayout L, PcgExact ex, Intrinsics in, const KfEntry* __restrict__ kfs, int num_kfs, SurfelsView s,
                float* __restrict__ r_, float* __restrict__ M_, uint32_t* __restrict__ tile_cost, const uint32_t* __restrict__ sched,
                Classes... classes_arg) {
  static_assert(sizeof...(Classes) == (kClassed ? 1 : 0), "a kClassed sweep takes one PcgClasses, the other none");
  uint32_t tile;   // heavy work first (wave_cull.h: scheduled_tile); tile_cost: the census the schedule is built from
  if (!scheduled_tile(blockIdx.x, gridDim.x - (sched ? kHeavySlots : 0u), sched, &tile)) return;
  uint32_t visited = 0;
  const uint32_t i = tile * kPcgSweepBlock + threadIdx.x;
  const bool in_range = i < s.size;
  const uint32_t ii = in_range ? i : 0;
  const Vec3 gp = surfel_position(s, ii);
  const Vec3 gn = surfel_normal(s, ii);
  const float radius_sq = s.row(kSurfelRadiusSquared)[ii];
  const float d1 = s.row(kSurfelDescriptor1)[ii], d2 = s.row(kSurfelDescriptor2)[ii];
  const TangentPoints tp = surfel_tangent_points(gp, gn, radius_sq);   // per surfel, not per pair
  const WaveBounds wb = wave_bounds(gp, in_range && (gp.x == gp.x));
  const int lane = threadIdx.x & 63;
  const int replica = (int)(tile & (kHotReplicas - 1));
  const uint32_t gi = L.optimize_geometry ? (L.surfel_start + (uint32_t)L.geom_stride * ii) : 0u;
  float gr[3] = {0, 0, 0}, gM[3] = {0, 0, 0};     // surfel entries
  if (!kClassed && L.accumulate && in_range && L.optimize_geometry) {   // per-keyframe calls continue the chain the earlier calls left
    gr[0] = r_[gi]; gM[0] = M_[gi];
    if (L.geom_stride == 3) { gr[1] = r_[gi + 1]; gM[1] = M_[gi + 1]; gr[2] = r_[gi + 2]; gM[2] = M_[gi + 2]; }
  }
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
  const auto may_project = [&](int k) { return sphere_may_project_item(in, kfs[k].pose.F, wb); };
  const auto candidate = [&](int k) {
    ++visited;
    pairs.candidate(kfs[k], [&] { return kf_pose_is_unknown(L, k); }, [&] { return kf_pose_index(L, k); });
  };
  if constexpr (!kClassed) {
    for_each_candidate(num_kfs, may_project, candidate);
    pairs.flush();
    if (tile_cost && lane == 0 && visited) atomicAdd(&tile_cost[tile], visited);

    if (in_range && L.optimize_geometry) {
      r_[gi] = gr[0]; M_[gi] = gM[0];
      if (L.geom_stride == 3) { r_[gi + 1] = gr[1]; M_[gi + 1] = gM[1]; r_[gi + 2] = gr[2]; M_[gi + 2] = gM[2]; }
    }
    return;
  }
  // class by class (wave-uniform): the chains of the surfel entries start from zero per class and go to the partials; the dense
  // head's (tile, keyframe) totals go to the exact accumulators as above (any order: integer sums)
  const PcgClasses pc = pcg_classes_of(classes_arg...);
  const int gs = L.geom_stride;
#pragma nounroll
  for (int c = 0; c < pc.classes; ++c) {
    if (!((pc.cp.owned >> c) & 1u)) continue;   // another rank holds this class's images
    for_each_candidate(num_kfs, may_project, candidate, pc.classes, c);
    if (in_range && L.optimize_geometry) {
      pcg_class_plane(pc, c, 0)[i] = gr[0]; pcg_class_plane(pc, c, gs)[i] = gM[0];
      if (gs == 3) {
        pcg_class_plane(pc, c, 1)[i] = gr[1]; pcg_class_plane(pc, c, 4)[i] = gM[1];
        pcg_class_plane(pc, c, 2)[i] = gr[2]; pcg_class_plane(pc, c, 5)[i] = gM[2];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { gr[q] = 0.f; gM[q] = 0.f; }
  }
  pairs.flush();
  if (tile_cost && lane == 0 && visited) atomicAdd(&tile_cost[tile], visited);
}

BAHIP_FLAVOURED_END
namespace bahip {
// ---- inner-loop control on the device -------------------------------------------------------------------------------------
// The reference reads beta_n back after every inner step and decides on the host whether the residual norm still improves
// (B/direct_ba_pcg.cc:427-456: stop after three steps without an improvement of 1e-3).  Here a one-wavefront kernel resolves
// beta_n and takes that decision after step 2; once `stop` is set the sweeps and vector kernels queued behind it return at
// once, so the host can queue several inner steps without waiting for any of them.
// (PcgControl: pcg_device.h)
}  // namespace bahip
#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
// The sticky flag travels in exchange 2 as a 64-bit integer sum: after an exchange it holds (ranks that raised it) x (what it held
// before), and a host that keeps queuing exchanges for the rest of a step group after the device has stopped would multiply it by the
// world size every time -- at 64 ranks the low 32 bits, which is all the readers look at, wrap to 0 after six exchanges.
// Every control step therefore puts it back to 0 / 1, stopped or not.
__device__ __forceinline__ void pcg_renormalise_invalid(const PcgExact& ex) {
  if (threadIdx.x == 0) {
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(ex.invalid);
    if (*flag != 0ull) *flag = 1ull;
  }
}
// after PCGInit2: alpha_n = the exact dot product, rounded; the control block starts over
__global__ void __launch_bounds__(64) pcg_control_init_kernel(PcgExact ex, PcgControl* ctl, float* alpha_n) {
  pcg_renormalise_invalid(ex);
  const double v = fold_hot(ex, kHotDotLocal, kHotDotHead, true);
  if (threadIdx.x == 0) {
    *alpha_n = (*ex.invalid) ? __builtin_nanf("") : (float)v;
    ctl->prev_r_norm = __builtin_huge_val(); ctl->no_improvement = 0; ctl->stop = 0; ctl->steps = 0;
  }
}
// after PCGStep2: beta_n, then the stopping rule.  r_norm is a PCGScalar (binary32 square root), the comparison is evaluated
// in double like the reference's `r_norm < prev_r_norm - 1e-3` (B/direct_ba_pcg.cc:441-446).
__global__ void __launch_bounds__(64) pcg_control_kernel(PcgExact ex, PcgControl* ctl, float* beta_n) {
  pcg_renormalise_invalid(ex);
  if (ctl->stop) return;
  const double v = fold_hot(ex, kHotDotLocal, kHotDotHead, true);
  if (threadIdx.x == 0) {
    const float bn = (*ex.invalid) ? __builtin_nanf("") : (float)v;
    *beta_n = bn;
    ctl->steps += 1;
    const float r_norm = __builtin_sqrtf(bn);   // IEEE (no fast-math): the correctly rounded root, like the oracle's sqrtf
    if ((double)r_norm < ctl->prev_r_norm - 1e-3) ctl->no_improvement = 0;
    else if (++ctl->no_improvement >= 3) ctl->stop = 1;
    ctl->prev_r_norm = (double)r_norm;
  }
}

// ---- resolving the exact accumulators into the PCGScalar vectors -------------------------------------------------------------
// Workgroups [0, head blocks): one thread per dense-head unknown: exact value -> va[u] (and vb[u]); the cell is cleared.  The
// last workgroup folds the replicated slots: the global intrinsics entries and, after PCGStep1, alpha_d.
template <bool kInit>
__global__ void __launch_bounds__(kPcgBlock)
pcg_resolve_kernel(PcgLayout L, PcgExact ex, float* __restrict__ va, float* __restrict__ vb, float* alpha_d, double eps_repeat,
                   const PcgControl* ctl) {
  if (!kInit && ctl->stop) return;
  const bool invalid = *ex.invalid != 0u;
  const uint32_t head_count = L.head_lo + (L.unknown_count - L.head_hi);
  if (blockIdx.x + 1 < gridDim.x) {
    const uint32_t h = blockIdx.x * kPcgBlock + threadIdx.x;
    if (h >= head_count) return;
    const uint32_t u = h < L.head_lo ? h : L.head_hi + (h - L.head_lo);
    if (intrinsics_slot(L, u) >= 0) return;   // written by the last workgroup
    ExactCell* ca = &ex.head_a[h];
    va[u] = invalid ? __builtin_nanf("") : (float)exact_value(ca->limb);
#pragma unroll
    for (int j = 0; j < kExactLimbs; ++j) ca->limb[j] = 0;
    if (kInit) {
      ExactCell* cb = &ex.head_b[h];
      vb[u] = invalid ? __builtin_nanf("") : (float)exact_value(cb->limb);
#pragma unroll
      for (int j = 0; j < kExactLimbs; ++j) cb->limb[j] = 0;
    }
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int task = wave; task < (kInit ? 18 : 10); task += kPcgBlock / 64) {
    if (!kInit && task == 9) {
      // alpha_d = pairs + repeat * epsilon terms (AddAlphaDEpsilonTerms runs once per keyframe in the reference,
      // B/kernel_pcg.cu:1102-1112: the term enters `repeat` times), both exact sums, combined in binary64
      const double pairs = fold_hot(ex, kHotAlphaD, -1, true);
      const double eps = fold_hot(ex, kHotEpsLocal, kHotEpsHead, true);
      if (lane == 0) *alpha_d = invalid ? __builtin_nanf("") : (float)(pairs + eps_repeat * eps);
      continue;
    }
    const int q = task % 9;
    const bool enabled = (q < 5) ? L.optimize_depth_intrinsics : L.optimize_color_intrinsics;
    if (!enabled) continue;
    const double v = fold_hot(ex, (task < 9 ? kHotA : kHotB) + q, -1, true);
    const uint32_t u = (q < 5) ? (L.depth_intr_start + q) : (L.color_intr_start + (q - 5));
    if (lane == 0) (task < 9 ? va : vb)[u] = invalid ? __builtin_nanf("") : (float)v;
  }
}

// ---- the surfel block from the class partials (C > 1, see "DEFINITION of the surfel block") ----------------------------------
// One thread per surfel: entry q = ((p0 + p1) + p2) + ..., classes ascending; entries [0, geom_stride) go to va (r / g), the others
// to vb (M).  After PCGStep1 it runs only while the inner loop has not stopped, like the resolve kernel.
__global__ void __launch_bounds__(kPcgBlock)
pcg_class_combine_kernel(PcgLayout L, PcgClasses pc, uint32_t surfels, float* __restrict__ va, float* __restrict__ vb, const PcgControl* ctl) {
  if (ctl && ctl->stop) return;
  const uint32_t i = blockIdx.x * kPcgBlock + threadIdx.x;
  if (i >= surfels) return;
  const uint32_t gs = (uint32_t)L.geom_stride, gi = L.surfel_start + gs * i;
  for (int q = 0; q < pc.entries; ++q) {
    float t = pcg_class_plane(pc, 0, q)[i];
    for (int c = 1; c < pc.classes; ++c) t += pcg_class_plane(pc, c, q)[i];
    if ((uint32_t)q < gs) va[gi + q] = t;
    else vb[gi + q - gs] = t;
  }
}

// (the exact dot products of the per-unknown kernels: pcg_device.h, BlockExact)
// PCGInit2 (B/kernel_pcg.cu:565-600); also the epsilon terms of the first step's alpha_d (they depend on p alone)
__global__ void __launch_bounds__(kPcgBlock)
pcg_init2_kernel(PcgLayout L, PcgExact ex, float a, const float* __restrict__ r_, const float* __restrict__ M_, float* __restrict__ delta,
                 float* __restrict__ g_, float* __restrict__ p_) {
  __shared__ BlockExact<2> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    g_[u] = 0;
    const float r_value = r_[u] + ((u == L.a_index) ? (-kAPriorWeight * kAPriorWeight * a) : 0);
    const float p_value = r_value / (M_[u] + kDiagEpsilon + prior_at(L, u));
    p_[u] = p_value;
    delta[u] = 0;
    const float dot_term = r_value * p_value;
    const float eps_term = (kDiagEpsilon + prior_at(L, u)) * p_value * p_value;
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

}  // namespace bahip
#endif
BAHIP_FLAVOURED_BEGIN
// ---- PCGStep1: g += J^T W J p, alpha_d += p^T J^T W J p  (B/kernel_pcg.cu:646-1026) -------------------
// Where the (tile, keyframe) totals of the dense head go: straight to the exact accumulators in global memory (two 64-bit integer
// atomics per total, issued one candidate late), or into a copy of the pose block of the head that a persistent workgroup keeps
// in LDS and flushes once (pcg_step1_lds_kernel).  The cfactor-cell entries (one per pair) go to global memory either way.
constexpr int kPcgLdsHotCells = 16;   // of the LDS form's table: [0] alpha_d, [1 .. 9] the nine global intrinsics entries of g; padded
__device__ __forceinline__ uint32_t pcg_lds_hot_index(int slot) { return slot == kHotAlphaD ? 0u : 1u + (uint32_t)(slot - kHotA); }
__device__ __forceinline__ int pcg_lds_hot_slot(uint32_t index) { return index == 0u ? (int)kHotAlphaD : (int)kHotA + (int)index - 1; }
struct PcgGlobalSink {
  PcgExact ex;
  int replica;
  __device__ __forceinline__ void add_pose(uint32_t head_index, float v, int part) const { exact_atomic_add_part_untracked(&ex.head_a[head_index], v, part, ex.invalid); }
  __device__ __forceinline__ void add_hot(int slot, float v, int part) const { exact_atomic_add_part_untracked(hot_cell(ex, slot, replica), v, part, ex.invalid); }
};
struct PcgLdsSink {
  PcgExact ex;
  uint32_t table;        // LDS byte address of the table: ExactCell[pose_cells + kPcgLdsHotCells]
  uint32_t pose_cells;   // 6 per pose unknown: head indices [0, pose_cells)
  __device__ __forceinline__ void add_cell(uint32_t cell, float v, int part) const {
    const ExactSplit sp = exact_split(v);
    if (sp.limb >= 0) {
      const long long addend = part ? sp.hi : sp.lo;
      auto* limb = reinterpret_cast<__attribute__((address_space(3))) long long*>(table + cell * (uint32_t)sizeof(ExactCell) + (uint32_t)(sp.limb + part) * 8u);
      if (addend != 0) __hip_atomic_fetch_add(limb, addend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (sp.limb == -2 && part == 0) {
      atomicOr(ex.invalid, 1u);
    }
  }
  __device__ __forceinline__ void add_pose(uint32_t head_index, float v, int part) const { add_cell(head_index, v, part); }
  __device__ __forceinline__ void add_hot(int slot, float v, int part) const { add_cell(pose_cells + pcg_lds_hot_index(slot), v, part); }
};
// kClassed: as pcg_init_kernel -- the owned classes' chains of the surfel entries of g to the partials of `pc`, g_'s surfel block not written
template <bool kDepthIntr, bool kColorIntr, bool kClassed, typename Sink>
__device__ __forceinline__ void pcg_step1_tile(const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* __restrict__ kfs, int num_kfs,
                                               const SurfelsView& s, const float* __restrict__ p_, float* __restrict__ g_, uint32_t tile, const Sink& sink,
                                               const PcgClasses& pc) {
  const uint32_t i = tile * kPcgSweepBlock + (threadIdx.x & 63);
  const bool in_range = i < s.size;
  const uint32_t ii = in_range ? i : 0;
  const Vec3 gp = surfel_position(s, ii);
  const Vec3 gn = surfel_normal(s, ii);
  const float radius_sq = s.row(kSurfelRadiusSquared)[ii];
  const float d1 = s.row(kSurfelDescriptor1)[ii], d2 = s.row(kSurfelDescriptor2)[ii];
  const TangentPoints tp = surfel_tangent_points(gp, gn, radius_sq);   // per surfel, not per pair
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
  if (!kClassed && L.accumulate && in_range && L.optimize_geometry) {
    gs[0] = g_[gi];
    if (L.geom_stride == 3) { gs[1] = g_[gi + 1]; gs[2] = g_[gi + 2]; }
  }
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
        if (j < 6) { if (pending_pose) sink.add_pose(pending_base + j, pending, part); }
        else if (j == 6) sink.add_hot(kHotAlphaD, pending, part);
        else if (kIntr && j < 16 && ((j - 7) < 5 ? kDepthIntr : kColorIntr)) sink.add_hot(kHotA + (j - 7), pending, part);
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
  const auto may_project = [&](int k) { return sphere_may_project_item(in, kfs[k].pose.F, wb); };
  const auto candidate = [&](int k) {
    pairs.candidate(kfs[k], [&] { return kf_pose_is_unknown(L, k); }, [&] { return kf_pose_index(L, k); }, flush_pending);
  };
  if constexpr (!kClassed) {
    for_each_candidate(num_kfs, may_project, candidate);
    flush_pending();

    if (in_range && L.optimize_geometry) {
      g_[gi] = gs[0];
      if (L.geom_stride == 3) { g_[gi + 1] = gs[1]; g_[gi + 2] = gs[2]; }
    }
    return;
  }
#pragma nounroll
  for (int c = 0; c < pc.classes; ++c) {
    if (!((pc.cp.owned >> c) & 1u)) continue;   // another rank holds this class's images
    for_each_candidate(num_kfs, may_project, candidate, pc.classes, c);
    if (in_range && L.optimize_geometry) {
      pcg_class_plane(pc, c, 0)[i] = gs[0];
      if (L.geom_stride == 3) { pcg_class_plane(pc, c, 1)[i] = gs[1]; pcg_class_plane(pc, c, 2)[i] = gs[2]; }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) gs[q] = 0.f;
  }
  flush_pending();
}

template <bool kDepthIntr, bool kColorIntr, bool kClassed, typename... Classes>   // (kClassed, Classes: as pcg_init_kernel)
__global__ void __launch_bounds__(kPcgSweepBlock) BAHIP_PCG_SWEEP_ATTR
pcg_step1_kernel(PcgLayout L, PcgExact ex, Intrinsics in, const KfEntry* __restrict__ kfs, int num_kfs, SurfelsView s,
                 const float* __restrict__ p_, float* __restrict__ g_, const PcgControl* ctl, const uint32_t* __restrict__ sched,
                 Classes... classes_arg) {
  static_assert(sizeof...(Classes) == (kClassed ? 1 : 0), "a kClassed sweep takes one PcgClasses, the other none");
  if (ctl->stop) return;
  uint32_t tile;   // heavy work first (wave_cull.h: scheduled_tile)
  if (!scheduled_tile(blockIdx.x, gridDim.x - (sched ? kHeavySlots : 0u), sched, &tile)) return;
  const PcgGlobalSink sink{ex, (int)(tile & (kHotReplicas - 1))};
  pcg_step1_tile<kDepthIntr, kColorIntr, kClassed>(L, ex, in, kfs, num_kfs, s, p_, g_, tile, sink, pcg_classes_of(classes_arg...));
}

// Persistent form (round 4), like pose_accumulate_lds_kernel: one workgroup of 16 wavefronts per compute unit keeps the pose
// block of g's dense head -- 6 exact cells per pose unknown, 72 bytes each: 86 KB at 200 keyframes -- and the hot scalars in
// LDS; its wavefronts draw tiles (batches from a counter per XCD, single tiles from a word in LDS) and add their (tile,
// keyframe) totals there; the workgroup adds its non-zero limbs to the global accumulators once.  The one-tile-per-wavefront
// form issued 14 global 64-bit atomics per (tile, keyframe) with an association -- 12 M per inner step at the bench size, half a
// millisecond of the memory side's 23.6 G atomic requests per second behind a 0.8 ms sweep.  Integer sums: the same bits.
constexpr int kPcgLdsWaves = 16;
constexpr uint32_t kPcgLdsBatch = 32;
template <bool kDepthIntr, bool kColorIntr, bool kClassed, typename... Classes>   // (kClassed, Classes: as pcg_init_kernel)
__global__ void __launch_bounds__(64 * kPcgLdsWaves) BAHIP_PCG_SWEEP_ATTR
pcg_step1_lds_kernel(PcgLayout L, PcgExact ex, Intrinsics in, const KfEntry* __restrict__ kfs, int num_kfs, SurfelsView s,
                     const float* __restrict__ p_, float* __restrict__ g_, const PcgControl* ctl, const uint32_t* __restrict__ sched,
                     uint32_t padded_tiles, uint32_t* __restrict__ tile_counters, int parity, uint32_t pose_cells, Classes... classes_arg) {
  static_assert(sizeof...(Classes) == (kClassed ? 1 : 0), "a kClassed sweep takes one PcgClasses, the other none");
  extern __shared__ long long pcg_table[];   // ExactCell[pose_cells + kPcgLdsHotCells], then the batch word
  if (blockIdx.x == 0 && threadIdx.x < 8) tile_counters[(parity ^ 1) * 8 + threadIdx.x] = 0;
  if (ctl->stop) return;
  const int lane = threadIdx.x & 63;
  const uint32_t cells = pose_cells + kPcgLdsHotCells, words = cells * kExactLimbs;
  unsigned long long& batch_state = *reinterpret_cast<unsigned long long*>(pcg_table + words);
  const uint32_t xcd = blockIdx.x & 7u, per_xcd = sched_positions(padded_tiles, sched) >> 3;
  uint32_t* counter = tile_counters + parity * 8 + xcd;
  for (uint32_t e = threadIdx.x; e < words; e += blockDim.x) pcg_table[e] = 0;
  if (threadIdx.x == 0) batch_state = ((unsigned long long)atomicAdd(counter, kPcgLdsBatch) << 32) | ((unsigned long long)kPcgLdsBatch << 24);
  __syncthreads();
  const PcgLdsSink sink{ex, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) long long*)pcg_table, pose_cells};
  for (;;) {
    unsigned long long taken = 0;
    if (lane == 0) taken = atomicAdd(&batch_state, 1ull);
    const uint32_t first = __builtin_amdgcn_readfirstlane((uint32_t)(taken >> 32));
    const uint32_t size = __builtin_amdgcn_readfirstlane((uint32_t)taken >> 24);
    const uint32_t index = __builtin_amdgcn_readfirstlane((uint32_t)taken & 0xffffffu);
    if (first >= per_xcd) break;
    if (index < size) {
      uint32_t tile;
      if (first + index < per_xcd && scheduled_tile((first + index) * 8u + xcd, padded_tiles, sched, &tile))
        pcg_step1_tile<kDepthIntr, kColorIntr, kClassed>(L, ex, in, kfs, num_kfs, s, p_, g_, tile, sink, pcg_classes_of(classes_arg...));
    } else if (index == size) {
      if (lane == 0) {
        const uint32_t left = per_xcd > first + size ? per_xcd - (first + size) : 0u;
        const uint32_t want = min(kPcgLdsBatch, max(2u, left / (4u * (gridDim.x >> 3))));
        const uint32_t next = atomicAdd(counter, want);
        __hip_atomic_store(&batch_state, ((unsigned long long)next << 32) | ((unsigned long long)want << 24), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    } else {
      while ((uint32_t)(__hip_atomic_load(&batch_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> 32) == first)
        __builtin_amdgcn_s_sleep(8);
    }
  }
  __syncthreads();
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (uint32_t e = threadIdx.x; e < words; e += blockDim.x) {
    const long long v = pcg_table[e];
    if (v != 0) {
      const uint32_t cell = e / kExactLimbs, limb = e - cell * kExactLimbs;
      if (cell >= pose_cells + 10u) continue;   // (padding)
      ExactCell* target = cell < pose_cells ? &ex.head_a[cell] : hot_cell(ex, pcg_lds_hot_slot(cell - pose_cells), replica);
      limb_atomic_add(&target->limb[limb], v);
    }
  }
}

BAHIP_FLAVOURED_END
#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
// PCGStep2 (B/kernel_pcg.cu:1117-1158)
__global__ void __launch_bounds__(kPcgBlock)
pcg_step2_kernel(PcgLayout L, PcgExact ex, float* __restrict__ r_, const float* __restrict__ M_, float* __restrict__ delta,
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
    float r_value = r_[u];
    r_value -= alpha * (g_[u] + (kDiagEpsilon + prior_at(L, u)) * p_value);
    r_[u] = r_value;
    const float z_value = r_value / (M_[u] + kDiagEpsilon + prior_at(L, u));
    g_[u] = z_value;
    const float term = z_value * r_value;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotDotHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotDotLocal};
  block_exact_flush(acc, ex, slots);
}

// PCGStep3 (B/kernel_pcg.cu:1212-1226), and the epsilon terms of the next step's alpha_d from the new p
// (AddAlphaDEpsilonTerms, B/kernel_pcg.cu:1028-1050)
__global__ void __launch_bounds__(kPcgBlock)
pcg_step3_kernel(PcgLayout L, PcgExact ex, const float* __restrict__ g_, float* __restrict__ p_, const float* alpha_n, const float* beta_n,
                 const PcgControl* ctl) {
  if (ctl->stop) return;
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  const float an = *alpha_n;
  const float beta = (an >= 1e-35f) ? (*beta_n / an) : 0;
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    const float pv = g_[u] + beta * p_[u];
    p_[u] = pv;
    const float term = (kDiagEpsilon + prior_at(L, u)) * pv * pv;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotEpsHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotEpsLocal};
  block_exact_flush(acc, ex, slots);
}
// the epsilon terms alone (per-stage entry points: a caller's PCGStep1 sees a p that no step 3 of ours produced)
__global__ void __launch_bounds__(kPcgBlock)
pcg_eps_terms_kernel(PcgLayout L, PcgExact ex, const float* __restrict__ p_) {
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (uint32_t u = blockIdx.x * kPcgBlock + threadIdx.x; u < L.unknown_count; u += gridDim.x * kPcgBlock) {
    const float pv = p_[u];
    const float term = (kDiagEpsilon + prior_at(L, u)) * pv * pv;
    if (is_local(L, u)) block_exact_add(acc, 0, term, ex.invalid);
    else exact_atomic_add(hot_cell(ex, kHotEpsHead, replica), term, ex.invalid);
  }
  const int slots[1] = {kHotEpsLocal};
  block_exact_flush(acc, ex, slots);
}

// UpdateSurfelsFromPCGDelta (B/kernel_pcg.cu:1306-1331)
__global__ void __launch_bounds__(kPcgBlock)
pcg_update_surfels_kernel(PcgLayout L, SurfelsView s, const float* __restrict__ delta) {
  const uint32_t i = blockIdx.x * kPcgBlock + threadIdx.x;
  if (i >= s.size) return;
  pcg_update_surfel(L, s, delta, i);
}

// UpdateCFactorsFromPCGDelta (B/kernel_pcg.cu:1361-1373)
__global__ void __launch_bounds__(kPcgBlock)
pcg_update_cfactors_kernel(Intrinsics in, uint32_t start, const float* __restrict__ delta, float* cfactor, uint32_t pitch) {
  const int idx = blockIdx.x * kPcgBlock + threadIdx.x;
  if (idx >= in.cf_width * in.cf_height) return;
  const int y = idx / in.cf_width, x = idx - y * in.cf_width;
  *pitched_ptr(cfactor, pitch, y, x) += delta[start + idx];
}

// ---- test hook: the exact sum of n binary32 values through the same device code paths ------------------------------------------
// mode 0: every term with exact_atomic_add into one of 64 replicas; mode 1: through the per-thread columns in workgroup memory
// and block_exact_flush, as the per-unknown kernels do.  The result is the binary64 value fold_hot + exact_value produce.
__global__ void __launch_bounds__(kPcgBlock) exact_sum_debug_kernel(PcgExact ex, const float* __restrict__ v, size_t n, int mode) {
  __shared__ BlockExact<1> acc;
  block_exact_clear(acc);
  const int replica = (int)(blockIdx.x & (kHotReplicas - 1));
  for (size_t i = (size_t)blockIdx.x * kPcgBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kPcgBlock) {
    if (mode == 0) exact_atomic_add(hot_cell(ex, kHotDotHead, replica), v[i], ex.invalid);
    else block_exact_add(acc, 0, v[i], ex.invalid);
  }
  const int slots[1] = {kHotDotLocal};
  block_exact_flush(acc, ex, slots);
}
__global__ void __launch_bounds__(64) exact_sum_debug_resolve_kernel(PcgExact ex, double* out) {
  const double v = fold_hot(ex, kHotDotLocal, kHotDotHead, true);
  if (threadIdx.x == 0) *out = (*ex.invalid) ? __builtin_nan("") : v;
}
void launch_exact_sum_debug(hipStream_t st, const PcgExact& ex, const float* values, size_t n, int mode, double* out) {
  const unsigned blocks = n ? (unsigned)((n + kPcgBlock - 1) / kPcgBlock < 512 ? (n + kPcgBlock - 1) / kPcgBlock : 512) : 1u;
  hipLaunchKernelGGL(exact_sum_debug_kernel, dim3(blocks), dim3(kPcgBlock), 0, st, ex, values, n, mode);
  hipLaunchKernelGGL(exact_sum_debug_resolve_kernel, dim3(1), dim3(64), 0, st, ex, out);
}

}  // namespace bahip
#endif
namespace bahip {
// ---- launchers -----------------------------------------------------------------------------------------------
static inline unsigned gU(uint32_t n) { return (n + kPcgBlock - 1) / kPcgBlock; }
static inline unsigned gR(uint32_t n) { return gU(n) < kPcgReduceBlocks ? gU(n) : kPcgReduceBlocks; }

// whole XCD chunks, as in kernels_surfel.hip (xcd_chunked_tile)
static inline unsigned gS(uint32_t n) { return xcd_padded_tiles((n + kPcgSweepBlock - 1) / kPcgSweepBlock); }

}  // namespace bahip
#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
size_t pcg_exact_cells(uint32_t head_count) { return (size_t)kHotSlots * kHotReplicas + 2 * (size_t)head_count + 1; }
PcgExact pcg_exact_view(void* buffer, uint32_t head_count) {
  PcgExact ex;
  ExactCell* base = static_cast<ExactCell*>(buffer);
  ex.hot = base;
  ex.head_a = base + (size_t)kHotExchanged1 * kHotReplicas;
  ex.head_b = ex.head_a + head_count;
  ex.invalid = reinterpret_cast<unsigned*>(ex.head_b + head_count);   // a whole cell: the first word of what exchange 2 carries
  ex.hot_tail = ex.head_b + head_count + 1;
  return ex;
}

}  // namespace bahip
#endif
BAHIP_FLAVOURED_BEGIN
template <bool kClassed, typename... Classes>
static void launch_pcg_init_sweep(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                                  const SurfelsView& s, float* r, float* M, uint32_t* tile_cost, const uint32_t* sched, Classes... cls) {
  const dim3 grid(sched_positions(gS(s.size), sched)), block(kPcgSweepBlock);
  const bool di = L.optimize_depth_intrinsics, ci = L.optimize_color_intrinsics;
  if (di && ci) hipLaunchKernelGGL((pcg_init_kernel<true, true, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, cls...);
  else if (di) hipLaunchKernelGGL((pcg_init_kernel<true, false, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, cls...);
  else if (ci) hipLaunchKernelGGL((pcg_init_kernel<false, true, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, cls...);
  else hipLaunchKernelGGL((pcg_init_kernel<false, false, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, cls...);
}
void launch_pcg_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                     const SurfelsView& s, float* r, float* M, uint32_t* tile_cost, const uint32_t* sched, const PcgClasses* classes) {
  if (!s.size) return;
  if (!classes) launch_pcg_init_sweep<false>(st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched);
  else launch_pcg_init_sweep<true>(st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, *classes);
}
BAHIP_FLAVOURED_END
#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
static inline unsigned resolve_grid(const PcgLayout& L) { return gU(L.head_lo + (L.unknown_count - L.head_hi)) + 1; }
void launch_pcg_resolve_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* r, float* M) {
  hipLaunchKernelGGL((pcg_resolve_kernel<true>), dim3(resolve_grid(L)), dim3(kPcgBlock), 0, st, L, ex, r, M, nullptr, 0.0, nullptr);
}
void launch_pcg_resolve_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* g, float* alpha_d, double eps_repeat, const void* ctl) {
  hipLaunchKernelGGL((pcg_resolve_kernel<false>), dim3(resolve_grid(L)), dim3(kPcgBlock), 0, st, L, ex, g, nullptr, alpha_d, eps_repeat,
                     static_cast<const PcgControl*>(ctl));
}
void launch_pcg_init2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float a, const float* r, const float* M, float* delta, float* g,
                      float* p) {
  if (L.unknown_count) hipLaunchKernelGGL(pcg_init2_kernel, dim3(gR(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, a, r, M, delta, g, p);
}
void launch_pcg_class_combine(hipStream_t st, const PcgLayout& L, const PcgClasses& classes, uint32_t surfels, float* va, float* vb, const void* ctl) {
  if (surfels) hipLaunchKernelGGL(pcg_class_combine_kernel, dim3(gU(surfels)), dim3(kPcgBlock), 0, st, L, classes, surfels, va, vb,
                                  static_cast<const PcgControl*>(ctl));
}
void launch_pcg_control_init(hipStream_t st, const PcgExact& ex, void* ctl, float* alpha_n) {
  hipLaunchKernelGGL(pcg_control_init_kernel, dim3(1), dim3(64), 0, st, ex, static_cast<PcgControl*>(ctl), alpha_n);
}
void launch_pcg_control(hipStream_t st, const PcgExact& ex, void* ctl, float* beta_n) {
  hipLaunchKernelGGL(pcg_control_kernel, dim3(1), dim3(64), 0, st, ex, static_cast<PcgControl*>(ctl), beta_n);
}
size_t pcg_control_bytes() { return sizeof(PcgControl); }

}  // namespace bahip
#endif
BAHIP_FLAVOURED_BEGIN
static int g_pcg_lds_form = bahip_env_int("BAHIP_PCG_LDS", 1);   // 0: always the one-tile-per-wavefront form
void set_pcg_lds_form(int mode) { g_pcg_lds_form = (mode >= 0 && mode <= 2) ? mode : 1; }   // 2: also on grids that do not fill the chip (tests)
constexpr size_t kPcgLdsTableLimit = 128 * 1024;
template <bool kDepthIntr, bool kColorIntr, bool kClassed, typename... Classes>
static bool launch_pcg_step1_lds(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                                 const SurfelsView& s, const float* p, float* g, const PcgControl* ctl, const uint32_t* sched,
                                 uint32_t* tile_counters, int* parity_inout, Classes... cls) {
  // the pose block of the unknown vector (and of the dense head: head index = unknown index there) ends where the next block begins
  uint32_t pose_end = L.unknown_count;
  if (L.optimize_geometry) pose_end = std::min(pose_end, L.surfel_start);
  if (L.optimize_depth_intrinsics) pose_end = std::min(pose_end, L.depth_intr_start);
  if (L.optimize_color_intrinsics) pose_end = std::min(pose_end, L.color_intr_start);
  const uint32_t pose_cells = L.optimize_poses ? pose_end : 0u;
  const size_t bytes = ((size_t)pose_cells + kPcgLdsHotCells) * sizeof(ExactCell) + sizeof(long long);
  if (bytes > kPcgLdsTableLimit) return false;
  static bool raised[64] = {}, failed[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!raised[dev] && !failed[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&pcg_step1_lds_kernel<kDepthIntr, kColorIntr, kClassed, Classes...>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kPcgLdsTableLimit) == hipSuccess) raised[dev] = true;
    else { failed[dev] = true; (void)hipGetLastError(); }
  }
  if (failed[dev] && bytes > 64 * 1024) return false;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
  const unsigned tiles = gS(s.size);
  const unsigned grid = std::max(8u, std::min((unsigned)cus, ((sched_positions(tiles, sched) + kPcgLdsWaves - 1) / kPcgLdsWaves + 7u) & ~7u));
  const int parity = *parity_inout;
  *parity_inout = parity ^ 1;
  hipLaunchKernelGGL((pcg_step1_lds_kernel<kDepthIntr, kColorIntr, kClassed, Classes...>), dim3(grid), dim3(64 * kPcgLdsWaves), bytes, st, L, ex, in, kfs, num_kfs,
                     s, p, g, ctl, sched, tiles, tile_counters, parity, pose_cells, cls...);
  return true;
}

// launches of the step-1 sweep by form since the process started: [0] one tile per wavefront, [1] persistent with the pose block in LDS
static long long g_pcg_step1_form_launches[2] = {0, 0};
void pcg_step1_form_launches(long long out[2]) { out[0] = g_pcg_step1_form_launches[0]; out[1] = g_pcg_step1_form_launches[1]; }
template <bool kClassed, typename... Classes>
static void launch_pcg_step1_sweep(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                                   const SurfelsView& s, const float* p, float* g, const PcgControl* ctl, const uint32_t* sched, uint32_t* tile_counters,
                                   int* parity_inout, Classes... cls) {
  const bool di = L.optimize_depth_intrinsics, ci = L.optimize_color_intrinsics;
  // the persistent LDS form when the grid fills the chip, the per-keyframe entry points (Route B) are not in play and the pose
  // block of the head fits the table
  if (tile_counters && parity_inout && L.single_keyframe < 0 && (g_pcg_lds_form == 2 || (g_pcg_lds_form == 1 && gS(s.size) >= 8192))) {
    bool launched;
    if (di && ci) launched = launch_pcg_step1_lds<true, true, kClassed>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, cls...);
    else if (di) launched = launch_pcg_step1_lds<true, false, kClassed>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, cls...);
    else if (ci) launched = launch_pcg_step1_lds<false, true, kClassed>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, cls...);
    else launched = launch_pcg_step1_lds<false, false, kClassed>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, cls...);
    if (launched) { ++g_pcg_step1_form_launches[1]; return; }
  }
  ++g_pcg_step1_form_launches[0];
  const dim3 grid(sched_positions(gS(s.size), sched)), block(kPcgSweepBlock);
  if (di && ci) hipLaunchKernelGGL((pcg_step1_kernel<true, true, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, cls...);
  else if (di) hipLaunchKernelGGL((pcg_step1_kernel<true, false, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, cls...);
  else if (ci) hipLaunchKernelGGL((pcg_step1_kernel<false, true, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, cls...);
  else hipLaunchKernelGGL((pcg_step1_kernel<false, false, kClassed, Classes...>), grid, block, 0, st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, cls...);
}
void launch_pcg_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                      const SurfelsView& s, const float* p, float* g, const void* ctl_, const uint32_t* sched, uint32_t* tile_counters,
                      int* parity_inout, const PcgClasses* classes) {
  const PcgControl* ctl = static_cast<const PcgControl*>(ctl_);
  if (!s.size) return;
  if (!classes) launch_pcg_step1_sweep<false>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout);
  else launch_pcg_step1_sweep<true>(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, *classes);
}
BAHIP_FLAVOURED_END
#ifndef BAHIP_FAST_MATH   // exists once (the exact unit)
namespace bahip {
void launch_pcg_eps_terms(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const float* p) {
  if (L.unknown_count) hipLaunchKernelGGL(pcg_eps_terms_kernel, dim3(gR(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, p);
}
void launch_pcg_step2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* r, const float* M, float* delta, float* g, const float* p,
                      const float* alpha_n, const float* alpha_d, const void* ctl) {
  if (L.unknown_count) hipLaunchKernelGGL(pcg_step2_kernel, dim3(gR(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, r, M, delta, g, p, alpha_n, alpha_d,
                                          static_cast<const PcgControl*>(ctl));
}
void launch_pcg_step3(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const float* g, float* p, const float* alpha_n, const float* beta_n,
                      const void* ctl) {
  if (L.unknown_count) hipLaunchKernelGGL(pcg_step3_kernel, dim3(gR(L.unknown_count)), dim3(kPcgBlock), 0, st, L, ex, g, p, alpha_n, beta_n,
                                          static_cast<const PcgControl*>(ctl));
}
void launch_pcg_update_surfels(hipStream_t st, const PcgLayout& L, const SurfelsView& s, const float* delta) {
  if (s.size) hipLaunchKernelGGL(pcg_update_surfels_kernel, dim3(gU(s.size)), dim3(kPcgBlock), 0, st, L, s, delta);
}
void launch_pcg_update_cfactors(hipStream_t st, const Intrinsics& in, uint32_t start, const float* delta, float* cfactor, uint32_t pitch) {
  hipLaunchKernelGGL(pcg_update_cfactors_kernel, dim3(gU(in.cf_width * in.cf_height)), dim3(kPcgBlock), 0, st, in, start, delta, cfactor, pitch);
}


// dispatchers (ba_launch.h: "Two arithmetic flavours")
void launch_pcg_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                     const SurfelsView& s, float* r, float* M, uint32_t* tile_cost, const uint32_t* sched, const PcgClasses* classes) {
  BAHIP_PICK(in, launch_pcg_init(st, L, ex, in, kfs, num_kfs, s, r, M, tile_cost, sched, classes));
}
void launch_pcg_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                      const SurfelsView& s, const float* p, float* g, const void* ctl, const uint32_t* sched, uint32_t* tile_counters,
                      int* parity_inout, const PcgClasses* classes) {
  BAHIP_PICK(in, launch_pcg_step1(st, L, ex, in, kfs, num_kfs, s, p, g, ctl, sched, tile_counters, parity_inout, classes));
}
void set_pcg_lds_form(int mode) { exact::set_pcg_lds_form(mode); fast::set_pcg_lds_form(mode); }
void pcg_step1_form_launches(long long out[2]) {
  long long a[2], b[2];
  exact::pcg_step1_form_launches(a); fast::pcg_step1_form_launches(b);
  out[0] = a[0] + b[0]; out[1] = a[1] + b[1];
}
}  // namespace bahip
#endif
