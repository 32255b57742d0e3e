// pose_device.h -- what the sweeps and the solve kernels of the pose phase share between kernels_pose.hip (the plain Gauss-Newton phase)
// and kernels_pose_trial.hip (the phase under step control): the tile body of every sweep (pose_tile, with the per-pair policy that
// lets the controlled sweep add its cost row), the accumulation chain of the normal equations, the LDS sink of the persistent forms,
// the 6x6 solve and the convergence test.  The kernels, the launchers and GlobalSink (the sink of the one-tile-per-wavefront form)
// stay in kernels_pose.hip, the cost policy in kernels_pose_trial.hip.  Every function here is inlined into its callers.
#pragma once

#include "ba_device.h"
#include "ba_launch.h"
#include "se3_device.h"
#include "wave_cull.h"
#include "wave_reduce.h"

namespace bahip {
constexpr int kPoseBlock = 64;    // one wavefront per workgroup: no LDS, no barriers, and finished waves free their slot at once
// Where a sweep reports a tile total it could not represent (hb_split): the low word of the unused 28th coefficient of work item
// 0's row -- inside the buffer the ranks of a sharded run exchange, so that after the exchange EVERY rank's solve launch sees the
// flag and every host fails the call alike (a flag in the rank's own counter record let the other ranks run on).
__host__ __device__ inline int* pose_invalid_word(HbFixed* Hb) { return reinterpret_cast<int*>(Hb + 27 * kHbLimbs); }
// The list of the work items still iterating that the plain phase keeps: behind the counter records of the work table (ba_device.h: pose_work_records).
__device__ __forceinline__ const int* pose_work_list(const PoseWork* work, int num_work) { return reinterpret_cast<const int*>(work + num_work + kPoseTailRecords); }
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

// What pose_tile does per (tile, work item) pair besides H, b.  The plain sweeps: nothing -- every hook is empty and the cull
// reads the kernel's own intrinsics.  (The depth hook takes `visible` as an argument: called under `if (visible)` an EMPTY hook
// still changed the code of three plain kernels per flavour.)
struct NoPairTerms {
  __device__ __forceinline__ const Intrinsics& cull_intrinsics(const Intrinsics& in) const { return in; }
  __device__ __forceinline__ void begin(int /*item*/) {}                              // a pair with at least one associated lane
  __device__ __forceinline__ void depth(bool /*visible*/, float /*raw*/) {}           // every lane; raw is 0 where not visible
  __device__ __forceinline__ void descriptors(const DescEval&) {}                     // lanes whose colour pixel is valid
  __device__ __forceinline__ void end(unsigned long long /*associated*/) {}           // every lane, before the reduction
};

#ifdef BAHIP_COUNT_CANDIDATES
// experiment build only: (surfel tile, keyframe) candidates the cull lets through / with at least one associated lane / lanes
static __device__ unsigned long long g_candidate_counters[4];
#endif
#ifdef BAHIP_TILE_TIMELINE
// experiment build only: candidates visited / with an association per tile of the last FULL round (kernels_pose.hip: g_pose_timeline)
static __device__ unsigned int g_pose_tile_stats[65536][2];
#endif

// One 64-surfel tile against the work items still iterating (every `parts`-th of them, starting at `part`).
//
// tile_bounds: one bounding sphere per 64-surfel tile.  The first Gauss-Newton round of a pose phase (stored_bounds == 0)
// computes them from the positions and stores them; the later rounds -- which iterate only the few keyframes that have not
// converged, yet launch one wavefront (or several) per tile all the same -- read the sphere back (one scalar load), test it
// against the remaining work items and return at once if none can see the tile, before any surfel is loaded.  Positions do
// not change between the rounds of a phase, so the stored sphere is the one that would be recomputed.
//
// Later rounds (stored_bounds): the items are the num_listed entries of `listed` -- the work items still iterating -- instead
// of all num_work work items (`listed` is not looked at in the first round).  A launch may cover a slice of the items only
// ([item_begin, item_begin + item_count): the LDS forms cut lists longer than their table); `item` below counts from the
// slice's start.
template <bool kUseDepth, bool kUseDesc, typename Sink, typename Terms = NoPairTerms>
__device__ __forceinline__ void pose_tile(const Intrinsics& in, const KfEntry* __restrict__ frames, const PoseWork* __restrict__ work,
                                          const int* __restrict__ listed, int num_work, const SurfelsView& s,
                                          WaveBounds* __restrict__ tile_bounds, int stored_bounds, int num_listed, uint32_t tile, int parts,
                                          int part, Sink& sink, uint32_t* __restrict__ tile_cost, int item_begin = 0, int item_count = -1,
                                          Terms terms = Terms()) {
  const int lane = threadIdx.x & 63;
  listed += item_begin;
  const int num_items = item_count >= 0 ? item_count : (stored_bounds ? num_listed : num_work);
  auto work_item_of = [&](int item) { return stored_bounds ? load_global(listed + item) : item_begin + item; };
  WaveBounds wb;
  if (stored_bounds) {
    wb = tile_bounds[tile];     // wave-uniform address: scalar loads
    if (wb.r < 0.f) return;
    bool any = false;
    for (int base = part; base < num_items && !any; base += 64 * parts) {
      const int item = base + lane * parts;
      bool sees = false;
      if (item < num_items) {
        float f[12];
        load_candidate(work[work_item_of(item)].F, nullptr, f, nullptr);
        sees = sphere_may_project(terms.cull_intrinsics(in), f, wb);
      }
      any = __any(sees) != 0;
    }
    if (!any) return;
  }
  const TileSurfel t = load_tile_surfel<kUseDesc>(s, tile, lane);
  const bool in_range = t.in_range;
  const Vec3 gp = t.gp, gn = t.gn;

  // Only the work items whose frustum can contain this wavefront's surfels are visited (wave_cull.h).
  if (!stored_bounds) {
    wb = wave_bounds(gp, in_range && (gp.x == gp.x));
    if (part == 0 && lane == 0) tile_bounds[tile] = wb;
  }
  int my_w = 0;   // the work item of this lane's candidate item in the current chunk of 64 (read back by lane in the body)
#ifdef BAHIP_TILE_TIMELINE
  uint32_t with_association = 0;
#endif
  uint32_t visited = 0;   // wave-uniform: candidates this wavefront visits = what the tile costs (feeds tile_order_kernel)
  for_each_candidate(
      num_items,
      [&](int item) {
        const int w = work_item_of(item);
        my_w = w;
        float f[12];
        int32_t done;
        load_candidate(work[w].F, &work[w].skip, f, &done);   // skip = done, or the keyframe's images live on another rank
        return !done && sphere_may_project(terms.cull_intrinsics(in), f, wb);
      },
      [&](int item) {
    // item = base + lane' * parts for the lane' that tested it: its w comes from that lane's register, not from memory
    // (a list lookup here was a dependent load and a wait at the top of every candidate of the later rounds)
    const int w = __builtin_amdgcn_readfirstlane(stored_bounds ? __builtin_amdgcn_readlane(my_w, ((item - part) / parts) & 63) : item_begin + item);
    const float* F = work[w].F;
    ++visited;
    // (the entry of the frame table that provides the images: today every writer binds work item w to entry w, but the field is what
    // pose_solve honours too, and reading frames[w] directly measured no gain over this dependent scalar load: ADVICE r5)
    const KfEntry& kf = frames[__builtin_amdgcn_readfirstlane(load_global(&work[w].kf_index))];
    // every gather of the pair goes out before the first one is waited for (ba_device.h: project_surfel)
    const Projected p = project_surfel(in, F, gp);
    const PixelWords pix = load_pixel_words(in, kf.geom, p);
    DescWords dw;
    if (kUseDesc) dw = load_descriptor_words(in, kf.lumafp, F, t.tp, p);   // (issued after the association instead: pose sweep +7 %)
    Assoc r;
    const bool visible = in_range && associate_from_words<false>(in, F, gn, p, pix, &r, nullptr);
    // every gather has arrived from here on, on every path (a load still pending at the loop's back edge would make the
    // compiler wait for it - and, vmcnt being in-order, for the atomics behind it - at the top of the next candidate)
    if (kUseDesc) gathers_arrived(pix, dw);
    else gathers_arrived(pix);
    sink.gathers_done();
    const unsigned long long associated = __builtin_amdgcn_ballot_w64(visible);   // (a scalar compare on the mask; __any costs a select and a compare per lane)
#ifdef BAHIP_COUNT_CANDIDATES
    if (!stored_bounds && lane == 0) {
      atomicAdd(&g_candidate_counters[0], 1ull);
      atomicAdd(&g_candidate_counters[1], associated ? 1ull : 0ull);
      atomicAdd(&g_candidate_counters[2], (unsigned long long)__popcll(associated));
    }
#endif
    if (associated == 0ull) return;
#ifdef BAHIP_TILE_TIMELINE
    ++with_association;
#endif
    terms.begin(item);

    float acc[28];   // 21 H + 6 b + 1 pad (kHbCoefficients)
    // The depth residual opens the 27 sums as plain products, in every lane: a lane without an association computes on whatever its
    // Assoc holds (no memory is touched), and eight selects then give it J = 0, weight 0, residual 0, so that its products are
    // zeros -- instead of 27 cleared accumulators + 27 fused multiply-adds onto them under the lanes' mask.  Same bits where it
    // matters: fma(a, b, +0) and a * b differ in the sign of a zero product only, a zero addend never changes a non-zero sum, and a
    // total that is a zero of either sign is the fixed-point 0 (hb_split).  (Not applicable to the lanes' garbage directly: their
    // Jacobians may be infinite or NaN, and 0 * inf is not 0.)
    if (kUseDepth) {
      float J[6];
      const float inv_std = assoc_inv_std(in, r);
      const Vec3 u = assoc_unproject(r);
      float raw = inv_std * dot3(r.nl, u - r.local);
      jac_depth_pose(r.nl, u, inv_std, J);
      float wgt = depth_residual_weight(raw);
#pragma unroll
      for (int c = 0; c < 6; ++c) J[c] = visible ? J[c] : 0.f;
      wgt = visible ? wgt : 0.f;
      raw = visible ? raw : 0.f;
      int q = 0;
#pragma unroll
      for (int row = 0; row < 6; ++row) {
        const float wj = wgt * J[row];
#pragma unroll
        for (int col = row; col < 6; ++col, ++q) acc[q] = wj * J[col];
      }
      const float wr = wgt * raw;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[21 + c] = wr * J[c];
      acc[27] = 0.f;
      terms.depth(visible, raw);   // (behind the products, where `raw` dies)
    } else {
#pragma unroll
      for (int q = 0; q < 28; ++q) acc[q] = 0.f;
    }

    if (visible) {
      float J[6];
      if (kUseDesc) {
        // B/kernel_opt_pose.cu:303-353: nothing is added when the colour-pixel transform fails.
        if (dw.color_ok) {
          DescEval e;
          eval_descriptor_from_words(in, kf.lumafp, dw, t.d1, t.d2, &e);
          // B/kernel_opt_pose.cu:96-142
          const Vec3 ls = r.local;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const float gx = (t ? e.gx2 : e.gx1) * in.cfx;
            const float gy = (t ? e.gy2 : e.gy1) * in.cfy;
            const float raw = t ? e.r2 : e.r1;
            jac_descriptor_pose(ls, r.inv_z, gx, gy, J);
            const float wgt = descriptor_residual_weight(raw);
            accumulate_jtj(acc, J, wgt, raw);
          }
          terms.descriptors(e);   // (behind the Jacobians, whose registers are free again)
        }
      }
    }
    terms.end(associated);

    // wave64 halving reduction (wave_reduce.h: a fixed tree over the 64 lanes), then two 64-bit integer adds per scalar
    // per wave on the fixed-point limbs: order-free, hence deterministic
    float total = wave_reduce28(acc, lane);
    // The cross-lane steps of the reduction must run with every lane enabled: a DPP / permlane source lane that EXEC has
    // switched off reads as zero.  The totals are consumed under `this lane holds one` (27 lanes), and the compiler sank the
    // last DPP add into that branch -- rows of the LDS table then received totals that lacked their odd neighbour's half.
    // The empty asm pins the finished value in uniform control flow.
    asm volatile("" : "+v"(total));
    sink.add(item, w, total);
  }, parts, part);
  sink.finish();
  // first round of a phase over the keyframe table: the tile's cost for the run order of the next launches (wave_cull.h)
  if (tile_cost && !stored_bounds && lane == 0 && visited) atomicAdd(&tile_cost[tile], visited);
#ifdef BAHIP_TILE_TIMELINE
  if (!stored_bounds && lane == 0 && tile < 65536) { g_pose_tile_stats[tile][0] = visited; g_pose_tile_stats[tile][1] = with_association; }
#endif
}

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
