// kernels_rcs.hip -- the reduced camera system: the 6K x 6K matrix S and the vector g that remain of the Gauss-Newton system over the
// bound keyframes' poses and the surfels when every surfel's unknowns are eliminated (bahip_reduced_camera_system, capi_rcs.hip;
// DESIGN.md section 3, "The reduced camera system").
//
// DEFINITION.  The pairs (surfel, keyframe) are those of the cost sweep (cost_device.h: cost_pairs -- the production association rule, a
// finite position, activation flags ignored), their words those of eval_pair_terms (pcg_device.h).  Per surfel, in binary32, one chain
// per word over its keyframes in ascending order: the eight sums of the geometry step (kernels_surfel.hip: a0 .. a8), C = sums + 1e-6
// on the diagonal, its in-place Cholesky factor L and z = L^-1 c, spelled as the geometry step spells them; without descriptors
// L = sqrtf(a0 + 1e-6f), z = a6 / L.  A surfel whose factor holds a non-finite word or a pivot that is not positive is degenerate: it
// is counted and not eliminated.  Per pair E (6 x m, m = 3 with descriptors, else 1):
//   E[i][0] = mad(w2 Jg2, Jp2[i], mad(w1 Jg1, Jp1[i], (w Jgeom) Jpose[i])),  E[i][1] = -(w1 Jp1[i]),  E[i][2] = -(w2 Jp2[i])
// (the descriptor words only where the colour pixel is valid, the depth word only with the depth term), and Y = E L^-T by forward
// substitution row by row.  Then
//   M_kl[i][j] = sum over the surfels of mad(Y_k[i][2], Y_l[j][2], mad(Y_k[i][1], Y_l[j][1], Y_k[i][0] Y_l[j][0])),
//   v_k[i]     = sum over the surfels of the same chain of Y_k[i][c] z[c],
// a DEFINED sum, with the definition of the pose equations (ba_device.h: HbFixed): the lanes of a 64-surfel tile by the fixed tile tree
// (wave_reduce.h), the tile totals in the two-limb fixed point, added as integers.  Launch shape, tile order, list capacity and the
// order the atomics arrive in cannot move a word; surfel shards are summed as integers.
//
// THE SWEEP.  One wavefront per tile.  A first traversal of the tile's keyframes forms the sums, L and z in registers.  The second is
// the co-visibility traversal (kernels_covisibility.hip): per keyframe with a non-zero ballot an entry (k, mask, Y) goes to the
// wavefront's list in LDS -- Y as [word][lane] --, and v_k is added.  After the traversal the pairs a <= b of the list whose masks meet
// are formed: 36 lane products (for a = b the 21 with i <= j are added), reduced by three halving butterflies, the totals split into limbs
// by the lanes that hold them and added with 64-bit atomics that return nothing to block (k_b, k_a) of the lower triangle.  A tile with
// more entries than the list is walked in passes, as there: pass p lists the entries p * capacity .. (p + 1) * capacity - 1 and pairs
// every later entry, Y in registers, with the whole list as it is met.
//
// The unit exists once, built with -ffp-contract=off: a context set to the fast flavour launches the same code.
#include <algorithm>

#include "ba_device.h"
#include "ba_launch.h"
#include "pcg_device.h"
#include "rcs_launch.h"
#include "wave_cull.h"

#ifndef BAHIP_FAST_MATH   // exists once (the exact unit); there is no fast flavour of this unit
#pragma clang fp contract(off)
namespace bahip {

namespace {
using namespace exact;

__device__ __forceinline__ void rcs_limb_add(long long* __restrict__ cell, float total, bool* invalid) {
  const HbSplit sp = hb_split(total);
  if (!sp.valid) { *invalid = true; return; }
  __hip_atomic_fetch_add(cell + 0, sp.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(cell + 1, sp.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a word every lane read from one LDS address, as the scalar it is: the branches on it stay uniform for the compiler, so that no
// cross-lane operation of the butterflies lands in a divergent region
__device__ __forceinline__ uint32_t rcs_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long rcs_uniform(unsigned long long v) {
  return ((unsigned long long)rcs_uniform((uint32_t)(v >> 32)) << 32) | rcs_uniform((uint32_t)v);
}

template <int kM>
__device__ __forceinline__ float rcs_chain(const float* x, const float* y) {
  if (kM == 1) return x[0] * y[0];
  return mad(x[2], y[2], mad(x[1], y[1], x[0] * y[0]));
}

// The products of entry b (its Y in registers) with entry a (its Y in the list), summed over the tile and added to `block`; of a
// diagonal block (a == b) the words i <= j only.  Every lane of the wavefront.
template <int kM>
__device__ __forceinline__ void rcs_add_block(const float (&yb)[6 * kM], const float* __restrict__ ya_lds, bool diagonal, long long* __restrict__ block,
                                              int lane, bool* invalid) {
  float ya[6 * kM];
#pragma unroll
  for (int w = 0; w < 6 * kM; ++w) ya[w] = ya_lds[w * 64 + lane];
  float p[40];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) p[i * 6 + j] = rcs_chain<kM>(yb + i * kM, ya + j * kM);
  p[36] = p[37] = p[38] = p[39] = 0.f;
  float p0[16], p1[16], p2[8];
#pragma unroll
  for (int q = 0; q < 16; ++q) { p0[q] = p[q]; p1[q] = p[16 + q]; }
#pragma unroll
  for (int q = 0; q < 8; ++q) p2[q] = p[32 + q];
  // lane 4 q holds total q of a butterfly of 16, lane 8 q total q of one of 8 (wave_reduce.h)
  const float t0 = wave_reduce_small<16>(p0, lane), t1 = wave_reduce_small<16>(p1, lane), t2 = wave_reduce_small<8>(p2, lane);
  if ((lane & 3) == 0) {
    const int q0 = lane >> 2, q1 = 16 + (lane >> 2);
    if (!diagonal || q0 / 6 <= q0 % 6) rcs_limb_add(block + 2 * q0, t0, invalid);
    if (!diagonal || q1 / 6 <= q1 % 6) rcs_limb_add(block + 2 * q1, t1, invalid);
  }
  if ((lane & 7) == 0 && lane < 32) {
    const int q2 = 32 + (lane >> 3);
    if (!diagonal || q2 / 6 <= q2 % 6) rcs_limb_add(block + 2 * q2, t2, invalid);
  }
}

// v_k += the tile's sum of Y z
template <int kM>
__device__ __forceinline__ void rcs_add_v(const float (&y)[6 * kM], const float (&z)[3], long long* __restrict__ vk, int lane, bool* invalid) {
  float p[8];
#pragma unroll
  for (int i = 0; i < 6; ++i) p[i] = rcs_chain<kM>(y + i * kM, z);
  p[6] = p[7] = 0.f;
  const float t = wave_reduce_small<8>(p, lane);
  if ((lane & 7) == 0 && lane < 48) rcs_limb_add(vk + 2 * (lane >> 3), t, invalid);
}

// the frustum cull of the cost sweep (cost_device.h: cost_pairs), the keyframes in ascending order
template <typename Body>
__device__ __forceinline__ void rcs_for_each_keyframe(const Intrinsics& in, const KfEntry* __restrict__ frames, int num_kfs, const WaveBounds& wb, Body body) {
  for_each_candidate(
      num_kfs,
      [&](int k) {
        float f[12];
        load_candidate(frames[k].pose.F, nullptr, f, nullptr);
        return sphere_may_project(in, f, wb);
      },
      body);
}
}  // namespace

// Persistent workgroups of `blockDim.x / 64` wavefronts, as the co-visibility sweep's (heavy tiles first when `sched` is given).
template <bool kUseDepth, bool kUseDesc>
__global__ void __launch_bounds__(64 * kRcsMaxWaves)
rcs_sweep_kernel(Intrinsics in, const KfEntry* __restrict__ frames, int num_kfs, SurfelsView s, uint32_t tiles, uint32_t padded_tiles,
                 const uint32_t* __restrict__ sched, int capacity, int pair_stage, long long* __restrict__ blocks, long long* __restrict__ v,
                 long long* __restrict__ census) {
  constexpr int kM = kUseDesc ? 3 : 1, kW = 6 * kM;
  extern __shared__ unsigned long long rcs_lds[];   // [waves][capacity] masks, [waves][capacity][kW][64] words of Y, [waves][capacity] keyframes
  const uint32_t waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  unsigned long long* masks = rcs_lds + (size_t)wave * capacity;
  float* ys_all = reinterpret_cast<float*>(rcs_lds + (size_t)waves * capacity);
  float* ys = ys_all + (size_t)wave * capacity * kW * 64;
  uint32_t* ks = reinterpret_cast<uint32_t*>(ys_all + (size_t)waves * capacity * kW * 64) + (size_t)wave * capacity;
  PcgLayout L{};
  L.use_depth = kUseDepth ? 1 : 0;
  L.use_desc = kUseDesc ? 1 : 0;
  long long entries = 0, pairs = 0, atomics = 0, degenerates = 0, overflowed = 0;
  bool invalid = false;
  const uint32_t positions = sched_positions(padded_tiles, sched);
  for (uint32_t pos = blockIdx.x * waves + wave; pos < positions; pos += gridDim.x * waves) {
    uint32_t tile;
    if (!scheduled_tile(pos, padded_tiles, sched, &tile) || tile >= tiles) continue;
    const TileSurfel t = load_tile_surfel<kUseDesc>(s, tile, lane);
    const WaveBounds wb = wave_bounds(t.gp, t.in_range && (t.gp.x == t.gp.x));

    // ---- the surfel's sums, its factor and z ----
    float a0 = 0, a1 = 0, a2 = 0, a3 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
    rcs_for_each_keyframe(in, frames, num_kfs, wb, [&](int k) {
      const KfEntry& kf = frames[k];
      PairGather pg;
      if (!gather_and_associate(L, in, kf, t.gp, t.gn, t.tp, t.in_range, &pg)) return;
      PairTerms pt;
      eval_pair_terms<false, false>(L, in, kf, pg.a, pg.pix, pg.dw, t.gn, t.d1, t.d2, &pt);
      if (kUseDepth) {
        a0 = mad(pt.w * pt.Jgeom, pt.Jgeom, a0);
        a6 = mad(pt.w * pt.raw, pt.Jgeom, a6);
      }
      if (kUseDesc && pt.color_ok) {
        const float jd = -1.f;
        const float wr1 = pt.w1 * pt.raw1, wr2 = pt.w2 * pt.raw2;
        a0 = mad(pt.w2 * pt.Jg2, pt.Jg2, mad(pt.w1 * pt.Jg1, pt.Jg1, a0));
        a1 += pt.w1 * pt.Jg1 * jd;
        a3 += pt.w1 * jd * jd;
        a6 = mad(wr2, pt.Jg2, mad(wr1, pt.Jg1, a6));
        a7 += wr1 * jd;
        a2 += pt.w2 * pt.Jg2 * jd;
        a5 += pt.w2 * jd * jd;
        a8 += wr2 * jd;
      }
    });
    float H00 = a0 + 1e-6f, H01 = 0.f, H02 = 0.f, H11 = 1.f, H12 = 0.f, H22 = 1.f;
    float z[3] = {0.f, 0.f, 0.f};
    H00 = sqrtf(H00);
    z[0] = a6 / H00;
    if (kUseDesc) {
      H01 = a1; H02 = a2; H11 = a3 + 1e-6f; H22 = a5 + 1e-6f;
      H01 = H01 / H00;
      H11 = sqrtf(H11 - H01 * H01);
      H02 = H02 / H00;
      H12 = (H12 - H02 * H01) / H11;
      H22 = sqrtf(H22 - H02 * H02 - H12 * H12);
      z[1] = (a7 - H01 * z[0]) / H11;
      z[2] = (a8 - H02 * z[0] - H12 * z[1]) / H22;
    }
    const float inf = __builtin_huge_valf();
    const bool sound = fabsf(H00) < inf && fabsf(H01) < inf && fabsf(H02) < inf && fabsf(H11) < inf && fabsf(H12) < inf && fabsf(H22) < inf &&
                       H00 > 0.f && H11 > 0.f && H22 > 0.f;
    degenerates += (long long)__popcll(__builtin_amdgcn_ballot_w64(!sound));
    if (!pair_stage) continue;   // (timing: the factor traversal alone)

    // ---- the entries of the tile and their pairs, in passes ----
    int skip = 0;
    bool first_pass = true;
#pragma unroll 1
    for (;;) {
      int seen = 0;
      rcs_for_each_keyframe(in, frames, num_kfs, wb, [&](int k) {
        const KfEntry& kf = frames[k];
        PairGather pg;
        const bool visible = gather_and_associate(L, in, kf, t.gp, t.gn, t.tp, t.in_range, &pg);
        const unsigned long long associated = __builtin_amdgcn_ballot_w64(visible);
        if (associated == 0ull) return;
        const int n = seen++;
        if (n < skip) return;
        float y[kW];
#pragma unroll
        for (int w = 0; w < kW; ++w) y[w] = 0.f;
        if (visible && sound) {
          PairTerms pt;
          eval_pair_terms<false, false>(L, in, kf, pg.a, pg.pix, pg.dw, t.gn, t.d1, t.d2, &pt);
          const bool desc = kUseDesc && pt.color_ok;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            float e0 = 0.f, e1 = 0.f, e2 = 0.f;
            if (kUseDepth) e0 = (pt.w * pt.Jgeom) * pt.Jpose[i];
            if (desc) {
              e0 = mad(pt.w2 * pt.Jg2, pt.Jp2[i], mad(pt.w1 * pt.Jg1, pt.Jp1[i], e0));
              e1 = -(pt.w1 * pt.Jp1[i]);
              e2 = -(pt.w2 * pt.Jp2[i]);
            }
            const float y0 = e0 / H00;
            y[i * kM] = y0;
            if (kUseDesc) {
              const float y1 = (e1 - H01 * y0) / H11;
              y[i * kM + 1] = y1;
              y[i * kM + 2] = (e2 - H02 * y0 - H12 * y1) / H22;
            }
          }
        }
        const int slot = n - skip;
        if (slot < capacity) {
          // listed in this pass and in no other: its words of v go with it
#pragma unroll
          for (int w = 0; w < kW; ++w) ys[((size_t)slot * kW + w) * 64 + lane] = y[w];
          if (lane == 0) { masks[slot] = associated; ks[slot] = (uint32_t)k; }
          rcs_add_v<kM>(y, z, v + (size_t)k * kRcsVWords, lane, &invalid);
          atomics += kRcsVWords;
          return;
        }
        // beyond the list, which is full: this entry against every entry of it (all of them earlier keyframes)
        __builtin_amdgcn_wave_barrier();
        for (int a = 0; a < capacity; ++a) {
          const unsigned long long ma = rcs_uniform(masks[a]);
          if ((ma & associated) == 0ull) continue;   // wave-uniform
          rcs_add_block<kM>(y, ys + (size_t)a * kW * 64, false, blocks + rcs_block_index((size_t)k, rcs_uniform(ks[a])) * kRcsBlockWords, lane, &invalid);
          ++pairs;
          atomics += kRcsBlockWords;
        }
      });
      __builtin_amdgcn_wave_barrier();
      const int listed = min(seen - skip, capacity);
      for (int b = 0; b < listed; ++b) {
        const unsigned long long mb = rcs_uniform(masks[b]);
        const uint32_t kb = rcs_uniform(ks[b]);
        float yb[kW];
#pragma unroll
        for (int w = 0; w < kW; ++w) yb[w] = ys[((size_t)b * kW + w) * 64 + lane];
        for (int a = 0; a <= b; ++a) {
          if ((rcs_uniform(masks[a]) & mb) == 0ull) continue;   // wave-uniform
          rcs_add_block<kM>(yb, ys + (size_t)a * kW * 64, a == b, blocks + rcs_block_index(kb, rcs_uniform(ks[a])) * kRcsBlockWords, lane, &invalid);
          ++pairs;
          atomics += a == b ? 42 : kRcsBlockWords;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (first_pass) {
        entries += (long long)seen;
        if (seen > capacity) ++overflowed;
        first_pass = false;
      }
      if (seen - skip <= capacity) break;
      skip += capacity;
    }
  }
  const bool any_invalid = __builtin_amdgcn_ballot_w64(invalid) != 0ull;
  if (lane == 0) {
    if (entries) __hip_atomic_fetch_add(census + kRcsEntries, entries, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pairs) __hip_atomic_fetch_add(census + kRcsPairs, pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (atomics) __hip_atomic_fetch_add(census + kRcsAtomics, atomics, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (degenerates) __hip_atomic_fetch_add(census + kRcsDegenerate, degenerates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (overflowed) __hip_atomic_fetch_add(census + kRcsOverflowTiles, overflowed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (any_invalid) __hip_atomic_fetch_add(census + kRcsInvalid, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

namespace {
// the value of a summed limb pair; a sum whose limb 1 reached 2^62 may have wrapped (ba_device.h: kHbSumLimit)
__device__ __forceinline__ double rcs_value(const long long* __restrict__ cell, bool* invalid) {
  const long long lo = cell[0], hi = cell[1];
  if (hi >= kHbSumLimit || hi <= -kHbSumLimit) *invalid = true;
  return hb_value(lo, hi);
}
__device__ __forceinline__ int rcs_upper_index(int i, int j) {   // word of (i, j), i <= j, in the row-major upper triangle of a 6 x 6 matrix
  return i * 6 - i * (i - 1) / 2 + (j - i);
}
}  // namespace

// one thread per word of S; the threads of column 0 of a keyframe's first row also write its words of g, A_diag and b
__global__ void __launch_bounds__(256) rcs_resolve_kernel(int num_kfs, const HbFixed* __restrict__ Hb, const long long* __restrict__ blocks,
                                                          const long long* __restrict__ v, double* __restrict__ S, size_t pitch, double* __restrict__ g,
                                                          double* __restrict__ A_diag, double* __restrict__ b, long long* __restrict__ census) {
  const size_t n = 6 * (size_t)num_kfs;
  const size_t word = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (word >= n * n) return;
  const size_t row = word / n, col = word % n;
  const int kr = (int)(row / 6), i = (int)(row % 6), kc = (int)(col / 6), j = (int)(col % 6);
  bool invalid = word == 0 && Hb[27 * kHbLimbs] != 0;   // the pose sweep's flag, summed over the ranks like the rest (pose_device.h: pose_invalid_word)
  double a = 0.0;
  if (kr == kc) a = rcs_value(Hb + (size_t)kr * kHbStride + rcs_upper_index(min(i, j), max(i, j)) * kHbLimbs, &invalid);
  double m = 0.0;
  if (blocks) {
    const long long* cell;
    if (kr > kc) cell = blocks + rcs_block_index(kr, kc) * kRcsBlockWords + 2 * (i * 6 + j);
    else if (kr < kc) cell = blocks + rcs_block_index(kc, kr) * kRcsBlockWords + 2 * (j * 6 + i);
    else cell = blocks + rcs_block_index(kr, kr) * kRcsBlockWords + 2 * (min(i, j) * 6 + max(i, j));
    m = rcs_value(cell, &invalid);
  }
  S[row * pitch + col] = a - m;
  if (kr == kc) {
    if (A_diag) A_diag[(size_t)kr * 36 + i * 6 + j] = a;
    if (j == 0) {
      const double bk = rcs_value(Hb + (size_t)kr * kHbStride + (21 + i) * kHbLimbs, &invalid);
      const double vk = blocks ? rcs_value(v + (size_t)kr * kRcsVWords + 2 * i, &invalid) : 0.0;
      g[row] = bk - vk;
      if (b) b[row] = bk;
    }
  }
  if (invalid) __hip_atomic_fetch_add(census + kRcsInvalid, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The work items of a pose sweep over EVERY bound keyframe at its current pose (the pose phase's own set-up leaves the inactive ones
// out): `records` records of 32 words, the first num_kfs the keyframes', the rest -- counters and list -- zero.
__global__ void __launch_bounds__(256) rcs_work_kernel(const KfEntry* __restrict__ frames, int num_kfs, PoseWork* __restrict__ work, uint32_t records) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= records) return;
  PoseWork pw;
  int32_t* words = reinterpret_cast<int32_t*>(&pw);
  for (int c = 0; c < (int)(sizeof(PoseWork) / sizeof(int32_t)); ++c) words[c] = 0;
  if (k < (uint32_t)num_kfs) {
    for (int c = 0; c < 12; ++c) pw.F[c] = frames[k].pose.F[c];
    for (int c = 0; c < 7; ++c) { pw.T[c] = frames[k].global_T_frame[c]; pw.T0[c] = frames[k].global_T_frame[c]; }
    pw.kf_index = (int32_t)k;
  }
  work[k] = pw;
}

void launch_rcs_work(hipStream_t stream, const KfEntry* frames, int num_kfs, PoseWork* work) {
  const uint32_t records = (uint32_t)pose_work_records((size_t)num_kfs);
  hipLaunchKernelGGL(rcs_work_kernel, dim3((records + 255u) / 256u), dim3(256), 0, stream, frames, num_kfs, work, records);
}

bool launch_rcs_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs,
                      const SurfelsView& s, const uint32_t* sched, const RcsShape& shape, bool pair_stage, long long* blocks, long long* v,
                      long long* census) {
  const uint32_t tiles = (s.size + 63u) / 64u;
  if (tiles == 0 || num_kfs <= 0) return true;
  const uint32_t waves = (uint32_t)shape.waves;
  const size_t lds = (size_t)waves * (size_t)shape.list_capacity * rcs_entry_bytes(use_desc);
  if (lds > kRcsMaxLdsBytes) return false;
  const uint32_t padded = pose_padded_tiles(s.size);
  const uint32_t positions = sched_positions(padded, sched);
  const uint32_t grid = std::max(1u, std::min((uint32_t)shape.workgroups, (positions + waves - 1) / waves));
  auto launch = [&](auto kernel, int variant) {
    static bool opted_in[3] = {false, false, false};   // dynamic LDS beyond 64 KB needs the opt-in: once per kernel
    if (lds > 64 * 1024 && !opted_in[variant]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRcsMaxLdsBytes) != hipSuccess) return false;
      opted_in[variant] = true;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, stream, in, frames, num_kfs, s, tiles, padded, sched, shape.list_capacity, pair_stage ? 1 : 0, blocks, v, census);
    return true;
  };
  if (use_depth && use_desc) return launch(rcs_sweep_kernel<true, true>, 0);
  if (use_depth) return launch(rcs_sweep_kernel<true, false>, 1);
  return launch(rcs_sweep_kernel<false, true>, 2);
}

void launch_rcs_resolve(hipStream_t stream, int num_kfs, const HbFixed* Hb, const long long* blocks, const long long* v, double* S, size_t pitch,
                        double* g, double* A_diag, double* b, long long* census) {
  if (num_kfs <= 0) return;
  const size_t words = 36 * (size_t)num_kfs * (size_t)num_kfs;
  hipLaunchKernelGGL(rcs_resolve_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, num_kfs, Hb, blocks, v, S, pitch, g, A_diag, b, census);
}

}  // namespace bahip
#endif
