// ba_launch.h -- host-callable launch wrappers shared between the kernel translation units and
// the C-ABI layer (capi*.hip; capi_internal.h lists the units).
#pragma once

#include "ba_device.h"
#include <cstdlib>

// An integer switch from the environment, read once at load time.  A plain function on purpose: these switches used to be initialised by
// lambdas at namespace scope, and hipcc gave two such lambdas in two openings of one namespace of one file the SAME mangled name (host
// and device passes number them per context) -- the linker kept one body, and `g_device_loop_enabled` was initialised by the lambda of
// BAHIP_FUSED_ITERATION_BEGIN (default 0): the device-driven loop silently declined every call (round 5, found in the kernel trace).
inline int bahip_env_int(const char* name, int fallback) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : fallback;
}

// ---- Two arithmetic flavours of the sweeps ----------------------------------------------------------------------------------------
// The sweeps over (surfel, keyframe) pairs -- activation, normals / geometry step, pose normal equations, intrinsics sweep, the PCG
// init and step-1 sweeps -- exist twice in the library, compiled from the same source:
//   exact  IEEE reciprocal / square root / division in few instructions (ba_device.h: rcp_exact, sqrt_exact), defined exp / sin / cos,
//          no contraction beyond the spelled fused multiply-adds: every bit is the oracle's (the checker's flavour, and the default);
//   fast   the hardware's v_rcp_f32 / v_sqrt_f32 / v_exp_f32 (<= 1 ulp), contraction at the compiler's discretion, denormals flushed
//          -- the arithmetic the reference itself ships with (B/../CMakeLists.txt:74: nvcc -use_fast_math), held to the reference's
//          kernels by tolerance (tests/test_gpu_fast_flavour.py), selected per context by bahip_context_set_arithmetic.
// What does NOT change with the flavour: the order of every sum (fixed trees, fixed-point pose sums, exact PCG sums, binary64
// intrinsics accumulation), so the fast flavour is as deterministic and as shard-invariant as the exact one; the rejection order of the
// association tests; preprocessing, lifecycle, the pose solve and the PCG vector kernels (compiled once, exact).
// Mechanics: a kernel translation unit wraps its sweeps in BAHIP_FLAVOURED_BEGIN / _END (namespace bahip::exact or bahip::fast); it
// is compiled once per flavour (Makefile: *_fast.o with -DBAHIP_FAST_MATH and the device-side flags); everything else in the unit
// sits under #ifndef BAHIP_FAST_MATH in plain bahip::, including the dispatchers that carry the public names below and pick the
// flavour from Intrinsics::fast_math.
#ifdef BAHIP_FAST_MATH
#define BAHIP_FLAVOUR fast
#else
#define BAHIP_FLAVOUR exact
#endif
#define BAHIP_FLAVOURED_BEGIN namespace bahip { namespace BAHIP_FLAVOUR {
#define BAHIP_FLAVOURED_END } }

namespace bahip {

struct SupportingView {
  uint32_t* b[BAHIP_MERGE_BUFFER_COUNT];
  uint32_t pitch;
};

// kernels_preprocess.hip
int launch_bilateral_filter(hipStream_t stream, float sigma_xy, float sigma_value, float radius_factor, uint16_t max_depth,
                            float raw_to_float_depth, const uint16_t* in, uint32_t in_pitch, uint16_t* out, uint32_t out_pitch, int w, int h);
void launch_brightness(hipStream_t stream, const uint8_t* rgb, uint32_t rgb_pitch, uint8_t* rgba, uint32_t rgba_pitch, int w, int h);
void launch_normals_from_depth(hipStream_t stream, const Intrinsics& in, const uint16_t* in_depth, uint32_t in_pitch,
                               uint16_t* out_depth, uint32_t out_pitch, uint16_t* out_normals, uint32_t normals_pitch);
void launch_point_radii(hipStream_t stream, const Intrinsics& in, float raw_to_float_depth, const uint16_t* depth,
                        uint32_t depth_pitch, uint16_t* radius, uint32_t radius_pitch, uint16_t* out_depth, uint32_t out_pitch);
void launch_min_max_depth(hipStream_t stream, const uint16_t* depth, uint32_t depth_pitch, int w, int h,
                          float raw_to_float_depth, int* result);
void launch_pack_planes(hipStream_t stream, const KfEntry& frame, int width, int height, int cwidth, int cheight, uint32_t* geom,
                        uint32_t* lumafp);

void launch_read_pattern(hipStream_t stream, const uint32_t* data, size_t words, int pattern, uint32_t* sink);

// kernels_surfel.hip
void launch_activation(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s,
                       uint32_t surfels_size);
void launch_assign_colors(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s);
void launch_normals(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s);
// The per-tile words of the geometry step's fused route (kernels_surfel.hip: geometry_fused_kernel), written by every tile of a launch:
// the lanes left to the fix-up launch behind it, and the route the tile took (0 held, 1 position pass run again, 2 deferred lanes).
struct GeometryFused {
  unsigned long long* deferred = nullptr;
  uint8_t* route = nullptr;
  uint32_t tiles = 0;   // entries of either array: at least geometry_fused_tiles(surfels) for a launch over `surfels`
  int threshold = 0;    // (filled in by the launcher)
  bool settled = false; // host side: the step is not among the first kGeometryFusedAfter of its BundleAdjustment call
};
// The first geometry steps after a disturbance -- a new keyframe, a loop closure, new poses: what a call of BundleAdjustment follows --
// move nearly every normal, and a walk whose sums are thrown away costs more than the normals pass it stands for (bench scene: 0.95 ms
// against 0.73 in the first step, level from the sixth on, 0.52 against 0.61 once settled; profiles/geometry_fused_ab.txt).  Nothing on
// the device announces a disturbance, so the host goes by the iteration's number in its call: the device-driven loop takes the classic
// kernel for its first kGeometryFusedAfter iterations and the fused route from then on; the single-step entry points, which do not
// know their place in a call, keep the classic kernel.  Forced shape 6 takes the fused route everywhere.
constexpr int kGeometryFusedAfter = 5;
// true: the step took the fused route (it does where `fused` has the room, descriptor residuals are in use, and either shape 6 is
// forced or no shape is, the step is settled and there are enough tiles for one wavefront per tile); false: the classic kernels
bool launch_geometry(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* kfs,
                     int num_kfs, const SurfelsView& s, long long activate_count = -1,
                     const uint32_t* sched = nullptr /* heavy work first (wave_cull.h: scheduled_tile) */,
                     const int* stop = nullptr /* device word: non-zero = the launch does nothing (device-driven BA loop) */,
                     const GeometryFused* fused = nullptr);
bool geometry_takes_fused_route(uint32_t surfels, bool use_desc, bool settled);
uint32_t geometry_fused_tiles(uint32_t surfels);   // tiles of the (padded) grid of a geometry step over `surfels`
void set_geometry_fused(int threshold, int window);   // 0 = default; threshold 1 .. 65, window >= 1 tiles (bahip_debug_set_geometry_fused)

// keyframe sharding (kernels_surfel.hip: geometry_step, kPhase): one phase of the geometry step over this rank's keyframe classes
int geometry_normals_sums(bool activate);     // sums per class and surfel of the normals pass (cpn) ...
int geometry_position_sums(bool use_desc);    // ... and of the position pass (cpp)
void launch_geometry_phase(hipStream_t stream, int phase, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                           const SurfelsView& s, long long activate_count, const ClassPartials& cpn, const ClassPartials& cpp);
void launch_activation_hits(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, uint32_t surfels_size,
                            int kf_rank, int kf_world, uint32_t* hits);
// ... and the normals update on its own (bahip_update_surfel_normals): phase 1 stores this rank's class partials (kNormalsSums per class and
// surfel) to cp, phase 2 takes the normals from the exchanged partials
constexpr int kNormalsSums = 4;
void launch_normals_phase(hipStream_t stream, int phase, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, const ClassPartials& cp);
void launch_activation_from_hits(hipStream_t stream, const SurfelsView& s, uint32_t surfels_size, const uint32_t* hits);

void launch_count_pairs(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s,
                        unsigned long long* counts);
// kernels_cull_probe.hip: per 64-entry tile in buffer order the bounding sphere of wave_cull.h (bounds: 4 floats per tile, may be NULL)
// and, per keyframe of the table, its frustum test against that sphere (masks: ceil(num_kfs / 64) words per tile, bit k % 64 of word
// k / 64), in the flavour of in.fast_math
void launch_tile_cull_probe(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, float* bounds,
                            unsigned long long* masks);

// kernels_pose.hip
size_t pose_tile_bounds_bytes(uint32_t surfels);   // size of the per-tile bounding-sphere buffer launch_pose_accumulate needs
void launch_pose_accumulate(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames,
                            const void* work, int num_work, const SurfelsView& s, HbFixed* Hb, void* tile_bounds, bool stored_bounds,
                            int num_listed /* stored_bounds: entries of the list of work items still iterating */,
                            uint32_t* tile_counters /* 16 words, zero before the first launch; NULL: never the persistent LDS form */,
                            int* parity_inout /* which half of tile_counters the next persistent launch draws from */,
                            uint32_t* tile_cost = nullptr /* one word per tile, zero before a first round: += the candidates the tile visits */,
                            const uint32_t* sched = nullptr /* heavy work first (wave_cull.h: scheduled_tile) */,
                            const int* listed_count = nullptr /* device word holding num_listed (a round queued before the host
                            knows it; num_listed is then an upper bound and sizes the LDS table); 0 there: the launch does nothing */,
                            const int* stop = nullptr /* device word: non-zero = the launch does nothing (device-driven BA loop) */);
// May a later round over at most num_items work items be queued ahead (launch_pose_accumulate with listed_count)?
bool pose_round_can_be_queued_ahead(uint32_t surfels, int num_items, bool have_tile_counters);
uint32_t pose_padded_tiles(uint32_t surfels);   // tiles of the (padded) grid the sweeps run over: the length of tile_cost
size_t tile_schedule_words(uint32_t padded_tiles);   // words of a schedule for such a grid
// sched := heavy tiles + runs by descending cost (wave_cull.h; clears tile_cost); false if there are more runs than the kernel
// handles (sched untouched)
bool launch_tile_order(hipStream_t stream, uint32_t* tile_cost, uint32_t padded_tiles, uint32_t* sched);
// The device-driven BA loop (capi_ba.hip: bahip_alternating_iterations): the control words the last solve launch of a pose phase
// updates and every launch of the loop looks at (ba_device.h: kLoop*), and what that solve launch needs to decide.
struct PoseLoopControl {
  int* ctl = nullptr;          // device, kLoopWords ints; ctl + kLoopStop is the `stop` word of the other launches
  int* host_ctl = nullptr;     // mapped host copy, written by the publishing workgroup before the sequence number
  int phase_end = 0;           // this launch is the last queued round of its phase: it decides
  int iteration = 0;           // index of the BA iteration the phase belongs to (for min_iterations)
  int min_iterations = 0;
  int* round_log = nullptr;    // mapped host memory: [log_slot] = work items that iterated in this round (for the stage timers)
  int log_slot = 0;
  // 0: this launch writes nothing to the host copies (counters, control words, sequence number) and needs no system-scope fence -- the
  // launches of a queued loop that the host does not wait for (round 6: every solve launch used to publish, ~5 us of posted PCIe writes
  // and two system-scope fences each, 2.7 launches per iteration); the launch whose sequence number the host polls publishes for all
  int publish = 1;
  // >= 0 (with phase_end, at most 1024 work items): when the phase is complete and the loop goes on, this launch also runs the top
  // of the next iteration -- mode 1: activation window + propagation, 2: propagation -- and sets up its work items
  // (kernels_pose.hip: iteration_begin_body); the caller then queues no launch_iteration_begin for that iteration
  int next_mode = -1;
  const uint8_t* in_window = nullptr;
  const int* covis_offsets = nullptr;
  const int* covis_indices = nullptr;
};
void launch_pose_solve(hipStream_t stream, void* work, int num_work, HbFixed* Hb, KfEntry* frames, int write_back,
                       int update_activation, int round, void* host_out,
                       int sequence /* published to the host copy of the counters when the launch is complete */,
                       const PoseLoopControl* loop = nullptr);
void launch_pose_init_from_keyframes(hipStream_t stream, const KfEntry* frames, int num_kfs, void* work, HbFixed* Hb, void* host_out,
                                     int kf_rank = 0, int kf_world = 1 /* keyframe sharding: the sweep skips keyframes of other ranks */,
                                     const int* stop = nullptr);

void launch_window_activation(hipStream_t stream, KfEntry* frames, int num_kfs, const uint8_t* in_window, const int* offsets,
                              const int* indices, const int* stop = nullptr);   // window activation + co-visible propagation
void launch_propagate_covisible(hipStream_t stream, KfEntry* frames, int num_kfs, const int* offsets, const int* indices,
                                const int* stop = nullptr);
// window (mode 1) / propagation (mode 2) / nothing (mode 0), then the work items of the pose phase, in one launch; false (and
// nothing launched) beyond 1024 keyframes
bool launch_iteration_begin(hipStream_t stream, KfEntry* frames, int num_kfs, int mode, const uint8_t* in_window, const int* offsets, const int* indices,
                            void* work, HbFixed* Hb, void* host_out, const int* stop);

void set_tile_waves(int waves);   // 0 = automatic; 1 | 4 wavefronts per surfel tile in the normals / geometry passes; 5 = the hybrid shape of the geometry step
long long geometry_hybrid_launches();   // launches of the geometry step in the hybrid shape so far (both flavours)
void set_pose_lds_waves(int waves);        // test hook: wavefronts per workgroup of the LDS form (0: 16)
void set_pose_lds_parts_shift(int shift);  // test hook: 2^shift wavefronts share a tile's work items in the LDS form (-1: from the grid size)
void set_pose_lds_items(int items);   // test hook: slices of that many work items per launch of the LDS form (0: as many as the table holds)
void pcg_step1_form_launches(long long out[2]);   // launches of the PCG step-1 sweep: [0] one tile per wavefront, [1] persistent LDS form
long long pose_kernel_dispatches();   // kernel dispatches of the accumulate sweep since the process started
void pose_form_launches(long long out[2], bool reset);   // launches of either form since the last reset (bench: which kernel to name)
void set_pose_form(int form);     // 0 = automatic; 1 = one tile per wavefront + global atomics; 2 = persistent workgroups with the normal equations in LDS
void set_pose_parts(int parts);   // 0 = automatic; 1 | 2 | 4 | 8 wavefronts share a tile's keyframes in the pose kernel
void launch_jacobian_debug(hipStream_t stream, int kind, const float* in, float* out);
void launch_pose_step_debug(hipStream_t stream, const float* in, float* out);
void launch_exact_math_debug(hipStream_t stream, int kind, const float* in, float* out, size_t n);
void launch_pose_limbs_debug(hipStream_t stream, const float* in, long long* out, size_t n);
void launch_wave_reduce_debug(hipStream_t stream, const float* in, float* out);
void launch_evaluate_pairs(hipStream_t stream, const Intrinsics& in, const KfEntry& frame, const SurfelsView& s,
                           const uint32_t* indices, int count, float* out);

// kernels_intrinsics.hip
// Intrinsics step (kernels_intrinsics.hip).  glob_d / cells_d: binary64 accumulators (34 sums; S records of 8: B0..B4, D, b2,
// observation count) -- what a multi-GPU run sums over the ranks; glob_f / cells_f: their binary32 roundings after the
// Schur complement (glob_f also carries x1 at [40..44] for the back-substitution).
// Append buffers of the intrinsics sweep's per-cell records (kernels_intrinsics.hip): several per block of 32 x 32 sparse cells, each
// 8 planes of `capacity` words; cursors[buffer] counts the records appended (and keeps counting when the buffer is full).
// capacity == 0: no binning, every record goes out as atomics.
struct IntrBins {
  uint32_t* cursors;
  uint32_t* records;
  uint32_t capacity;
  int bins_x;
};
int intrinsics_bin_count(const Intrinsics& in, int* bins_x_out);
size_t intrinsics_bin_record_bytes();
void launch_intrinsics_accumulate(hipStream_t st, bool depth, bool color, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                                  const SurfelsView& s, double* glob, double* cells, const IntrBins& bins, const uint32_t* sched,
                                  uint32_t position_begin = 0, uint32_t position_count = 0 /* 0: all positions of the schedule */,
                                  int classes = 1 /* the global sums' keyframe classes (bahip_context_set_intrinsics_sum_classes) */,
                                  int kf_rank = 0, int kf_world = 1 /* keyframe sharding: the sweep visits this rank's classes only */);
uint32_t intrinsics_sweep_positions(uint32_t surfels, const uint32_t* sched);   // positions of a full sweep (what the slices cut)
void launch_intrinsics_bin_reduce(hipStream_t st, bool depth, const Intrinsics& in, const SurfelsView& s, double* cells, const IntrBins& bins);
void set_intrinsics_reduce_form(int form);   // 0: LDS table of ds_add_f64, 1: records sorted by cell in LDS, sums in registers
size_t intrinsics_schur_partials(int S);   // floats of scratch launch_intrinsics_finish needs
void launch_intrinsics_finish(hipStream_t st, bool schur, int S, const double* glob_d, const double* cells_d, float* glob_f, float* cells_f,
                              float* partials);
void launch_intrinsics_solve_cells(hipStream_t st, const Intrinsics& in, int S, float* cells_f, const float* x1, float* cfactor,
                                   uint32_t cfactor_pitch);

#ifdef BAHIP_TILE_TIMELINE
void geometry_timeline_dump(const char* path);   // experiment build only (kernels_surfel.hip, kernels_pose.hip; scripts/tile_timeline.py)
void pose_timeline_dump(const char* path);
#endif
#ifdef BAHIP_COUNT_CANDIDATES
void pose_counters_dump();   // experiment build only (kernels_pose.hip)
#endif
// kernels_pcg.hip
// `ex`: the exact accumulators of the solve (pcg_exact_cells(head_count) cells of 72 bytes, zeroed once; every kernel that
// resolves a sum clears what it read).  ctl: device-side inner-loop control block (pcg_control_bytes(); stopping rule of
// B/direct_ba_pcg.cc:427-456 evaluated on the device).
size_t pcg_exact_cells(uint32_t head_count);
PcgExact pcg_exact_view(void* buffer, uint32_t head_count);
size_t pcg_control_bytes();
void launch_pcg_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                     const SurfelsView& s, float* r, float* M,
                     uint32_t* tile_cost = nullptr /* census for the schedule, as in launch_pose_accumulate */, const uint32_t* sched = nullptr,
                     const PcgClasses* classes = nullptr /* C > 1 (bahip_context_set_pcg_sum_classes): the surfel entries go to class partials */);
void launch_pcg_resolve_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* r, float* M);
void launch_pcg_init2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float a, const float* r, const float* M, float* delta, float* g,
                      float* p);
void launch_pcg_control_init(hipStream_t st, const PcgExact& ex, void* ctl, float* alpha_n);
void launch_pcg_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,
                      const SurfelsView& s, const float* p, float* g, const void* ctl, const uint32_t* sched = nullptr,
                      uint32_t* tile_counters = nullptr /* the context's two sets of eight tile counters: allows the persistent LDS form */,
                      int* parity_inout = nullptr, const PcgClasses* classes = nullptr /* as launch_pcg_init */);
// the surfel block of r and M (va, vb; ctl NULL: after PCGInit) or of g (va; after PCGStep1, stopped by ctl like the other kernels of a
// step) from the class partials of `classes`, summed in the defined order (kernels_pcg.hip: "DEFINITION of the surfel block")
void launch_pcg_class_combine(hipStream_t st, const PcgLayout& L, const PcgClasses& classes, uint32_t surfels, float* va, float* vb, const void* ctl);
void set_pcg_lds_form(int mode);   // test hook: 0 = always the one-tile-per-wavefront form of the step-1 sweep, 1 = automatic, 2 = the LDS form whenever the table fits
void launch_pcg_eps_terms(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const float* p);
void launch_pcg_resolve_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* g, float* alpha_d, double eps_repeat, const void* ctl);
void launch_pcg_step2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float* r, const float* M, float* delta, float* g, const float* p,
                      const float* alpha_n, const float* alpha_d, const void* ctl);
void launch_pcg_control(hipStream_t st, const PcgExact& ex, void* ctl, float* beta_n);
void launch_pcg_step3(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const float* g, float* p, const float* alpha_n, const float* beta_n,
                      const void* ctl);
void launch_exact_sum_debug(hipStream_t st, const PcgExact& ex, const float* values, size_t n, int mode, double* out);
void launch_pcg_update_surfels(hipStream_t st, const PcgLayout& L, const SurfelsView& s, const float* delta);
void launch_pcg_update_cfactors(hipStream_t st, const Intrinsics& in, uint32_t start, const float* delta, float* cfactor, uint32_t pitch);
// kernels_pcg_window.hip: the sweeps over a keyframe window (PcgWindow), the tile list they run over (`count` zeroed by the caller) and
// the surfel update that leaves inactive surfels alone
void launch_pcg_window_tiles(hipStream_t st, const SurfelsView& s, uint32_t* tiles, uint32_t* count);
void launch_pcg_window_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                            const SurfelsView& s, float* r, float* M);
void launch_pcg_window_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, const PcgWindow& w,
                             const SurfelsView& s, const float* p, float* g, const void* ctl);
void launch_pcg_window_update_surfels(hipStream_t st, const PcgLayout& L, const SurfelsView& s, const float* delta);

// kernels_pcg_trial.hip: the per-unknown kernels under a damping factor (lambda == 0: the kernels above themselves), and the
// snapshot / restore of what a PCG outer iteration writes (`snap`: pcg_trial_snapshot_words(t) words)
void launch_pcg_damped_init2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, float a, const float* r, const float* M,
                             float* delta, float* g, float* p);
void launch_pcg_damped_eps_terms(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, const float* M, const float* p);
void launch_pcg_damped_step2(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, float* r, const float* M, float* delta, float* g,
                             const float* p, const float* alpha_n, const float* alpha_d, const void* ctl);
void launch_pcg_damped_step3(hipStream_t st, const PcgLayout& L, const PcgExact& ex, float lambda, const float* M, const float* g, float* p,
                             const float* alpha_n, const float* beta_n, const void* ctl);
size_t pcg_trial_snapshot_words(const PcgTrialShape& t);
void launch_pcg_trial_snapshot(hipStream_t st, const SurfelsView& s, const PcgTrialShape& t, uint32_t* snap);
void launch_pcg_trial_restore(hipStream_t st, const SurfelsView& s, const PcgTrialShape& t, uint32_t* snap);

// kernels_lifecycle.hip
void launch_supporting_fill(hipStream_t st, const SupportingView& sup, int w, int h);
void launch_lifecycle_bounds(hipStream_t st, const SurfelsView& s, uint32_t tiles, void* spheres);   // bounding spheres of tiles [0, tiles)
// What a per-keyframe sweep of a lifecycle batch may skip (kernels_lifecycle.hip: LifecycleBounds): the bounding spheres of the
// tiles [0, tiles) taken at the start of the batch, and -- when the batch knows its frames -- the list of those tiles this frame sees.
struct LifecycleCull {
  const void* spheres = nullptr;
  uint32_t tiles = 0;
  const uint32_t* list = nullptr;
  uint32_t list_count = 0;
};
// cursors[f] (zeroed) <- the number of bounded tiles frame f can see, lists[f * tiles + ...] <- those tiles (no particular order)
void launch_lifecycle_visible_tiles(hipStream_t st, const Intrinsics& in, const float* frames_F, int num_frames, const void* spheres, uint32_t tiles,
                                    uint32_t* cursors, uint32_t* lists);
void launch_supporting_insert(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const SurfelsView& s, const SupportingView& sup,
                              const LifecycleCull& cull = LifecycleCull(),
                              const uint32_t* size_on_device = nullptr /* a creation batch: min(*size_on_device, s.size) surfels exist */);
void launch_merge(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const SurfelsView& s, const SupportingView& sup,
                  float cell_merge_dist_sq, float cos_thr, uint32_t* flags, uint32_t* cell_of, bool empty_the_planes, uint32_t* deleted_count,
                  const LifecycleCull& cull = LifecycleCull());
void launch_merge_decide(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const SurfelsView& s, const SupportingView& sup,
                         float cell_merge_dist_sq, float cos_thr, uint32_t* flags, uint32_t* cell_of, const LifecycleCull& cull);
// one launch: the apply sweep of apply_frame (NULL: none) beside the insert sweep of insert_frame (NULL: none); flags must have been
// cleared before the batch's first decide (kernels_lifecycle.hip: merge_apply_insert_kernel)
void launch_merge_apply_insert(hipStream_t st, const Intrinsics& in, const KfEntry* apply_frame, const KfEntry* insert_frame, const SurfelsView& s,
                               const uint32_t* flags, const uint32_t* cell_of, const SupportingView& apply_sup, const SupportingView& insert_sup,
                               uint32_t* deleted_count, const LifecycleCull& apply_cull, const LifecycleCull& insert_cull);
// a merge batch by cell lists (kernels_lifecycle.hip: merge_pairs_kernel): the associated (surfel, frame) pairs grouped by (frame, cell)
// up front -- counts and offsets [num_frames * cells + 1] words; pair_cells and pair_ranks [64 * total sweep positions] words; members
// (words) and member_cell (uint2) [pairs <= 64 * total sweep positions] --, then one launch per frame over its pairs
// (frame_first[j] = offsets[j * cells], read back by the caller) and one launch that writes the deleted markers.  deleted_at: one word per surfel, ~0 before.
struct MergeBatchFrame {
  KfEntry entry;
  uint32_t list_offset, list_count;   // its visible bounded tiles in `lists`
  uint32_t pair_offset;               // its first sweep position (wavefront) in pair_cells / pair_ranks
  uint32_t pad_;
};
hipError_t launch_merge_batch_lists(hipStream_t st, const Intrinsics& in, const MergeBatchFrame* frames, int num_frames, uint32_t max_positions, const SurfelsView& s,
                                    const uint32_t* lists, uint32_t bounded_tiles, uint32_t* counts, uint32_t* offsets, uint32_t* pair_cells, uint32_t* pair_ranks,
                                    uint32_t* members, void* member_cell, uint32_t* frame_first /* [num_frames + 1] */, void* scan_temp, size_t scan_temp_bytes);
size_t merge_batch_scan_temp_bytes(size_t entries);
void launch_merge_pairs(hipStream_t st, const SurfelsView& s, const uint32_t* members, const void* member_cell, uint32_t first_pair,
                        uint32_t end_pair, uint32_t step, uint32_t* deleted_at, float cell_merge_dist_sq, float cos_thr);
void launch_merge_batch_apply(hipStream_t st, const SurfelsView& s, const uint32_t* deleted_at, uint32_t* deleted_count);   // writes the markers, adds their number
// a creation batch: scan + append at *size_in + the new size into *size_out (or *capacity_exceeded raised and nothing appended) in one
// launch; group_words: create_append_groups() words, cleared before tag 1 and whenever a tag (1 .. 255) would repeat
int create_append_groups();
void set_append_groups_limit(int groups);   // test hook: the fused append's grid as on a device that holds at most `groups` of its workgroups (0: ask the device)
void launch_create_append_fused(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const uint8_t* flags, const SurfelsView& s,
                                const uint32_t* size_in, uint32_t* size_out, uint32_t capacity, uint32_t* capacity_exceeded,
                                uint32_t* group_words, uint32_t tag);
size_t create_padded_count(const Intrinsics& in);   // length of the tile-major flag / index vectors
// a creation batch whose keyframes do not wait for each other's sweeps (kernels_lifecycle.hip: create_chain_kernel).  Up front, for all
// keyframes of the batch: occupancy [n][cells] bytes (cleared by the caller) <- the cloud at the batch's begin, candidates [n][padded]
// bytes (cleared by the caller) <- the pixels that would create a surfel, filtered; then one launch per keyframe of the chain.
struct CreateBatchItem {
  int kf_index;                       // bound keyframe
  uint32_t list_offset, list_count;   // its visible bounded tiles in `lists`
  int covis_offset, n_covis;          // its slice of the batch's co-visibility lists
};
// scan: [num_items * padded] words; cand_cell: one word, records: kSurfelAccum0 rows (a view whose pitch is the row length), per list
// position -- at most one candidate per sparse cell and keyframe; first_of_item: [num_items + 1] words (read back by the caller)
size_t create_batch_scan_temp_bytes(size_t entries);
hipError_t launch_create_batch_prepare(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, const CreateBatchItem* items, int num_items, uint32_t max_list_count,
                                       const SurfelsView& cloud_at_begin, const uint32_t* lists, uint32_t bounded_tiles, uint8_t* occupancy, uint8_t* candidates,
                                       bool filter_new_surfels, const int* covis, const float* covis_T_frame, int min_obs, uint32_t* scan, void* scan_temp,
                                       size_t scan_temp_bytes, uint32_t* cand_cell, const SurfelsView& records, uint32_t* first_of_item);
void launch_create_chain(hipStream_t st, const Intrinsics& in, const KfEntry* next_frame, const uint32_t* cand_cell, const SurfelsView& records, uint32_t first,
                         uint32_t end_of_frame, const uint8_t* occupancy, uint8_t* next_occupancy, const SurfelsView& s, uint32_t batch_begin_size,
                         const uint32_t* size_in, uint32_t* size_out, uint32_t capacity, uint32_t* capacity_exceeded, uint32_t* group_words, uint32_t tag,
                         uint32_t appended_bound);
void launch_create_flag(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const SupportingView& sup, uint8_t* flags, bool leave_planes_empty = false);
void launch_create_filter(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const KfEntry* kfs, const int* covis,
                          const float* covis_T_frame, int n_covis, int min_obs, uint8_t* flags);
void launch_create_append(hipStream_t st, const Intrinsics& in, const KfEntry& frame, const uint8_t* flags,
                          const uint32_t* indices, uint32_t surfels_size, const SurfelsView& s);
void launch_delete_update(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s,
                          int min_obs, uint32_t* deleted_count);
// Keyframe sharding of the lifecycle (capi_lifecycle.hip): the owner of a frame / item runs its part of the batch kernels alone (a grid
// of one row over pointers advanced to its rows); the filter of a creation batch is cut into count (over this rank's co-visible
// keyframes, from the owner's raw words of each candidate) and decide; deletion into a partial sweep over this rank's keyframes and a
// decide launch.
void launch_merge_batch_associate_frame(hipStream_t st, const Intrinsics& in, const MergeBatchFrame* frame, uint32_t positions, const SurfelsView& s,
                                        const uint32_t* lists, uint32_t bounded_tiles, uint32_t* counts_row, uint32_t* pair_cells, uint32_t* pair_ranks);
void launch_merge_batch_fill_frame(hipStream_t st, const Intrinsics& in, const MergeBatchFrame* frame, uint32_t positions, uint32_t surfels_size,
                                   const uint32_t* lists, uint32_t bounded_tiles, const uint32_t* offsets_row, const uint32_t* pair_cells,
                                   const uint32_t* pair_ranks, uint32_t* members, void* member_cell);
hipError_t launch_merge_batch_offsets(hipStream_t st, const Intrinsics& in, int num_frames, const uint32_t* counts, uint32_t* offsets, uint32_t* frame_first,
                                      void* scan_temp, size_t scan_temp_bytes);
void launch_create_batch_item_candidates(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, const CreateBatchItem* item, uint32_t positions,
                                         const SurfelsView& cloud_at_begin, const uint32_t* lists, uint32_t bounded_tiles, uint8_t* occupancy_row,
                                         uint8_t* candidates_row, uint32_t* cand_px_row, const KfEntry& frame);
void launch_create_batch_filter_count(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, const CreateBatchItem* items, int num_items, const int* covis,
                                      const float* covis_T_frame, const uint8_t* candidates, const uint32_t* cand_px, void* counts /* uint2 [n][cells] */,
                                      int kf_rank, int kf_world);
void launch_create_batch_filter_decide(hipStream_t st, const Intrinsics& in, int num_items, const void* counts, int min_obs, uint8_t* candidates);
hipError_t launch_create_batch_scan(hipStream_t st, const Intrinsics& in, int num_items, const uint8_t* candidates, uint32_t* scan, void* scan_temp, size_t scan_temp_bytes);
void launch_create_batch_item_records(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, const CreateBatchItem* item, const uint8_t* candidates_row,
                                      const uint32_t* scan_row, uint32_t* cand_cell, const SurfelsView& records, uint32_t* first_of_item2);
void launch_delete_partial(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, int kf_rank, int kf_world,
                           uint32_t* partial, uint32_t stride);
void launch_delete_decide(hipStream_t st, const SurfelsView& s, const uint32_t* partial, uint32_t stride, int kf_world, int min_obs, uint32_t* deleted_count);
// The lifecycle dealt over a surfel partition (kernels_lifecycle_dealt.hip): deletion + radius update over this rank's chunks of the
// gathered cloud (chunk c belongs to rank c % world) into packed[i] = (x, radius^2) words of a zero-filled vector of s.size uint2, the
// count of what it newly deleted into *deleted_count; after the sum over the ranks, the unpack writes the two rows for every surfel.
uint32_t dealt_surfel_count(uint32_t total, uint32_t rank, uint32_t world, uint32_t chunk);   // surfels of `total` in rank's chunks
void launch_delete_chunks(hipStream_t st, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, uint32_t rank, uint32_t world,
                          uint32_t chunk, int min_obs, void* packed, uint32_t* deleted_count);
void launch_delete_unpack(hipStream_t st, const SurfelsView& s, const void* packed);
void launch_shard_to_cloud(hipStream_t st, const SurfelsView& shard, const SurfelsView& cloud, uint32_t rank, uint32_t world, uint32_t chunk);
void launch_cloud_to_shard(hipStream_t st, const SurfelsView& cloud, const SurfelsView& shard, uint32_t rank, uint32_t world, uint32_t chunk);
size_t sort_scratch_bytes(uint32_t n);
hipError_t sort_surfels_spatially(hipStream_t st, const SurfelsView& s, float inv_cell, void* scratch, size_t scratch_bytes);   // stream-ordered, no host wait
size_t scan_temp_bytes(size_t n);
hipError_t scan_flags_inclusive(hipStream_t st, void* temp, size_t temp_bytes, const uint8_t* flags, uint32_t* out, int n);
hipError_t scan_u32_exclusive(hipStream_t st, void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, int n);
hipError_t launch_compact(hipStream_t st, const SurfelsView& s, uint32_t* invalid, uint32_t* free_rank, uint32_t* free_list,
                          uint32_t surfel_count, void* temp, size_t temp_bytes);


// The flavoured launchers (same parameters as the public names above, no defaults: only the dispatchers call them) and the test
// hooks / counters that live with them, declared in both flavour namespaces.
#define BAHIP_FLAVOURED_DECLARATIONS                                                                                                          \
  /* kernels_surfel.hip */                                                                                                                    \
  void launch_activation(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, uint32_t surfels_size); \
  void launch_normals(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s);                       \
  bool launch_geometry(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* kfs, int num_kfs,              \
                       const SurfelsView& s, long long activate_count, const uint32_t* sched, const int* stop, const GeometryFused* fused);   \
  void set_geometry_fused(int threshold, int window);                                                                                         \
  bool geometry_takes_fused_route(uint32_t surfels, bool use_desc, bool settled);                                                             \
  void launch_geometry_phase(hipStream_t stream, int phase, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* kfs,          \
                             int num_kfs, const SurfelsView& s, long long activate_count, const ClassPartials& cpn, const ClassPartials& cpp); \
  void launch_activation_hits(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s,                \
                              uint32_t surfels_size, int kf_rank, int kf_world, uint32_t* hits);                                              \
  void launch_normals_phase(hipStream_t stream, int phase, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s,      \
                            const ClassPartials& cp);                                                                                         \
  void set_tile_waves(int waves);                                                                                                             \
  long long geometry_hybrid_launches();                                                                                                       \
  /* kernels_pose.hip */                                                                                                                      \
  void launch_pose_accumulate(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames,                 \
                              const void* work, int num_work, const SurfelsView& s, HbFixed* Hb, void* tile_bounds, bool stored_bounds,       \
                              int num_listed, uint32_t* tile_counters, int* parity_inout, uint32_t* tile_cost, const uint32_t* sched,         \
                              const int* listed_count, const int* stop);                                                                      \
  bool pose_round_can_be_queued_ahead(uint32_t surfels, int num_items, bool have_tile_counters);                                              \
  void set_pose_lds_waves(int waves);                                                                                                         \
  void set_pose_lds_parts_shift(int shift);                                                                                                   \
  void set_pose_lds_items(int items);                                                                                                         \
  long long pose_kernel_dispatches();                                                                                                         \
  void pose_form_launches(long long out[2], bool reset);                                                                                      \
  void set_pose_form(int form);                                                                                                               \
  void set_pose_parts(int parts);                                                                                                             \
  void launch_evaluate_pairs(hipStream_t stream, const Intrinsics& in, const KfEntry& frame, const SurfelsView& s, const uint32_t* indices,   \
                             int count, float* out);                                                                                          \
  /* kernels_intrinsics.hip */                                                                                                                \
  void launch_intrinsics_accumulate(hipStream_t st, bool depth, bool color, const Intrinsics& in, const KfEntry* kfs, int num_kfs,            \
                                    const SurfelsView& s, double* glob, double* cells, const IntrBins& bins, const uint32_t* sched,           \
                                    uint32_t position_begin, uint32_t position_count, int classes, int kf_rank, int kf_world);                \
  /* kernels_pcg.hip */                                                                                                                       \
  void launch_pcg_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,         \
                       const SurfelsView& s, float* r, float* M, uint32_t* tile_cost, const uint32_t* sched, const PcgClasses* classes);      \
  void launch_pcg_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs, int num_kfs,        \
                        const SurfelsView& s, const float* p, float* g, const void* ctl, const uint32_t* sched, uint32_t* tile_counters,      \
                        int* parity_inout, const PcgClasses* classes);                                                                        \
  void set_pcg_lds_form(int mode);                                                                                                            \
  void pcg_step1_form_launches(long long out[2]);                                                                                             \
  /* kernels_pcg_window.hip */                                                                                                                \
  void launch_pcg_window_init(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs,              \
                              const PcgWindow& w, const SurfelsView& s, float* r, float* M);                                                  \
  void launch_pcg_window_step1(hipStream_t st, const PcgLayout& L, const PcgExact& ex, const Intrinsics& in, const KfEntry* kfs,             \
                               const PcgWindow& w, const SurfelsView& s, const float* p, float* g, const void* ctl);                    \
  /* kernels_cull_probe.hip */                                                                                                                \
  void launch_tile_cull_probe(hipStream_t stream, const Intrinsics& in, const KfEntry* kfs, int num_kfs, const SurfelsView& s, float* bounds, \
                              unsigned long long* masks);
namespace exact { BAHIP_FLAVOURED_DECLARATIONS }
namespace fast { BAHIP_FLAVOURED_DECLARATIONS }
#define BAHIP_PICK(in, call) do { if ((in).fast_math) fast::call; else exact::call; } while (0)

// kernels_cost.hip: the value of the BA objective per keyframe.  Output row of a keyframe (kCostWords int64, summed over workgroups and
// ranks as integers): the ExactCells of the depth, descriptor-1 and descriptor-2 sums, the depth residual count, the descriptor pair
// count and a non-finite flag.  Launch shape: `waves` wavefronts per workgroup, at most `workgroups` of them, keyframes in slices of
// at most `slice` (the LDS table of a workgroup: slice x kCostWords x 8 bytes).
constexpr int kCostCellWords = 9;   // = kExactLimbs (exact_sum.h; kernels_cost.hip checks)
constexpr int kCostWords = 3 * kCostCellWords + 3;
constexpr int kCostDepthCountWord = 3 * kCostCellWords, kCostPairCountWord = kCostDepthCountWord + 1, kCostFlagWord = kCostDepthCountWord + 2;
constexpr int kCostMaxWaves = 8;
constexpr int kCostMaxSlice = 256;   // 60 KB of LDS: two workgroups of 8 wavefronts per compute unit
struct CostShape {
  int waves, workgroups, slice;
};
namespace exact {
void launch_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                 int kf_world, const SurfelsView& s, const uint32_t* sched, const CostShape& shape, long long* out);
}
namespace fast {
void launch_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                 int kf_world, const SurfelsView& s, const uint32_t* sched, const CostShape& shape, long long* out);
}
void launch_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                 int kf_world, const SurfelsView& s, const uint32_t* sched, const CostShape& shape, long long* out);
// rows [num][kCostWords] (summed over the ranks) -> out[0 .. num): per row, out[num]: the total from the summed limbs; `total`: kCostWords
// zeroed words of scratch
void launch_cost_resolve(hipStream_t stream, const long long* rows, int num, long long* total, bahip_cost* out);

// kernels_surfel_cost.hip: the value of the BA objective per surfel.  Output planes (device, one entry per surfel, any may be NULL);
// launch shape: `waves` wavefronts per workgroup (each with its own accumulator block in LDS), at most `workgroups` of them.
constexpr int kSurfelCostMaxWaves = 8;
constexpr int kSurfelCostLdsPerWave = 3 * kCostCellWords * 64 * 8;   // 13 824 bytes: three exact accumulators per lane
// default shape: one wavefront per workgroup (13.5 KB), 11 workgroups per compute unit (148.5 of its 160 KB) -- the fastest of the
// shapes scripts/surfel_cost_eval.py times ("The objective per surfel")
constexpr int kSurfelCostDefaultWaves = 1, kSurfelCostWorkgroupsPerUnit = 11;
struct SurfelCostPlanes {
  double *depth, *descriptor_1, *descriptor_2;
  uint32_t *depth_residuals, *descriptor_pairs;
};
struct SurfelCostShape {
  int waves, workgroups;
};
// The sweep over the surfels [surfel_begin, min(surfel_end, s.size)) (surfel_begin a multiple of 64) against the keyframes of `frames`
// this rank owns.  rows == NULL: every entry of that range of `out` is written, resolved.  rows != NULL (keyframe sharding): word w of
// surfel i goes to rows[w * row_stride + (i - surfel_begin)] (kCostWords planes), for the sum over the ranks and
// launch_surfel_cost_resolve.  *error: a refused opt-in for the LDS of more than 4 wavefronts per workgroup (nothing launched).
namespace exact {
void launch_surfel_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                        int kf_world, const SurfelsView& s, uint32_t surfel_begin, uint32_t surfel_end, const uint32_t* sched,
                        const SurfelCostShape& shape, const SurfelCostPlanes& out, long long* rows, uint32_t row_stride, hipError_t* error);
}
namespace fast {
void launch_surfel_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                        int kf_world, const SurfelsView& s, uint32_t surfel_begin, uint32_t surfel_end, const uint32_t* sched,
                        const SurfelCostShape& shape, const SurfelCostPlanes& out, long long* rows, uint32_t row_stride, hipError_t* error);
}
void launch_surfel_cost(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, int num_kfs, int kf_rank,
                        int kf_world, const SurfelsView& s, uint32_t surfel_begin, uint32_t surfel_end, const uint32_t* sched,
                        const SurfelCostShape& shape, const SurfelCostPlanes& out, long long* rows, uint32_t row_stride, hipError_t* error);
// the summed staging planes of the surfels [begin, begin + count) -> their entries of `out`
void launch_surfel_cost_resolve(hipStream_t stream, const long long* rows, uint32_t stride, uint32_t begin, uint32_t count, const SurfelCostPlanes& out);

// kernels_pose_trial.hip: the pose phase under step control.  The record the controlled solve keeps per work item: the limbs of the
// normal equations and the cost at the accepted pose (PoseWork::T), the cost the phase began with, the candidate the next sweep
// evaluates (its frame_T_global is PoseWork::F), the damping factor and the counters.
struct PoseTrialRecord {
  HbFixed Hb[kHbStride];
  bahip_cost cost, cost_before;
  float T_candidate[7];
  float lambda;
  int32_t candidate_converged;     // the step to the candidate passed the convergence test on x
  int32_t consecutive_rejected;
  int32_t trials, rejected;        // candidates evaluated / rejected so far
  int32_t evaluated, pad_;         // round 0 has run for this item: it is a work item of the phase (its keyframe was not kInactive)
};
static_assert(sizeof(PoseTrialRecord) % 8 == 0, "the records sit in a buffer of 64-bit words");
// control words of a controlled phase: [0], [1] = entries of the two lists of items still iterating (round r appends to list r & 1, the
// sweep of round r + 1 reads it), [kPoseTrialInvalid] = the sticky flag of the plain phase's kPoseCounterInvalid
constexpr int kPoseTrialInvalid = 2, kPoseTrialWords = 4;
namespace exact {
int launch_pose_trial_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, const void* work,
                            int num_work, const int* listed, int num_items, const SurfelsView& s, HbFixed* Hb, long long* cost_rows,
                            void* tile_bounds, bool stored_bounds, const uint32_t* sched);
void set_pose_trial_shape(int waves, int parts_shift);
}
namespace fast {
int launch_pose_trial_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, const void* work,
                            int num_work, const int* listed, int num_items, const SurfelsView& s, HbFixed* Hb, long long* cost_rows,
                            void* tile_bounds, bool stored_bounds, const uint32_t* sched);
void set_pose_trial_shape(int waves, int parts_shift);
}
// The fused sweep: Hb[w] += the normal equations and cost_rows[w] += the cost row (kCostWords) of every item's pose PoseWork::F, for the
// items listed[0 .. num_items) (NULL: the work items 0 .. num_items) that are not skipped.  stored_bounds as launch_pose_accumulate.
// Returns a hipError_t (the opt-in for a large LDS table can be refused).
int launch_pose_trial_sweep(hipStream_t stream, bool use_depth, bool use_desc, const Intrinsics& in, const KfEntry* frames, const void* work,
                            int num_work, const int* listed, int num_items, const SurfelsView& s, HbFixed* Hb, long long* cost_rows,
                            void* tile_bounds, bool stored_bounds, const uint32_t* sched);
void launch_pose_trial_solve(hipStream_t stream, void* work, int num_work, PoseTrialRecord* records, HbFixed* Hb, long long* cost_rows, KfEntry* frames,
                             const bahip_pose_step_control& control, int update_activation, int round, const float* lambda_in, int* ctl,
                             int* list_next);
void set_pose_trial_shape(int waves, int parts_shift);   // test hook: wavefronts per workgroup (0: 16), 2^shift wavefronts share a tile's items (-1: from the grid size)
void launch_pose_step_damped_debug(hipStream_t stream, const float* in, float* out);

// kernels_geometry_trial.hip: the geometry phase under step control.  Per surfel the five words a geometry step may write (x, y, z,
// descriptor_1, descriptor_2; plane r of `saved`), whether its trial is still open, and its outcome so far; `stride` entries per plane.
constexpr int kGeometryTrialWords = 5, kGeometryTrialBlock = 256;
struct GeometryTrialState {
  uint32_t* saved;
  uint8_t* open;
  uint8_t* outcome;
  uint32_t stride;
};
// control words of a controlled step, kept by the one-workgroup count launch behind every decide launch: the surfels still open (what
// the host reads per trial) and the totals of bahip_geometry_step_stats
constexpr int kGeometryTrialCtlOpen = 0, kGeometryTrialCtlCandidates = 1, kGeometryTrialCtlAccepted = 2, kGeometryTrialCtlRejectedCost = 3,
              kGeometryTrialCtlRejectedPairs = 4, kGeometryTrialCtlWords = 8;
void launch_geometry_trial_snapshot(hipStream_t st, const SurfelsView& s, const GeometryTrialState& state);
// the candidate of trial `trial` (damping `lambda`) for the open surfels from the position pass's class partials `cpp` (2 or 8 sums)
void launch_geometry_trial_solve(hipStream_t st, const SurfelsView& s, const ClassPartials& cpp, int classes, bool use_desc, float lambda, int trial,
                                 const GeometryTrialState& state);
// keep or undo per open surfel (c0: the cost planes before the trials, c1: of the candidate state), then the counts into `ctl`;
// partials: 4 words per workgroup of kGeometryTrialBlock surfels
void launch_geometry_trial_decide(hipStream_t st, const SurfelsView& s, const SurfelCostPlanes& c0, const SurfelCostPlanes& c1, bool guard_pairs,
                                  int trial, const GeometryTrialState& state, uint32_t* partials, uint32_t* ctl);
void launch_geometry_trial_finish(hipStream_t st, uint32_t size, const GeometryTrialState& state, uint8_t* out /* may be NULL */);
void launch_geometry_trial_restore(hipStream_t st, const SurfelsView& s, const GeometryTrialState& state);

// kernels_intrinsics_trial.hip: the intrinsics step under step control.  The damped Schur complement from the binary64 sums the sweep
// left (arguments and scratch as launch_intrinsics_finish; lambda = 0: its bits), the back-substitution from a source plane into a
// destination plane, and the copy of a pitched plane that leaves the padding alone.
constexpr int kIntrinsicsTrialBlock = 256;
void launch_intrinsics_trial_schur(hipStream_t st, bool schur, int S, float lambda, const double* glob_d, const double* cells_d, float* glob_f,
                                   float* cells_f, float* partials);
void launch_intrinsics_trial_backsub(hipStream_t st, int cf_width, int S, const float* cells_f, const float* x1, const float* src,
                                     uint32_t src_pitch, float* dst, uint32_t dst_pitch);
void launch_intrinsics_trial_plane_copy(hipStream_t st, int width, int height, const float* src, uint32_t src_pitch, float* dst, uint32_t dst_pitch);

// kernels_render.hip: the surfel map rendered into a camera view (exists once: exact arithmetic under either flavour).  The view camera
// travels as an Intrinsics of which only the depth camera's members are filled (make_intrinsics of the view for both cameras).
constexpr int kRenderMaxWaves = 8, kRenderMaxRadiusPx = 16;
constexpr int kRenderDefaultWaves = 4, kRenderWorkgroupsPerUnit = 16;
struct RenderParams {
  float F[12];               // frame_T_global
  int mode, max_radius_px, cull_backfaces;
  float radius_factor, min_depth, max_depth;
  float max_focal;           // max(fx, fy) of the view camera
  uint32_t index_base;
};
struct RenderPlanes {        // device, dense row-major width x height; any may be NULL
  unsigned long long* key;
  float* depth;
  uint32_t* index;
  float* normal;             // three floats per pixel
  uint32_t* color;           // the winner's row-5 word
};
struct RenderShape {
  int waves, workgroups;
};
void launch_render_clear(hipStream_t stream, unsigned long long* keys, uint32_t pixels);
// one lane per surfel, atomic minima into `keys`; counters != NULL: the census variant, which adds the candidate tests to counters[0]
// and the candidates that contributed a key (each one atomic) to counters[1]
void launch_render_splat(hipStream_t stream, const Intrinsics& view, const RenderParams& rp, const SurfelsView& s, const RenderShape& shape,
                         unsigned long long* keys, unsigned long long* counters);
void launch_render_resolve(hipStream_t stream, const RenderParams& rp, const SurfelsView& s, const unsigned long long* keys, uint32_t pixels,
                           const RenderPlanes& out);

// kernels_residual_image.hip: a frame's depth and descriptor residuals per pixel (exists once: the exact flavour's association under
// either flavour).  What the kernels need of the frame; the planes (device, dense row-major width x height of the depth camera, any of
// the resolve's may be NULL); the sweep's launch shape.
constexpr int kResidualImageMaxWaves = 8;
constexpr int kResidualImageDefaultWaves = 4, kResidualImageWorkgroupsPerUnit = 16;
struct ResidualFrame {
  float F[12];               // frame_T_global
  const uint32_t* geom;      // the frame's tiled BA planes (KfEntry::geom, ::lumafp)
  const uint32_t* lumafp;
};
struct ResidualImagePlanes {
  uint32_t* index;
  float* depth_residual;
  float* inv_stddev;
  float* desc_residual;      // two floats per pixel
  uint8_t* color_valid;
};
struct ResidualImageShape {
  int waves, workgroups;
};
void launch_residual_image_clear(hipStream_t stream, unsigned long long* keys, uint32_t* counts, uint32_t pixels);
// one lane per surfel: on associated lanes an atomic minimum into `keys` and an atomic add into `counts`; select 0 = best, 1 = worst
void launch_residual_image_sweep(hipStream_t stream, const Intrinsics& in, const ResidualFrame& frame, const SurfelsView& s, int select,
                                 uint32_t index_base, const ResidualImageShape& shape, unsigned long long* keys, uint32_t* counts);
// the planes from the winning keys; descriptors are evaluated only when desc_residual or color_valid is asked for
void launch_residual_image_resolve(hipStream_t stream, const Intrinsics& in, const ResidualFrame& frame, const SurfelsView& s, uint32_t index_base,
                                   const unsigned long long* keys, uint32_t pixels, const ResidualImagePlanes& out);

// kernels_covisibility.hip: observed co-visibility, the surfels every pair of keyframes shares (exists once: the exact flavour's
// association under either flavour).  counts: device, num_kfs rows of `pitch` words; launch shape: `waves` wavefronts per workgroup, at
// most `workgroups` of them, `list_capacity` (keyframe, mask) entries per wavefront in LDS (12 bytes each) before a tile takes passes.
constexpr int kCovisMaxWaves = 8, kCovisMaxListCapacity = 512, kCovisEntryBytes = 12;   // 8 x 512 x 12 bytes = 48 KB of LDS at most
// default shape: 8 wavefronts per workgroup (12 KB), 4 workgroups per compute unit -- the fastest of the shapes
// scripts/covisibility_eval.py times ("Observed co-visibility")
constexpr int kCovisDefaultWaves = 8, kCovisWorkgroupsPerUnit = 4, kCovisDefaultListCapacity = 128;
struct CovisShape {
  int waves, workgroups, list_capacity;
};
void launch_covisibility_clear(hipStream_t stream, uint32_t* counts, int num_kfs, uint32_t pitch);
// counts[i][j] += surfels of s associated with both keyframes, for i >= j (the lower triangle: launch_covisibility_mirror completes the
// matrix); pair_stage false: the traversal and the lists only, no atomic (timing);
// census: NULL or three zeroed words (entries with a non-zero mask, atomic adds issued, tiles with more entries than the list holds)
void launch_covisibility_sweep(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                               const uint32_t* sched, const CovisShape& shape, bool pair_stage, uint32_t* counts, uint32_t pitch,
                               unsigned long long* census);
void launch_covisibility_mirror(hipStream_t stream, uint32_t* counts, int num_kfs, uint32_t pitch);
// the compact num_kfs x num_kfs words as int64 (what the ranks of a surfel partition sum), and the summed words into pitched rows
void launch_covisibility_widen(hipStream_t stream, const uint32_t* compact, int num_kfs, long long* wide);
void launch_covisibility_narrow(hipStream_t stream, const long long* wide, int num_kfs, uint32_t* counts, uint32_t pitch);

// kernels_observations.hip: observation lists, the keyframes paired with each surfel in compressed rows (exists once: the exact
// flavour's association and residual bits under either flavour).  Launch shape: `waves` wavefronts per workgroup, at most `workgroups`
// of them; stage_entries 0: the direct fill (each lane stores into its own list), > 0: the staged fill, the first stage_entries entries
// of a tile assembled in LDS per wavefront and written with coalesced stores, the entries beyond stored at once.
constexpr int kObsMaxWaves = 8, kObsMaxStageEntries = 4096;
constexpr int kObsKeyframeBytes = 2, kObsDepthBytes = 4, kObsDescriptorBytes = 8;   // of a staged entry, per plane asked for
constexpr int kObsMaxLdsBytes = 65536;                                              // waves x stage_entries x entry bytes at most
// default shape and window: the fastest of those scripts/surfel_observations_eval.py times ("Observation lists")
constexpr int kObsDefaultWaves = 4, kObsWorkgroupsPerUnit = 4, kObsDefaultStageEntries = 1024;
struct ObsShape {
  int waves, workgroups, stage_entries;
};
struct ObsPlanes {   // device; keyframes required for a fill, the payload planes may be NULL
  uint16_t* keyframes;
  float* depth_raw;
  float* descriptor_raw;
};
inline size_t obs_entry_bytes(const ObsPlanes& p) {
  return (size_t)kObsKeyframeBytes + (p.depth_raw ? kObsDepthBytes : 0) + (p.descriptor_raw ? kObsDescriptorBytes : 0);
}
// counts[s] = the keyframes paired with surfel s, for s < s.size (counts[s.size] is not written); *total (zeroed) += their sum
void launch_observations_count(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                               const uint32_t* sched, const ObsShape& shape, uint32_t* counts, unsigned long long* total);
// the entries [first[s], first[s + 1]) of every plane given, for s < s.size: first is the exclusive scan of the counts (s.size + 1 words)
void launch_observations_fill(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                              const uint32_t* sched, const ObsShape& shape, const uint32_t* first, const ObsPlanes& planes);

// kernels_redundancy.hip: keyframe redundancy, per keyframe its surfels by the number of other keyframes that observe them (exists
// once: the exact flavour's association under either flavour).  hist: device, num_kfs rows of `pitch` words, `bins` of them written;
// launch shape: `waves` wavefronts per workgroup, at most `workgroups` of them, `list_capacity` (keyframe, mask) entries per wavefront
// in LDS before a tile is traversed a second time.  A wavefront's LDS: list_capacity + 64 entries of 12 bytes (the list, and one
// (bin, mask) entry per bin present in the tile).
constexpr int kRedundancyMaxBins = 64, kRedundancyMaxWaves = 8, kRedundancyMaxListCapacity = 448, kRedundancyEntryBytes = 12;   // 48 KB at most
constexpr int kRedundancyDefaultWaves = 8, kRedundancyWorkgroupsPerUnit = 4, kRedundancyDefaultListCapacity = 128;
struct RedundancyShape {
  int waves, workgroups, list_capacity;
};
void launch_redundancy_clear(hipStream_t stream, uint32_t* hist, int num_kfs, int bins, uint32_t pitch);
// hist[k][min(o, bins - 1)] += the surfels of s associated with keyframe k that o other keyframes are associated with; attribute false:
// the traversal, the counts and the lists only, no atomic (timing);
// census: NULL or three zeroed words ((tile, keyframe) entries, atomic adds issued, tiles traversed a second time)
void launch_redundancy_sweep(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, const SurfelsView& s,
                             const uint32_t* sched, const RedundancyShape& shape, bool attribute, int bins, uint32_t* hist, uint32_t pitch,
                             unsigned long long* census);
// the compact num_kfs x bins words as int64 (what the ranks of a surfel partition sum), and the summed words into pitched rows
void launch_redundancy_widen(hipStream_t stream, const uint32_t* compact, uint32_t words, long long* wide);
void launch_redundancy_narrow(hipStream_t stream, const long long* wide, int num_kfs, int bins, uint32_t* hist, uint32_t pitch);

// kernels_tile_masks.hip: the tile mask table -- per tile of 64 surfels the (keyframe, 64-bit ballot) entries with a non-zero ballot,
// ascending by keyframe -- built over a keyframe partition, and the observed co-visibility, the keyframe redundancy and the
// observation lists computed from it (exists once: the exact flavour's association under either flavour).  Launch shape: `waves`
// wavefronts per workgroup, at most `workgroups` of them.
constexpr int kTileMaskMaxWaves = 8, kTileMaskBinBytes = 12;   // LDS of the redundancy reduction: 64 (bin, mask) entries per wavefront
constexpr int kTileMaskDefaultWaves = 4, kTileMaskWorkgroupsPerUnit = 4;   // the observation sweeps' shape: the same traversal
struct TileMaskShape {
  int waves, workgroups;
};
struct TileMaskTable {   // device
  const uint32_t* tile_first;          // tiles + 1 words
  const uint32_t* keyframes;           // entries
  const unsigned long long* masks;     // entries
  uint32_t tiles, entries;
};
// the entries of the keyframes k with (k & owner_mask) == owner_rank per tile: counts[t] (zeroed) and this rank's 16-bit field of
// plane[t * plane_words + owner_rank / 4] (zeroed); *listed (zeroed) += their number
void launch_tile_mask_count(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                            const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, uint32_t* counts, long long* plane,
                            uint32_t plane_words, unsigned long long* listed);
// from the summed plane: totals[t] (tiles + 1 words, the last zero: the input of the scan into tile_first) and the entries of the
// ranks below `rank` per tile
void launch_tile_mask_offsets(hipStream_t stream, const long long* plane, uint32_t plane_words, uint32_t tiles, uint32_t rank, uint32_t world,
                              uint32_t* totals, uint32_t* rank_offset);
// this rank's entries at tile_first[t] + rank_offset[t] + the running index of zero-filled planes of `entries` entries
void launch_tile_mask_fill(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                           const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, const uint32_t* counts,
                           const uint32_t* tile_first, const uint32_t* rank_offset, uint32_t entries, uint32_t* keyframes,
                           unsigned long long* masks);
// the entries [begin, begin + count) as count + ceil(count / 4) int64 words (masks, then keyframe indices four to a word), and back
inline size_t tile_mask_slice_words(size_t count) { return count + (count + 3) / 4; }
void launch_tile_mask_pack(hipStream_t stream, const uint32_t* keyframes, const unsigned long long* masks, uint32_t begin, uint32_t count,
                           long long* stage);
void launch_tile_mask_unpack(hipStream_t stream, const long long* stage, uint32_t begin, uint32_t count, uint32_t* keyframes,
                             unsigned long long* masks);
// per tile the runs of the ranks merged into one run ascending in k
void launch_tile_mask_merge(hipStream_t stream, const TileMaskShape& shape, const uint32_t* tile_first, uint32_t tiles, uint32_t entries,
                            const uint32_t* in_kf, const unsigned long long* in_mask, uint32_t* out_kf, unsigned long long* out_mask);
// the reductions over the tiles t with t % world == rank; *adds += the atomic adds issued.  counts: the lower triangle, as
// launch_covisibility_sweep; hist: as launch_redundancy_sweep
void launch_tile_mask_covisibility(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t rank, uint32_t world,
                                   int num_kfs, uint32_t* counts, uint32_t pitch, unsigned long long* adds);
void launch_tile_mask_redundancy(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t rank, uint32_t world,
                                 int num_kfs, int bins, uint32_t* hist, uint32_t pitch, unsigned long long* adds);
// counts[s] for s < surfels and *total (zeroed) += their sum; the keyframes plane from the scan of the counts; the payload of this
// rank's keyframes into zero-filled planes (either may be NULL), *words += the payload words written
void launch_tile_mask_observation_counts(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t surfels,
                                         uint32_t* counts, unsigned long long* total);
void launch_tile_mask_observation_keyframes(hipStream_t stream, const TileMaskShape& shape, const TileMaskTable& table, uint32_t surfels,
                                            const uint32_t* first, uint16_t* keyframes);
void launch_tile_mask_payload(hipStream_t stream, const Intrinsics& in, const KfEntry* frames, int num_kfs, uint32_t owner_mask, uint32_t owner_rank,
                              const SurfelsView& s, const uint32_t* sched, const TileMaskShape& shape, const TileMaskTable& table,
                              const uint32_t* first, float* depth_plane, float* desc_plane, unsigned long long* words);
// the 32-bit words [begin, begin + count) of a plane as ceil(count / 2) int64 words, and back
void launch_tile_mask_words_pack(hipStream_t stream, const uint32_t* plane, size_t begin, uint32_t count, long long* stage);
void launch_tile_mask_words_unpack(hipStream_t stream, const long long* stage, size_t begin, uint32_t count, uint32_t* plane);
// census[0 .. 3) = (entries, *adds, 0)
void launch_tile_mask_census(hipStream_t stream, unsigned long long entries, const unsigned long long* adds, unsigned long long* census);

// kernels_ingest.hip: a frame brought to the BA's pyramid level (exists once: integer rules and one correctly rounded division, the same
// under either flavour).  The callers have checked sizes and pitches; the downscale's blocks are at most kIngestMaxBlock on a side.
constexpr int kIngestMaxBlock = 9, kIngestMaxLevels = 3;
void launch_median_densify(hipStream_t stream, const uint16_t* in, uint32_t in_pitch, uint16_t* out, uint32_t out_pitch, int w, int h);
void launch_downscale_depth_median(hipStream_t stream, const uint16_t* in, uint32_t in_pitch, int in_w, int in_h, uint16_t* out,
                                   uint32_t out_pitch, int out_w, int out_h);
// non-zero: levels outside 1 .. kIngestMaxLevels
int launch_downscale_rgb_half(hipStream_t stream, const uint8_t* in, uint32_t in_pitch, int w, int h, int levels, uint8_t* out, uint32_t out_pitch);

}  // namespace bahip
