// capi_internal.h -- what the translation units of the C boundary (include/badslam_hip.h) share: the context, the error helpers and the
// helpers one unit defines and the others call.  Not part of the ABI.
//   capi.hip            context, allocation, streams, preprocessing entry points, scene binding, stage timers
//   capi_rccl.hip       transports of a multi-GPU run: the RCCL loader, the reduction over the ranks, shard gather / extract
//   capi_ba.hip         the stages of the alternating scheme, the Gauss-Newton rounds, the device-driven loop
//   capi_lifecycle.hip  supporting surfels, merging, creation (single and batched), deletion, compaction, spatial order
//   capi_solvers.hip    the intrinsics step and the PCG scheme (whole iteration and stage by stage)
//   capi_debug.hip      test hooks and experiment switches
//   capi_cost.hip       the value of the BA objective (bahip_evaluate_cost, bahip_evaluate_frame_cost)
//   capi_surfel_cost.hip the value of the BA objective per surfel (bahip_evaluate_surfel_costs)
//   capi_render.hip     the surfel map rendered into a camera view (bahip_render_surfels)
//   capi_residual_image.hip a frame's residuals per pixel (bahip_frame_residual_image)
//   capi_covisibility.hip the surfels every pair of keyframes shares (bahip_observed_covisibility)
//   capi_observations.hip the keyframes paired with each surfel, in compressed rows (bahip_surfel_observations)
//   capi_redundancy.hip per keyframe its surfels by the number of other observers (bahip_keyframe_observer_histogram)
//   capi_tile_masks.hip the tile mask table: those three calls under keyframe sharding, and on route 1 elsewhere
//   capi_pcg_trial.hip  step control of the PCG scheme
//   capi_pose_trial.hip step control of the pose phase of the alternating scheme
//   capi_geometry_trial.hip step control of the geometry phase of the alternating scheme
//   capi_intrinsics_trial.hip step control of the intrinsics step of the alternating scheme
// Ownership: every block of device or page-locked memory the boundary allocates for itself is a DeviceBuffer / PinnedBuffer
// (capi_buffers.h) -- a member of bahip_context, of bahip_frame_planes or of an UploadStage, or a local of a test hook -- and is freed
// with its owner; a unit grows one with reserve().  Only memory handed to the caller (bahip_malloc_pitch, bahip_host_alloc) is raw.
#pragma once

#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <thread>

#include <string>
#include <vector>

#include "ba_launch.h"
#include "capi_buffers.h"
#include "exact_sum.h"
#include "ldlt.h"
#include "se3_device.h"

namespace bahip_capi {
using namespace bahip;

int fail(const char* what, const char* file, int line, hipError_t e = hipSuccess);   // sets the error text, returns 1

#define HIP_TRY(expr)                                                  \
  do {                                                                 \
    hipError_t _e = (expr);                                            \
    if (_e != hipSuccess) return fail(#expr, __FILE__, __LINE__, _e);  \
  } while (0)
#define REQUIRE(cond, msg)                                             \
  do {                                                                 \
    if (!(cond)) return fail(msg, __FILE__, __LINE__);                 \
  } while (0)
#define CHECK_LAUNCH() HIP_TRY(hipGetLastError())

struct StageTimer {
  std::vector<hipEvent_t> ev;   // pairs (start, stop)
  std::vector<char> skip;       // per pair: not a launch that did work (queued ahead in vain): left out of sums and counts
  int used = 0;                 // number of pairs used by the last call (mode 1) / since set_profiling (mode 2)
  long long units = 0;          // work units of those launches (stage 2: keyframes still iterating)
};


}  // namespace bahip_capi
using bahip_capi::DeviceBuffer;
using bahip_capi::PinnedBuffer;
using bahip_capi::kHostVisible;
using bahip_capi::StageTimer;
using namespace bahip;

// Tiled BA planes of one frame (ba_device.h).  Opaque to the C API.
struct bahip_frame_planes {
  DeviceBuffer<uint32_t> geom, lumafp;
  int width = 0, height = 0, cwidth = 0, cheight = 0;
};

// A small host-to-device upload without a host wait: the bytes are copied into a page-locked buffer the context owns and go out with
// hipMemcpyAsync; the event says when the buffer may be overwritten (checked -- normally long over -- by the next upload through the
// same stage).  Scene binding used to synchronise the stream three times per BundleAdjustment call for its three tables.
struct UploadStage {
  PinnedBuffer<char> pinned;
  hipEvent_t done = nullptr;
  bool pending = false;
};
int stage_upload(UploadStage* stage, void* dev_dst, const void* src, size_t bytes, hipStream_t stream,
                 const void* src2 = nullptr, size_t bytes2 = 0, void* dev_dst2 = nullptr);
void stage_free(UploadStage* stage);

constexpr int kGatherTableWords = 128;   // bahip_gather_surfel_shards: (size, count) of at most 64 ranks
constexpr int kDealStats = 8;            // bahip_debug_lifecycle_deal_stats
constexpr int kIntrMaxSlices = 16;   // slices of the intrinsics sweep (capi_solvers.hip): automatic up to 8, forced up to 16 (half the record memory again)
struct bahip_context {
  UploadStage stage_kfs, stage_covis, stage_window;
  UploadStage stage_gather;        // bahip_gather_surfel_shards: the (size, count) table goes up and comes back through its page-locked buffer
  DeviceBuffer<long long> dev_gather_table;   // ... and is summed here (kGatherTableWords int64, allocated once)
  hipStream_t stream = nullptr;
  bool have_intrinsics = false;
  bahip_camera color_cam{}, depth_cam{};
  bahip_depth_params dp{};
  Intrinsics in{};

  std::vector<KfEntry> host_kfs;
  DeviceBuffer<KfEntry> dev_kfs;
  int num_kfs = 0;

  DeviceBuffer<PoseWork> dev_work;
  DeviceBuffer<HbFixed> dev_Hb;   // pose normal equations in fixed point (ba_device.h: HbFixed)
  int work_capacity = 0;          // keyframes dev_work, dev_Hb and pinned_work are laid out for (ensure_work)
  DeviceBuffer<KfEntry> dev_frame1;   // single-frame table for EstimateFramePose / AccumulatePoseEstimationCoeffs
  DeviceBuffer<PoseWork> dev_work1;
  PinnedBuffer<PoseWork> pinned_work1{kHostVisible};
  DeviceBuffer<HbFixed> dev_Hb1;
  DeviceBuffer<uint32_t> dev_tile_counters;   // persistent pose sweep: two sets of 8 tile counters (kernels_pose.hip)
  int pose_parity = 0;                     // the set the next persistent launch draws from

  DeviceBuffer<int> dev_counter;   // [0] generic counter, [1..2] min/max depth bits
  PinnedBuffer<int> pinned_i;      // 16 ints
  PinnedBuffer<float> pinned_f;    // 128 floats

  DeviceBuffer<uint8_t> dev_flags;     // W*H new-surfel flags
  DeviceBuffer<uint32_t> dev_indices;  // W*H scan output
  DeviceBuffer<void> scan_temp;
  DeviceBuffer<int> dev_covis;
  DeviceBuffer<float> dev_covis_T;     // 12 floats per entry of dev_covis
  // co-visibility lists of the bound keyframes (CSR over bound indices), for the device-side activation state machine
  std::vector<int> covis_offsets, covis_indices;
  DeviceBuffer<int> dev_covis_csr; // offsets (K + 1) followed by the indices
  bool capacity_exceeded = false;  // last bahip_create_surfels_for_keyframe did not fit (bahip_context_take_capacity_exceeded)
  bool have_covisibility = false;
  std::vector<uint8_t> window;     // per bound keyframe: inside the fixed active window (bahip_set_activation_window)
  DeviceBuffer<uint8_t> dev_window;
  PinnedBuffer<PoseWork> pinned_work{kHostVisible};   // read-back of the pose work items + their counter records (page-locked)
  // a creation batch as a chain of one launch per keyframe (bahip_create_surfels_for_keyframes; kernels_lifecycle.hip: create_chain_kernel):
  // per keyframe of the batch the bytes "cell occupied" and "pixel would create a surfel", and the batch's item table
  DeviceBuffer<void> dev_merge_batch;    // bahip_merge_surfels_for_keyframes by cell lists: frame table, counts, offsets, pair cells, members, scan temporary
  DeviceBuffer<void> dev_sort_scratch;   // bahip_sort_surfels_spatially: keys, indices, a dense copy of the data rows, the library's temporary
  DeviceBuffer<void> dev_create_batch;   // occupancy, candidates, their scan, the compact candidate list with its records, the item table
  DeviceBuffer<uint32_t> merge_planes[BAHIP_MERGE_BUFFER_COUNT];   // the second set of supporting planes of a pipelined merge batch (bahip_merge_surfels_for_keyframes)
  const void* supporting_planes_empty = nullptr;   // the supporting planes (by their first plane) that the last merge call left empty
  bool row_major_creation = false;   // new surfels of a keyframe appended in row-major pixel order (the reference's) instead of tile-major
  bool poll_disabled = false;        // the host copy of the pose counters is not updated by the kernel on this system: synchronise instead
  // lifecycle batch (bahip_lifecycle_batch_begin): bounding spheres of the cloud's whole tiles, for the per-keyframe sweeps of a batch
  DeviceBuffer<void> dev_lifecycle_bounds;
  size_t lifecycle_bounds_capacity = 0;   // tiles
  uint32_t lifecycle_bounds_tiles = 0;    // 0: no batch open
  const void* lifecycle_bounds_data = nullptr;   // the surfel buffer they describe
  // ... and, when the batch knows its frames (bahip_lifecycle_batch_set_frames), which of those tiles each frame can see
  std::vector<float> lifecycle_frames;           // 12 floats per frame: frame_T_global as given
  std::vector<uint32_t> lifecycle_list_offsets, lifecycle_list_counts;
  DeviceBuffer<float> dev_lifecycle_frames;
  DeviceBuffer<uint32_t> dev_lifecycle_cursors;  // [2 * frames]: cursors, offsets
  DeviceBuffer<uint32_t> dev_lifecycle_lists;
  DeviceBuffer<void> dev_tile_bounds;   // bounding sphere per 64-surfel tile, written by the first pose round of a phase
  // heavy work first (wave_cull.h: scheduled_tile): candidates per tile counted by the first pose round of a phase over the
  // keyframe table (or by the PCG init sweep), and the schedule built from them, valid for grids of tile_order_tiles (padded)
  // tiles (0: none yet)
  DeviceBuffer<uint32_t> dev_tile_cost, dev_tile_order;
  size_t tile_schedule_capacity = 0;   // tiles
  uint32_t tile_order_tiles = 0;
  int phases_since_schedule = 0;       // the schedule is rebuilt when the grid changes and every kSchedulePhases-th phase
  uint32_t tile_order_unavailable_tiles = 0;   // a grid the order kernel cannot schedule (too many runs): no census for it again
  bool tile_order_unavailable_for(uint32_t padded_tiles) const { return padded_tiles != 0 && tile_order_unavailable_tiles == padded_tiles; }
  // the geometry step's fused route (ba_launch.h: GeometryFused): per tile the word of deferred lanes and the route byte, sized with the
  // surfel capacity when the route is first taken; fused_launch_tiles: tiles of the last launch ENQUEUED on it (bahip_debug_geometry_fused_stats;
  // a launch behind a raised stop word writes nothing, the arrays then hold what the launch before it left)
  DeviceBuffer<unsigned long long> dev_fused_deferred;
  DeviceBuffer<uint8_t> dev_fused_route;
  uint32_t fused_launch_tiles = 0;
  DeviceBuffer<int> dev_loop_ctl;  // device-driven BA loop (bahip_alternating_iterations): kLoopWords control words ...
  PinnedBuffer<int> host_loop_ctl{kHostVisible};   // ... their mapped host copy, followed by kLoopLogSlots words of per-round log
  int rounds_hint_table = 1, rounds_hint_frame = 1;   // Gauss-Newton rounds the previous pose phase took (keyframe table / single frame)

  DeviceBuffer<void> intr_scratch; // intrinsics step: (64 + 8 S) doubles, then (64 + 8 S) floats + Schur partials
  int intr_capacity = 0;
  // append buffers of the intrinsics sweep's per-cell records (ba_launch.h: IntrBins), sized from the previous call's counts
  DeviceBuffer<uint32_t> intr_bin_cursors;   // device, intr_bin_count words
  DeviceBuffer<uint32_t> intr_bin_records;
  PinnedBuffer<uint32_t> intr_bin_counts_host;   // pinned copy of the cursors after the sweep
  int intr_bin_count = 0;
  int intr_bin_sets = 0;                  // buffer sets allocated: 2 when the sweep runs in slices (one is reduced while the other fills)
  int intr_bin_rows = 0;                  // rows of counts (one per slice) the last call left in intr_bin_counts_host
  int intr_slices_forced = 0;             // bahip_debug_set_intrinsics_slices: > 0 fixes the number of slices of the sweep
  hipStream_t intr_aux_stream = nullptr;  // the reductions of a sliced sweep run here
  hipEvent_t intr_events[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t intr_bin_capacity = 0;         // records per block the buffers hold
  uint32_t intr_bin_wanted = 0;           // records per block the next call should have room for (0: estimate)
  int intr_bin_forced = -1;
  int intr_bin_last_overflow = 0;         // did the last call have records that did not fit?               // bahip_debug_set_intrinsics_bin_capacity: >= 0 fixes the capacity (0: no binning)

  DeviceBuffer<float> pcg_buf;     // PCG vectors r, M, delta, g, p (5 * pcg_capacity floats) + 16 scalars
  size_t pcg_capacity = 0;
  DeviceBuffer<ExactCell> pcg_exact;   // exact accumulators of the PCG solve (kernels_pcg.hip)
  DeviceBuffer<uint32_t> pcg_window;   // windowed PCG (kernels_pcg_window.hip): [tile count | keyframe list | pose indices | tile list]
  uint32_t pcg_window_last_tiles = 0;   // tiles and swept keyframes of the last windowed call (bahip_pcg_window_size)
  int pcg_window_last_kfs = 0;
  DeviceBuffer<void> pcg_stage_ctl;   // stage API (bahip_pcg_begin ...): a control block that never stops, the head size the
  uint32_t pcg_stage_head = 0;     // accumulators were set up for, and the bahip_pcg_step1 calls since the last step 2
  int pcg_stage_step1_calls = 0;
  float pcg_damping = 0.f;         // lambda of the damped PCG system (bahip_context_set_pcg_damping; kernels_pcg_trial.hip)
  DeviceBuffer<uint32_t> pcg_trial;    // bahip_pcg_iteration_controlled: [tile count | tile list] followed by the snapshot
  DeviceBuffer<long long> pose_trial;  // bahip_estimate_keyframe_poses_controlled: [Hb | cost rows] (what the ranks exchange), records, lambdas, lists, control words
  // bahip_optimize_geometry_iteration_controlled: [position class partials | saved words | cost planes c0, c1 | open | outcome | count
  // partials | control words]; the partials stay until the next controlled call (bahip_debug_read_geometry_sums)
  DeviceBuffer<double> geometry_trial;
  int geometry_trial_sums = 0;           // sums per surfel the last controlled call consumed (2 or 8; 0: none yet), their classes,
  int geometry_trial_classes = 0;        // surfels and plane stride
  uint32_t geometry_trial_size = 0, geometry_trial_stride = 0;
  int geometry_trial_timing = 0;         // bahip_debug_geometry_trial_timing
  double geometry_trial_ms[4] = {};
  DeviceBuffer<float> intrinsics_trial;  // bahip_optimize_intrinsics_controlled: the saved cfactor plane (rows of cf_width words, no padding)
  double intrinsics_trial_ms[4] = {};    // bahip_debug_intrinsics_trial_timing: sweep, cost sweeps, solve + back-substitution, host waits
  int intrinsics_trial_timing = 0;
  int world = 0;                   // ranks of the RCCL communicator (0 = none)
  int kf_rank = 0, kf_world = 1;   // keyframe sharding (bahip_context_set_keyframe_sharding): keyframe k lives on rank k % kf_world (1, 2, 4 or 8)
  int arithmetic = 0;              // BAHIP_ARITHMETIC_EXACT / _FAST: flavour of the sweeps (bahip_context_set_arithmetic), mirrored in in.fast_math
  int sum_classes = 4;             // interleaved partial sums per surfel of the normals / geometry passes: 4 or 8 (bahip_context_set_sum_classes)
  int intrinsics_sum_classes = 1;  // keyframe classes of the intrinsics step's global sums: 1, 2, 4 or 8 (bahip_context_set_intrinsics_sum_classes)
  int pcg_sum_classes = 1;         // keyframe classes of the surfel block of the PCG scheme's r, M and g: 1, 2, 4 or 8 (bahip_context_set_pcg_sum_classes)
  int intr_sums_cells = -1;        // sparse cells of the accumulators the last intrinsics step left in intr_scratch (-1: none; bahip_debug_read_intrinsics_sums)
  DeviceBuffer<float> kf_partials; // class partials of the geometry step (normals, then position) / hit words of the activation
  DeviceBuffer<long long> dev_cost;   // rows of the cost sweep (kernels_cost.hip): kCostWords int64 per keyframe
  DeviceBuffer<long long> dev_surfel_cost_rows;   // keyframe sharding: staged words of one slice of the per-surfel cost sweep (kernels_surfel_cost.hip)
  DeviceBuffer<unsigned long long> render_keys;   // bahip_render_surfels: the dense width x height key plane the splat takes its minima in (kernels_render.hip)
  DeviceBuffer<unsigned long long> render_counters;   // bahip_debug_render_census: two counters
  // bahip_frame_residual_image: the dense key and pair-count planes of the sweep, when the caller passes NULL for them (kernels_residual_image.hip)
  DeviceBuffer<unsigned long long> residual_keys;
  DeviceBuffer<uint32_t> residual_counts;
  // bahip_observed_covisibility: the three census words of the last call, and, with a transport installed, the words of a shard
  // ([K x K int64 | K x K uint32]) that are summed over the ranks (kernels_covisibility.hip)
  DeviceBuffer<unsigned long long> covis_census;
  DeviceBuffer<long long> covis_stage;
  // bahip_surfel_observations: the per-surfel counts (surfels_size + 1 words, the last zero), their 64-bit total and the scan's
  // storage (kernels_observations.hip)
  DeviceBuffer<uint32_t> obs_counts;
  DeviceBuffer<unsigned long long> obs_total;
  DeviceBuffer<void> obs_scan_temp;
  // bahip_keyframe_observer_histogram: the three census words of the last call, and, with a transport installed, the words of a shard
  // ([K x bins int64 | K x bins uint32]) that are summed over the ranks (kernels_redundancy.hip)
  DeviceBuffer<unsigned long long> redundancy_census;
  DeviceBuffer<long long> redundancy_stage;
  // the tile mask table of the last call that built one (capi_tile_masks.hip, kernels_tile_masks.hip): per-tile words ([own counts
  // T + 1 | totals T + 1 | entries of the lower ranks T | tile_first T + 1]), the count plane the ranks sum, the entries in the
  // rank-major layout and merged, one slice of staging for the sums over the ranks, four counters (entries this rank listed, atomic
  // adds, payload words, the pair total) and the scan's storage; what the last call left (bahip_debug_read_tile_masks, _stats)
  DeviceBuffer<uint32_t> tile_mask_words;
  DeviceBuffer<long long> tile_mask_plane;
  DeviceBuffer<uint32_t> tile_mask_raw_keyframes, tile_mask_keyframes;
  DeviceBuffer<unsigned long long> tile_mask_raw_masks, tile_mask_masks;
  DeviceBuffer<long long> tile_mask_stage;
  DeviceBuffer<unsigned long long> tile_mask_counters;
  DeviceBuffer<void> tile_mask_scan_temp;
  uint32_t tile_mask_tiles = 0, tile_mask_entries = 0;
  bool tile_mask_valid = false;
  long long tile_mask_exchanges = 0, tile_mask_consumer_tiles = 0;
  // dealing the lifecycle under surfel sharding (bahip_context_set_lifecycle_dealing): the switch, and the surfel partition of the
  // whole-cloud phase in progress -- set by bahip_gather_surfel_shards, cleared by bahip_extract_surfel_shard (deal_world 1: none) --
  // with the gathered cloud it belongs to: lifecycle calls on any other buffer are not dealt
  int lifecycle_dealing = 0;
  int deal_rank = 0, deal_world = 1;
  uint32_t deal_chunk = 0;
  const void* deal_data = nullptr;
  long long deal_stats[kDealStats] = {};   // what this rank swept of the dealt phases (bahip_debug_lifecycle_deal_stats)
  long long exchange_calls = 0;    // sums over the ranks requested since the last reset (bahip_exchange_stats), and their bytes
  long long exchange_bytes = 0;

  // planes packed by the library itself for frames handed over without bahip_frame.planes:
  // slot 0 = the single frame of the per-frame entry points, slot 1 + k = bound keyframe k
  std::vector<std::unique_ptr<bahip_frame_planes>> auto_planes;
  // and for frame j of a merge batch by cell lists (at most 64 frames): a pool of its own, so that a batch in any order never
  // writes into the planes a bound keyframe's table entry points at
  std::vector<std::unique_ptr<bahip_frame_planes>> batch_planes;

  bahip_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  void* rccl_comm = nullptr;       // ncclComm_t created by bahip_context_init_rccl (native all-reduce on ctx->stream)

  int profiling = 0;               // 0 off, 1 last call of each stage, 2 cumulative since bahip_set_profiling
  StageTimer timers[8];              // 0 activation, 1 geometry, 2 pose accumulate, 3 pose solve, 4 intrinsics (whole step), 5 PCG step-1 sweep,
                                     // 6 intrinsics sweep alone, 7 intrinsics reduction of the binned records alone
};

namespace bahip_capi {

// ---- defined in capi.hip --------------------------------------------------------------------------------------------------------
Intrinsics make_intrinsics(const bahip_camera& cc, const bahip_camera& dc, const bahip_depth_params& dp);
void fill_pose(KfEntry* e, const float* global_T_frame);
int planes_alloc(int width, int height, int cwidth, int cheight, bahip_frame_planes** out);
void planes_free(bahip_frame_planes* p);
KfEntry raw_entry(const bahip_frame& f);
int make_entry(bahip_context* ctx, const bahip_frame& f, size_t slot, KfEntry* out);
int make_batch_entry(bahip_context* ctx, const bahip_frame& f, size_t j, KfEntry* out);
SurfelsView make_view(const bahip_surfels* s);
int ensure_work(bahip_context* ctx, int n);
int ensure_px(bahip_context* ctx, size_t px, size_t scan_n);
inline bool timer_on(const bahip_context* ctx, int stage) { return ctx->profiling && (ctx->profiling != 3 || stage == 2); }
void timer_begin(bahip_context* ctx, int stage, bool first, int units = 1);
void timer_end(bahip_context* ctx, int stage);
inline bool kf_sharded(const bahip_context* ctx) { return ctx->kf_world > 1; }
int ensure_tile_bounds(bahip_context* ctx, uint32_t surfels);
int geometry_fused_for(bahip_context* ctx, const bahip_surfels* surfels, bool use_desc, bool settled, GeometryFused* out);
inline uint32_t surfel_tiles(uint32_t surfels) { return (surfels + 63u) / 64u; }
extern int g_tile_order_enabled;
int ensure_tile_schedule(bahip_context* ctx, uint32_t padded_tiles);
const uint32_t* tile_order_for(const bahip_context* ctx, uint32_t surfels);

// ---- defined in capi_ba.hip -----------------------------------------------------------------------------------------------------
int wait_for_pose_sequence(bahip_context* ctx, PoseWork* host_work, const PoseWork* dev_work, int num_work, int sequence);
extern int g_fused_iteration_begin, g_pose_rounds_ahead, g_device_loop_enabled;
int run_pose_rounds(bahip_context* ctx, bool use_depth, bool use_desc, const KfEntry* dev_frames, KfEntry* dev_frames_rw,
                    PoseWork* dev_work, HbFixed* dev_Hb, int num_work, const SurfelsView& s, int write_back, int update_activation,
                    PoseWork* host_work /* page-locked, num_work + kPoseTailRecords records */, int* rounds_out,
                    bool schedule = false /* a phase over the keyframe table: its first round counts the candidates per tile and the
                    run order of the following sweeps is rebuilt from them */, int* rounds_hint = nullptr,
                    int first_round = 0, int first_iterating = -1 /* continue a phase whose rounds [0, first_round) have run (the
                    device-driven loop hands over a phase that needs more rounds than it had queued) */,
                    const PoseLoopControl* loop_stats = nullptr /* keeps the loop's totals going (never ends a phase) */);
int geometry_keyframe_sharded(bahip_context* ctx, bool use_depth, bool use_desc, const SurfelsView& v, long long activate_count);

// ---- defined in capi_solvers.hip ------------------------------------------------------------------------------------------------
// What the accumulate part of the intrinsics step leaves: the binary64 sums (after the exchange over the ranks) and the scratch of the
// Schur complement, all inside ctx->intr_scratch; and what the record buffers' bookkeeping needs once the stream has been waited for.
struct IntrinsicsSweep {
  bool swept = false;   // false: nothing was swept (no surfels and no sharding); nothing below is set
  int S = 0;            // sparse cells
  double* glob_d = nullptr; double* cells_d = nullptr;
  float* glob = nullptr; float* cells = nullptr; float* partials = nullptr;
  uint32_t bin_capacity = 0;
  int num_bins = 0, slices = 1;
};
int intrinsics_accumulate(bahip_context* ctx, int optimize_depth, int optimize_color, const bahip_surfels* surfels,
                          bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a, IntrinsicsSweep* sweep);
void intrinsics_accumulate_done(bahip_context* ctx, const IntrinsicsSweep& sweep);

// ---- defined in capi_rccl.hip ---------------------------------------------------------------------------------------------------
int reduce_over_ranks(bahip_context* ctx, void* buffer, size_t count, int dtype);
void rccl_destroy_communicator(bahip_context* ctx);   // (context destruction)
inline bool is_sharded(const bahip_context* ctx) { return ctx->allreduce != nullptr || ctx->rccl_comm != nullptr; }
inline bool kf_owned(const bahip_context* ctx, int k) { return (k & (ctx->kf_world - 1)) == ctx->kf_rank; }
// owned[c]: this rank sweeps keyframe class c of `classes` -- class c lives on rank c % kf_world (both powers of two, kf_world <= classes)
inline uint32_t owned_classes(const bahip_context* ctx, int classes) {
  uint32_t owned = 0;
  for (int c = 0; c < classes; ++c) if ((c & (ctx->kf_world - 1)) == ctx->kf_rank) owned |= 1u << c;
  return owned;
}
// The lifecycle dealt over the ranks of a surfel partition (bahip_context_set_lifecycle_dealing): on, inside a whole-cloud phase of two or
// more ranks (a power of two: the dealt kernels test ownership as k & (world - 1)), with a transport, never under keyframe sharding.
// Bound keyframe k belongs to rank k % deal_world; surfel i of the gathered cloud to rank (i / deal_chunk) % deal_world.  Only a call on
// the buffer the phase's gather filled is dealt (a host that gathers without extracting leaves no stale partition for other buffers).
inline bool lifecycle_dealt(const bahip_context* ctx, const bahip_surfels* surfels) {
  return ctx->lifecycle_dealing && ctx->deal_world > 1 && (ctx->deal_world & (ctx->deal_world - 1)) == 0 && !kf_sharded(ctx) && is_sharded(ctx) &&
         surfels != nullptr && surfels->data != nullptr && surfels->data == ctx->deal_data;
}
inline bool deal_owned(const bahip_context* ctx, int k) { return (k & (ctx->deal_world - 1)) == ctx->deal_rank; }
// ---- defined in capi_tile_masks.hip ---------------------------------------------------------------------------------------------
// The observed structure by way of the tile mask table: under keyframe sharding always, elsewhere on route 1
// (bahip_debug_set_observed_structure_route).  The three entry points hand over after their refusals, with K > 0.
bool observed_structure_by_table(const bahip_context* ctx);
int tile_mask_covisibility(bahip_context* ctx, const bahip_surfels* surfels, uint32_t* counts, int pitch_words);
int tile_mask_histogram(bahip_context* ctx, const bahip_surfels* surfels, int bins, uint32_t* hist, int pitch_words);
int tile_mask_observations(bahip_context* ctx, const bahip_surfels* surfels, const bahip_observations* out, uint64_t pair_limit, uint64_t* pairs);

#define REQUIRE_NO_KF_SHARDING(what) \
  REQUIRE(!kf_sharded(ctx), what " is not available under keyframe sharding (its per-surfel sums run over all keyframes in order): use surfel sharding")

}  // namespace bahip_capi
