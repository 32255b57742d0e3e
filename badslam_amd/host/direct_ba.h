// direct_ba.h -- vis::DirectBA, the direct bundle-adjustment back-end of BAD SLAM, with the public
// surface of the reference class (B/direct_ba.h:65-550; B/ = applications/badslam/src/badslam/):
// same constructor arguments, same method names, argument meaning and defaults, same accessors.
// Everything below the surface is new: the scene lives in HIP buffers, and every stage is one call
// into the C ABI of the MI355X backend (include/badslam_hip.h) instead of a loop of per-keyframe
// kernel launches.  Differences forced by the platform:
//   - cudaStream_t -> hipStream_t (opaque), cudaTextureObject_t -> hipTextureHandle_t (gfx950 has
//     no texture sampling; the handle names the colour buffer),
//   - render window / OpenGL interop and loop-detector hooks are not part of the BA path
//     (OUT) and are omitted,
//   - SetRunParallel is declared but never defined in the reference (B/direct_ba.h:172): omitted.
#pragma once

#include <limits>
#include <string>
#include <utility>

#include "camera_frustum.h"
#include "keyframe.h"

namespace vis {

constexpr int kMergeBufferCount = BAHIP_MERGE_BUFFER_COUNT;       // B/kernels.cuh:51
constexpr int kSurfelAttributeCount = BAHIP_SURFEL_ATTRIBUTE_COUNT;
constexpr int kSurfelX = 0, kSurfelY = 1, kSurfelZ = 2, kSurfelNormal = 3, kSurfelRadiusSquared = 4, kSurfelColor = 5,
              kSurfelDescriptor1 = 6, kSurfelDescriptor2 = 7, kSurfelAccum0 = 8;   // B/kernels.cuh:69-88

struct Point3fC3u8Nf;   // rgbd_io.h (L/point_cloud.h: the element of Point3fC3u8NfCloud)
class DirectBA {
 public:
  DirectBA(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
           float surfel_merge_dist_factor, int min_observation_count_while_bootstrapping_1,
           int min_observation_count_while_bootstrapping_2, int min_observation_count,
           const PinholeCamera4f& color_camera_initial_estimate, const PinholeCamera4f& depth_camera_initial_estimate,
           int pyramid_level_for_color, bool use_depth_residuals, bool use_descriptor_residuals,
           void* render_window /* must be nullptr */, const SE3f& global_T_anchor_frame);
  ~DirectBA();

  void AddKeyframe(const shared_ptr<Keyframe>& new_keyframe);
  void DeleteKeyframe(int keyframe_index, void* loop_detector = nullptr);
  void MergeKeyframes(hipStream_t stream, void* loop_detector, usize approx_merge_count = 10);
  // B/direct_ba.h:175, B/direct_ba.cc:461-547: the valid surfels as a point cloud (position, colour, normal), in index order
  void ExportToPointCloud(hipStream_t stream, vector<Point3fC3u8Nf>* cloud);
  void CreateSurfelsForKeyframe(hipStream_t stream, bool filter_new_surfels, const shared_ptr<Keyframe>& keyframe);
  void EstimateFramePose(hipStream_t stream, const SE3f& global_T_frame_initial_estimate, const CUDABuffer<u16>& depth_buffer,
                         const CUDABuffer<u16>& normals_buffer, hipTextureHandle_t color_texture,
                         SE3f* out_global_T_frame_estimate, bool called_within_ba);
  void BundleAdjustment(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool do_surfel_updates,
                        bool optimize_poses, bool optimize_geometry, int min_iterations, int max_iterations, bool use_pcg,
                        int active_keyframe_window_start, int active_keyframe_window_end, bool increase_ba_iteration_count,
                        int* iterations_done = nullptr, bool* converged = nullptr, double time_limit = 0, Timer* timer = nullptr,
                        int pcg_max_inner_iterations = 30, int pcg_max_keyframes = 2500,
                        std::function<bool(int)> progress_function = nullptr);
  // The value of the objective BundleAdjustment minimises (bahip_evaluate_cost: exact sums, the same bits under either sharding), with
  // this object's residual switches, over every keyframe and surfel.  per_keyframe: indexed by keyframe id, deleted ids left at zero.
  struct BACost {
    double depth = 0, descriptor_1 = 0, descriptor_2 = 0;
    uint64_t depth_residuals = 0, descriptor_pairs = 0;
  };
  void ComputeCost(hipStream_t stream, BACost* total, vector<BACost>* per_keyframe = nullptr);
  // The same objective per surfel (bahip_evaluate_surfel_costs): for every entry of the surfel buffer, in buffer order, the exact sums
  // of its terms over all keyframes and its counts -- zeros for a deleted surfel or one no keyframe sees, NaN sums for a surfel with a
  // non-finite term.  Each vector gets surfels_size() entries.  Keyframe sharding: every rank gets the unsharded values; surfel
  // sharding: the values of this rank's shard (nothing is exchanged).  Waits for the stream.
  struct SurfelCosts {
    vector<double> depth, descriptor_1, descriptor_2;
    vector<uint32_t> depth_residuals, descriptor_pairs;
  };
  void ComputeSurfelCosts(hipStream_t stream, SurfelCosts* out);
  // Observed co-visibility (bahip_observed_covisibility; DESIGN.md section 3, "Observed co-visibility"): counts[i * K + j] = the surfels
  // the association rule pairs with both the i-th and the j-th existing keyframe, K x K row-major, both triangles, the diagonal a
  // keyframe's own pair count; keyframe_ids[i] = the id of row i (deleted keyframes are not rows, as with ComputeCost).  Nothing acts on
  // the values: the co-visibility lists of the keyframes stay the frustum test's.  Surfel sharding with an all-reduce installed: every
  // rank gets the unsharded matrix; keyframe sharding: the same, by way of the tile mask table.  Waits for the stream.
  void ComputeObservedCovisibility(hipStream_t stream, vector<uint32_t>* counts, vector<int>* keyframe_ids);
  // The reduced camera system (bahip_reduced_camera_system; DESIGN.md section 3, "The reduced camera system") with this object's
  // residual switches: S (6K x 6K row-major) and g (6K) -- the Gauss-Newton system over the poses of the K existing keyframes with every
  // surfel eliminated, 6 unknowns per keyframe in the tangent convention of the pose phase, no gauge removed --, A_diag (K x 36) and b
  // (K x 6) the keyframes' own pose equations; keyframe_ids[i] = the id of block i.  marginalise false: S = blockdiag(A), g = b.
  // Nothing acts on the values.  Surfel sharding with an all-reduce installed: the unsharded system on every rank; not available under
  // keyframe sharding.  Waits for the stream.
  struct ReducedCameraSystem {
    vector<double> S, g, A_diag, b;
    vector<int> keyframe_ids;
    uint64_t list_entries = 0, pairs_visited = 0, atomics_issued = 0, degenerate_surfels = 0, overflow_tiles = 0, invalid = 0;
  };
  void ComputeReducedCameraSystem(hipStream_t stream, ReducedCameraSystem* out, bool marginalise = true);
  // Marginal pose covariances from the reduced camera system: the 6 rows and columns of gauge_keyframe_id are deleted, the rest is
  // factored in binary64 (L D L^T in the order of the blocks, no pivoting) and inverted.  keyframe_ids: the remaining keyframes in
  // order; marginal: their 6 x 6 covariance blocks (36 words each); for every pair (i, j) of ids in `pairs` the 6 x 6 block between
  // them goes to cross (rows of i, columns of j).  Returns false with *error set and nothing else written when the gauge keyframe does
  // not exist, a pair names it or an unknown id, or a pivot is not positive (the poses are not determined: too few observations, or
  // the sums were invalid).
  struct PoseCovariances {
    vector<int> keyframe_ids;
    vector<double> marginal, cross;
  };
  bool ComputePoseCovariances(hipStream_t stream, int gauge_keyframe_id, PoseCovariances* out, const vector<std::pair<int, int>>* pairs = nullptr,
                              std::string* error = nullptr);
  // The same from a system already computed (no GPU work).
  static bool PoseCovariancesOf(const ReducedCameraSystem& system, int gauge_keyframe_id, PoseCovariances* out,
                                const vector<std::pair<int, int>>* pairs, std::string* error);
  // Observation lists (bahip_surfel_observations; DESIGN.md section 3, "Observation lists"): the associated (surfel, keyframe) pairs in
  // compressed rows by surfel.  first: surfels_size + 1 offsets, first.back() = the number of pairs; keyframes[first[s] .. first[s + 1]):
  // the keyframes paired with surfel s as indices into keyframe_ids, ascending; keyframe_ids[k] = the id of bound index k (deleted
  // keyframes are not bound, as with ComputeCost).  with_residuals: entry for entry depth_raw (the pair's raw depth residual) and
  // descriptor_raw (two words per entry; NaN twice where the pair's colour pixel is not valid); otherwise both stay empty.  A count
  // call sizes the buffers, a second call fills them.  Surfel sharding: this rank's shard; keyframe sharding: the unsharded lists on
  // every rank (every rank must ask for the same).  Waits for the stream.
  struct SurfelObservations {
    vector<uint32_t> first;
    vector<uint16_t> keyframes;
    vector<int> keyframe_ids;
    vector<float> depth_raw, descriptor_raw;
  };
  void ComputeSurfelObservations(hipStream_t stream, SurfelObservations* out, bool with_residuals = false);
  // Keyframe redundancy (bahip_keyframe_observer_histogram; DESIGN.md section 3, "Keyframe redundancy"): hist[i * bins + j] = the
  // surfels the association rule pairs with the i-th existing keyframe that min(o, bins - 1) = j OTHER keyframes are paired with as
  // well, K x bins row-major, 1 <= bins <= 64; keyframe_ids[i] = the id of row i (deleted keyframes are not rows, as with
  // ComputeObservedCovisibility).  Surfel sharding with an all-reduce installed: every rank gets the unsharded table; keyframe
  // sharding: the same, by way of the tile mask table (FindRedundantKeyframes and CullRedundantKeyframes with it: DeleteKeyframe moves
  // the ownership of the later keyframes, whose images the object must hold).  Waits for the stream.
  void ComputeKeyframeRedundancy(hipStream_t stream, int bins, vector<uint32_t>* hist, vector<int>* keyframe_ids);
  // The keyframes the map does without: with total = a row's sum and covered = its sum over the bins j >= min_other_observers
  // (<= bins - 1), a keyframe qualifies when total > 0 and (double)covered >= min_fraction * (double)total.  keyframe_ids: the ids of
  // the qualifying keyframes, most redundant first (covered / total compared by the 64-bit cross products covered_a * total_b and
  // covered_b * total_a), ties to the lower id.  Deletes nothing.
  void FindRedundantKeyframes(hipStream_t stream, int min_other_observers, double min_fraction, vector<int>* keyframe_ids, int bins = 16);
  // Greedy culling by that rule: in each round the table is computed again (a deletion lowers the observer counts of the deleted
  // keyframe's surfels) and DeleteKeyframe is called on the first keyframe of FindRedundantKeyframes that is neither the first existing
  // keyframe nor among the protect_newest last ones; stops when none qualifies or max_deletions keyframes are deleted.  deleted_ids: the
  // ids in the order of deletion.  Nothing in the library calls it.
  void CullRedundantKeyframes(hipStream_t stream, int min_other_observers, double min_fraction, int max_deletions, int protect_newest,
                              vector<int>* deleted_ids);
  // The surfel map seen from a camera (bahip_render_surfels; DESIGN.md section 3, "Rendered views of the map"): per pixel of `view` at
  // pose global_T_frame the nearest surfel's depth, buffer index, normal in the view's frame and colour, row-major.  Empty pixels hold
  // depth 0, index 0xFFFFFFFF, normal (0, 0, 0), colour 0.  Binds nothing; under surfel sharding the view of this rank's shard.  Waits
  // for the stream.
  struct RenderOptions {
    bool disc = true;              // false: one pixel per surfel
    int max_radius_px = 4;         // 0 .. 16: half-width of a disc's candidate box (part of the definition of the image)
    bool cull_backfaces = true;
    float radius_factor = 1.f;
    float min_depth = 0.f, max_depth = std::numeric_limits<float>::infinity();
    uint32_t index_base = 0;
  };
  struct RenderedView {
    int width = 0, height = 0;
    vector<float> depth;           // width * height
    vector<uint32_t> index;        // width * height
    vector<float> normal;          // 3 * width * height
    vector<uint8_t> color;         // 4 * width * height: the surfels' colour row as stored (r, g, b, the fourth byte)
  };
  void RenderSurfels(hipStream_t stream, const PinholeCamera4f& view, const SE3f& global_T_frame, const RenderOptions& options, RenderedView* out);
  // ... from keyframe `keyframe_index` (an id; it must exist): the depth camera at that keyframe's pose
  void RenderKeyframeView(hipStream_t stream, int keyframe_index, const RenderOptions& options, RenderedView* out);
  // The objective in image space (bahip_frame_residual_image; DESIGN.md section 3, "Residual images"): per pixel of a frame's depth
  // image, row-major, the surfel the BA's association rule pairs with it -- the one with the smallest (worst = false) or largest |depth
  // residual| among the pixel's pairs -- and that pair's residuals, with this object's cameras, depth parameters and cfactor image.
  // Empty pixels hold key all ones, pairs 0, index 0xFFFFFFFF, residuals +0.0, color_valid 0.  Binds nothing; under surfel sharding the
  // image of this rank's shard, as RenderSurfels.  Waits for the stream.
  struct ResidualImageOptions {
    bool worst = false;
    uint32_t index_base = 0;
  };
  struct ResidualImage {
    int width = 0, height = 0;
    vector<uint64_t> key;            // width * height: (magnitude word << 32) | index
    vector<uint32_t> pairs, index;   // width * height
    vector<float> depth_residual;    // width * height: signed, in standard deviations
    vector<float> inv_stddev;        // width * height: depth_residual / inv_stddev is metres
    vector<float> desc_residual;     // 2 * width * height
    vector<uint8_t> color_valid;     // width * height
  };
  // keyframe `keyframe_index` (an id; it must exist) at its own pose
  void KeyframeResidualImage(hipStream_t stream, int keyframe_index, const ResidualImageOptions& options, ResidualImage* out);
  // any frame with this object's image sizes at any pose; it need not be part of the map (a held-out frame made with
  // CreateKeyframeFromFrame, say)
  void FrameResidualImage(hipStream_t stream, const Keyframe& frame, const SE3f& global_T_frame, const ResidualImageOptions& options,
                          ResidualImage* out);
  void UpdateKeyframeCoVisibility(const shared_ptr<Keyframe>& keyframe);
  // B/direct_ba.h:167, B/direct_ba.cc:456-459: surfel colours := mean of their observations in all keyframes (before an export).
  void AssignColors(hipStream_t stream);

  void Lock() const { ba_thread_mutex_.lock(); }
  void Unlock() const { ba_thread_mutex_.unlock(); }
  std::mutex& Mutex() const { return ba_thread_mutex_; }

  int GetMinObservationCount() const {
    return (keyframes_.size() < 10) ? ((keyframes_.size() < 5) ? min_observation_count_while_bootstrapping_1_
                                                                : min_observation_count_while_bootstrapping_2_)
                                    : min_observation_count_;
  }

  // --- accessors (B/direct_ba.h:226-388) ---
  const vector<shared_ptr<Keyframe>>& keyframes() const { return keyframes_; }
  vector<shared_ptr<Keyframe>>* keyframes_mutable() { return &keyframes_; }
  PinholeCamera4f color_camera() const { lock_guard<mutex> lock(ba_thread_mutex_); return color_camera_; }
  PinholeCamera4f color_camera_no_lock() const { return color_camera_; }
  void SetColorCamera(const PinholeCamera4f& camera) { lock_guard<mutex> lock(ba_thread_mutex_); color_camera_ = camera; }
  int pyramid_level_for_color() const { return pyramid_level_for_color_; }
  void SetPyramidLevelForColor(int level) { pyramid_level_for_color_ = level; }
  PinholeCamera4f depth_camera() const { lock_guard<mutex> lock(ba_thread_mutex_); return depth_camera_; }
  PinholeCamera4f depth_camera_no_lock() const { return depth_camera_; }
  void SetDepthCamera(const PinholeCamera4f& camera) { lock_guard<mutex> lock(ba_thread_mutex_); depth_camera_ = camera; }
  DepthParameters depth_params() const { lock_guard<mutex> lock(ba_thread_mutex_); return depth_params_; }
  DepthParameters depth_params_no_lock() const { return depth_params_; }
  void SetDepthParams(const DepthParameters& params) { lock_guard<mutex> lock(ba_thread_mutex_); depth_params_ = params; }
  float& a() { return depth_params_.a; }
  float a() const { return depth_params_.a; }
  CUDABufferPtr<float> cfactor_buffer() { return cfactor_buffer_; }
  CUDABufferConstPtr<float> cfactor_buffer() const { return cfactor_buffer_; }
  void SetCFactorBuffer(const CUDABufferPtr<float>& cfactor_buffer) {
    cfactor_buffer_ = cfactor_buffer;
    depth_params_.cfactor_buffer = cfactor_buffer_->ToCUDA();
  }
  void IncreaseBAIterationCount() { lock_guard<mutex> lock(ba_thread_mutex_); ++ba_iteration_count_; }
  bool use_depth_residuals() const { return use_depth_residuals_; }
  void SetUseDepthResiduals(bool v) { use_depth_residuals_ = v; }
  bool use_descriptor_residuals() const { return use_descriptor_residuals_; }
  void SetUseDescriptorResiduals(bool v) { use_descriptor_residuals_ = v; }
  int sparse_surfel_cell_size() const { return depth_params_.sparse_surfel_cell_size; }
  void SetSparsificationSideFactor(int cell) { depth_params_.sparse_surfel_cell_size = cell; }
  int min_observation_count_while_bootstrapping_1() const { return min_observation_count_while_bootstrapping_1_; }
  void SetMinObservationCountWhileBootstrapping1(int c) { min_observation_count_while_bootstrapping_1_ = c; }
  int min_observation_count_while_bootstrapping_2() const { return min_observation_count_while_bootstrapping_2_; }
  void SetMinObservationCountWhileBootstrapping2(int c) { min_observation_count_while_bootstrapping_2_ = c; }
  int min_observation_count() const { return min_observation_count_; }
  void SetMinObservationCount(int c) { min_observation_count_ = c; }
  void SetIntrinsicsUpdatedCallback(const std::function<void()>& callback) { intrinsics_updated_callback_ = callback; }
  u32 surfel_count() const { lock_guard<mutex> lock(ba_thread_mutex_); return surfel_count_; }
  u32 surfels_size() const { lock_guard<mutex> lock(ba_thread_mutex_); return surfels_size_; }
  void SetSurfelCount(u32 surfel_count, u32 surfels_size) {
    surfel_count_ = surfel_count; surfels_size_ = surfels_size;
    if (unsorted_surfels_ > surfels_size) unsorted_surfels_ = surfels_size;   // (an emptied buffer has nothing out of order)
  }
  // Not in the reference.  Reorders the surfel buffer along a Morton curve over a world grid (bahip_sort_surfels_spatially):
  // surfels that an image region shows become neighbours in the buffer, which the sweeps' cache behaviour wants.  No
  // result depends on the order; call it when the surfel set has grown (after adding keyframes), not per iteration.
  void SortSurfelsSpatially(hipStream_t stream, float grid_cell_size = 0.02f);
  // Spatial order as part of the reference's own call path (round 4): PerformBASchemeEndTasks -- which compacts, i.e. moves
  // surfels, anyway (B/direct_ba.cc:619-640) -- puts the buffer back into Morton order whenever surfels were appended or moved
  // since the last reorder, so a caller that knows only B/direct_ba.h:73-388 gets the buffer the sweeps are fast on.
  // cell size 0 switches it off (the reference's surfel order stays observable); default 0.02 m.
  // Round 6: the compaction INSIDE the loop (after a merge pass) is followed by the same reorder once the surfels out of order amount
  // to one per 64-surfel tile, so that the call's remaining iterations sweep a coherent buffer (direct_ba.cc: SortAfterInLoopCompaction).
  void SetSpatialSortCellSize(float grid_cell_size) { spatial_sort_cell_size_ = grid_cell_size; }
  void SortAfterInLoopCompaction(hipStream_t stream);
  // Ours: the creations of a BA iteration and the merges of a merge pass as ONE call of the backend each (default:
  // bahip_create_surfels_for_keyframes, bahip_merge_surfels_for_keyframes) or keyframe by keyframe with the host in between (the
  // reference's shape).  Same surfels either way.
  void SetBatchedCreation(bool enabled) { batched_creation_ = enabled; }
  float spatial_sort_cell_size() const { return spatial_sort_cell_size_; }
  u32 unsorted_surfels() const { return unsorted_surfels_; }
  CUDABufferConstPtr<float> surfels() const { return surfels_; }
  CUDABufferPtr<float> surfels() { return surfels_; }
  CUDABufferPtr<u8> active_surfels() { return active_surfels_; }
  int ba_iteration_count() const { return ba_iteration_count_; }
  void SetBAIterationCount(int count) { ba_iteration_count_ = count; }
  int last_ba_iteration_count() const { return last_ba_iteration_count_; }
  void SetLastBAIterationCount(int count) { last_ba_iteration_count_ = count; }
  float surfel_merge_dist_factor() const { return surfel_merge_dist_factor_; }
  void SetSurfelMergeDistFactor(float factor) { surfel_merge_dist_factor_ = factor; }
  void SetSaveTimings(std::ostream* stream) { timings_stream_ = stream; }

  // --- additions of this backend ---
  // The gauge keyframe of the PCG scheme; the reference draws rand() % K per outer iteration
  // (B/direct_ba_pcg.cc:328).  < 0 (default) = same rand() stream; under keyframe sharding keyframe 0 (every rank must hold the
  // same gauge).
  void SetPCGGaugeKeyframe(int keyframe_id) { pcg_gauge_keyframe_ = keyframe_id; }
  // Windowed PCG scheme (ours; default off).  Off: BundleAdjustment(use_pcg) behaves as the reference -- it ignores an active window
  // and does nothing while a keyframe is deleted.  On: deleted keyframes are skipped (the gauge id of SetPCGGaugeKeyframe is
  // translated to its place among the living keyframes), and a fixed window (start > 0 or end > 0) that leaves out a living keyframe
  // runs every outer iteration over it: window activation with co-visible keyframes, surfel creation for the kActive keyframes,
  // surfel activation, normals, bahip_pcg_iteration_windowed.  Every other window is the whole-map iteration.  Refused (returns
  // false) under keyframe sharding and after SetPCGSumClasses(c > 1).
  bool SetWindowedPCG(bool enabled);
  bool windowed_pcg() const { return windowed_pcg_; }
  // Step control of the PCG scheme (ours; default off = NULL: every update is applied, as the reference does).  On: every outer
  // iteration of BundleAdjustment(use_pcg) is bahip_pcg_iteration_controlled -- Marquardt-damped steps (lambda * diag of the
  // Gauss-Newton matrix) that are kept only if ComputeCost's scalar falls strictly, and undone bit for bit otherwise.  lambda starts
  // at lambda_initial when the control is set and is carried across outer iterations and across calls.  An outer iteration without
  // an accepted trial ends the call as converged.  The normals update of each outer iteration runs inside the trial.  Refused
  // (returns false) under keyframe sharding.  The defaults: DESIGN.md section 3.
  struct PCGStepControl {
    float lambda_initial = 1e-3f, lambda_up = 10.f, lambda_down = 0.33f, lambda_min = 0.f, lambda_max = 1e6f;
    int max_trials = 6;
  };
  bool SetPCGStepControl(const PCGStepControl* control);
  bool pcg_step_control() const { return pcg_step_control_on_; }
  float last_pcg_lambda() const { return pcg_lambda_; }                        // the factor the next outer iteration will start with
  int last_pcg_trials() const { return last_pcg_trials_; }                     // trial steps of the last BundleAdjustment() call
  int last_pcg_rejected_steps() const { return last_pcg_rejected_steps_; }     // ... and those of them that were undone
  // Step control of the pose phase of the alternating scheme (ours; default off = NULL: every Gauss-Newton step is taken, as the
  // reference does).  On: BundleAdjustment(!use_pcg) drives its iterations through the stage entry points (the device-driven loop is
  // not used) and its pose phase is bahip_estimate_keyframe_poses_controlled -- per keyframe, a Marquardt-damped step is kept only if
  // that keyframe's cost falls strictly.  The damping factor is kept per keyframe id across iterations and across calls; a keyframe
  // seen for the first time starts at lambda_initial.  Refused (returns false) under keyframe sharding.
  struct PoseStepControl {
    float lambda_initial = 1e-3f, lambda_up = 10.f, lambda_down = 0.33f, lambda_min = 0.f, lambda_max = 1e6f;
    int max_trials = 4;
  };
  bool SetPoseStepControl(const PoseStepControl* control);
  bool pose_step_control() const { return pose_step_control_on_; }
  int last_pose_trials() const { return last_pose_trials_; }                   // candidates evaluated in the last BundleAdjustment() call
  int last_pose_rejected_steps() const { return last_pose_rejected_steps_; }   // ... and those of them that were rejected
  float pose_lambda(int keyframe_id) const {                                   // the factor keyframe_id's next pose phase starts with
    const auto it = pose_lambdas_.find(keyframe_id);
    return it == pose_lambdas_.end() ? pose_step_control_.lambda_initial : it->second;
  }
  // Step control of the geometry phase of the alternating scheme (ours; default off = NULL: every Gauss-Newton step of a surfel is
  // applied, as the reference does).  On: both geometry calls of BundleAdjustment(!use_pcg) are
  // bahip_optimize_geometry_iteration_controlled -- per surfel, a damped step is kept only if that surfel's cost falls strictly (and,
  // with guard_pairs, it loses no associated pair), otherwise its words come back bit for bit; the full-window call passes the
  // activation range, the windowed one keeps the flags.  The device-driven loop is not used.  Allowed under either sharding.
  struct GeometryStepControl {
    float lambda_initial = 0.f, lambda_up = 4.f, lambda_min = 1.f, lambda_max = 1e4f;
    int max_trials = 4;
    bool guard_pairs = true;
  };
  bool SetGeometryStepControl(const GeometryStepControl* control);
  bool geometry_step_control() const { return geometry_step_control_on_; }
  // totals over the geometry calls of the last BundleAdjustment() call: surfels with a candidate, those that ended with an accepted
  // candidate, those that ended with their old words (candidates = accepted + restored), and the trials run
  long long last_geometry_candidates() const { return last_geometry_candidates_; }
  long long last_geometry_accepted() const { return last_geometry_accepted_; }
  long long last_geometry_restored() const { return last_geometry_restored_; }
  int last_geometry_trials() const { return last_geometry_trials_; }
  // Step control of the intrinsics step of the alternating scheme (ours; default off = NULL: every update is applied, as the reference
  // does).  On: the intrinsics step of BundleAdjustment(!use_pcg) is bahip_optimize_intrinsics_controlled -- damped trials up a ladder
  // of factors (0, lambda_first, lambda_first * lambda_up, ... lambda_max), the first one that lowers the objective
  // (bahip_evaluate_cost) strictly is kept, otherwise cameras, a and the cfactor image come back bit for bit; depth and colour updates
  // are kept or undone together.  The factor persists across iterations and calls (an accepted step at l leaves l / lambda_up, a
  // rejected ladder the next rung).  intrinsics_updated_callback is called only after an accepted step.  Allowed under either sharding
  // (keyframe sharding: the plain step's condition on the class count).
  struct IntrinsicsStepControl {
    float lambda_first = 1.f, lambda_up = 4.f, lambda_max = 1e4f;
    int max_trials = 4;
  };
  bool SetIntrinsicsStepControl(const IntrinsicsStepControl* control);
  bool intrinsics_step_control() const { return intrinsics_step_control_on_; }
  // over the intrinsics steps of the last BundleAdjustment() call: trials run, steps accepted, the factor of the last accepted step
  // (-1: none was accepted); and the factor the next step starts with
  int last_intrinsics_trials() const { return last_intrinsics_trials_; }
  int last_intrinsics_accepted() const { return last_intrinsics_accepted_; }
  float last_intrinsics_lambda() const { return last_intrinsics_lambda_; }
  float intrinsics_lambda() const { return intrinsics_lambda_; }
  // ... and by how much those accepted steps lowered the objective (depth + descriptor_1 + descriptor_2): in total, and the smallest
  // drop of one step (0 when none was accepted; positive otherwise, by the accept rule)
  double last_intrinsics_cost_drop() const { return last_intrinsics_cost_drop_; }
  double last_intrinsics_smallest_drop() const { return last_intrinsics_smallest_drop_; }
  // Multi-GPU surfel sharding: sums of the per-keyframe normal equations go through this hook
  // (see include/badslam_hip.h, bahip_allreduce_fn).
  void SetAllReduce(bahip_allreduce_fn fn, void* user) { BAHIP_CHECKED_CALL(bahip_context_set_allreduce(ctx_, fn, user)); }
  // Multi-GPU surfel sharding WITH surfel updates: this object holds rank `rank`'s chunk-cyclic shard of one surfel cloud
  // (chunks of `chunk` surfels, a multiple of 64; see bahip_gather_surfel_shards).  The sweeps of an iteration work on the
  // shard; every phase of the surfel lifecycle (creation, merging, deletion, compaction) assembles the whole cloud on every
  // rank, runs unchanged, and takes the shard back out -- so a sharded BundleAdjustment with do_surfel_updates ends with the
  // bits of the unsharded one.  Needs SetAllReduce (or an RCCL communicator on the backend context) when world > 1.
  void SetSurfelSharding(int rank, int world, u32 chunk);
  // Under surfel sharding (ours; default off): deal the surfel lifecycle's sweeps over the ranks instead of running them on every rank
  // (bahip_context_set_lifecycle_dealing).  The creation batch's and the merge batches' per-keyframe sweeps run on the keyframe's owner
  // (bound index % world), deletion on each rank's own surfel chunks; the results are exchanged and every rank ends with the same bits
  // as with the mode off.  Merging then goes through the by-index batch call, so SetBatchedCreation(false) leaves it replicated.
  // Refused (returns false) under keyframe sharding; does nothing at world 1.
  bool SetDistributedLifecycle(bool enabled);
  bool distributed_lifecycle() const { return distributed_lifecycle_; }
  // Multi-GPU KEYFRAME sharding (bahip_context_set_keyframe_sharding): this object holds ALL surfels; of the keyframes it needs
  // the images of those with (index among the non-deleted keyframes) % world == rank only (world = 1, 2, 4, or 8 after
  // SetSumClasses(8)).  Covers the
  // whole BundleAdjustment call: the alternating scheme over poses, geometry and the depth / colour intrinsics (the intrinsics after
  // SetIntrinsicsSumClasses(c) with c >= world), the PCG scheme (use_pcg, after SetPCGSumClasses(c) with c >= world) and the surfel
  // lifecycle -- creation, merging, deletion and the end tasks (do_surfel_updates, increase_ba_iteration_count) through the batched
  // backend calls by keyframe index, so SetBatchedCreation(false) is refused -- and ends with the unsharded run's bits (same class
  // counts) on every rank.  Needs SetAllReduce or an RCCL communicator when world > 1.
  void SetKeyframeSharding(int rank, int world);
  // The per-surfel sums of the normals / geometry passes are defined over 4 (default) or 8 interleaved keyframe classes
  // (bahip_context_set_sum_classes); keyframe sharding over 8 ranks needs 8 -- and so does the single-GPU run it is compared with.
  void SetSumClasses(int classes);
  // The global sums of the intrinsics step are defined over 1 (default), 2, 4 or 8 keyframe classes
  // (bahip_context_set_intrinsics_sum_classes); keyframe sharding of that step over `world` ranks needs at least `world` -- and the
  // single-GPU run it is compared with the same count.
  void SetIntrinsicsSumClasses(int classes);
  // The surfel block of the PCG scheme's r, M and g is defined over 1 (default), 2, 4 or 8 keyframe classes
  // (bahip_context_set_pcg_sum_classes); keyframe sharding of the PCG scheme over `world` ranks needs at least `world` -- and the
  // single-GPU run it is compared with the same count.
  void SetPCGSumClasses(int classes);
  // Ours: new surfels of a keyframe in the reference's row-major append order (B/kernel_create_surfels.cu:357-390) instead of this
  // backend's tile-major one (bahip_context_set_creation_order): the same surfels, the reference's indices -- and therefore the
  // reference's survivors when surfels merge.  Slower sweeps until the next spatial reorder (SetSpatialSortCellSize).
  void SetRowMajorCreation(bool enabled);
  // Ours: the arithmetic flavour of the sweeps (bahip_context_set_arithmetic).  false (default): every bit is the CPU oracle's; true:
  // hardware reciprocal / square root / exp, contraction, flushed denormals -- what the reference's own -use_fast_math build computes
  // with -- a few percent faster, same determinism and shard invariance, results within the reference's own tolerance.
  void SetFastArithmetic(bool enabled);
  bahip_context* backend_context() { return ctx_; }
  // Binds intrinsics + all non-null keyframes to the backend context; fills index maps between
  // keyframe ids and the dense bound list.  Public so that a caller can drive single bahip_* stages
  // on this scene (the stage-level parity tests do).
  void BindScene(hipStream_t stream);
  bahip_surfels SurfelsStruct(bool with_active = true) const;
  // Statistics of the last BundleAdjustment() call: Gauss-Newton rounds (batched over keyframes)
  // and total per-keyframe GN steps, PCG inner steps.
  int last_pose_rounds() const { return last_pose_rounds_; }
  int last_pose_steps() const { return last_pose_steps_; }
  int last_pcg_inner_steps() const { return last_pcg_inner_steps_; }

 private:
  void BundleAdjustmentAlternating(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics,
                                   bool do_surfel_updates, bool optimize_poses, bool optimize_geometry, int min_iterations,
                                   int max_iterations, int active_keyframe_window_start, int active_keyframe_window_end,
                                   bool increase_ba_iteration_count, int* num_iterations_done, bool* converged, double time_limit,
                                   Timer* timer, std::function<bool(int)> progress_function);
  void BundleAdjustmentPCG(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics, bool do_surfel_updates,
                           bool optimize_poses, bool optimize_geometry, int min_iterations, int max_iterations,
                           int max_inner_iterations, int max_keyframe_count, int active_keyframe_window_start,
                           int active_keyframe_window_end, bool increase_ba_iteration_count, int* num_iterations_done,
                           bool* converged, double time_limit, Timer* timer, std::function<bool(int)> progress_function);
  void DetermineCovisibleActiveKeyframes();
  void DetermineNewKeyframeCoVisibility(const shared_ptr<Keyframe>& new_keyframe);
  void PerformBASchemeEndTasks(hipStream_t stream, bool do_surfel_updates);

  void MergeForKeyframe(const Keyframe& keyframe, bool defer_count = false);
  void TakeDeferredMergeCount();
  void MergeForKeyframes(const vector<u32>& keyframe_ids);
  void CreateSurfelsForKeyframes(hipStream_t stream, bool filter_new_surfels, const vector<u32>& keyframe_ids);
  bool batched_creation_ = true;
  class LifecycleBatch {   // RAII: bahip_lifecycle_batch_begin / _end around the creations or merges of a batch of keyframes
   public:
    explicit LifecycleBatch(DirectBA* ba);
    ~LifecycleBatch();
    LifecycleBatch(const LifecycleBatch&) = delete;
    LifecycleBatch& operator=(const LifecycleBatch&) = delete;
   private:
    DirectBA* ba_;
  };
  bool creation_batch_bound_ = false;
  // Whole-cloud phases under surfel sharding (no-ops without it); they nest, only the outermost pair moves data.
  void EnterWholeCloud(hipStream_t stream);
  void LeaveWholeCloud(hipStream_t stream);
  struct WholeCloudScope {
    WholeCloudScope(DirectBA* ba, hipStream_t stream) : ba_(ba), stream_(stream) { ba_->EnterWholeCloud(stream_); }
    ~WholeCloudScope() { ba_->LeaveWholeCloud(stream_); }
    DirectBA* ba_; hipStream_t stream_;
  };

  PinholeCamera4f color_camera_;
  int pyramid_level_for_color_;
  PinholeCamera4f depth_camera_;
  CUDABufferPtr<float> cfactor_buffer_;
  DepthParameters depth_params_;
  vector<shared_ptr<Keyframe>> keyframes_;
  u32 surfel_count_ = 0, surfels_size_ = 0;
  u32 unsorted_surfels_ = 0;            // appended, or moved by a compaction, since the buffer was last in Morton order
  float spatial_sort_cell_size_ = 0.02f;
  CUDABufferPtr<float> surfels_;
  CUDABufferPtr<u8> active_surfels_;
  int ba_iteration_count_ = 0, last_ba_iteration_count_ = -1;
  bool use_depth_residuals_, use_descriptor_residuals_;
  int min_observation_count_while_bootstrapping_1_, min_observation_count_while_bootstrapping_2_, min_observation_count_;
  float surfel_merge_dist_factor_;
  CUDABufferPtr<u32> supporting_surfels_[kMergeBufferCount];
  mutable mutex ba_thread_mutex_;
  std::ostream* timings_stream_ = nullptr;
  std::function<void()> intrinsics_updated_callback_;
  SE3f global_T_anchor_frame_;

  bahip_context* ctx_ = nullptr;
  vector<int> bound_ids_;        // bound list index -> keyframe id
  vector<int> id_to_bound_;      // keyframe id -> bound list index (-1 for deleted keyframes)
  int pcg_gauge_keyframe_ = -1;
  bool windowed_pcg_ = false;
  bool pcg_step_control_on_ = false;
  PCGStepControl pcg_step_control_;
  float pcg_lambda_ = 0.f;
  int last_pcg_trials_ = 0, last_pcg_rejected_steps_ = 0;
  bool pose_step_control_on_ = false;
  PoseStepControl pose_step_control_;
  std::unordered_map<int, float> pose_lambdas_;   // keyframe id -> damping factor
  int last_pose_trials_ = 0, last_pose_rejected_steps_ = 0;
  bool geometry_step_control_on_ = false;
  GeometryStepControl geometry_step_control_;
  long long last_geometry_candidates_ = 0, last_geometry_accepted_ = 0, last_geometry_restored_ = 0;
  int last_geometry_trials_ = 0;
  bool intrinsics_step_control_on_ = false;
  IntrinsicsStepControl intrinsics_step_control_;
  float intrinsics_lambda_ = 0.f;            // the factor the next controlled intrinsics step starts with
  int last_intrinsics_trials_ = 0, last_intrinsics_accepted_ = 0;
  float last_intrinsics_lambda_ = -1.f;
  double last_intrinsics_cost_drop_ = 0, last_intrinsics_smallest_drop_ = 0;
  bool distributed_lifecycle_ = false;   // SetDistributedLifecycle
  int pcg_sum_classes_ = 1;        // (SetPCGSumClasses: the windowed scheme needs 1)
  int shard_rank_ = 0, shard_world_ = 1, whole_cloud_depth_ = 0;
  int keyframe_shard_world_ = 1;
  u32 shard_chunk_ = 0;
  CUDABufferPtr<float> other_surfels_;      // under surfel sharding: the buffer not in use (whole cloud <-> shard)
  CUDABufferPtr<u8> other_active_surfels_;
  int last_pose_rounds_ = 0, last_pose_steps_ = 0, last_pcg_inner_steps_ = 0;
};

}  // namespace vis
