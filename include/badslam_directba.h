/*
 * badslam_directba.h -- flat C view of the C++ host classes vis::DirectBA / vis::Keyframe
 * (badslam_amd/host/direct_ba.h, keyframe.h), for bindings that cannot consume C++ (the Python
 * test / bench harness via ctypes).  One function per public method of the reference class that
 * the BA path uses (applications/badslam/src/badslam/direct_ba.h:73-388); argument order and
 * meaning are the reference's.  Poses are 7 floats (qx qy qz qw tx ty tz), cameras 4 floats
 * (fx fy cx cy, pixel-corner convention).  Return 0 = ok.
 */
#ifndef BADSLAM_DIRECTBA_H_
#define BADSLAM_DIRECTBA_H_

#include <stddef.h>
#include <stdint.h>

#include "badslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dba_handle dba_handle;

/* DirectBA::DirectBA (direct_ba.h:73-88; render window and anchor pose omitted) */
dba_handle* dba_create(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
                       float surfel_merge_dist_factor, int min_observation_count_while_bootstrapping_1,
                       int min_observation_count_while_bootstrapping_2, int min_observation_count,
                       int width, int height, const float color_camera[4], const float depth_camera[4],
                       int use_depth_residuals, int use_descriptor_residuals);
void dba_destroy(dba_handle* h);

/* Keyframe ctor #2 (keyframe.cc:81-158) + DirectBA::AddKeyframe; returns the keyframe id. */
int dba_add_keyframe(dba_handle* h, void* hip_stream, const uint16_t* depth_image, const uint8_t* rgb_image,
                     const float global_T_frame[7]);
int dba_keyframe_count(dba_handle* h);
int dba_get_keyframe_pose(dba_handle* h, int keyframe_id, float global_T_frame[7]);
int dba_set_keyframe_pose(dba_handle* h, int keyframe_id, const float global_T_frame[7]);
int dba_get_keyframe_activation(dba_handle* h, int keyframe_id);
/* Keyframe::last_active_in_ba_iteration / last_covis_in_ba_iteration: the BA iteration count of the last surfel-creation loop that met
 * the keyframe kActive (it then created surfels) / kCovisibleActive; -1 before any */
int dba_get_keyframe_ba_iterations(dba_handle* h, int keyframe_id, int* last_active_in_ba_iteration, int* last_covis_in_ba_iteration);
/* Keyframe image access (tests poke depth / normals in place like the reference's do):
 * which: 0 depth u16, 1 normals u16, 2 radius u16, 3 colour rgba u8x4.  Dense host arrays. */
int dba_download_keyframe_image(dba_handle* h, void* hip_stream, int keyframe_id, int which, void* out);
int dba_upload_keyframe_image(dba_handle* h, void* hip_stream, int keyframe_id, int which, const void* in);
int dba_delete_keyframe(dba_handle* h, int keyframe_id);
/* DirectBA::MergeKeyframes(stream, loop_detector = NULL, approx_merge_count) (B/direct_ba.h:98-101, B/direct_ba.cc:251-338): deletes
 * up to approx_merge_count keyframes whose neighbours in the sequence are closest (never keyframe 0); dba_keyframe_exists: 1 while
 * the slot of that id still holds a keyframe.  dba_export_point_count: DirectBA::ExportToPointCloud (B/direct_ba.h:175), size only. */
int dba_merge_keyframes(dba_handle* h, void* hip_stream, int approx_merge_count);
int dba_keyframe_exists(dba_handle* h, int keyframe_id);
int dba_export_point_count(dba_handle* h, void* hip_stream, unsigned* count_out);

/* DirectBA::CreateSurfelsForKeyframe */
int dba_create_surfels_for_keyframe(dba_handle* h, void* hip_stream, int filter_new_surfels, int keyframe_id);
/* DirectBA::EstimateFramePose against the images of keyframe `keyframe_id` */
int dba_estimate_frame_pose(dba_handle* h, void* hip_stream, int keyframe_id, const float init[7], float out[7]);
/* DirectBA::BundleAdjustment */
int dba_bundle_adjustment(dba_handle* h, void* hip_stream, int optimize_depth_intrinsics, int optimize_color_intrinsics,
                          int do_surfel_updates, int optimize_poses, int optimize_geometry, int min_iterations,
                          int max_iterations, int use_pcg, int active_keyframe_window_start, int active_keyframe_window_end,
                          int increase_ba_iteration_count, int* iterations_done, int* converged,
                          int pcg_max_inner_iterations);

/* DirectBA::ComputeCost (ours): the value of the BA objective with the object's residual switches (bahip_evaluate_cost; the same bits
 * under surfel or keyframe sharding).  per_keyframe: NULL or dba_keyframe_count entries indexed by keyframe id, deleted ids zero. */
int dba_compute_cost(dba_handle* h, void* hip_stream, bahip_cost* total, bahip_cost* per_keyframe);
/* DirectBA::ComputeSurfelCosts (ours): the same objective per surfel (bahip_evaluate_surfel_costs), in buffer order.  Host arrays of
 * `capacity` >= dba_surfels_size entries, any may be NULL; the first dba_surfels_size entries are written.  Keyframe sharding: the
 * unsharded values on every rank; surfel sharding: this rank's shard.  Returns non-zero when capacity is too small. */
int dba_compute_surfel_costs(dba_handle* h, void* hip_stream, uint32_t capacity, double* depth, double* descriptor_1, double* descriptor_2,
                             uint32_t* depth_residuals, uint32_t* descriptor_pairs);
/* DirectBA::ComputeObservedCovisibility (ours): the surfels the association rule pairs with both of two keyframes
 * (bahip_observed_covisibility), over the existing keyframes in id order (deleted ids are not rows).  *num_rows_out = K, the number of
 * rows; when capacity_rows >= K: keyframe_ids[0 .. K) = the id of each row (may be NULL) and counts[i * K + j], K x K row-major, both
 * triangles, the diagonal a keyframe's own pair count.  Returns non-zero, with *num_rows_out set and nothing else written, when
 * capacity_rows < K.  Surfel sharding with an all-reduce installed: the unsharded matrix on every rank; keyframe sharding: the same. */
int dba_observed_covisibility(dba_handle* h, void* hip_stream, int capacity_rows, uint32_t* counts, int* keyframe_ids, int* num_rows_out);
/* DirectBA::ComputeReducedCameraSystem (ours): the Gauss-Newton system over the poses of the K existing keyframes with every surfel
 * eliminated (bahip_reduced_camera_system), blocks in id order (deleted ids are not blocks).  *num_rows_out = K; when capacity_rows >= K:
 * S (6K x 6K row-major), g (6K), A_diag (K x 36) and b (K x 6) -- the last two may be NULL --, keyframe_ids[0 .. K) (may be NULL) and
 * stats[0 .. 6) (may be NULL: list entries, pairs visited, atomics issued, degenerate surfels, overflow tiles, invalid).  marginalise 0:
 * S = blockdiag(A), g = b.  Returns non-zero, with *num_rows_out set and nothing else written, when capacity_rows < K or S or g is NULL. */
int dba_reduced_camera_system(dba_handle* h, void* hip_stream, int marginalise, int capacity_rows, double* S, double* g, double* A_diag, double* b,
                              int* keyframe_ids, uint64_t* stats, int* num_rows_out);
/* DirectBA::ComputePoseCovariances (ours): the gauge keyframe's rows and columns deleted from S, the rest factored (L D L^T, binary64)
 * and inverted.  *num_rows_out = R, the remaining keyframes; when capacity_rows >= R: marginal (R x 36: each keyframe's 6 x 6 covariance),
 * keyframe_ids[0 .. R) (may be NULL) and, for the num_pairs pairs of ids in pair_ids (two ids each), cross (num_pairs x 36: the block
 * between them).  Returns 1 when a capacity or a pointer is missing; 2 with the reason in error (error_capacity bytes, may be NULL) and
 * nothing else written when the gauge keyframe does not exist, a pair names it or an unknown id, or a pivot is not positive. */
int dba_pose_covariances(dba_handle* h, void* hip_stream, int gauge_keyframe_id, int capacity_rows, double* marginal, int* keyframe_ids,
                         int* num_rows_out, int num_pairs, const int* pair_ids, double* cross, char* error, int error_capacity);
/* DirectBA::ComputeSurfelObservations (ours): the observation lists (bahip_surfel_observations) into host arrays -- first
 * (surfels_size + 1 offsets, the last one the number of pairs P), keyframes (P indices into keyframe_ids, ascending within a list),
 * depth_raw (P words) and descriptor_raw (2 P words), either or both may be NULL, and keyframe_ids (the id of each bound index, may be
 * NULL; deleted ids are not bound).  *pairs_out = P and *num_keyframes_out = K are always set.  Returns non-zero, with nothing else
 * written, when capacity_surfels < surfels_size, capacity_pairs < P, capacity_keyframes < K or first or keyframes is NULL: call with
 * zero capacities to size the arrays.  Surfel sharding: this rank's shard; keyframe sharding: the unsharded
 * lists on every rank (every rank must ask for the same planes). */
int dba_surfel_observations(dba_handle* h, void* hip_stream, uint32_t capacity_surfels, uint64_t capacity_pairs, int capacity_keyframes,
                            uint32_t* first, uint16_t* keyframes, float* depth_raw, float* descriptor_raw, int* keyframe_ids, uint64_t* pairs_out,
                            int* num_keyframes_out);
/* DirectBA::ComputeKeyframeRedundancy (ours): per existing keyframe, in id order (deleted ids are not rows), its surfels by the number
 * of other keyframes the association rule pairs them with (bahip_keyframe_observer_histogram), 1 <= bins <= 64.  *num_rows_out = K;
 * when capacity_rows >= K: keyframe_ids[0 .. K) = the id of each row (may be NULL) and hist[i * bins + j], K x bins row-major.  Returns
 * non-zero, with *num_rows_out set and nothing else written, when capacity_rows < K or bins is out of range.  Surfel sharding with an
 * all-reduce installed: the unsharded table on every rank; keyframe sharding: the same. */
int dba_keyframe_redundancy(dba_handle* h, void* hip_stream, int bins, int capacity_rows, uint32_t* hist, int* keyframe_ids, int* num_rows_out);
/* DirectBA::FindRedundantKeyframes (ours): the ids of the keyframes with total > 0 and covered >= min_fraction * total -- total a row's
 * sum, covered its sum over the bins j >= min_other_observers (0 .. bins - 1) -- most redundant first, ties to the lower id.
 * *num_out = their number; non-zero, with nothing but *num_out written, when capacity is smaller.  Deletes nothing. */
int dba_find_redundant_keyframes(dba_handle* h, void* hip_stream, int min_other_observers, double min_fraction, int bins, int capacity,
                                 int* keyframe_ids, int* num_out);
/* DirectBA::CullRedundantKeyframes (ours): greedy deletion by that rule with a table of 16 bins (min_other_observers 0 .. 15), the table
 * computed again after each deletion; never the first existing keyframe nor one of the protect_newest last ones; at most
 * min(max_deletions, capacity) deletions.  deleted_ids[0 .. *num_deleted_out) = the ids in the order of deletion. */
int dba_cull_redundant_keyframes(dba_handle* h, void* hip_stream, int min_other_observers, double min_fraction, int max_deletions,
                                 int protect_newest, int capacity, int* deleted_ids, int* num_deleted_out);
/* DirectBA::RenderSurfels / RenderKeyframeView (ours): the surfel map seen from a camera (bahip_render_surfels), row-major host planes
 * of width * height pixels, any may be NULL: depth, index, normal (3 floats per pixel), color (4 bytes per pixel).  keyframe_id >= 0:
 * the depth camera at that keyframe's pose (view_camera, width, height and global_T_frame are ignored; the planes have the depth
 * image's size); keyframe_id < 0: the camera (fx, fy, cx, cy; pixel-corner convention) and pose given.  options->mode: BAHIP_RENDER_POINT
 * or BAHIP_RENDER_DISC.  frame_T_global_out: NULL or the 3 x 4 matrix the render used.  Returns non-zero on a bad argument. */
int dba_render_surfels(dba_handle* h, void* hip_stream, int keyframe_id, const float view_camera[4], int width, int height,
                       const float global_T_frame[7], const bahip_render_options* options, float* depth, uint32_t* index, float* normal,
                       uint8_t* color, float frame_T_global_out[12]);
/* DirectBA::KeyframeResidualImage / FrameResidualImage (ours): the objective in image space (bahip_frame_residual_image) for the images
 * of keyframe `keyframe_id`, row-major host planes of the depth image's width * height pixels, any may be NULL: key, pairs, index,
 * depth_residual, inv_stddev, desc_residual (2 floats per pixel), color_valid.  global_T_frame NULL: the keyframe's own pose
 * (KeyframeResidualImage); else the pose given, 7 floats (FrameResidualImage on the keyframe's images).  options->select:
 * BAHIP_RESIDUAL_BEST or BAHIP_RESIDUAL_WORST.  frame_T_global_out: NULL or the 3 x 4 matrix the call used.  Returns non-zero on a bad
 * argument. */
int dba_keyframe_residual_image(dba_handle* h, void* hip_stream, int keyframe_id, const float global_T_frame[7],
                                const bahip_residual_image_options* options, uint64_t* key, uint32_t* pairs, uint32_t* index,
                                float* depth_residual, float* inv_stddev, float* desc_residual, uint8_t* color_valid,
                                float frame_T_global_out[12]);

/* accessors */
uint32_t dba_surfel_count(dba_handle* h);
uint32_t dba_surfels_size(dba_handle* h);
int dba_set_surfel_count(dba_handle* h, uint32_t surfel_count, uint32_t surfels_size);
/* DirectBA::SortSurfelsSpatially (ours: Morton order of the surfel buffer over a world grid of grid_cell_size metres) */
int dba_sort_surfels_spatially(dba_handle* h, void* hip_stream, float grid_cell_size);
/* DirectBA::SetBatchedCreation (ours): 1 (default) = the surfel creations of a BA iteration and the merges of a merge pass go to the
 * backend as one batch each (bahip_create_surfels_for_keyframes, bahip_merge_surfels_for_keyframes), 0 = keyframe by keyframe with the
 * host in between.  Same surfels. */
int dba_set_batched_creation(dba_handle* h, int enabled);
/* DirectBA::SetSpatialSortCellSize: the grid cell PerformBASchemeEndTasks re-establishes that order with whenever surfels were
 * appended or moved since the last reorder (default 0.02 m; 0 = never: the reference's surfel order stays observable);
 * dba_unsorted_surfels: how many were appended / moved since then */
int dba_set_spatial_sort_cell_size(dba_handle* h, float grid_cell_size);
uint32_t dba_unsorted_surfels(dba_handle* h);
/* surfels()->Download/UploadPartAsync of `rows` attribute rows x `count` surfels starting at row 0 */
int dba_download_surfels(dba_handle* h, void* hip_stream, int rows, uint32_t count, float* out);
int dba_upload_surfels(dba_handle* h, void* hip_stream, int rows, uint32_t count, const float* in);
int dba_get_cameras(dba_handle* h, float color_camera[4], float depth_camera[4], float* a);
int dba_set_cameras(dba_handle* h, const float color_camera[4], const float depth_camera[4], float a);
int dba_cfactor_size(dba_handle* h, int* width, int* height);
int dba_download_cfactor(dba_handle* h, void* hip_stream, float* out);
int dba_clear_cfactor(dba_handle* h, void* hip_stream);
int dba_set_pcg_gauge_keyframe(dba_handle* h, int keyframe_id);
/* DirectBA::SetWindowedPCG (ours, default off): BundleAdjustment(use_pcg) honours a fixed active keyframe window and skips deleted
 * keyframes; returns 1 (refused) under keyframe sharding and with more than one PCG sum class */
int dba_set_windowed_pcg(dba_handle* h, int enabled);
/* DirectBA::SetPCGStepControl (ours, default off): BundleAdjustment(use_pcg) takes damped steps that are kept only if the objective
 * falls (bahip_pcg_iteration_controlled; the fields of bahip_pcg_step_control).  enabled = 0: off.  Returns 1 (refused) under keyframe
 * sharding and for values out of range.  dba_pcg_step_stats: the damping factor the next outer iteration starts with, and the trial
 * steps / undone trial steps of the last BundleAdjustment call. */
int dba_set_pcg_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_down, float lambda_min,
                             float lambda_max, int max_trials);
int dba_pcg_step_stats(dba_handle* h, float* lambda, int* trials, int* rejected_steps);
/* DirectBA::SetPoseStepControl (ours, default off): the pose phase of BundleAdjustment(!use_pcg) keeps a damped Gauss-Newton step of a
 * keyframe only if that keyframe's cost falls (bahip_estimate_keyframe_poses_controlled; lambda_initial is where a keyframe seen for the
 * first time starts, the other fields are bahip_pose_step_control's).  enabled = 0: off.  Returns 1 (refused) under keyframe sharding and
 * for values out of range.  dba_get_pose_step_stats: candidates evaluated / rejected in the last BundleAdjustment call, and the damping
 * factor keyframe_id's next pose phase starts with. */
int dba_set_pose_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_down, float lambda_min,
                              float lambda_max, int max_trials);
int dba_get_pose_step_stats(dba_handle* h, int* trials, int* rejected_steps, int keyframe_id, float* lambda);
/* DirectBA::SetGeometryStepControl (ours, default off): both geometry calls of BundleAdjustment(!use_pcg) keep a damped step of a surfel
 * only if that surfel's cost falls (bahip_optimize_geometry_iteration_controlled; the fields are bahip_geometry_step_control's).
 * enabled = 0: off.  Allowed under either sharding; returns 1 (refused) for values out of range.  dba_get_geometry_step_stats: the totals
 * over the geometry calls of the last BundleAdjustment call (candidates = accepted + restored) and the trials run; any may be NULL. */
int dba_set_geometry_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_min, float lambda_max,
                                  int max_trials, int guard_pairs);
int dba_get_geometry_step_stats(dba_handle* h, long long* candidates, long long* accepted, long long* restored, int* trials);
/* DirectBA::SetIntrinsicsStepControl (ours, default off): the intrinsics step of BundleAdjustment(!use_pcg) runs damped trials and keeps
 * the first that lowers the objective, otherwise nothing changes (bahip_optimize_intrinsics_controlled; the fields are
 * bahip_intrinsics_step_control's).  enabled = 0: off.  Allowed under either sharding; returns 1 (refused) for values out of range.
 * The damping factor persists across iterations and calls.  The intrinsics-updated callback fires only after an accepted step.
 * dba_get_intrinsics_step_stats: trials run and steps accepted in the last BundleAdjustment call, the factor of its last accepted step
 * (-1: none), and the factor the next step starts with; any may be NULL. */
int dba_set_intrinsics_step_control(dba_handle* h, int enabled, float lambda_first, float lambda_up, float lambda_max, int max_trials);
int dba_get_intrinsics_step_stats(dba_handle* h, int* trials, int* accepted, float* lambda_accepted, float* lambda_next);
/* By how much the accepted steps of the last BundleAdjustment call lowered the objective: in total, and the smallest drop of one step
 * (both 0 when none was accepted; positive otherwise). */
int dba_get_intrinsics_step_drops(dba_handle* h, double* total, double* smallest);
/* DirectBA::SetIntrinsicsUpdatedCallback: called from BundleAdjustment after an intrinsics step has changed the cameras or the depth
 * parameters (with the step control on: after an accepted step only); NULL removes it. */
int dba_set_intrinsics_updated_callback(dba_handle* h, void (*callback)(void* user), void* user);
/* DirectBA::SetSurfelSharding: this object holds rank `rank`'s chunk-cyclic shard of one surfel cloud (bahip_gather_surfel_shards) */
int dba_set_surfel_sharding(dba_handle* h, int rank, int world, uint32_t chunk);
/* DirectBA::SetDistributedLifecycle (ours, default off): under surfel sharding the lifecycle's sweeps are dealt over the ranks
 * (bahip_context_set_lifecycle_dealing) with the same bits; returns 1 (refused) under keyframe sharding */
int dba_set_distributed_lifecycle(dba_handle* h, int enabled);
/* DirectBA::SetSumClasses: 4 (default) or 8 interleaved keyframe classes in the definition of the per-surfel sums
 * (bahip_context_set_sum_classes) */
int dba_set_sum_classes(dba_handle* h, int classes);
/* DirectBA::SetIntrinsicsSumClasses: 1 (default), 2, 4 or 8 keyframe classes in the definition of the intrinsics step's global sums
 * (bahip_context_set_intrinsics_sum_classes; keyframe sharding of that step over world ranks needs >= world) */
int dba_set_intrinsics_sum_classes(dba_handle* h, int classes);
/* DirectBA::SetPCGSumClasses: 1 (default), 2, 4 or 8 keyframe classes in the definition of the surfel block of the PCG scheme's r, M and g
 * (bahip_context_set_pcg_sum_classes; keyframe sharding of the PCG scheme over world ranks needs >= world) */
int dba_set_pcg_sum_classes(dba_handle* h, int classes);
/* DirectBA::SetRowMajorCreation (ours): 1 = the surfels a keyframe creates are appended in the reference's row-major pixel order
 * (B/kernel_create_surfels.cu:357-390), 0 (default) = tile-major (bahip_context_set_creation_order) */
int dba_set_row_major_creation(dba_handle* h, int enabled);
/* DirectBA::SetFastArithmetic (ours): 1 = the fast arithmetic flavour of the sweeps, 0 (default) = the exact one (bahip_context_set_arithmetic) */
int dba_set_fast_arithmetic(dba_handle* h, int enabled);
/* DirectBA::SetKeyframeSharding: this object holds all surfels and the images of the keyframes k with k % world == rank
 * (bahip_context_set_keyframe_sharding; world = 1, 2, 4, or 8 after dba_set_sum_classes(h, 8)); the alternating scheme over poses,
 * geometry and -- after dba_set_intrinsics_sum_classes(h, c), c >= world -- the intrinsics, and the PCG scheme after
 * dba_set_pcg_sum_classes(h, c), c >= world; without surfel updates or end tasks */
int dba_set_keyframe_sharding(dba_handle* h, int rank, int world);
/* DirectBA::SetBAIterationCount / SetLastBAIterationCount (direct_ba.h:362-366) */
int dba_set_ba_iteration_counts(dba_handle* h, int ba_iteration_count, int last_ba_iteration_count);
int dba_last_stats(dba_handle* h, int* pose_rounds, int* pose_steps, int* pcg_inner_steps);
/* backend context of this DirectBA (for bahip_context_set_allreduce, bahip_set_profiling, ...) */
bahip_context* dba_backend_context(dba_handle* h);
/* Borrowed views for callers that drive individual bahip_* stages on a DirectBA-owned scene (the stage-level parity
 * tests): the images (and BA planes) of one keyframe, the surfel buffer, and DirectBA::BindScene (cameras, depth
 * parameters and the keyframe list as the backend sees them; bound index = position among the non-deleted keyframes). */
int dba_keyframe_frame(dba_handle* h, int keyframe_id, bahip_frame* out);
int dba_surfels_struct(dba_handle* h, bahip_surfels* out);
int dba_bind_scene(dba_handle* h, void* hip_stream);
/* Keyframe::co_visibility_list() (keyframe ids); returns the list length (entries beyond `capacity` are not written), -1 for a bad id. */
int dba_keyframe_covisibility(dba_handle* h, int keyframe_id, int* out, int capacity);

#ifdef __cplusplus
}
#endif
#endif
