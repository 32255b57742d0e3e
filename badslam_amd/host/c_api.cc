// c_api.cc -- include/badslam_directba.h: flat C view of vis::DirectBA / vis::Keyframe.
#include "../../include/badslam_directba.h"

#include "direct_ba.h"
#include "rgbd_io.h"   // Point3fC3u8Nf

using namespace vis;

struct dba_handle {
  std::unique_ptr<DirectBA> ba;
  int width, height;
};

extern "C" {

dba_handle* dba_create(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
                       float surfel_merge_dist_factor, int boot1, int boot2, int min_observation_count, int width, int height,
                       const float color_camera[4], const float depth_camera[4], int use_depth_residuals,
                       int use_descriptor_residuals) {
  if (bahip_device_count() <= 0) return nullptr;   // no CPU fallback
  dba_handle* h = new dba_handle();
  h->width = width; h->height = height;
  PinholeCamera4f cc(width, height, color_camera), dc(width, height, depth_camera);
  h->ba.reset(new DirectBA(max_surfel_count, raw_to_float_depth, baseline_fx, sparse_surfel_cell_size, surfel_merge_dist_factor,
                           boot1, boot2, min_observation_count, cc, dc, 0, use_depth_residuals != 0,
                           use_descriptor_residuals != 0, nullptr, SE3f()));
  return h;
}

void dba_destroy(dba_handle* h) { delete h; }

int dba_add_keyframe(dba_handle* h, void* stream, const uint16_t* depth_image, const uint8_t* rgb_image, const float pose[7]) {
  Image<u16> depth(h->width, h->height);
  memcpy(depth.data(), depth_image, sizeof(u16) * (size_t)h->width * h->height);
  Image<Vec3u8> color(h->width, h->height);
  memcpy(color.data(), rgb_image, 3 * (size_t)h->width * h->height);
  shared_ptr<Keyframe> kf(new Keyframe(stream, (u32)h->ba->keyframes().size(), h->ba->depth_params(), h->ba->depth_camera(), depth,
                                       color, SE3f(pose)));
  h->ba->AddKeyframe(kf);
  return kf->id();
}

int dba_keyframe_count(dba_handle* h) { return (int)h->ba->keyframes().size(); }

static Keyframe* get_kf(dba_handle* h, int id) {
  if (id < 0 || id >= (int)h->ba->keyframes().size()) return nullptr;
  return h->ba->keyframes()[id].get();
}

int dba_get_keyframe_pose(dba_handle* h, int id, float pose[7]) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  memcpy(pose, kf->global_T_frame().data(), 7 * sizeof(float));
  return 0;
}
int dba_set_keyframe_pose(dba_handle* h, int id, const float pose[7]) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  kf->set_global_T_frame(SE3f(pose));
  return 0;
}
int dba_get_keyframe_activation(dba_handle* h, int id) {
  Keyframe* kf = get_kf(h, id);
  return kf ? (int)kf->activation() : -1;
}
int dba_get_keyframe_ba_iterations(dba_handle* h, int id, int* last_active_in_ba_iteration, int* last_covis_in_ba_iteration) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  if (last_active_in_ba_iteration) *last_active_in_ba_iteration = kf->last_active_in_ba_iteration();
  if (last_covis_in_ba_iteration) *last_covis_in_ba_iteration = kf->last_covis_in_ba_iteration();
  return 0;
}

int dba_download_keyframe_image(dba_handle* h, void* stream, int id, int which, void* out) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  switch (which) {
    case 0: kf->depth_buffer().DownloadAsync(stream, static_cast<u16*>(out)); break;
    case 1: kf->normals_buffer().DownloadAsync(stream, static_cast<u16*>(out)); break;
    case 2: kf->radius_buffer().DownloadAsync(stream, static_cast<u16*>(out)); break;
    case 3: kf->color_buffer().DownloadAsync(stream, static_cast<uchar4*>(out)); break;
    default: return 1;
  }
  return 0;
}
int dba_upload_keyframe_image(dba_handle* h, void* stream, int id, int which, const void* in) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  // the reference's tests do exactly this const_cast (test_geometry_optimization_geometric_residual.cc:121-136)
  switch (which) {
    case 0: const_cast<CUDABuffer<u16>&>(kf->depth_buffer()).UploadAsync(stream, static_cast<const u16*>(in)); break;
    case 1: const_cast<CUDABuffer<u16>&>(kf->normals_buffer()).UploadAsync(stream, static_cast<const u16*>(in)); break;
    case 2: const_cast<CUDABuffer<u16>&>(kf->radius_buffer()).UploadAsync(stream, static_cast<const u16*>(in)); break;
    case 3: const_cast<CUDABuffer<uchar4>&>(kf->color_buffer()).UploadAsync(stream, static_cast<const uchar4*>(in)); break;
    default: return 1;
  }
  kf->RefreshPlanes(static_cast<hipStream_t>(stream));
  return 0;
}
int dba_keyframe_exists(dba_handle* h, int id) { return (id >= 0 && id < (int)h->ba->keyframes().size() && h->ba->keyframes()[id]) ? 1 : 0; }
int dba_merge_keyframes(dba_handle* h, void* stream, int approx_merge_count) {
  h->ba->MergeKeyframes(static_cast<hipStream_t>(stream), nullptr, (vis::usize)approx_merge_count);
  return 0;
}
int dba_export_point_count(dba_handle* h, void* stream, unsigned* count_out) {
  std::vector<vis::Point3fC3u8Nf> cloud;
  h->ba->ExportToPointCloud(static_cast<hipStream_t>(stream), &cloud);
  *count_out = (unsigned)cloud.size();
  return 0;
}
int dba_delete_keyframe(dba_handle* h, int id) {
  if (!get_kf(h, id)) return 1;
  h->ba->DeleteKeyframe(id, nullptr);
  return 0;
}

int dba_create_surfels_for_keyframe(dba_handle* h, void* stream, int filter_new_surfels, int id) {
  if (!get_kf(h, id)) return 1;
  h->ba->CreateSurfelsForKeyframe(stream, filter_new_surfels != 0, h->ba->keyframes()[id]);
  return 0;
}

int dba_estimate_frame_pose(dba_handle* h, void* stream, int id, const float init[7], float out[7]) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return 1;
  SE3f result;
  h->ba->EstimateFramePose(stream, SE3f(init), kf->depth_buffer(), kf->normals_buffer(), kf->color_texture(), &result, false);
  memcpy(out, result.data(), 7 * sizeof(float));
  return 0;
}

int dba_bundle_adjustment(dba_handle* h, void* stream, int optimize_depth_intrinsics, int optimize_color_intrinsics,
                          int do_surfel_updates, int optimize_poses, int optimize_geometry, int min_iterations, int max_iterations,
                          int use_pcg, int window_start, int window_end, int increase_ba_iteration_count, int* iterations_done,
                          int* converged, int pcg_max_inner_iterations) {
  bool conv = false;
  int done = 0;
  h->ba->BundleAdjustment(stream, optimize_depth_intrinsics != 0, optimize_color_intrinsics != 0, do_surfel_updates != 0,
                          optimize_poses != 0, optimize_geometry != 0, min_iterations, max_iterations, use_pcg != 0, window_start,
                          window_end, increase_ba_iteration_count != 0, &done, &conv, 0, nullptr, pcg_max_inner_iterations);
  if (iterations_done) *iterations_done = done;
  if (converged) *converged = conv ? 1 : 0;
  return 0;
}

int dba_compute_cost(dba_handle* h, void* stream, bahip_cost* total, bahip_cost* per_keyframe) {
  DirectBA::BACost sum;
  std::vector<DirectBA::BACost> per;
  h->ba->ComputeCost(static_cast<hipStream_t>(stream), &sum, per_keyframe ? &per : nullptr);
  auto convert = [](const DirectBA::BACost& c) {
    bahip_cost out;
    out.depth = c.depth; out.descriptor_1 = c.descriptor_1; out.descriptor_2 = c.descriptor_2;
    out.depth_residuals = c.depth_residuals; out.descriptor_pairs = c.descriptor_pairs;
    return out;
  };
  if (total) *total = convert(sum);
  for (size_t id = 0; per_keyframe && id < per.size(); ++id) per_keyframe[id] = convert(per[id]);
  return 0;
}

int dba_compute_surfel_costs(dba_handle* h, void* stream, uint32_t capacity, double* depth, double* descriptor_1, double* descriptor_2,
                             uint32_t* depth_residuals, uint32_t* descriptor_pairs) {
  if (capacity < h->ba->surfels_size()) return 1;
  DirectBA::SurfelCosts costs;
  h->ba->ComputeSurfelCosts(static_cast<hipStream_t>(stream), &costs);
  if (depth) std::copy(costs.depth.begin(), costs.depth.end(), depth);
  if (descriptor_1) std::copy(costs.descriptor_1.begin(), costs.descriptor_1.end(), descriptor_1);
  if (descriptor_2) std::copy(costs.descriptor_2.begin(), costs.descriptor_2.end(), descriptor_2);
  if (depth_residuals) std::copy(costs.depth_residuals.begin(), costs.depth_residuals.end(), depth_residuals);
  if (descriptor_pairs) std::copy(costs.descriptor_pairs.begin(), costs.descriptor_pairs.end(), descriptor_pairs);
  return 0;
}

int dba_observed_covisibility(dba_handle* h, void* stream, int capacity_rows, uint32_t* counts, int* keyframe_ids, int* num_rows_out) {
  int rows = 0;
  for (int id = 0; id < (int)h->ba->keyframes().size(); ++id)
    if (h->ba->keyframes()[id]) ++rows;
  if (num_rows_out) *num_rows_out = rows;
  if (capacity_rows < rows || !counts) return 1;
  std::vector<uint32_t> words;
  std::vector<int> ids;
  h->ba->ComputeObservedCovisibility(static_cast<hipStream_t>(stream), &words, &ids);
  std::copy(words.begin(), words.end(), counts);
  if (keyframe_ids) std::copy(ids.begin(), ids.end(), keyframe_ids);
  return 0;
}

int dba_reduced_camera_system(dba_handle* h, void* stream, int marginalise, int capacity_rows, double* S, double* g, double* A_diag, double* b,
                              int* keyframe_ids, uint64_t* stats, int* num_rows_out) {
  int rows = 0;
  for (int id = 0; id < (int)h->ba->keyframes().size(); ++id)
    if (h->ba->keyframes()[id]) ++rows;
  if (num_rows_out) *num_rows_out = rows;
  if (capacity_rows < rows || !S || !g) return 1;
  DirectBA::ReducedCameraSystem system;
  h->ba->ComputeReducedCameraSystem(static_cast<hipStream_t>(stream), &system, marginalise != 0);
  std::copy(system.S.begin(), system.S.end(), S);
  std::copy(system.g.begin(), system.g.end(), g);
  if (A_diag) std::copy(system.A_diag.begin(), system.A_diag.end(), A_diag);
  if (b) std::copy(system.b.begin(), system.b.end(), b);
  if (keyframe_ids) std::copy(system.keyframe_ids.begin(), system.keyframe_ids.end(), keyframe_ids);
  if (stats) {
    stats[0] = system.list_entries; stats[1] = system.pairs_visited; stats[2] = system.atomics_issued;
    stats[3] = system.degenerate_surfels; stats[4] = system.overflow_tiles; stats[5] = system.invalid;
  }
  return 0;
}

int dba_pose_covariances(dba_handle* h, void* stream, int gauge_keyframe_id, int capacity_rows, double* marginal, int* keyframe_ids, int* num_rows_out,
                         int num_pairs, const int* pair_ids, double* cross, char* error, int error_capacity) {
  int rows = -1;   // the existing keyframes but the gauge one
  for (int id = 0; id < (int)h->ba->keyframes().size(); ++id)
    if (h->ba->keyframes()[id]) ++rows;
  if (num_rows_out) *num_rows_out = std::max(rows, 0);
  if (capacity_rows < rows || !marginal || (num_pairs > 0 && (!pair_ids || !cross))) return 1;
  std::vector<std::pair<int, int>> pairs;
  for (int q = 0; q < num_pairs; ++q) pairs.emplace_back(pair_ids[2 * q], pair_ids[2 * q + 1]);
  DirectBA::PoseCovariances covariances;
  std::string why;
  if (!h->ba->ComputePoseCovariances(static_cast<hipStream_t>(stream), gauge_keyframe_id, &covariances, &pairs, &why)) {
    if (error && error_capacity > 0) snprintf(error, (size_t)error_capacity, "%s", why.c_str());
    return 2;
  }
  if (num_rows_out) *num_rows_out = (int)covariances.keyframe_ids.size();
  std::copy(covariances.marginal.begin(), covariances.marginal.end(), marginal);
  if (keyframe_ids) std::copy(covariances.keyframe_ids.begin(), covariances.keyframe_ids.end(), keyframe_ids);
  if (cross) std::copy(covariances.cross.begin(), covariances.cross.end(), cross);
  return 0;
}

int dba_surfel_observations(dba_handle* h, void* stream, uint32_t capacity_surfels, uint64_t capacity_pairs, int capacity_keyframes, uint32_t* first,
                            uint16_t* keyframes, float* depth_raw, float* descriptor_raw, int* keyframe_ids, uint64_t* pairs_out, int* num_keyframes_out) {
  DirectBA::SurfelObservations t;
  h->ba->ComputeSurfelObservations(static_cast<hipStream_t>(stream), &t, depth_raw != nullptr || descriptor_raw != nullptr);
  if (pairs_out) *pairs_out = t.keyframes.size();
  if (num_keyframes_out) *num_keyframes_out = (int)t.keyframe_ids.size();
  if (capacity_surfels < t.first.size() - 1 || capacity_pairs < t.keyframes.size() || capacity_keyframes < (int)t.keyframe_ids.size() || !first ||
      !keyframes)
    return 1;
  std::copy(t.first.begin(), t.first.end(), first);
  std::copy(t.keyframes.begin(), t.keyframes.end(), keyframes);
  if (depth_raw) std::copy(t.depth_raw.begin(), t.depth_raw.end(), depth_raw);
  if (descriptor_raw) std::copy(t.descriptor_raw.begin(), t.descriptor_raw.end(), descriptor_raw);
  if (keyframe_ids) std::copy(t.keyframe_ids.begin(), t.keyframe_ids.end(), keyframe_ids);
  return 0;
}

int dba_keyframe_redundancy(dba_handle* h, void* stream, int bins, int capacity_rows, uint32_t* hist, int* keyframe_ids, int* num_rows_out) {
  int rows = 0;
  for (int id = 0; id < (int)h->ba->keyframes().size(); ++id)
    if (h->ba->keyframes()[id]) ++rows;
  if (num_rows_out) *num_rows_out = rows;
  if (capacity_rows < rows || !hist || bins < 1 || bins > 64) return 1;
  std::vector<uint32_t> words;
  std::vector<int> ids;
  h->ba->ComputeKeyframeRedundancy(static_cast<hipStream_t>(stream), bins, &words, &ids);
  std::copy(words.begin(), words.end(), hist);
  if (keyframe_ids) std::copy(ids.begin(), ids.end(), keyframe_ids);
  return 0;
}

int dba_find_redundant_keyframes(dba_handle* h, void* stream, int min_other_observers, double min_fraction, int bins, int capacity, int* keyframe_ids,
                                 int* num_out) {
  if (bins < 1 || bins > 64 || min_other_observers < 0 || min_other_observers > bins - 1 || !keyframe_ids || !num_out) return 1;
  std::vector<int> ids;
  h->ba->FindRedundantKeyframes(static_cast<hipStream_t>(stream), min_other_observers, min_fraction, &ids, bins);
  *num_out = (int)ids.size();
  if (capacity < (int)ids.size()) return 1;
  std::copy(ids.begin(), ids.end(), keyframe_ids);
  return 0;
}

int dba_cull_redundant_keyframes(dba_handle* h, void* stream, int min_other_observers, double min_fraction, int max_deletions, int protect_newest,
                                 int capacity, int* deleted_ids, int* num_deleted_out) {
  // (the default table of FindRedundantKeyframes has 16 bins)
  if (min_other_observers < 0 || min_other_observers > 15 || !deleted_ids || !num_deleted_out) return 1;
  std::vector<int> ids;
  h->ba->CullRedundantKeyframes(static_cast<hipStream_t>(stream), min_other_observers, min_fraction, std::min(max_deletions, capacity), protect_newest,
                                &ids);
  *num_deleted_out = (int)ids.size();
  std::copy(ids.begin(), ids.end(), deleted_ids);
  return 0;
}

int dba_render_surfels(dba_handle* h, void* stream, int keyframe_id, const float view_camera[4], int width, int height,
                       const float global_T_frame[7], const bahip_render_options* options, float* depth, uint32_t* index, float* normal,
                       uint8_t* color, float frame_T_global_out[12]) {
  if (!options) return 1;
  DirectBA::RenderOptions o;
  o.disc = options->mode == BAHIP_RENDER_DISC;
  o.max_radius_px = options->max_radius_px;
  o.cull_backfaces = options->cull_backfaces != 0;
  o.radius_factor = options->radius_factor;
  o.min_depth = options->min_depth;
  o.max_depth = options->max_depth;
  o.index_base = options->index_base;
  DirectBA::RenderedView view;
  SE3f pose;
  if (keyframe_id >= 0) {
    Keyframe* kf = get_kf(h, keyframe_id);
    if (!kf) return 1;
    pose = kf->global_T_frame();
    h->ba->RenderKeyframeView(static_cast<hipStream_t>(stream), keyframe_id, o, &view);
  } else {
    if (!view_camera || !global_T_frame || width < 1 || height < 1) return 1;
    pose = SE3f(global_T_frame);
    h->ba->RenderSurfels(static_cast<hipStream_t>(stream), PinholeCamera4f(width, height, view_camera), pose, o, &view);
  }
  if (depth) std::copy(view.depth.begin(), view.depth.end(), depth);
  if (index) std::copy(view.index.begin(), view.index.end(), index);
  if (normal) std::copy(view.normal.begin(), view.normal.end(), normal);
  if (color) std::copy(view.color.begin(), view.color.end(), color);
  if (frame_T_global_out) pose.inverse().matrix3x4(frame_T_global_out);
  return 0;
}

int dba_keyframe_residual_image(dba_handle* h, void* stream, int keyframe_id, const float global_T_frame[7],
                                const bahip_residual_image_options* options, uint64_t* key, uint32_t* pairs, uint32_t* index,
                                float* depth_residual, float* inv_stddev, float* desc_residual, uint8_t* color_valid,
                                float frame_T_global_out[12]) {
  if (!options || (options->select != BAHIP_RESIDUAL_BEST && options->select != BAHIP_RESIDUAL_WORST)) return 1;
  Keyframe* kf = get_kf(h, keyframe_id);
  if (!kf) return 1;
  DirectBA::ResidualImageOptions o;
  o.worst = options->select == BAHIP_RESIDUAL_WORST;
  o.index_base = options->index_base;
  DirectBA::ResidualImage image;
  SE3f pose = kf->global_T_frame();
  if (global_T_frame) {
    pose = SE3f(global_T_frame);
    h->ba->FrameResidualImage(static_cast<hipStream_t>(stream), *kf, pose, o, &image);
  } else {
    h->ba->KeyframeResidualImage(static_cast<hipStream_t>(stream), keyframe_id, o, &image);
  }
  if (key) std::copy(image.key.begin(), image.key.end(), key);
  if (pairs) std::copy(image.pairs.begin(), image.pairs.end(), pairs);
  if (index) std::copy(image.index.begin(), image.index.end(), index);
  if (depth_residual) std::copy(image.depth_residual.begin(), image.depth_residual.end(), depth_residual);
  if (inv_stddev) std::copy(image.inv_stddev.begin(), image.inv_stddev.end(), inv_stddev);
  if (desc_residual) std::copy(image.desc_residual.begin(), image.desc_residual.end(), desc_residual);
  if (color_valid) std::copy(image.color_valid.begin(), image.color_valid.end(), color_valid);
  if (frame_T_global_out) pose.inverse().matrix3x4(frame_T_global_out);
  return 0;
}

uint32_t dba_surfel_count(dba_handle* h) { return h->ba->surfel_count(); }
uint32_t dba_surfels_size(dba_handle* h) { return h->ba->surfels_size(); }
int dba_set_surfel_count(dba_handle* h, uint32_t surfel_count, uint32_t surfels_size) {
  h->ba->SetSurfelCount(surfel_count, surfels_size);
  return 0;
}

int dba_sort_surfels_spatially(dba_handle* h, void* stream, float grid_cell_size) {
  h->ba->SortSurfelsSpatially(stream, grid_cell_size);
  return 0;
}

int dba_set_batched_creation(dba_handle* h, int enabled) {
  h->ba->SetBatchedCreation(enabled != 0);
  return 0;
}
int dba_set_spatial_sort_cell_size(dba_handle* h, float grid_cell_size) {
  h->ba->SetSpatialSortCellSize(grid_cell_size);
  return 0;
}
uint32_t dba_unsorted_surfels(dba_handle* h) { return h->ba->unsorted_surfels(); }

int dba_download_surfels(dba_handle* h, void* stream, int rows, uint32_t count, float* out) {
  auto s = h->ba->surfels();
  for (int r = 0; r < rows; ++r)
    s->DownloadPartAsync((size_t)r * s->ToCUDA().pitch(), (size_t)count * sizeof(float), stream, out + (size_t)r * count);
  return 0;
}
int dba_upload_surfels(dba_handle* h, void* stream, int rows, uint32_t count, const float* in) {
  auto s = h->ba->surfels();
  if ((int)count > s->width()) return 1;
  for (int r = 0; r < rows; ++r)
    s->UploadPartAsync((size_t)r * s->ToCUDA().pitch(), (size_t)count * sizeof(float), stream, in + (size_t)r * count);
  bahip_context_surfels_rearranged(h->ba->backend_context());   // (other surfels in every tile: the sweeps' run order is rebuilt)
  return 0;
}

int dba_get_cameras(dba_handle* h, float color_camera[4], float depth_camera[4], float* a) {
  memcpy(color_camera, h->ba->color_camera().parameters(), 4 * sizeof(float));
  memcpy(depth_camera, h->ba->depth_camera().parameters(), 4 * sizeof(float));
  *a = h->ba->a();
  return 0;
}
int dba_set_cameras(dba_handle* h, const float color_camera[4], const float depth_camera[4], float a) {
  h->ba->SetColorCamera(PinholeCamera4f(h->width, h->height, color_camera));
  h->ba->SetDepthCamera(PinholeCamera4f(h->width, h->height, depth_camera));
  h->ba->a() = a;
  return 0;
}
int dba_cfactor_size(dba_handle* h, int* width, int* height) {
  *width = h->ba->cfactor_buffer()->width();
  *height = h->ba->cfactor_buffer()->height();
  return 0;
}
int dba_download_cfactor(dba_handle* h, void* stream, float* out) {
  h->ba->cfactor_buffer()->DownloadAsync(stream, out);
  return 0;
}
int dba_clear_cfactor(dba_handle* h, void* stream) {
  h->ba->cfactor_buffer()->Clear(0, stream);
  return 0;
}
int dba_set_ba_iteration_counts(dba_handle* h, int count, int last) {
  h->ba->SetBAIterationCount(count);
  h->ba->SetLastBAIterationCount(last);
  return 0;
}
int dba_set_surfel_sharding(dba_handle* h, int rank, int world, uint32_t chunk) {
  h->ba->SetSurfelSharding(rank, world, chunk);
  return 0;
}
int dba_set_row_major_creation(dba_handle* h, int enabled) {
  h->ba->SetRowMajorCreation(enabled != 0);
  return 0;
}
int dba_set_fast_arithmetic(dba_handle* h, int enabled) {
  h->ba->SetFastArithmetic(enabled != 0);
  return 0;
}
int dba_set_sum_classes(dba_handle* h, int classes) {
  h->ba->SetSumClasses(classes);
  return 0;
}
int dba_set_intrinsics_sum_classes(dba_handle* h, int classes) {
  h->ba->SetIntrinsicsSumClasses(classes);
  return 0;
}
int dba_set_pcg_sum_classes(dba_handle* h, int classes) {
  h->ba->SetPCGSumClasses(classes);
  return 0;
}
int dba_set_keyframe_sharding(dba_handle* h, int rank, int world) {
  h->ba->SetKeyframeSharding(rank, world);
  return 0;
}
int dba_set_pcg_gauge_keyframe(dba_handle* h, int id) {
  h->ba->SetPCGGaugeKeyframe(id);
  return 0;
}
int dba_set_windowed_pcg(dba_handle* h, int enabled) { return h->ba->SetWindowedPCG(enabled != 0) ? 0 : 1; }
int dba_set_pcg_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_down, float lambda_min,
                             float lambda_max, int max_trials) {
  if (!enabled) return h->ba->SetPCGStepControl(nullptr) ? 0 : 1;
  vis::DirectBA::PCGStepControl control;
  control.lambda_initial = lambda_initial; control.lambda_up = lambda_up; control.lambda_down = lambda_down;
  control.lambda_min = lambda_min; control.lambda_max = lambda_max; control.max_trials = max_trials;
  return h->ba->SetPCGStepControl(&control) ? 0 : 1;
}
int dba_pcg_step_stats(dba_handle* h, float* lambda, int* trials, int* rejected_steps) {
  if (lambda) *lambda = h->ba->last_pcg_lambda();
  if (trials) *trials = h->ba->last_pcg_trials();
  if (rejected_steps) *rejected_steps = h->ba->last_pcg_rejected_steps();
  return 0;
}
int dba_set_pose_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_down, float lambda_min,
                              float lambda_max, int max_trials) {
  if (!enabled) return h->ba->SetPoseStepControl(nullptr) ? 0 : 1;
  vis::DirectBA::PoseStepControl control;
  control.lambda_initial = lambda_initial; control.lambda_up = lambda_up; control.lambda_down = lambda_down;
  control.lambda_min = lambda_min; control.lambda_max = lambda_max; control.max_trials = max_trials;
  return h->ba->SetPoseStepControl(&control) ? 0 : 1;
}
int dba_get_pose_step_stats(dba_handle* h, int* trials, int* rejected_steps, int keyframe_id, float* lambda) {
  if (trials) *trials = h->ba->last_pose_trials();
  if (rejected_steps) *rejected_steps = h->ba->last_pose_rejected_steps();
  if (lambda) *lambda = h->ba->pose_lambda(keyframe_id);
  return 0;
}
int dba_set_geometry_step_control(dba_handle* h, int enabled, float lambda_initial, float lambda_up, float lambda_min, float lambda_max,
                                  int max_trials, int guard_pairs) {
  if (!enabled) return h->ba->SetGeometryStepControl(nullptr) ? 0 : 1;
  vis::DirectBA::GeometryStepControl control;
  control.lambda_initial = lambda_initial; control.lambda_up = lambda_up; control.lambda_min = lambda_min; control.lambda_max = lambda_max;
  control.max_trials = max_trials; control.guard_pairs = guard_pairs != 0;
  return h->ba->SetGeometryStepControl(&control) ? 0 : 1;
}
int dba_get_geometry_step_stats(dba_handle* h, long long* candidates, long long* accepted, long long* restored, int* trials) {
  if (candidates) *candidates = h->ba->last_geometry_candidates();
  if (accepted) *accepted = h->ba->last_geometry_accepted();
  if (restored) *restored = h->ba->last_geometry_restored();
  if (trials) *trials = h->ba->last_geometry_trials();
  return 0;
}
int dba_set_intrinsics_step_control(dba_handle* h, int enabled, float lambda_first, float lambda_up, float lambda_max, int max_trials) {
  if (!enabled) return h->ba->SetIntrinsicsStepControl(nullptr) ? 0 : 1;
  vis::DirectBA::IntrinsicsStepControl control;
  control.lambda_first = lambda_first; control.lambda_up = lambda_up; control.lambda_max = lambda_max; control.max_trials = max_trials;
  return h->ba->SetIntrinsicsStepControl(&control) ? 0 : 1;
}
int dba_set_intrinsics_updated_callback(dba_handle* h, void (*callback)(void*), void* user) {
  if (callback) h->ba->SetIntrinsicsUpdatedCallback([callback, user]() { callback(user); });
  else h->ba->SetIntrinsicsUpdatedCallback(std::function<void()>());
  return 0;
}
int dba_get_intrinsics_step_drops(dba_handle* h, double* total, double* smallest) {
  if (total) *total = h->ba->last_intrinsics_cost_drop();
  if (smallest) *smallest = h->ba->last_intrinsics_smallest_drop();
  return 0;
}
int dba_get_intrinsics_step_stats(dba_handle* h, int* trials, int* accepted, float* lambda_accepted, float* lambda_next) {
  if (trials) *trials = h->ba->last_intrinsics_trials();
  if (accepted) *accepted = h->ba->last_intrinsics_accepted();
  if (lambda_accepted) *lambda_accepted = h->ba->last_intrinsics_lambda();
  if (lambda_next) *lambda_next = h->ba->intrinsics_lambda();
  return 0;
}
int dba_set_distributed_lifecycle(dba_handle* h, int enabled) { return h->ba->SetDistributedLifecycle(enabled != 0) ? 0 : 1; }
int dba_last_stats(dba_handle* h, int* pose_rounds, int* pose_steps, int* pcg_inner_steps) {
  if (pose_rounds) *pose_rounds = h->ba->last_pose_rounds();
  if (pose_steps) *pose_steps = h->ba->last_pose_steps();
  if (pcg_inner_steps) *pcg_inner_steps = h->ba->last_pcg_inner_steps();
  return 0;
}
bahip_context* dba_backend_context(dba_handle* h) { return h->ba->backend_context(); }
int dba_keyframe_frame(dba_handle* h, int id, bahip_frame* out) {
  Keyframe* kf = get_kf(h, id);
  if (!kf || !out) return 1;
  *out = kf->ToBahipFrame();
  return 0;
}
int dba_surfels_struct(dba_handle* h, bahip_surfels* out) {
  if (!out) return 1;
  *out = h->ba->SurfelsStruct(true);
  return 0;
}
int dba_keyframe_covisibility(dba_handle* h, int id, int* out, int capacity) {
  Keyframe* kf = get_kf(h, id);
  if (!kf) return -1;
  const auto& list = kf->co_visibility_list();
  for (int i = 0; i < (int)list.size() && i < capacity; ++i) out[i] = list[i];
  return (int)list.size();
}
int dba_bind_scene(dba_handle* h, void* stream) {
  h->ba->BindScene(static_cast<hipStream_t>(stream));
  return 0;
}

}  // extern "C"
