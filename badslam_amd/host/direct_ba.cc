// direct_ba.cc -- host driver of the MI355X direct-BA backend behind the reference's DirectBA surface.
// Control flow follows B/direct_ba.cc, B/direct_ba_alternating.cc and B/direct_ba_pcg.cc
// (B/ = applications/badslam/src/badslam/ of ETH3D/badslam); all device work goes through the C ABI
// (include/badslam_hip.h).  Where the reference loops over keyframes and launches one kernel per
// keyframe, this driver makes ONE call per stage.
#include "direct_ba.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <memory>

namespace vis {

namespace {
int ToBahipActivation(Keyframe::Activation a) { return static_cast<int>(a); }
}  // namespace

DirectBA::DirectBA(int max_surfel_count, float raw_to_float_depth, float baseline_fx, int sparse_surfel_cell_size,
                   float surfel_merge_dist_factor, int min_observation_count_while_bootstrapping_1,
                   int min_observation_count_while_bootstrapping_2, int min_observation_count,
                   const PinholeCamera4f& color_camera_initial_estimate, const PinholeCamera4f& depth_camera_initial_estimate,
                   int pyramid_level_for_color, bool use_depth_residuals, bool use_descriptor_residuals, void* render_window,
                   const SE3f& global_T_anchor_frame)
    : color_camera_(color_camera_initial_estimate), pyramid_level_for_color_(pyramid_level_for_color),
      depth_camera_(depth_camera_initial_estimate), use_depth_residuals_(use_depth_residuals),
      use_descriptor_residuals_(use_descriptor_residuals),
      min_observation_count_while_bootstrapping_1_(min_observation_count_while_bootstrapping_1),
      min_observation_count_while_bootstrapping_2_(min_observation_count_while_bootstrapping_2),
      min_observation_count_(min_observation_count), surfel_merge_dist_factor_(surfel_merge_dist_factor),
      global_T_anchor_frame_(global_T_anchor_frame) {
  CHECK(render_window == nullptr) << "the render window is not part of the BA backend";
  BAHIP_CHECKED_CALL(bahip_context_create(&ctx_, nullptr));
  // B/direct_ba.cc:107-121
  depth_params_.a = 0;
  cfactor_buffer_.reset(new CUDABuffer<float>((depth_camera_.height() - 1) / sparse_surfel_cell_size + 1,
                                              (depth_camera_.width() - 1) / sparse_surfel_cell_size + 1));
  cfactor_buffer_->Clear(0, nullptr);
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(nullptr));
  depth_params_.cfactor_buffer = cfactor_buffer_->ToCUDA();
  depth_params_.raw_to_float_depth = raw_to_float_depth;
  depth_params_.baseline_fx = baseline_fx;
  depth_params_.sparse_surfel_cell_size = sparse_surfel_cell_size;
  surfels_.reset(new CUDABuffer<float>(kSurfelAttributeCount, max_surfel_count));
  active_surfels_.reset(new CUDABuffer<u8>(1, max_surfel_count));
  for (int i = 0; i < kMergeBufferCount; ++i)
    supporting_surfels_[i].reset(new CUDABuffer<u32>(depth_camera_.height(), depth_camera_.width()));
}

DirectBA::~DirectBA() { bahip_context_destroy(ctx_); }

// ---- keyframe bookkeeping (B/direct_ba.cc:214-338,549-564,710-738) --------------------------------------------
void DirectBA::AddKeyframe(const shared_ptr<Keyframe>& new_keyframe) {
  new_keyframe->SetID(static_cast<int>(keyframes_.size()));
  DetermineNewKeyframeCoVisibility(new_keyframe);
  keyframes_.push_back(new_keyframe);
}

void DirectBA::DeleteKeyframe(int keyframe_index, void* /*loop_detector*/) {
  shared_ptr<Keyframe> frame_to_delete = keyframes_[keyframe_index];
  for (int covis_index : frame_to_delete->co_visibility_list()) {
    auto& list = keyframes_[covis_index]->co_visibility_list();
    auto it = std::find(list.begin(), list.end(), keyframe_index);
    if (it != list.end()) list.erase(it);
  }
  keyframes_[keyframe_index].reset();
}

void DirectBA::DetermineNewKeyframeCoVisibility(const shared_ptr<Keyframe>& new_keyframe) {
  CameraFrustum new_frustum(depth_camera_, new_keyframe->min_depth(), new_keyframe->max_depth(), new_keyframe->global_T_frame());
  for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
    if (!keyframe) continue;
    CameraFrustum frustum(depth_camera_, keyframe->min_depth(), keyframe->max_depth(), keyframe->global_T_frame());
    if (new_frustum.Intersects(frustum)) {
      new_keyframe->co_visibility_list().push_back(keyframe->id());
      keyframe->co_visibility_list().push_back(new_keyframe->id());
      if (keyframe->activation() == Keyframe::Activation::kInactive) keyframe->SetActivation(Keyframe::Activation::kCovisibleActive);
    }
  }
}

void DirectBA::AssignColors(hipStream_t stream) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  BAHIP_CHECKED_CALL(bahip_assign_colors(ctx_, &s));
}

void DirectBA::UpdateKeyframeCoVisibility(const shared_ptr<Keyframe>& keyframe) {
  for (int covis_index : keyframe->co_visibility_list()) {
    auto& list = keyframes_[covis_index]->co_visibility_list();
    auto it = std::find(list.begin(), list.end(), keyframe->id());
    if (it != list.end()) list.erase(it);
  }
  keyframe->co_visibility_list().clear();
  CameraFrustum frustum(depth_camera_, keyframe->min_depth(), keyframe->max_depth(), keyframe->global_T_frame());
  for (const shared_ptr<Keyframe>& other : keyframes_) {
    if (!other) continue;
    CameraFrustum other_frustum(depth_camera_, other->min_depth(), other->max_depth(), other->global_T_frame());
    if (frustum.Intersects(other_frustum)) {
      keyframe->co_visibility_list().push_back(other->id());
      other->co_visibility_list().push_back(keyframe->id());
    }
  }
}

void DirectBA::DetermineCovisibleActiveKeyframes() {
  for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
    if (!keyframe || keyframe->activation() != Keyframe::Activation::kActive) continue;
    for (int covisible_index : keyframe->co_visibility_list()) {
      shared_ptr<Keyframe>& other = keyframes_[covisible_index];
      if (other && other->activation() == Keyframe::Activation::kInactive) other->SetActivation(Keyframe::Activation::kCovisibleActive);
    }
  }
}

// B/direct_ba.cc:251-338: drops the keyframes that are closest to their neighbours (frees memory).
void DirectBA::MergeKeyframes(hipStream_t /*stream*/, void* loop_detector, usize approx_merge_count) {
  constexpr float kMaxAngleDifference = 0.5f * 1.57079632679f;
  constexpr float kMaxEuclideanDistance = 0.3f;
  if (keyframes_.size() <= 1) return;
  struct Candidate { float distance; usize prev_id, id, next_id; };
  vector<Candidate> distances;
  float prev_half_distance = 0;
  usize prev_keyframe_id = 0;
  for (usize id = 0; id + 1 < keyframes_.size(); ++id) {
    const shared_ptr<Keyframe>& keyframe = keyframes_[id];
    if (!keyframe) continue;
    const Keyframe* next = nullptr;
    for (usize n = id + 1; n < keyframes_.size(); ++n) if (keyframes_[n]) { next = keyframes_[n].get(); break; }
    if (!next) break;
    float Ra[9], Rb[9];
    keyframe->global_T_frame().rotationMatrix(Ra);
    next->global_T_frame().rotationMatrix(Rb);
    const float dot = Ra[2] * Rb[2] + Ra[5] * Rb[5] + Ra[8] * Rb[8];   // z axes
    const float angle_difference = acosf(dot);
    if (angle_difference > kMaxAngleDifference) continue;
    const float* ta = keyframe->global_T_frame().translation();
    const float* tb = next->global_T_frame().translation();
    const float dist = sqrtf((ta[0] - tb[0]) * (ta[0] - tb[0]) + (ta[1] - tb[1]) * (ta[1] - tb[1]) + (ta[2] - tb[2]) * (ta[2] - tb[2]));
    if (dist > kMaxEuclideanDistance) continue;
    const float next_half_distance = dist + (0.5f / 1.57079632679f) * angle_difference;
    if (id > 0) distances.push_back({prev_half_distance + next_half_distance, prev_keyframe_id, id, (usize)next->id()});
    prev_half_distance = next_half_distance;
    prev_keyframe_id = id;
  }
  const usize count = std::min(approx_merge_count, distances.size());
  std::partial_sort(distances.begin(), distances.begin() + count, distances.end(),
                    [](const Candidate& a, const Candidate& b) { return a.distance < b.distance; });
  for (usize i = 0; i < count; ++i) {
    const Candidate& m = distances[i];
    if (!keyframes_[m.prev_id] || !keyframes_[m.id] || !keyframes_[m.next_id]) continue;
    DeleteKeyframe((int)m.id, loop_detector);
    LOG(WARNING) << "Deleted keyframe with ID " << m.id;
  }
}

// ---- scene binding ---------------------------------------------------------------------------------------------
bahip_surfels DirectBA::SurfelsStruct(bool with_active) const {
  bahip_surfels s;
  s.data = surfels_->ToCUDA().address();
  s.pitch_bytes = (uint32_t)surfels_->ToCUDA().pitch();
  s.active = with_active ? active_surfels_->ToCUDA().address() : nullptr;
  s.surfels_size = surfels_size_;
  s.capacity = (uint32_t)surfels_->width();
  return s;
}

void DirectBA::BindScene(hipStream_t stream) {
  static const bool host_timing = getenv("BADSLAM_HOST_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = host_timing ? now() : 0;
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_camera cc = ToBahipCamera(color_camera_), dc = ToBahipCamera(depth_camera_);
  const bahip_depth_params dp = ToBahipDepthParams(depth_params_);
  BAHIP_CHECKED_CALL(bahip_set_intrinsics(ctx_, &cc, &dc, &dp));
  vector<bahip_keyframe> list;
  bound_ids_.clear();
  id_to_bound_.assign(keyframes_.size(), -1);
  for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
    if (!keyframe) continue;
    bahip_keyframe k;
    k.frame = keyframe->ToBahipFrame();
    memcpy(k.global_T_frame, keyframe->global_T_frame().data(), 7 * sizeof(float));
    k.activation = ToBahipActivation(keyframe->activation());
    id_to_bound_[keyframe->id()] = (int)list.size();
    bound_ids_.push_back(keyframe->id());
    list.push_back(k);
  }
  const double t1 = host_timing ? now() : 0;
  BAHIP_CHECKED_CALL(bahip_set_keyframes(ctx_, list.data(), (int)list.size()));
  const double t2 = host_timing ? now() : 0;
  // co-visibility lists over bound indices: the activation state machine of the alternating scheme runs on the device table
  vector<int> offsets(1, 0), indices;
  for (int id : bound_ids_) {
    for (int other : keyframes_[id]->co_visibility_list())
      if (other >= 0 && other < (int)id_to_bound_.size() && id_to_bound_[other] >= 0) indices.push_back(id_to_bound_[other]);
    offsets.push_back((int)indices.size());
  }
  const double t3 = host_timing ? now() : 0;
  BAHIP_CHECKED_CALL(bahip_set_covisibility(ctx_, offsets.data(), indices.data(), (int)bound_ids_.size()));
  if (host_timing)
    fprintf(stderr, "[BindScene, us] list %.0f | set_keyframes %.0f | covisibility lists (%zu entries) %.0f | set_covisibility %.0f\n", t1 - t0,
            t2 - t1, indices.size(), t3 - t2, now() - t3);
}

// ---- surfel sharding: whole-cloud phases -----------------------------------------------------------------------------
void DirectBA::SetSurfelSharding(int rank, int world, u32 chunk) {
  CHECK(world >= 1 && rank >= 0 && rank < world && chunk > 0 && chunk % 64 == 0) << "bad surfel partition";
  CHECK(world == 1 || keyframe_shard_world_ == 1) << "surfel and keyframe sharding exclude each other";
  CHECK_EQ(whole_cloud_depth_, 0);
  shard_rank_ = rank; shard_world_ = world; shard_chunk_ = chunk;
  if (world > 1 && !other_surfels_) {
    CHECK_EQ(surfels_->width() % 8, 0) << "surfel sharding needs max_surfel_count to be a multiple of 8";
    other_surfels_.reset(new CUDABuffer<float>(kSurfelAttributeCount, surfels_->width()));
    other_active_surfels_.reset(new CUDABuffer<u8>(1, surfels_->width()));
  }
}

void DirectBA::SetSumClasses(int classes) { BAHIP_CHECKED_CALL(bahip_context_set_sum_classes(ctx_, classes)); }
void DirectBA::SetIntrinsicsSumClasses(int classes) { BAHIP_CHECKED_CALL(bahip_context_set_intrinsics_sum_classes(ctx_, classes)); }
void DirectBA::SetPCGSumClasses(int classes) {
  CHECK(!windowed_pcg_ || classes == 1) << "the windowed PCG scheme needs one PCG sum class: SetWindowedPCG(false) first";
  BAHIP_CHECKED_CALL(bahip_context_set_pcg_sum_classes(ctx_, classes));
  pcg_sum_classes_ = classes;
}
void DirectBA::SetFastArithmetic(bool enabled) { BAHIP_CHECKED_CALL(bahip_context_set_arithmetic(ctx_, enabled ? BAHIP_ARITHMETIC_FAST : BAHIP_ARITHMETIC_EXACT)); }
void DirectBA::SetRowMajorCreation(bool enabled) { BAHIP_CHECKED_CALL(bahip_context_set_creation_order(ctx_, enabled ? 1 : 0)); }

bool DirectBA::SetWindowedPCG(bool enabled) {
  if (enabled && keyframe_shard_world_ > 1) {
    LOG(ERROR) << "SetWindowedPCG: the windowed PCG scheme is not available under keyframe sharding";
    return false;
  }
  if (enabled && pcg_sum_classes_ > 1) {
    LOG(ERROR) << "SetWindowedPCG: the windowed PCG scheme needs one PCG sum class (SetPCGSumClasses(1))";
    return false;
  }
  windowed_pcg_ = enabled;
  return true;
}

bool DirectBA::SetPCGStepControl(const PCGStepControl* control) {
  if (!control) {
    pcg_step_control_on_ = false;
    return true;
  }
  if (keyframe_shard_world_ > 1) {
    LOG(ERROR) << "SetPCGStepControl: step control of the PCG scheme is not available under keyframe sharding";
    return false;
  }
  if (!(control->max_trials >= 1 && control->lambda_up >= 1.f && control->lambda_down > 0.f && control->lambda_down <= 1.f &&
        control->lambda_min >= 0.f && control->lambda_min <= control->lambda_max && control->lambda_initial >= 0.f)) {
    LOG(ERROR) << "SetPCGStepControl: needs max_trials >= 1, lambda_up >= 1, 0 < lambda_down <= 1, 0 <= lambda_min <= lambda_max, lambda_initial >= 0";
    return false;
  }
  pcg_step_control_ = *control;
  pcg_step_control_on_ = true;
  pcg_lambda_ = control->lambda_initial;
  return true;
}

bool DirectBA::SetPoseStepControl(const PoseStepControl* control) {
  if (!control) {
    pose_step_control_on_ = false;
    return true;
  }
  if (keyframe_shard_world_ > 1) {
    LOG(ERROR) << "SetPoseStepControl: step control of the pose phase is not available under keyframe sharding";
    return false;
  }
  // (the checks of bahip_estimate_keyframe_poses_controlled, which would otherwise refuse in the middle of BundleAdjustment)
  if (!(control->max_trials >= 1 && std::isfinite(control->lambda_up) && control->lambda_up >= 1.f && control->lambda_down > 0.f &&
        control->lambda_down <= 1.f && control->lambda_min >= 0.f && std::isfinite(control->lambda_max) &&
        control->lambda_min <= control->lambda_max && std::isfinite(control->lambda_initial) && control->lambda_initial >= 0.f)) {
    LOG(ERROR) << "SetPoseStepControl: needs max_trials >= 1, finite lambda_up >= 1, 0 < lambda_down <= 1, 0 <= lambda_min <= finite lambda_max, "
                  "finite lambda_initial >= 0";
    return false;
  }
  pose_step_control_ = *control;
  pose_step_control_on_ = true;
  return true;
}

bool DirectBA::SetGeometryStepControl(const GeometryStepControl* control) {
  if (!control) {
    geometry_step_control_on_ = false;
    return true;
  }
  // (the checks of bahip_optimize_geometry_iteration_controlled, which would otherwise refuse in the middle of BundleAdjustment)
  if (!(control->max_trials >= 1 && control->max_trials <= 254 && std::isfinite(control->lambda_initial) && control->lambda_initial >= 0.f &&
        std::isfinite(control->lambda_up) && control->lambda_up > 1.f && std::isfinite(control->lambda_min) && control->lambda_min > 0.f &&
        std::isfinite(control->lambda_max) && control->lambda_min <= control->lambda_max)) {
    LOG(ERROR) << "SetGeometryStepControl: needs 1 <= max_trials <= 254, finite lambda_initial >= 0, finite lambda_up > 1, "
                  "0 < lambda_min <= finite lambda_max";
    return false;
  }
  geometry_step_control_ = *control;
  geometry_step_control_on_ = true;
  return true;
}

bool DirectBA::SetIntrinsicsStepControl(const IntrinsicsStepControl* control) {
  if (!control) {
    intrinsics_step_control_on_ = false;
    return true;
  }
  // (the checks of bahip_optimize_intrinsics_controlled, which would otherwise refuse in the middle of BundleAdjustment)
  if (!(control->max_trials >= 1 && std::isfinite(control->lambda_first) && control->lambda_first > 0.f && std::isfinite(control->lambda_up) &&
        control->lambda_up > 1.f && std::isfinite(control->lambda_max) && control->lambda_first <= control->lambda_max)) {
    LOG(ERROR) << "SetIntrinsicsStepControl: needs max_trials >= 1, finite lambda_first > 0, finite lambda_up > 1, lambda_first <= finite lambda_max";
    return false;
  }
  intrinsics_step_control_ = *control;
  intrinsics_step_control_on_ = true;
  return true;
}

bool DirectBA::SetDistributedLifecycle(bool enabled) {
  if (enabled && keyframe_shard_world_ > 1) {
    LOG(ERROR) << "SetDistributedLifecycle: keyframe sharding deals its lifecycle by keyframe already";
    return false;
  }
  if (bahip_context_set_lifecycle_dealing(ctx_, enabled ? 1 : 0) != 0) {
    LOG(ERROR) << "SetDistributedLifecycle: " << bahip_last_error();
    return false;
  }
  distributed_lifecycle_ = enabled;
  return true;
}

void DirectBA::SetKeyframeSharding(int rank, int world) {
  CHECK(!distributed_lifecycle_ || world == 1) << "keyframe sharding deals its own lifecycle: SetDistributedLifecycle(false) first";
  CHECK(!windowed_pcg_ || world == 1) << "the windowed PCG scheme is not available under keyframe sharding: SetWindowedPCG(false) first";
  CHECK(!pcg_step_control_on_ || world == 1) << "step control of the PCG scheme is not available under keyframe sharding: SetPCGStepControl(nullptr) first";
  CHECK(!pose_step_control_on_ || world == 1) << "step control of the pose phase is not available under keyframe sharding: SetPoseStepControl(nullptr) first";
  CHECK_EQ(shard_world_, 1) << "surfel and keyframe sharding exclude each other";
  BAHIP_CHECKED_CALL(bahip_context_set_keyframe_sharding(ctx_, rank, world));
  keyframe_shard_world_ = world;
}

void DirectBA::EnterWholeCloud(hipStream_t stream) {
  if (shard_world_ <= 1 || whole_cloud_depth_++ > 0) return;
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_surfels shard = SurfelsStruct();
  std::swap(surfels_, other_surfels_);
  std::swap(active_surfels_, other_active_surfels_);
  bahip_surfels cloud = SurfelsStruct();
  uint32_t size = 0, count = 0;
  BAHIP_CHECKED_CALL(bahip_gather_surfel_shards(ctx_, &shard, surfel_count_, shard_rank_, shard_world_, shard_chunk_, &cloud, &size, &count));
  Lock();
  surfels_size_ = size;
  surfel_count_ = count;
  Unlock();
}

void DirectBA::LeaveWholeCloud(hipStream_t stream) {
  if (shard_world_ <= 1 || --whole_cloud_depth_ > 0) return;
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  CHECK_EQ(surfels_size_, surfel_count_) << "a whole-cloud phase must end compacted";
  const bahip_surfels cloud = SurfelsStruct();
  std::swap(surfels_, other_surfels_);
  std::swap(active_surfels_, other_active_surfels_);
  bahip_surfels shard = SurfelsStruct();
  uint32_t mine = 0;
  BAHIP_CHECKED_CALL(bahip_extract_surfel_shard(ctx_, &cloud, shard_rank_, shard_world_, shard_chunk_, &shard, &mine));
  Lock();
  surfels_size_ = mine;
  surfel_count_ = mine;
  Unlock();
}

// ---- surfel creation (B/direct_ba.cc:340-405) ---------------------------------------------------------------------
void DirectBA::CreateSurfelsForKeyframe(hipStream_t stream, bool filter_new_surfels, const shared_ptr<Keyframe>& keyframe) {
  WholeCloudScope whole_cloud(this, stream);
  // inside a batch (the BA loop's creation pass) the scene was bound once for all its keyframes: nothing the binding reads
  // (poses, activations, co-visibility lists, intrinsics) changes between the creations of one batch
  if (!creation_batch_bound_) BindScene(stream);
  vector<int> covis;
  for (int id : keyframe->co_visibility_list())
    if (id >= 0 && id < (int)id_to_bound_.size() && id_to_bound_[id] >= 0) covis.push_back(id_to_bound_[id]);
  uint32_t* sup[kMergeBufferCount];
  for (int i = 0; i < kMergeBufferCount; ++i) sup[i] = supporting_surfels_[i]->ToCUDA().address();
  const bahip_surfels s = SurfelsStruct();
  uint32_t new_surfel_count = 0;
  BAHIP_CHECKED_CALL(bahip_create_surfels_for_keyframe(ctx_, id_to_bound_[keyframe->id()], filter_new_surfels ? 1 : 0,
                                                       GetMinObservationCount(), covis.data(), (int)covis.size(), &s, sup,
                                                       (uint32_t)supporting_surfels_[0]->ToCUDA().pitch(), &new_surfel_count));
  if (bahip_context_take_capacity_exceeded(ctx_)) LOG(ERROR) << "Maximum surfel count exceeded! Retry with a higher max_surfel_count.";
  Lock();
  surfels_size_ += new_surfel_count;
  surfel_count_ += new_surfel_count;
  unsorted_surfels_ += new_surfel_count;
  Unlock();
}

// A batch of keyframes in one call of the backend (bahip_create_surfels_for_keyframes): the creations of B/direct_ba_alternating.cc:
// 389-425 in their order, the cloud's size on the device in between.
void DirectBA::CreateSurfelsForKeyframes(hipStream_t stream, bool filter_new_surfels, const vector<u32>& keyframe_ids) {
  if (keyframe_ids.empty()) return;
  CHECK(batched_creation_ || keyframe_shard_world_ == 1) << "keyframe sharding creates surfels through the batched call only";
  if (!batched_creation_) {
    for (u32 id : keyframe_ids) CreateSurfelsForKeyframe(stream, filter_new_surfels, keyframes_[id]);
    return;
  }
  WholeCloudScope whole_cloud(this, stream);
  if (!creation_batch_bound_) BindScene(stream);
  vector<int> bound, offsets(1, 0), covis;
  for (u32 id : keyframe_ids) {
    bound.push_back(id_to_bound_[id]);
    for (int other : keyframes_[id]->co_visibility_list())
      if (other >= 0 && other < (int)id_to_bound_.size() && id_to_bound_[other] >= 0) covis.push_back(id_to_bound_[other]);
    offsets.push_back((int)covis.size());
  }
  uint32_t* sup[kMergeBufferCount];
  for (int i = 0; i < kMergeBufferCount; ++i) sup[i] = supporting_surfels_[i]->ToCUDA().address();
  const bahip_surfels s = SurfelsStruct();
  uint32_t new_surfel_count = 0;
  BAHIP_CHECKED_CALL(bahip_lifecycle_batch_set_keyframes(ctx_, bound.data(), (int)bound.size()));   // (nothing without an open batch)
  BAHIP_CHECKED_CALL(bahip_create_surfels_for_keyframes(ctx_, bound.data(), (int)bound.size(), filter_new_surfels ? 1 : 0, GetMinObservationCount(),
                                                        offsets.data(), covis.data(), &s, sup, (uint32_t)supporting_surfels_[0]->ToCUDA().pitch(),
                                                        &new_surfel_count));
  if (bahip_context_take_capacity_exceeded(ctx_)) LOG(ERROR) << "Maximum surfel count exceeded! Retry with a higher max_surfel_count.";
  Lock();
  surfels_size_ += new_surfel_count;
  surfel_count_ += new_surfel_count;
  unsorted_surfels_ += new_surfel_count;
  Unlock();
}

void DirectBA::MergeForKeyframe(const Keyframe& keyframe, bool defer_count) {
  uint32_t* sup[kMergeBufferCount];
  for (int i = 0; i < kMergeBufferCount; ++i) sup[i] = supporting_surfels_[i]->ToCUDA().address();
  const bahip_frame frame = keyframe.ToBahipFrame();
  float F[12];
  keyframe.frame_T_global().matrix3x4(F);
  const bahip_surfels s = SurfelsStruct();
  uint32_t merged = 0;
  BAHIP_CHECKED_CALL(bahip_determine_supporting_surfels(ctx_, 1, surfel_merge_dist_factor_, &frame, F, &s, sup,
                                                        (uint32_t)supporting_surfels_[0]->ToCUDA().pitch(), defer_count ? nullptr : &merged));
  surfel_count_ -= merged;
}

// Tile bounds for the per-keyframe sweeps of a batch (include/badslam_hip.h: bahip_lifecycle_batch_begin).
DirectBA::LifecycleBatch::LifecycleBatch(DirectBA* ba) : ba_(ba) {
  const bahip_surfels s = ba_->SurfelsStruct();
  BAHIP_CHECKED_CALL(bahip_lifecycle_batch_begin(ba_->ctx_, &s));
}
DirectBA::LifecycleBatch::~LifecycleBatch() { bahip_lifecycle_batch_end(ba_->ctx_); }

// The merges of a batch of keyframes (the BA loop's merge pass, the end tasks'): one lifecycle batch that knows its frames -- each
// keyframe's sweeps then run over the tiles it can see --, counts deferred to one read at the end.
void DirectBA::MergeForKeyframes(const vector<u32>& keyframe_ids) {
  vector<float> frames;
  for (u32 id : keyframe_ids) {
    if (!keyframes_[id]) continue;
    float F[12];
    keyframes_[id]->frame_T_global().matrix3x4(F);   // what MergeForKeyframe passes: the list is found by these coefficients
    frames.insert(frames.end(), F, F + 12);
  }
  if (frames.empty()) return;
  LifecycleBatch batch(this);
  if (keyframe_shard_world_ > 1 || (distributed_lifecycle_ && shard_world_ > 1 && batched_creation_)) {
    // by bound index: a rank knows which keyframes it owns (the bound poses are the keyframes' current ones: every merge pass follows a
    // binding of the scene); the same deletions as the frame-based call below
    CHECK(batched_creation_) << "keyframe sharding merges through the batched call only";
    vector<int> bound;
    for (u32 id : keyframe_ids)
      if (keyframes_[id]) bound.push_back(id_to_bound_[id]);
    uint32_t* sup[kMergeBufferCount];
    for (int i = 0; i < kMergeBufferCount; ++i) sup[i] = supporting_surfels_[i]->ToCUDA().address();
    const bahip_surfels s = SurfelsStruct();
    BAHIP_CHECKED_CALL(bahip_lifecycle_batch_set_keyframes(ctx_, bound.data(), (int)bound.size()));
    BAHIP_CHECKED_CALL(bahip_merge_surfels_for_bound_keyframes(ctx_, surfel_merge_dist_factor_, bound.data(), (int)bound.size(), &s, sup,
                                                               (uint32_t)supporting_surfels_[0]->ToCUDA().pitch(), nullptr));
    TakeDeferredMergeCount();
    return;
  }
  BAHIP_CHECKED_CALL(bahip_lifecycle_batch_set_frames(ctx_, frames.data(), (int)(frames.size() / 12)));
  if (batched_creation_) {
    // one call for the batch: two dependent launches per keyframe instead of three (bahip_merge_surfels_for_keyframes)
    vector<bahip_frame> structs;
    for (u32 id : keyframe_ids)
      if (keyframes_[id]) structs.push_back(keyframes_[id]->ToBahipFrame());
    uint32_t* sup[kMergeBufferCount];
    for (int i = 0; i < kMergeBufferCount; ++i) sup[i] = supporting_surfels_[i]->ToCUDA().address();
    const bahip_surfels s = SurfelsStruct();
    BAHIP_CHECKED_CALL(bahip_merge_surfels_for_keyframes(ctx_, surfel_merge_dist_factor_, structs.data(), frames.data(), (int)structs.size(), &s, sup,
                                                         (uint32_t)supporting_surfels_[0]->ToCUDA().pitch(), nullptr));
  } else {
    for (u32 id : keyframe_ids)
      if (keyframes_[id]) MergeForKeyframe(*keyframes_[id], /*defer_count*/ true);
  }
  TakeDeferredMergeCount();
}

// The merges of a batch of keyframes run back to back on the stream; their total is read once, before the compaction that needs it
// (the reference reads one count per keyframe, B/direct_ba.cc:618-622 -- the buffer contents are the same either way).
void DirectBA::TakeDeferredMergeCount() {
  uint32_t merged = 0;
  BAHIP_CHECKED_CALL(bahip_take_merged_count(ctx_, &merged));
  surfel_count_ -= merged;
}

// ---- single-frame pose estimation (B/direct_ba_alternating.cc:42-283) -----------------------------------------------
void DirectBA::EstimateFramePose(hipStream_t stream, const SE3f& global_T_frame_initial_estimate, const CUDABuffer<u16>& depth_buffer,
                                 const CUDABuffer<u16>& normals_buffer, hipTextureHandle_t color_texture,
                                 SE3f* out_global_T_frame_estimate, bool /*called_within_ba*/) {
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_camera cc = ToBahipCamera(color_camera_), dc = ToBahipCamera(depth_camera_);
  const bahip_depth_params dp = ToBahipDepthParams(depth_params_);
  BAHIP_CHECKED_CALL(bahip_set_intrinsics(ctx_, &cc, &dc, &dp));
  bahip_frame frame{};
  frame.depth = depth_buffer.ToCUDA().address(); frame.depth_pitch_bytes = (uint32_t)depth_buffer.ToCUDA().pitch();
  frame.normals = normals_buffer.ToCUDA().address(); frame.normals_pitch_bytes = (uint32_t)normals_buffer.ToCUDA().pitch();
  frame.color = reinterpret_cast<uint8_t*>(color_texture->ToCUDA().address());
  frame.color_pitch_bytes = (uint32_t)color_texture->ToCUDA().pitch();
  const bahip_surfels s = SurfelsStruct();
  int iterations = 0, converged = 0;
  BAHIP_CHECKED_CALL(bahip_estimate_frame_pose(ctx_, use_depth_residuals_, use_descriptor_residuals_, &frame,
                                               global_T_frame_initial_estimate.data(), &s, out_global_T_frame_estimate->data(),
                                               &iterations, &converged));
  if (!converged) LOG(WARNING) << "Pose estimation not converged";
}

// ---- dispatcher (B/direct_ba.cc:407-454) ---------------------------------------------------------------------------------
void DirectBA::ComputeCost(hipStream_t stream, BACost* total, vector<BACost>* per_keyframe) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  bahip_cost sum{};
  vector<bahip_cost> bound(bound_ids_.size());
  BAHIP_CHECKED_CALL(bahip_evaluate_cost(ctx_, use_depth_residuals_ ? 1 : 0, use_descriptor_residuals_ ? 1 : 0, &s, &sum,
                                         per_keyframe ? bound.data() : nullptr));
  auto convert = [](const bahip_cost& c) {
    BACost out;
    out.depth = c.depth; out.descriptor_1 = c.descriptor_1; out.descriptor_2 = c.descriptor_2;
    out.depth_residuals = c.depth_residuals; out.descriptor_pairs = c.descriptor_pairs;
    return out;
  };
  if (total) *total = convert(sum);
  if (per_keyframe) {
    per_keyframe->assign(keyframes_.size(), BACost());
    for (size_t j = 0; j < bound_ids_.size(); ++j) (*per_keyframe)[bound_ids_[j]] = convert(bound[j]);
  }
}

void DirectBA::ComputeSurfelCosts(hipStream_t stream, SurfelCosts* out) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const size_t n = s.surfels_size;
  out->depth.assign(n, 0.0); out->descriptor_1.assign(n, 0.0); out->descriptor_2.assign(n, 0.0);
  out->depth_residuals.assign(n, 0u); out->descriptor_pairs.assign(n, 0u);
  if (n == 0) return;
  // one device block for the five planes: 3 x n binary64 followed by 2 x n words
  CUDABuffer<uint32_t> planes(1, (int)(8 * n));
  char* base = reinterpret_cast<char*>(planes.ToCUDA().address());
  bahip_surfel_costs dev{};
  dev.depth = reinterpret_cast<double*>(base);
  dev.descriptor_1 = dev.depth + n;
  dev.descriptor_2 = dev.depth + 2 * n;
  dev.depth_residuals = reinterpret_cast<uint32_t*>(dev.depth + 3 * n);
  dev.descriptor_pairs = dev.depth_residuals + n;
  BAHIP_CHECKED_CALL(bahip_evaluate_surfel_costs(ctx_, use_depth_residuals_ ? 1 : 0, use_descriptor_residuals_ ? 1 : 0, &s, &dev));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->depth.data(), dev.depth, sizeof(double) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->descriptor_1.data(), dev.descriptor_1, sizeof(double) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->descriptor_2.data(), dev.descriptor_2, sizeof(double) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->depth_residuals.data(), dev.depth_residuals, sizeof(uint32_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->descriptor_pairs.data(), dev.descriptor_pairs, sizeof(uint32_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::ComputeObservedCovisibility(hipStream_t stream, vector<uint32_t>* counts, vector<int>* keyframe_ids) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const size_t K = bound_ids_.size();
  counts->assign(K * K, 0u);
  if (keyframe_ids) keyframe_ids->assign(bound_ids_.begin(), bound_ids_.end());
  if (K == 0) return;
  CUDABuffer<uint32_t> words(1, (int)(K * K));
  uint32_t* dev = words.ToCUDA().address();
  BAHIP_CHECKED_CALL(bahip_observed_covisibility(ctx_, &s, dev, (int)K));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, counts->data(), dev, sizeof(uint32_t) * K * K, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::ComputeReducedCameraSystem(hipStream_t stream, ReducedCameraSystem* out, bool marginalise) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const size_t K = bound_ids_.size(), n = 6 * K;
  *out = ReducedCameraSystem();
  out->S.assign(n * n, 0.0); out->g.assign(n, 0.0); out->A_diag.assign(36 * K, 0.0); out->b.assign(n, 0.0);
  out->keyframe_ids.assign(bound_ids_.begin(), bound_ids_.end());
  if (K == 0) return;
  // one device block for the four planes, in doubles: S, g, A_diag, b
  const size_t doubles = n * n + n + 36 * K + n;
  if (2 * doubles > (size_t)0x7fffffff) LOG(FATAL) << "ComputeReducedCameraSystem: " << K << " keyframes are too many for one buffer";
  CUDABuffer<uint32_t> planes(1, (int)(2 * doubles));
  double* dev_S = reinterpret_cast<double*>(planes.ToCUDA().address());
  double* dev_g = dev_S + n * n;
  double* dev_A = dev_g + n;
  double* dev_b = dev_A + 36 * K;
  bahip_rcs_stats stats{};
  BAHIP_CHECKED_CALL(bahip_reduced_camera_system(ctx_, use_depth_residuals_ ? 1 : 0, use_descriptor_residuals_ ? 1 : 0, marginalise ? 1 : 0, &s, dev_S, n,
                                                 dev_g, dev_A, dev_b, &stats));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->S.data(), dev_S, sizeof(double) * n * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->g.data(), dev_g, sizeof(double) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->A_diag.data(), dev_A, sizeof(double) * 36 * K, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->b.data(), dev_b, sizeof(double) * n, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
  out->list_entries = stats.list_entries; out->pairs_visited = stats.pairs_visited; out->atomics_issued = stats.atomics_issued;
  out->degenerate_surfels = stats.degenerate_surfels; out->overflow_tiles = stats.overflow_tiles; out->invalid = stats.invalid;
}

bool DirectBA::PoseCovariancesOf(const ReducedCameraSystem& system, int gauge_keyframe_id, PoseCovariances* out,
                                 const vector<std::pair<int, int>>* pairs, std::string* error) {
  auto refuse = [&](const std::string& why) { if (error) *error = why; return false; };
  const size_t K = system.keyframe_ids.size();
  vector<int> ids;           // the remaining keyframes
  vector<size_t> blocks;     // ... and their blocks in the system
  bool found = false;
  for (size_t i = 0; i < K; ++i) {
    if (system.keyframe_ids[i] == gauge_keyframe_id) { found = true; continue; }
    ids.push_back(system.keyframe_ids[i]);
    blocks.push_back(i);
  }
  if (!found) return refuse("pose covariances: the gauge keyframe " + std::to_string(gauge_keyframe_id) + " does not exist");
  auto row_of = [&](int id) { for (size_t r = 0; r < ids.size(); ++r) if (ids[r] == id) return (long)r; return -1l; };
  if (pairs)
    for (const auto& p : *pairs)
      if (row_of(p.first) < 0 || row_of(p.second) < 0)
        return refuse("pose covariances: the pair (" + std::to_string(p.first) + ", " + std::to_string(p.second) + ") names the gauge keyframe or a keyframe that does not exist");
  if (system.invalid) return refuse("pose covariances: the sums of the reduced camera system were invalid");
  const size_t m = 6 * ids.size(), n = 6 * K;
  // R = S without the gauge rows and columns; R = L D L^T in place (L unit lower in the strict lower triangle, D on the diagonal)
  vector<double> R(m * m);
  for (size_t r = 0; r < m; ++r)
    for (size_t c = 0; c < m; ++c) R[r * m + c] = system.S[(6 * blocks[r / 6] + r % 6) * n + 6 * blocks[c / 6] + c % 6];
  for (size_t j = 0; j < m; ++j) {
    double d = R[j * m + j];
    for (size_t k = 0; k < j; ++k) d -= R[j * m + k] * R[j * m + k] * R[k * m + k];
    if (!(d > 0.0) || !std::isfinite(d))
      return refuse("pose covariances: pivot " + std::to_string(j) + " (keyframe " + std::to_string(ids[j / 6]) + ", unknown " + std::to_string(j % 6) +
                    ") is not positive: the poses are not determined");
    R[j * m + j] = d;
    for (size_t i = j + 1; i < m; ++i) {
      double v = R[i * m + j];
      for (size_t k = 0; k < j; ++k) v -= R[i * m + k] * R[j * m + k] * R[k * m + k];
      R[i * m + j] = v / d;
    }
  }
  // W = L^-1 (unit lower), then the inverse = W^T D^-1 W
  vector<double> W(m * m, 0.0);
  for (size_t c = 0; c < m; ++c) {
    W[c * m + c] = 1.0;
    for (size_t i = c + 1; i < m; ++i) {
      double v = 0.0;
      for (size_t k = c; k < i; ++k) v -= R[i * m + k] * W[k * m + c];
      W[i * m + c] = v;
    }
  }
  auto inverse = [&](size_t r, size_t c) {
    double v = 0.0;
    for (size_t k = std::max(r, c); k < m; ++k) v += W[k * m + r] * W[k * m + c] / R[k * m + k];
    return v;
  };
  PoseCovariances result;
  result.keyframe_ids = ids;
  result.marginal.resize(36 * ids.size());
  for (size_t q = 0; q < ids.size(); ++q)
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) result.marginal[36 * q + 6 * i + j] = inverse(6 * q + std::min(i, j), 6 * q + std::max(i, j));
  if (pairs) {
    result.cross.resize(36 * pairs->size());
    for (size_t q = 0; q < pairs->size(); ++q) {
      const size_t a = (size_t)row_of((*pairs)[q].first), b = (size_t)row_of((*pairs)[q].second);
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) result.cross[36 * q + 6 * i + j] = inverse(6 * a + i, 6 * b + j);
    }
  }
  *out = std::move(result);
  return true;
}

bool DirectBA::ComputePoseCovariances(hipStream_t stream, int gauge_keyframe_id, PoseCovariances* out, const vector<std::pair<int, int>>* pairs,
                                      std::string* error) {
  ReducedCameraSystem system;
  ComputeReducedCameraSystem(stream, &system, /*marginalise*/ true);
  return PoseCovariancesOf(system, gauge_keyframe_id, out, pairs, error);
}

void DirectBA::ComputeSurfelObservations(hipStream_t stream, SurfelObservations* out, bool with_residuals) {
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const size_t n = s.surfels_size;
  out->keyframe_ids.assign(bound_ids_.begin(), bound_ids_.end());
  out->first.assign(n + 1, 0u);
  out->keyframes.clear(); out->depth_raw.clear(); out->descriptor_raw.clear();
  CUDABuffer<uint32_t> first(1, (int)(n + 1));
  bahip_observations dev{};
  dev.surfel_first = first.ToCUDA().address();
  uint64_t pairs = 0;
  BAHIP_CHECKED_CALL(bahip_surfel_observations(ctx_, &s, &dev, &pairs));   // the count: sizes the planes
  if (pairs > 0) {
    // one device block for the planes: the words of the payload first, the 16-bit indices last
    const size_t payload_words = with_residuals ? 3 * pairs : 0;
    if (payload_words + (pairs + 1) / 2 > (size_t)0x7fffffff) LOG(FATAL) << "ComputeSurfelObservations: " << pairs << " pairs are too many for one buffer";
    CUDABuffer<uint32_t> planes(1, (int)(payload_words + (pairs + 1) / 2));
    uint32_t* base = planes.ToCUDA().address();
    if (with_residuals) {
      dev.descriptor_raw = reinterpret_cast<float*>(base);
      dev.depth_raw = reinterpret_cast<float*>(base) + 2 * pairs;
    }
    dev.keyframes = reinterpret_cast<uint16_t*>(base + payload_words);
    dev.capacity = pairs;
    uint64_t filled = 0;
    BAHIP_CHECKED_CALL(bahip_surfel_observations(ctx_, &s, &dev, &filled));
    if (filled != pairs) LOG(FATAL) << "ComputeSurfelObservations: the pairs changed between the count and the fill";
    out->keyframes.resize(pairs);
    BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->keyframes.data(), dev.keyframes, sizeof(uint16_t) * pairs, 2));
    if (with_residuals) {
      out->depth_raw.resize(pairs); out->descriptor_raw.resize(2 * pairs);
      BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->depth_raw.data(), dev.depth_raw, sizeof(float) * pairs, 2));
      BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->descriptor_raw.data(), dev.descriptor_raw, sizeof(float) * 2 * pairs, 2));
    }
  }
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->first.data(), dev.surfel_first, sizeof(uint32_t) * (n + 1), 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::ComputeKeyframeRedundancy(hipStream_t stream, int bins, vector<uint32_t>* hist, vector<int>* keyframe_ids) {
  CHECK(bins >= 1 && bins <= 64) << "ComputeKeyframeRedundancy: bins outside 1 .. 64";
  BindScene(stream);
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const size_t K = bound_ids_.size();
  hist->assign(K * (size_t)bins, 0u);
  if (keyframe_ids) keyframe_ids->assign(bound_ids_.begin(), bound_ids_.end());
  if (K == 0) return;
  CUDABuffer<uint32_t> words(1, (int)(K * (size_t)bins));
  uint32_t* dev = words.ToCUDA().address();
  BAHIP_CHECKED_CALL(bahip_keyframe_observer_histogram(ctx_, &s, bins, dev, bins));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, hist->data(), dev, sizeof(uint32_t) * K * (size_t)bins, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::FindRedundantKeyframes(hipStream_t stream, int min_other_observers, double min_fraction, vector<int>* keyframe_ids, int bins) {
  CHECK(min_other_observers >= 0 && min_other_observers <= bins - 1) << "FindRedundantKeyframes: min_other_observers outside 0 .. bins - 1";
  vector<uint32_t> hist;
  vector<int> ids;
  ComputeKeyframeRedundancy(stream, bins, &hist, &ids);
  struct Row {
    int id;
    uint64_t covered, total;
  };
  vector<Row> rows;
  for (size_t i = 0; i < ids.size(); ++i) {
    uint64_t total = 0, covered = 0;
    for (int j = 0; j < bins; ++j) {
      total += hist[i * (size_t)bins + j];
      if (j >= min_other_observers) covered += hist[i * (size_t)bins + j];
    }
    if (total > 0 && (double)covered >= min_fraction * (double)total) rows.push_back(Row{ids[i], covered, total});
  }
  // covered and total are below 2^32 each (a row's words count distinct surfels): the cross products are exact in 64 bits
  std::stable_sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
    const uint64_t ab = a.covered * b.total, ba = b.covered * a.total;
    return ab != ba ? ab > ba : a.id < b.id;
  });
  keyframe_ids->clear();
  for (const Row& r : rows) keyframe_ids->push_back(r.id);
}

void DirectBA::CullRedundantKeyframes(hipStream_t stream, int min_other_observers, double min_fraction, int max_deletions, int protect_newest,
                                      vector<int>* deleted_ids) {
  deleted_ids->clear();
  while ((int)deleted_ids->size() < max_deletions) {
    vector<int> candidates;
    FindRedundantKeyframes(stream, min_other_observers, min_fraction, &candidates);
    // (FindRedundantKeyframes bound the scene: bound_ids_ holds the existing keyframes in order)
    const int existing = (int)bound_ids_.size();
    int chosen = -1;
    for (int id : candidates) {
      const int position = (int)(std::find(bound_ids_.begin(), bound_ids_.end(), id) - bound_ids_.begin());
      if (position == 0 || position >= existing - std::max(0, protect_newest)) continue;
      chosen = id;
      break;
    }
    if (chosen < 0) break;
    DeleteKeyframe(chosen);
    deleted_ids->push_back(chosen);
  }
}

void DirectBA::RenderSurfels(hipStream_t stream, const PinholeCamera4f& view, const SE3f& global_T_frame, const RenderOptions& options,
                             RenderedView* out) {
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const bahip_camera cam = ToBahipCamera(view);
  CHECK_GE(cam.width, 1); CHECK_GE(cam.height, 1);
  const size_t n = (size_t)cam.width * (size_t)cam.height;
  float F[12];
  global_T_frame.inverse().matrix3x4(F);
  bahip_render_options o{};
  o.mode = options.disc ? BAHIP_RENDER_DISC : BAHIP_RENDER_POINT;
  o.max_radius_px = options.max_radius_px;
  o.cull_backfaces = options.cull_backfaces ? 1 : 0;
  o.radius_factor = options.radius_factor;
  o.min_depth = options.min_depth;
  o.max_depth = options.max_depth;
  o.index_base = options.index_base;
  // one device block for the four planes: depth, index, three words of normal and one of colour per pixel
  CUDABuffer<uint32_t> planes(1, (int)(6 * n));
  uint32_t* base = planes.ToCUDA().address();
  bahip_render_out dev{};
  dev.depth = reinterpret_cast<float*>(base);
  dev.index = base + n;
  dev.normal = reinterpret_cast<float*>(base + 2 * n);
  dev.color = reinterpret_cast<uint8_t*>(base + 5 * n);
  BAHIP_CHECKED_CALL(bahip_render_surfels(ctx_, &s, &cam, F, &o, &dev));
  out->width = cam.width; out->height = cam.height;
  out->depth.resize(n); out->index.resize(n); out->normal.resize(3 * n); out->color.resize(4 * n);
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->depth.data(), dev.depth, sizeof(float) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->index.data(), dev.index, sizeof(uint32_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->normal.data(), dev.normal, sizeof(float) * 3 * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->color.data(), dev.color, 4 * n, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::RenderKeyframeView(hipStream_t stream, int keyframe_index, const RenderOptions& options, RenderedView* out) {
  CHECK_GE(keyframe_index, 0); CHECK_LT(keyframe_index, (int)keyframes_.size());
  CHECK(keyframes_[keyframe_index] != nullptr);
  RenderSurfels(stream, depth_camera_, keyframes_[keyframe_index]->global_T_frame(), options, out);
}

void DirectBA::FrameResidualImage(hipStream_t stream, const Keyframe& frame, const SE3f& global_T_frame, const ResidualImageOptions& options,
                                  ResidualImage* out) {
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_camera cc = ToBahipCamera(color_camera_), dc = ToBahipCamera(depth_camera_);
  const bahip_depth_params dp = ToBahipDepthParams(depth_params_);
  BAHIP_CHECKED_CALL(bahip_set_intrinsics(ctx_, &cc, &dc, &dp));
  const bahip_surfels s = SurfelsStruct(/*with_active*/ false);
  const bahip_frame f = frame.ToBahipFrame();
  const size_t n = (size_t)dc.width * (size_t)dc.height;
  float F[12];
  global_T_frame.inverse().matrix3x4(F);
  bahip_residual_image_options o{};
  o.select = options.worst ? BAHIP_RESIDUAL_WORST : BAHIP_RESIDUAL_BEST;
  o.index_base = options.index_base;
  // one device block for the seven planes: two words of key, then pairs, index, the two depth planes, two words of descriptor
  // residuals and (a byte each, in the last quarter of a word's worth) color_valid per pixel
  CUDABuffer<uint32_t> planes(1, (int)(8 * n + (n + 3) / 4));
  uint32_t* base = planes.ToCUDA().address();
  bahip_residual_image_out dev{};
  dev.key = reinterpret_cast<uint64_t*>(base);
  dev.pairs = base + 2 * n;
  dev.index = base + 3 * n;
  dev.depth_residual = reinterpret_cast<float*>(base + 4 * n);
  dev.inv_stddev = reinterpret_cast<float*>(base + 5 * n);
  dev.desc_residual = reinterpret_cast<float*>(base + 6 * n);
  dev.color_valid = reinterpret_cast<uint8_t*>(base + 8 * n);
  BAHIP_CHECKED_CALL(bahip_frame_residual_image(ctx_, &f, F, &s, &o, &dev));
  out->width = dc.width; out->height = dc.height;
  out->key.resize(n); out->pairs.resize(n); out->index.resize(n); out->depth_residual.resize(n); out->inv_stddev.resize(n);
  out->desc_residual.resize(2 * n); out->color_valid.resize(n);
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->key.data(), dev.key, sizeof(uint64_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->pairs.data(), dev.pairs, sizeof(uint32_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->index.data(), dev.index, sizeof(uint32_t) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->depth_residual.data(), dev.depth_residual, sizeof(float) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->inv_stddev.data(), dev.inv_stddev, sizeof(float) * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->desc_residual.data(), dev.desc_residual, sizeof(float) * 2 * n, 2));
  BAHIP_CHECKED_CALL(bahip_memcpy_async(stream, out->color_valid.data(), dev.color_valid, n, 2));
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

void DirectBA::KeyframeResidualImage(hipStream_t stream, int keyframe_index, const ResidualImageOptions& options, ResidualImage* out) {
  CHECK_GE(keyframe_index, 0); CHECK_LT(keyframe_index, (int)keyframes_.size());
  CHECK(keyframes_[keyframe_index] != nullptr);
  FrameResidualImage(stream, *keyframes_[keyframe_index], keyframes_[keyframe_index]->global_T_frame(), options, out);
}

void DirectBA::BundleAdjustment(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics,
                                bool do_surfel_updates, bool optimize_poses, bool optimize_geometry, int min_iterations,
                                int max_iterations, bool use_pcg, int active_keyframe_window_start,
                                int active_keyframe_window_end, bool increase_ba_iteration_count, int* iterations_done,
                                bool* converged, double time_limit, Timer* timer, int pcg_max_inner_iterations,
                                int pcg_max_keyframes, std::function<bool(int)> progress_function) {
  if (optimize_depth_intrinsics && !use_depth_residuals_) {
    LOG(WARNING) << "optimize_depth_intrinsics set to true, but use_depth_residuals_ set to false. Depth intrinsics will not be optimized.";
    optimize_depth_intrinsics = false;
  }
  if (optimize_color_intrinsics && !use_descriptor_residuals_) {
    LOG(WARNING) << "optimize_color_intrinsics set to true, but use_descriptor_residuals_ set to false. Color intrinsics will not be optimized.";
    optimize_color_intrinsics = false;
  }
  last_pose_rounds_ = last_pose_steps_ = last_pcg_inner_steps_ = last_pcg_trials_ = last_pcg_rejected_steps_ = last_pose_trials_ = last_pose_rejected_steps_ = 0;
  last_geometry_candidates_ = last_geometry_accepted_ = last_geometry_restored_ = 0;
  last_geometry_trials_ = 0;
  last_intrinsics_trials_ = last_intrinsics_accepted_ = 0;
  last_intrinsics_lambda_ = -1.f;
  last_intrinsics_cost_drop_ = last_intrinsics_smallest_drop_ = 0;
  if (keyframe_shard_world_ > 1)
    CHECK(batched_creation_ || (!do_surfel_updates && !increase_ba_iteration_count))
        << "keyframe sharding runs the surfel lifecycle through the batched calls only (SetBatchedCreation(true))";
  if (use_pcg) {
    BundleAdjustmentPCG(stream, optimize_depth_intrinsics, optimize_color_intrinsics, do_surfel_updates, optimize_poses,
                        optimize_geometry, min_iterations, max_iterations, pcg_max_inner_iterations, pcg_max_keyframes,
                        active_keyframe_window_start, active_keyframe_window_end, increase_ba_iteration_count, iterations_done,
                        converged, time_limit, timer, progress_function);
  } else {
    BundleAdjustmentAlternating(stream, optimize_depth_intrinsics, optimize_color_intrinsics, do_surfel_updates, optimize_poses,
                                optimize_geometry, min_iterations, max_iterations, active_keyframe_window_start,
                                active_keyframe_window_end, increase_ba_iteration_count, iterations_done, converged, time_limit,
                                timer, progress_function);
  }
}

// ---- end-of-scheme tasks (B/direct_ba.cc:566-653) -----------------------------------------------------------------------
void DirectBA::PerformBASchemeEndTasks(hipStream_t stream, bool do_surfel_updates) {
  WholeCloudScope whole_cloud(this, stream);
  BindScene(stream);
  if (do_surfel_updates) {
    vector<u32> active_this_call;
    for (shared_ptr<Keyframe>& keyframe : keyframes_)
      if (keyframe && keyframe->last_active_in_ba_iteration() == ba_iteration_count_) active_this_call.push_back(keyframe->id());
    MergeForKeyframes(active_this_call);
  }
  const bahip_surfels s = SurfelsStruct();
  uint32_t deleted = 0;
  BAHIP_CHECKED_CALL(bahip_delete_surfels_and_update_radii(ctx_, GetMinObservationCount(), &s, &deleted));
  u32 surfel_count = surfel_count_ - deleted;
  const bahip_surfels s2 = SurfelsStruct(/*with_active*/ false);   // B/direct_ba.cc:619: no active-flag buffer
  unsorted_surfels_ += surfels_size_ - surfel_count;               // the holes compaction fills with surfels from the end
  BAHIP_CHECKED_CALL(bahip_compact_surfels(ctx_, surfel_count, &s2));
  Lock();
  surfels_size_ = surfel_count;
  surfel_count_ = surfel_count;
  Unlock();
  // Ours: back into Morton order if anything was appended or moved since the last reorder (direct_ba.h: SetSpatialSortCellSize;
  // the oracle's end tasks do the same, oracle_ba.c).  Under surfel sharding this runs on the gathered cloud, on every rank alike.
  if (spatial_sort_cell_size_ > 0.f) {
    if (unsorted_surfels_ > 0 && surfels_size_ > 1) SortSurfelsSpatially(stream, spatial_sort_cell_size_);
    unsorted_surfels_ = 0;
  }
}

// Ours: the compaction inside the loop fills the holes of merged surfels with surfels from the END of the buffer (the reference's rule,
// B/kernel_compact_surfels.cu:101-157) -- after a creation + merge pass over many keyframes nearly every 64-surfel tile of the Morton-
// ordered part then holds a surfel from somewhere else, its bounding sphere covers half the scene, and the sweeps of the call's remaining
// iterations cull nothing (measured: geometry 1.0 ms instead of 0.47 at 2.2 M surfels, profiles/r6_drop_in_trace_by_kernel.csv).  So once
// the surfels out of order amount to one per tile, the buffer goes back into Morton order here instead of at the end tasks only
// (same switch: SetSpatialSortCellSize(0) leaves the reference's order alone; the oracle's loop applies the same rule, oracle_ba.c).
void DirectBA::SortAfterInLoopCompaction(hipStream_t stream) {
  if (spatial_sort_cell_size_ > 0.f && surfels_size_ > 1 && (uint64_t)unsorted_surfels_ * 64 >= (uint64_t)surfels_size_)
    SortSurfelsSpatially(stream, spatial_sort_cell_size_);
}

void DirectBA::SortSurfelsSpatially(hipStream_t stream, float grid_cell_size) {
  BAHIP_CHECKED_CALL(bahip_context_set_stream(ctx_, stream));
  const bahip_surfels s = SurfelsStruct();
  BAHIP_CHECKED_CALL(bahip_sort_surfels_spatially(ctx_, &s, grid_cell_size));
  unsorted_surfels_ = 0;
}

// ---- alternating scheme (B/direct_ba_alternating.cc:285-738) ----------------------------------------------------------------
void DirectBA::BundleAdjustmentAlternating(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics,
                                           bool do_surfel_updates, bool optimize_poses, bool optimize_geometry, int min_iterations,
                                           int max_iterations, int active_keyframe_window_start, int active_keyframe_window_end,
                                           bool increase_ba_iteration_count, int* num_iterations_done, bool* converged,
                                           double time_limit, Timer* timer, std::function<bool(int)> progress_function) {
  if (converged) *converged = false;
  if (num_iterations_done) *num_iterations_done = 0;
  Lock();
  const int fixed_ba_iteration_count = ba_iteration_count_;
  Unlock();
  if (!increase_ba_iteration_count && fixed_ba_iteration_count != last_ba_iteration_count_) {
    last_ba_iteration_count_ = fixed_ba_iteration_count;
    PerformBASchemeEndTasks(stream, do_surfel_updates);
  }
  vector<u32> keyframes_with_new_surfels;
  const bool fixed_active_keyframe_set = active_keyframe_window_start > 0 || active_keyframe_window_end > 0;
  const bool full_window = active_keyframe_window_start == 0 && active_keyframe_window_end == (int)keyframes_.size() - 1;
  if (!full_window)
    LOG(WARNING) << "Currently, only using all keyframes in every optimization iteration will work properly.";
  BAHIP_CHECKED_CALL(bahip_memset_async(stream, active_surfels_->ToCUDA().address(), 0, surfels_size_));

  // During the loop the device keyframe table is authoritative: the pose phase updates poses AND activations there
  // (bahip_estimate_keyframe_poses_and_update_activation, bahip_propagate_covisible_activation), so the next iteration's sweeps
  // can be queued at once, and the results are copied into the Keyframe objects ("pending") while the GPU already works on
  // them.  Anything that reads the Keyframe objects applies the pending results first.
  // Deferred host bookkeeping: operations on the Keyframe objects that mirror what the device table already went through,
  // run in order under the lock.
  vector<std::function<void()>> pending;
  auto apply_pending = [&]() {
    if (pending.empty()) return;
    Lock();
    for (auto& op : pending) op();
    Unlock();
    pending.clear();
  };
  auto set_window_activation = [this, active_keyframe_window_start, active_keyframe_window_end]() {
    for (u32 i = 0; i < keyframes_.size(); ++i) {
      if (!keyframes_[i]) continue;
      keyframes_[i]->SetActivation(((int)i >= active_keyframe_window_start && (int)i <= active_keyframe_window_end)
                                       ? Keyframe::Activation::kActive : Keyframe::Activation::kInactive);
    }
    DetermineCovisibleActiveKeyframes();
  };
  bool scene_bound = false;   // does the backend context hold the current keyframes / poses / activations / intrinsics?
  // BADSLAM_HOST_TIMING=1: wall time the host spends in each part of an iteration (printed once per call; diagnostics)
  const bool host_timing = getenv("BADSLAM_HOST_TIMING") != nullptr;
  double t_phase[6] = {0, 0, 0, 0, 0, 0};
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = now();
  auto lap = [&](int phase) { if (host_timing) { const double t = now(); t_phase[phase] += t - t_mark; t_mark = t; } };

  // ---- the loop driven by the device (bahip_alternating_iterations): poses + geometry over a fixed surfel set, nothing the
  // host has to look at between the iterations.  All iterations are queued at once; the stopping rule of :693-701 is evaluated
  // by the last solve launch of every pose phase, and the host waits once.  Everything else takes the loop below.
  bool device_loop_done = false;
  if (host_timing)
    fprintf(stderr, "[DirectBA] loop conditions: poses %d geometry %d updates %d intr %d/%d progress %d timer %d timings %d kfworld %d full_window %d max_it %d\n",
            (int)optimize_poses, (int)optimize_geometry, (int)do_surfel_updates, (int)optimize_depth_intrinsics, (int)optimize_color_intrinsics,
            progress_function ? 1 : 0, timer ? 1 : 0, timings_stream_ ? 1 : 0, keyframe_shard_world_, (int)full_window, max_iterations);
  if (optimize_poses && optimize_geometry && !do_surfel_updates && !optimize_depth_intrinsics && !optimize_color_intrinsics &&
      !progress_function && !timer && !timings_stream_ && keyframe_shard_world_ == 1 && full_window && max_iterations > 0 &&
      !pose_step_control_on_ /* the controlled pose phase is a stage call: the iterations go through the loop below */ &&
      !geometry_step_control_on_ /* ... and so is the controlled geometry phase */) {
    if (fixed_active_keyframe_set) {
      Lock();
      set_window_activation();
      Unlock();
    }
    BindScene(stream);
    if (fixed_active_keyframe_set) {
      vector<uint8_t> in_window(bound_ids_.size());
      for (usize b = 0; b < bound_ids_.size(); ++b)
        in_window[b] = (bound_ids_[b] >= active_keyframe_window_start && bound_ids_[b] <= active_keyframe_window_end) ? 1 : 0;
      BAHIP_CHECKED_CALL(bahip_set_activation_window(ctx_, in_window.data(), (int)in_window.size()));
    }
    const int K = (int)bound_ids_.size();
    vector<float> poses(7 * (size_t)std::max(K, 1));
    vector<int> activation(std::max(K, 1));
    bahip_alternating_options options;
    options.use_depth_residuals = use_depth_residuals_; options.use_descriptor_residuals = use_descriptor_residuals_;
    options.fixed_window = fixed_active_keyframe_set ? 1 : 0;
    options.activate_in_geometry = 1;                        // full window: UpdateSurfelActivation inside the geometry sweep
    options.activation_surfels_size = surfels_size_;
    options.min_iterations = min_iterations; options.max_iterations = max_iterations;
    const bahip_surfels s = SurfelsStruct();
    int handled = 0, done = 0, conv = 0, rounds = 0, steps = 0, not_converged = 0;
    const double t_before_loop = host_timing ? now() : 0;
    BAHIP_CHECKED_CALL(bahip_alternating_iterations(ctx_, &options, &s, poses.data(), activation.data(), &handled, &done, &conv, &rounds, &steps,
                                                    &not_converged));
    const double t_after_loop = host_timing ? now() : 0;
    if (host_timing) fprintf(stderr, "[DirectBA] device loop %s\n", handled ? "handled the call" : "declined");
    if (handled) {
      device_loop_done = true;
      Lock();
      for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
        if (!keyframe) continue;
        const int b = id_to_bound_[keyframe->id()];
        // Only a keyframe whose pose the loop changed gets it written back: a keyframe that stayed kInactive (or converged without
        // moving a bit) keeps the SE3f object it has -- set_global_T_frame rebuilds frame_T_global as the inverse, which is not
        // bit for bit what a caller may have set through set_frame_T_global (the host loop and the reference touch only the
        // keyframes that took a Gauss-Newton step).
        if (memcmp(keyframe->global_T_frame().data(), &poses[7 * (size_t)b], 7 * sizeof(float)) != 0)
          keyframe->set_global_T_frame(SE3f(&poses[7 * (size_t)b]));
        keyframe->SetActivation(static_cast<Keyframe::Activation>(activation[b]));
      }
      // the device table is in the state after the last pose phase; an iteration that did not end the loop is followed by
      // DetermineCovisibleActiveKeyframes (:703-709)
      if (!conv) DetermineCovisibleActiveKeyframes();
      Unlock();
      if (num_iterations_done) *num_iterations_done = done;
      if (converged) *converged = conv != 0;
      last_pose_rounds_ += rounds;
      last_pose_steps_ += steps;
      if (not_converged) LOG(WARNING) << "Pose estimation not converged (" << not_converged << " estimations)";
    }
    if (host_timing)
      fprintf(stderr, "[DirectBA, us] bind + window %.0f | bahip_alternating_iterations %.0f | write-back %.0f\n", t_before_loop - t_mark,
              t_after_loop - t_before_loop, now() - t_after_loop);
  }

  bool have_intrinsics_cost = false;   // intrinsics step control: the objective after the previous controlled step of this call
  bahip_cost intrinsics_cost{};
  for (int iteration = 0; iteration < max_iterations && !device_loop_done; ++iteration) {
    if (progress_function) {
      apply_pending();   // the callback may look at the keyframes
      if (!progress_function(iteration)) break;
    }
    if (num_iterations_done) ++*num_iterations_done;
    if (fixed_active_keyframe_set) {
      if (scene_bound) {
        // the device table takes the window activation itself; the Keyframe objects follow when the pending work is applied
        BAHIP_CHECKED_CALL(bahip_apply_activation_window(ctx_));
        pending.push_back(set_window_activation);
      } else {
        apply_pending();
        Lock();
        set_window_activation();
        Unlock();
      }
    }

    // --- surfel creation ---
    keyframes_with_new_surfels.clear();
    CHECK_EQ(surfels_size_, surfel_count_);
    const usize old_surfels_size = surfels_size_;
    if (optimize_geometry && do_surfel_updates) {
      apply_pending();
      Lock();
      for (shared_ptr<Keyframe>& keyframe : keyframes_) {
        if (!keyframe) continue;
        if (keyframe->activation() == Keyframe::Activation::kActive && keyframe->last_active_in_ba_iteration() != fixed_ba_iteration_count) {
          keyframe->SetLastActiveInBAIteration(fixed_ba_iteration_count);
          keyframes_with_new_surfels.push_back(keyframe->id());
        } else if (keyframe->activation() == Keyframe::Activation::kCovisibleActive &&
                   keyframe->last_covis_in_ba_iteration() != fixed_ba_iteration_count) {
          keyframe->SetLastCovisInBAIteration(fixed_ba_iteration_count);
        }
      }
      Unlock();
      if (!keyframes_with_new_surfels.empty()) {
        WholeCloudScope whole_cloud(this, stream);   // one gather for the whole batch
        apply_pending();
        BindScene(stream);                           // ... and one binding
        creation_batch_bound_ = true;
        LifecycleBatch batch(this);
        CreateSurfelsForKeyframes(stream, /*filter_new_surfels*/ true, keyframes_with_new_surfels);
        creation_batch_bound_ = false;
      }
      if (!keyframes_with_new_surfels.empty()) scene_bound = false;   // CreateSurfelsForKeyframe re-bound the keyframes: lists and window go again
    }

    lap(0);
    if (!scene_bound) {
      apply_pending();
      BindScene(stream);
      if (fixed_active_keyframe_set) {
        vector<uint8_t> in_window(bound_ids_.size());
        for (usize b = 0; b < bound_ids_.size(); ++b)
          in_window[b] = (bound_ids_[b] >= active_keyframe_window_start && bound_ids_[b] <= active_keyframe_window_end) ? 1 : 0;
        BAHIP_CHECKED_CALL(bahip_set_activation_window(ctx_, in_window.data(), (int)in_window.size()));
      }
      scene_bound = true;
    }
    lap(1);

    // --- surfel activation + geometry ---
    if (optimize_geometry && surfels_size_ > old_surfels_size)
      BAHIP_CHECKED_CALL(bahip_memset_async(stream, active_surfels_->ToCUDA().address() + old_surfels_size, 1, surfels_size_ - old_surfels_size));
    if (!full_window) {
      BAHIP_CHECKED_CALL(bahip_memset_async(stream, active_surfels_->ToCUDA().address(), 1, old_surfels_size));
    } else if (!optimize_geometry) {
      const bahip_surfels s = SurfelsStruct();
      BAHIP_CHECKED_CALL(bahip_update_surfel_activation(ctx_, &s, (uint32_t)old_surfels_size));
    }
    if (optimize_geometry) {
      const bahip_surfels s = SurfelsStruct();
      if (geometry_step_control_on_) {
        // the same two calls under step control: per surfel a damped step that is kept only if the surfel's cost falls
        const bahip_geometry_step_control control{geometry_step_control_.lambda_initial, geometry_step_control_.lambda_up,
                                                  geometry_step_control_.lambda_min, geometry_step_control_.lambda_max,
                                                  geometry_step_control_.max_trials, geometry_step_control_.guard_pairs ? 1 : 0};
        bahip_geometry_step_stats stats{};
        BAHIP_CHECKED_CALL(bahip_optimize_geometry_iteration_controlled(ctx_, use_depth_residuals_, use_descriptor_residuals_, &control, &s,
                                                                        full_window ? (long long)old_surfels_size : -1, nullptr, &stats));
        last_geometry_candidates_ += stats.candidates;
        last_geometry_accepted_ += stats.accepted;
        last_geometry_restored_ += stats.restored;
        last_geometry_trials_ += stats.trials;
      } else if (full_window) {
        // UpdateSurfelActivationCUDA + OptimizeGeometryIterationCUDA (B/direct_ba_alternating.cc:441-487) as one sweep
        BAHIP_CHECKED_CALL(bahip_update_activation_and_optimize_geometry(ctx_, use_depth_residuals_, use_descriptor_residuals_, &s,
                                                                         (uint32_t)old_surfels_size));
      } else {
        BAHIP_CHECKED_CALL(bahip_optimize_geometry_iteration(ctx_, use_depth_residuals_, use_descriptor_residuals_, &s));
      }
    }
    lap(2);
    // the previous iteration's pose results go into the Keyframe objects while the GPU runs the sweep queued above
    apply_pending();
    lap(3);

    // --- surfel merge + compaction ---
    if (do_surfel_updates && !keyframes_with_new_surfels.empty()) {
      WholeCloudScope whole_cloud(this, stream);
      MergeForKeyframes(keyframes_with_new_surfels);
      {
        const bahip_surfels s = SurfelsStruct();
        unsorted_surfels_ += surfels_size_ - surfel_count_;
        BAHIP_CHECKED_CALL(bahip_compact_surfels(ctx_, surfel_count_, &s));
        Lock();
        surfels_size_ = surfel_count_;
        Unlock();
      }
      SortAfterInLoopCompaction(stream);
    }

    // --- poses: every non-inactive keyframe, batched per Gauss-Newton round; activations updated on the device ---
    usize num_converged = 0;
    if (optimize_poses) {
      const int K = (int)bound_ids_.size();
      auto poses = std::make_shared<vector<float>>(7 * (size_t)K, 0.f);
      auto moved = std::make_shared<vector<int>>(K, 0);
      vector<int> its(K), conv(K);
      int rounds = 0, converged_bound = 0;
      const bahip_surfels s = SurfelsStruct();
      if (pose_step_control_on_) {
        // per keyframe id: the damping factor its last pose phase left (a new keyframe: lambda_initial)
        const bahip_pose_step_control control{pose_step_control_.lambda_up, pose_step_control_.lambda_down, pose_step_control_.lambda_min,
                                              pose_step_control_.lambda_max, pose_step_control_.max_trials};
        vector<float> lambdas(std::max(K, 1));
        vector<int> trials(std::max(K, 1)), rejected(std::max(K, 1));
        for (int b = 0; b < K; ++b) lambdas[b] = pose_lambda(bound_ids_[b]);
        BAHIP_CHECKED_CALL(bahip_estimate_keyframe_poses_controlled(ctx_, use_depth_residuals_, use_descriptor_residuals_, &control, &s, /*update_activation*/ 1,
                                                                    lambdas.data(), poses->data(), its.data(), conv.data(), moved->data(), trials.data(),
                                                                    rejected.data(), nullptr, nullptr, &rounds, &converged_bound));
        for (int b = 0; b < K; ++b) {
          pose_lambdas_[bound_ids_[b]] = lambdas[b];
          last_pose_trials_ += trials[b];
          last_pose_rejected_steps_ += rejected[b];
        }
      } else {
        BAHIP_CHECKED_CALL(bahip_estimate_keyframe_poses_and_update_activation(ctx_, use_depth_residuals_, use_descriptor_residuals_, &s,
                                                                               poses->data(), its.data(), conv.data(), moved->data(),
                                                                               &rounds, &converged_bound));
      }
      pending.push_back([this, poses, moved]() {
        for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
          if (!keyframe || keyframe->activation() == Keyframe::Activation::kInactive) continue;
          const int b = id_to_bound_[keyframe->id()];
          keyframe->set_global_T_frame(SE3f(&(*poses)[7 * (size_t)b]));
          keyframe->SetActivation((*moved)[b] ? Keyframe::Activation::kActive : Keyframe::Activation::kInactive);
        }
      });
      lap(4);
      last_pose_rounds_ += rounds;
      num_converged = (usize)converged_bound + (keyframes_.size() - (usize)K);   // deleted keyframes count as converged
      for (const shared_ptr<Keyframe>& keyframe : keyframes_) {
        if (!keyframe || keyframe->activation() == Keyframe::Activation::kInactive) continue;
        const int b = id_to_bound_[keyframe->id()];
        last_pose_steps_ += its[b];
        if (!conv[b]) LOG(WARNING) << "Pose estimation not converged (keyframe " << keyframe->id() << ")";
      }
    }

    // --- intrinsics ---
    if ((optimize_depth_intrinsics || optimize_color_intrinsics) && intrinsics_step_control_on_) {
      // the same step under step control: damped trials, the first that lowers the objective is kept (the backend context then holds
      // the new cameras / depth parameters already), otherwise nothing changes
      const bahip_intrinsics_step_control control{intrinsics_step_control_.lambda_first, intrinsics_step_control_.lambda_up,
                                                  intrinsics_step_control_.lambda_max, intrinsics_step_control_.max_trials};
      bahip_camera out_color, out_depth;
      float out_a = depth_params_.a, lambda_accepted = 0.f;
      int trials = 0, accepted = 0;
      // the previous controlled step's cost_after is this step's cost_before only if nothing touched the state in between
      const bool reuse_cost = have_intrinsics_cost && !optimize_poses && !optimize_geometry && !do_surfel_updates;
      bahip_cost cost_before = intrinsics_cost, cost_after{};
      const bahip_surfels s = SurfelsStruct();
      BAHIP_CHECKED_CALL(bahip_optimize_intrinsics_controlled(ctx_, optimize_depth_intrinsics, optimize_color_intrinsics, use_depth_residuals_,
                                                              use_descriptor_residuals_, &control, &s, &intrinsics_lambda_, &out_color, &out_depth,
                                                              &out_a, reuse_cost ? 1 : 0, &cost_before, &cost_after, &trials, &accepted,
                                                              &lambda_accepted));
      intrinsics_cost = cost_after;
      have_intrinsics_cost = true;
      last_intrinsics_trials_ += trials;
      if (accepted) {
        const double drop = ((cost_before.depth + cost_before.descriptor_1) + cost_before.descriptor_2) -
                            ((cost_after.depth + cost_after.descriptor_1) + cost_after.descriptor_2);
        last_intrinsics_smallest_drop_ = last_intrinsics_accepted_ ? std::min(last_intrinsics_smallest_drop_, drop) : drop;
        last_intrinsics_cost_drop_ += drop;
        ++last_intrinsics_accepted_;
        last_intrinsics_lambda_ = lambda_accepted;
        Lock();
        if (optimize_color_intrinsics) color_camera_ = PinholeCamera4f(out_color.width, out_color.height, &out_color.fx);
        if (optimize_depth_intrinsics) {
          depth_camera_ = PinholeCamera4f(out_depth.width, out_depth.height, &out_depth.fx);
          depth_params_.a = out_a;
        }
        Unlock();
        if (intrinsics_updated_callback_) { apply_pending(); intrinsics_updated_callback_(); }
      }
    } else if (optimize_depth_intrinsics || optimize_color_intrinsics) {
      bahip_camera out_color, out_depth;
      float out_a = depth_params_.a;
      const bahip_surfels s = SurfelsStruct();
      BAHIP_CHECKED_CALL(bahip_optimize_intrinsics(ctx_, optimize_depth_intrinsics, optimize_color_intrinsics, &s, &out_color, &out_depth, &out_a));
      // under surfel sharding every rank takes the globally solved cameras, also one whose own shard is empty (else the ranks
      // would bind different intrinsics from here on and disagree on convergence tests, i.e. on the number of collectives)
      if (surfels_size_ > 0 || bahip_context_is_sharded(ctx_)) {
        Lock();
        if (optimize_color_intrinsics) color_camera_ = PinholeCamera4f(out_color.width, out_color.height, &out_color.fx);
        if (optimize_depth_intrinsics) {
          depth_camera_ = PinholeCamera4f(out_depth.width, out_depth.height, &out_depth.fx);
          depth_params_.a = out_a;
        }
        Unlock();
        // the backend context takes over the new cameras / depth parameters (the keyframe table is unaffected)
        const bahip_camera cc = ToBahipCamera(color_camera_), dc = ToBahipCamera(depth_camera_);
        const bahip_depth_params dp = ToBahipDepthParams(depth_params_);
        BAHIP_CHECKED_CALL(bahip_set_intrinsics(ctx_, &cc, &dc, &dp));
      }
      if (intrinsics_updated_callback_) { apply_pending(); intrinsics_updated_callback_(); }
    }

    if (timings_stream_) {
      *timings_stream_ << "BA_count " << fixed_ba_iteration_count << " inner_iteration " << iteration << " keyframe_count "
                       << keyframes_.size() << " surfel_count " << surfel_count_ << std::endl;
      static const char* keys[4] = {"BA_surfel_activation", "BA_geometry_optimization", "BA_pose_optimization", nullptr};
      for (int stage = 0; stage < 3; ++stage) {
        float ms = 0; int launches = 0;
        if (bahip_last_stage_time_ms(ctx_, stage, &ms, &launches) == 0 && launches > 0) *timings_stream_ << keys[stage] << " " << ms << std::endl;
      }
    }

    // --- convergence ---
    if (iteration >= min_iterations - 1 && (num_converged == keyframes_.size() || !optimize_poses)) {
      if (converged) *converged = true;
      break;
    }
    if (timer && timer->GetTimeSinceStart() > time_limit) break;
    // DetermineCovisibleActiveKeyframes: on the device table now, on the Keyframe objects when the pending results are applied
    // (with a fixed window the next iteration overwrites every activation on the device first thing, so only the Keyframe objects
    // need this step there)
    if (!fixed_active_keyframe_set) BAHIP_CHECKED_CALL(bahip_propagate_covisible_activation(ctx_));
    pending.push_back([this]() { DetermineCovisibleActiveKeyframes(); });
  }
  apply_pending();
  lap(5);
  if (host_timing)
    fprintf(stderr, "[DirectBA host timing, us] loop top %.0f | bind %.0f | geometry launch %.0f | apply pending %.0f | pose phase %.0f | rest %.0f\n",
            t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4], t_phase[5]);

  if (increase_ba_iteration_count) {
    PerformBASchemeEndTasks(stream, do_surfel_updates);
    ++ba_iteration_count_;
  }
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

// ---- PCG scheme (B/direct_ba_pcg.cc:43-819) -----------------------------------------------------------------------------------
void DirectBA::BundleAdjustmentPCG(hipStream_t stream, bool optimize_depth_intrinsics, bool optimize_color_intrinsics,
                                   bool do_surfel_updates, bool optimize_poses, bool optimize_geometry, int min_iterations,
                                   int max_iterations, int max_inner_iterations, int max_keyframe_count,
                                   int active_keyframe_window_start, int active_keyframe_window_end, bool increase_ba_iteration_count,
                                   int* num_iterations_done, bool* converged, double time_limit, Timer* timer,
                                   std::function<bool(int)> progress_function) {
  // SetWindowedPCG(false): the reference's refusals (B/direct_ba_pcg.cc:125,140).  SetWindowedPCG(true): deleted keyframes are left
  // out, and a fixed window that excludes a living keyframe runs bahip_pcg_iteration_windowed over it.
  const bool windowed = windowed_pcg_;
  if (!windowed && (active_keyframe_window_start != -1 || active_keyframe_window_end != -1) &&
      (active_keyframe_window_start != 0 || active_keyframe_window_end != (int)keyframes_.size() - 1))
    LOG(WARNING) << "The PCG-based solver implementation does not support an active window! These parameters will be ignored.";
  if (num_iterations_done) *num_iterations_done = 0;
  if (converged) *converged = false;
  int living = 0;
  bool window_excludes = false;   // does the fixed window leave out a living keyframe?
  const bool fixed_active_keyframe_set = active_keyframe_window_start > 0 || active_keyframe_window_end > 0;
  for (auto& keyframe : keyframes_) {
    if (!keyframe) {
      if (windowed) continue;
      LOG(ERROR) << "The PCG-based solver implementation does not support having deleted keyframes yet! Aborting.";
      return;
    }
    ++living;
    const int id = (int)keyframe->id();
    if (id < active_keyframe_window_start || id > active_keyframe_window_end) window_excludes = true;
  }
  const bool use_window = windowed && fixed_active_keyframe_set && window_excludes;
  CHECK_LE(living, max_keyframe_count);
  auto set_window_activation = [this, active_keyframe_window_start, active_keyframe_window_end]() {   // as in the alternating scheme
    for (u32 i = 0; i < keyframes_.size(); ++i) {
      if (!keyframes_[i]) continue;
      keyframes_[i]->SetActivation(((int)i >= active_keyframe_window_start && (int)i <= active_keyframe_window_end)
                                       ? Keyframe::Activation::kActive : Keyframe::Activation::kInactive);
    }
    DetermineCovisibleActiveKeyframes();
  };
  if (!increase_ba_iteration_count && ba_iteration_count_ != last_ba_iteration_count_) {
    last_ba_iteration_count_ = ba_iteration_count_;
    PerformBASchemeEndTasks(stream, do_surfel_updates);
  }
  vector<u32> keyframes_with_new_surfels;
  auto merge_and_compact = [&]() {
    if (keyframes_with_new_surfels.empty()) return;
    WholeCloudScope whole_cloud(this, stream);
    MergeForKeyframes(keyframes_with_new_surfels);
    if (!keyframes_with_new_surfels.empty()) {
      const bahip_surfels s = SurfelsStruct();
      unsorted_surfels_ += surfels_size_ - surfel_count_;
      BAHIP_CHECKED_CALL(bahip_compact_surfels(ctx_, surfel_count_, &s));
      surfels_size_ = surfel_count_;
      SortAfterInLoopCompaction(stream);
    }
  };

  bahip_cost carried_cost{};   // step control: the cost the previous outer iteration of this call left
  bool have_carried_cost = false;
  for (int iteration = 0; iteration < max_iterations; ++iteration) {
    if (progress_function && !progress_function(iteration)) break;
    if (num_iterations_done) ++*num_iterations_done;
    keyframes_with_new_surfels.clear();
    if (use_window) {
      Lock();
      set_window_activation();
      Unlock();
    }
    if (optimize_geometry && do_surfel_updates) {
      bool any_new = false;
      for (const shared_ptr<Keyframe>& keyframe : keyframes_)
        any_new |= keyframe && keyframe->activation() == Keyframe::Activation::kActive && keyframe->last_active_in_ba_iteration() != ba_iteration_count_;
      std::unique_ptr<WholeCloudScope> whole_cloud(any_new ? new WholeCloudScope(this, stream) : nullptr);   // one gather for the batch
      if (any_new) BindScene(stream);                                                                          // ... and one binding
      creation_batch_bound_ = any_new;
      std::unique_ptr<LifecycleBatch> batch(any_new ? new LifecycleBatch(this) : nullptr);
      for (shared_ptr<Keyframe>& keyframe : keyframes_) {
        if (!keyframe) continue;
        if (keyframe->activation() == Keyframe::Activation::kActive && keyframe->last_active_in_ba_iteration() != ba_iteration_count_) {
          keyframe->SetLastActiveInBAIteration(ba_iteration_count_);
          keyframes_with_new_surfels.push_back(keyframe->id());
        } else if (keyframe->activation() == Keyframe::Activation::kCovisibleActive &&
                   keyframe->last_covis_in_ba_iteration() != ba_iteration_count_) {
          keyframe->SetLastCovisInBAIteration(ba_iteration_count_);
        }
      }
      CreateSurfelsForKeyframes(stream, /*filter_new_surfels*/ true, keyframes_with_new_surfels);   // in keyframe order, as the loop above met them
      creation_batch_bound_ = false;
    }
    BindScene(stream);
    if (use_window) {
      // the window on the device table (BindScene took the Keyframe objects' activations; this re-derives them there), and the surfels
      // the kActive keyframes see
      vector<uint8_t> in_window(bound_ids_.size());
      for (usize b = 0; b < bound_ids_.size(); ++b)
        in_window[b] = (bound_ids_[b] >= active_keyframe_window_start && bound_ids_[b] <= active_keyframe_window_end) ? 1 : 0;
      BAHIP_CHECKED_CALL(bahip_set_activation_window(ctx_, in_window.data(), (int)in_window.size()));
      BAHIP_CHECKED_CALL(bahip_apply_activation_window(ctx_));
      const bahip_surfels s = SurfelsStruct();
      BAHIP_CHECKED_CALL(bahip_update_surfel_activation(ctx_, &s, (uint32_t)surfels_size_));
    } else {
      BAHIP_CHECKED_CALL(bahip_memset_async(stream, active_surfels_->ToCUDA().address(), 1, surfels_size_));
    }
    const bool controlled = pcg_step_control_on_;
    if (optimize_geometry && !controlled) {   // (under step control the normals update runs inside the trial and is undone with it)
      const bahip_surfels s = SurfelsStruct();
      BAHIP_CHECKED_CALL(bahip_update_surfel_normals(ctx_, &s));
    }

    bahip_pcg_options opt;
    opt.optimize_poses = optimize_poses; opt.optimize_geometry = optimize_geometry;
    opt.optimize_depth_intrinsics = optimize_depth_intrinsics; opt.optimize_color_intrinsics = optimize_color_intrinsics;
    opt.use_depth_residuals = use_depth_residuals_; opt.use_descriptor_residuals = use_descriptor_residuals_;
    opt.max_inner_iterations = max_inner_iterations;
    // B/direct_ba_pcg.cc:328 draws rand() % K; under keyframe sharding every rank must hold the same gauge, and a rand() stream is
    // neither shared by the instances of one process nor by those of several: there the default is keyframe 0
    // (a keyframe id; the gauge is a bound index: the same number while no keyframe is deleted, and rand() % living keyframes then
    // draws what rand() % K does)
    opt.gauge_keyframe = (pcg_gauge_keyframe_ >= 0) ? pcg_gauge_keyframe_ : keyframe_shard_world_ > 1 ? 0 : (rand() % living);
    if (windowed && pcg_gauge_keyframe_ >= 0)
      opt.gauge_keyframe = pcg_gauge_keyframe_ < (int)id_to_bound_.size() ? id_to_bound_[pcg_gauge_keyframe_] : -1;
    bahip_camera out_color, out_depth;
    float out_a = depth_params_.a;
    int inner_steps = 0, num_converged = 0;
    const bahip_surfels s = SurfelsStruct();
    bool step_accepted = true;
    if (controlled) {
      const bahip_pcg_step_control control{pcg_step_control_.lambda_initial, pcg_step_control_.lambda_up, pcg_step_control_.lambda_down,
                                           pcg_step_control_.lambda_min, pcg_step_control_.lambda_max, pcg_step_control_.max_trials};
      bahip_cost cost_before = carried_cost, cost_after;
      int trials = 0, accepted = 0;
      // (the previous outer iteration's cost_after is this one's cost_before unless something changed the state in between: surfel
      // creation and merging do)
      BAHIP_CHECKED_CALL(bahip_pcg_iteration_controlled(ctx_, &opt, &control, use_window ? 1 : 0, optimize_geometry ? 1 : 0, &s, &pcg_lambda_,
                                                        &out_color, &out_depth, &out_a, &inner_steps, &num_converged,
                                                        (have_carried_cost && !do_surfel_updates) ? 1 : 0, &cost_before, &cost_after, &trials,
                                                        &accepted));
      carried_cost = cost_after;
      have_carried_cost = true;
      last_pcg_trials_ += trials;
      last_pcg_rejected_steps_ += trials - accepted;
      step_accepted = accepted != 0;
    } else if (use_window) {
      BAHIP_CHECKED_CALL(bahip_pcg_iteration_windowed(ctx_, &opt, &s, &out_color, &out_depth, &out_a, &inner_steps, &num_converged));
    } else {
      BAHIP_CHECKED_CALL(bahip_pcg_iteration(ctx_, &opt, &s, &out_color, &out_depth, &out_a, &inner_steps, &num_converged));
    }
    last_pcg_inner_steps_ += inner_steps;
    num_converged += (int)keyframes_.size() - (int)bound_ids_.size();   // deleted keyframes count as converged
    if (!step_accepted) num_converged = (int)keyframes_.size();         // no step lowers the cost: converged for the stopping rule
    if (optimize_poses) {
      const int K = (int)bound_ids_.size();
      vector<float> poses(7 * (size_t)K);
      BAHIP_CHECKED_CALL(bahip_get_keyframe_poses(ctx_, poses.data(), K));
      for (int b = 0; b < K; ++b) {
        Keyframe* keyframe = keyframes_[bound_ids_[b]].get();
        // windowed: the poses that were not unknowns keep their SE3f objects bit for bit (set_global_T_frame would rebuild
        // frame_T_global as the inverse)
        if (use_window && memcmp(keyframe->global_T_frame().data(), &poses[7 * (size_t)b], 7 * sizeof(float)) == 0) continue;
        keyframe->set_global_T_frame(SE3f(&poses[7 * (size_t)b]));
      }
    }
    if (optimize_color_intrinsics) color_camera_ = PinholeCamera4f(out_color.width, out_color.height, &out_color.fx);
    if (optimize_depth_intrinsics) {
      depth_camera_ = PinholeCamera4f(out_depth.width, out_depth.height, &out_depth.fx);
      depth_params_.a = out_a;
    }
    if ((optimize_depth_intrinsics || optimize_color_intrinsics) && intrinsics_updated_callback_) intrinsics_updated_callback_();
    if (do_surfel_updates) {
      BindScene(stream);   // merges use the updated poses / intrinsics
      merge_and_compact();
    }

    if (iteration >= min_iterations - 1 && ((usize)num_converged == keyframes_.size() || !optimize_poses)) {
      if (converged) *converged = true;
      break;
    }
    if (timer && timer->GetTimeSinceStart() > time_limit) break;
  }

  if (increase_ba_iteration_count) {
    PerformBASchemeEndTasks(stream, do_surfel_updates);
    ++ba_iteration_count_;
  } else if (do_surfel_updates) {
    BindScene(stream);
    merge_and_compact();   // B/direct_ba_pcg.cc:775-812
  }
  BAHIP_CHECKED_CALL(bahip_stream_synchronize(stream));
}

}  // namespace vis
