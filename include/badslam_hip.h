/*
 * badslam_hip.h -- C ABI of the MI355X-native direct bundle-adjustment backend.
 *
 * This is the drop-in boundary for the BA hot path of ETH3D/badslam: every entry point below
 * replaces one of the free functions that the reference's DirectBA class calls
 * (applications/badslam/src/badslam/kernels.h:94-495, abbreviated B/kernels.h) or one of its
 * keyframe preprocessing calls (B/keyframe.cc:96-144).  Plain pointers and sizes only, no C++
 * types.  All device pointers are BORROWED: the caller owns every allocation (the reference's
 * CUDABuffer objects own theirs, B/direct_ba.h:441-507); the library only owns the scratch held
 * inside a bahip_context.
 *
 * Conventions
 *   - return value 0 = success; non-zero = failure, message via bahip_last_error() (the C++ shim
 *     turns non-zero into LOG(FATAL), matching the reference's CUDA_CHECK() semantics,
 *     libvis/src/libvis/cuda/cuda_util.h:35-49).
 *   - "stream" is the hipStream_t a bahip_context was created on; every call is asynchronous on
 *     that stream unless documented as synchronising (those that return host values).
 *   - images are pitched row-major: element (y, x) of type T at (char*)data + y*pitch_bytes + x*sizeof(T),
 *     exactly libvis CUDABuffer_<T> (libvis/src/libvis/cuda/cuda_buffer.cuh:44-119).
 *   - the surfel buffer is the reference's 17-row SoA (B/kernels.cuh:69-93): row r, surfel i at
 *     (float*)((char*)data + r*pitch_bytes) + i.
 *   - cameras are PinholeCamera4f parameter vectors in the pixel-corner convention.
 *   - poses are SE3f stored like Sophus: unit quaternion (x, y, z, w) then translation = 7 floats.
 */
#ifndef BADSLAM_HIP_H_
#define BADSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAHIP_SURFEL_ATTRIBUTE_COUNT 17   /* B/kernels.cuh:93 */
#define BAHIP_MERGE_BUFFER_COUNT 3        /* B/kernels.cuh:51 */
#define BAHIP_MAX_POSE_ITERATIONS 30      /* B/direct_ba_alternating.cc:130 */

enum { BAHIP_KF_ACTIVE = 0, BAHIP_KF_COVISIBLE_ACTIVE = 1, BAHIP_KF_INACTIVE = 2 };  /* B/keyframe.h:54-67 */

typedef struct bahip_camera {       /* libvis PinholeCamera4f */
  float fx, fy, cx, cy;
  int32_t width, height;
} bahip_camera;

typedef struct bahip_depth_params { /* B/surfel_projection.cuh:129-149 */
  float a;
  float raw_to_float_depth;
  float baseline_fx;
  int32_t sparse_surfel_cell_size;
  float* cfactor;                   /* device, ((H-1)/cell+1) x ((W-1)/cell+1) floats */
  uint32_t cfactor_pitch_bytes;
  int32_t cfactor_width, cfactor_height;
} bahip_depth_params;

/* Tiled copies ("BA planes") of a frame's depth+normals and of its luma, the layout the surfel sweeps
 * read (DESIGN.md "HBM layout").  Opaque; owned by whoever owns the images (vis::Keyframe does). */
typedef struct bahip_frame_planes bahip_frame_planes;

typedef struct bahip_frame {        /* the four images a Keyframe owns, B/keyframe.h:227-231 */
  uint16_t* depth;   uint32_t depth_pitch_bytes;
  uint16_t* normals; uint32_t normals_pitch_bytes;
  uint16_t* radius;  uint32_t radius_pitch_bytes;
  uint8_t* color;    uint32_t color_pitch_bytes;   /* uchar4 (R, G, B, luma) */
  /* Optional.  NULL: the library packs the planes itself on every call that receives this frame (correct, but a
   * K-image repack per bahip_set_keyframes).  Non-NULL: must have been refreshed with bahip_frame_planes_update
   * after the last change of depth / normals / color. */
  const bahip_frame_planes* planes;
} bahip_frame;

typedef struct bahip_keyframe {     /* one entry of the keyframe list handed to the *_CUDA functions */
  bahip_frame frame;
  float global_T_frame[7];          /* qx qy qz qw tx ty tz */
  int32_t activation;               /* BAHIP_KF_*; a deleted (null) keyframe is simply left out */
} bahip_keyframe;

typedef struct bahip_surfels {      /* B/direct_ba.cc:122-123 */
  float* data;
  uint32_t pitch_bytes;
  uint8_t* active;                  /* may be NULL where the reference passes none */
  uint32_t surfels_size;
  uint32_t capacity;
} bahip_surfels;

typedef struct bahip_context bahip_context;

/* ---- library / context ---------------------------------------------------------------------- */
const char* bahip_last_error(void);
int bahip_device_count(void);
/* hip_stream: a hipStream_t (NULL = the legacy default stream). */
int bahip_context_create(bahip_context** out, void* hip_stream);
void bahip_context_destroy(bahip_context* ctx);
int bahip_context_synchronize(bahip_context* ctx);
/* Multi-GPU surfel sharding (one process per GPU, DESIGN.md "Multi-GPU"): the per-keyframe pose normal equations, the
 * intrinsics accumulators and the dense head of the PCG vectors are summed element-wise over all ranks, in place.
 *
 * Native path: bahip_context_init_rccl creates an RCCL communicator for this context (rank 0 obtains the 128-byte id with
 * bahip_rccl_get_unique_id and distributes it by any means, e.g. a torch.distributed broadcast) and every sum becomes one
 * ncclAllReduce on the context's stream: no host round trip, ordered with the kernels around it.  librccl.so is loaded
 * on first use (dlopen), so a single-GPU process never touches it.
 *
 * Hook path: any other transport (a hook, when installed, takes precedence over the communicator).  The hook receives the stream the producers of `device_buffer` were queued on and must
 * order the reduction after them and before later work on that stream (e.g. torch.cuda.ExternalStream(stream) around
 * dist.all_reduce).  dtype: BAHIP_SUM_F32 (count floats), BAHIP_SUM_I64 (count int64_t: the pose normal equations are
 * summed in fixed point, which makes a sharded run bit-identical to the unsharded one) or BAHIP_SUM_F64 (count doubles: the
 * accumulators of the intrinsics step).  NULL (default) = single GPU. */
/* 1 if sums go over several ranks (a hook or an RCCL communicator is installed), else 0. */
int bahip_context_is_sharded(bahip_context* ctx);
enum { BAHIP_SUM_F32 = 0, BAHIP_SUM_I64 = 1, BAHIP_SUM_F64 = 2 };
typedef int (*bahip_allreduce_fn)(void* device_buffer, size_t count, int dtype, void* hip_stream, void* user);
int bahip_context_set_allreduce(bahip_context* ctx, bahip_allreduce_fn fn, void* user);
/* Multi-GPU KEYFRAME sharding (BASELINE configs[3]: "sharded by keyframe, RCCL all-reduce of pose Hessians"; the loop it
 * partitions: B/kernel_opt_geometry.cc:108-200, B/kernel_opt_pose.cc:67-96, B/kernel_surfel_activation.cc:53-66).  Every rank
 * holds ALL surfels and the images of its own keyframes only: bound keyframe k lives on rank k % world, world = 1, 2, 4 or 8
 * (the per-surfel sums are defined as C interleaved partial sums over the keyframe classes k % C, kernels_surfel.hip, so whole
 * classes per rank reproduce the unsharded bits: C = 4 by default, which serves 2 and 4 ranks; 8 ranks -- BASELINE configs[3] as
 * written -- need C = 8, bahip_context_set_sum_classes, which is then also the definition the single-GPU run it is compared with
 * must use).  bahip_set_keyframes still
 * takes all keyframes -- poses and activation states are replicated -- but the image pointers of keyframes that live elsewhere
 * are not looked at (pass NULL).  With it
 *   - bahip_update_surfel_activation sums one hit word per surfel over the ranks (BAHIP_SUM_I64, N / 2 words);
 *   - bahip_optimize_geometry_iteration / bahip_update_activation_and_optimize_geometry run in three launches with two
 *     exchanges of the class partials (bit patterns as BAHIP_SUM_I64: 4 x 5 and 4 x 8 binary32 values per surfel);
 *   - bahip_estimate_keyframe_poses* sweep this rank's keyframes, sum the fixed-point normal equations over the ranks
 *     (K x 56 int64 per Gauss-Newton round, the exchange surfel sharding makes too) and solve every pose on every rank;
 *   - bahip_optimize_intrinsics sweeps this rank's classes of the global sums' keyframe classes (world must not exceed the count
 *     of bahip_context_set_intrinsics_sum_classes) and sums the binary64 accumulators over the ranks (BAHIP_SUM_F64, 64 + 8 S
 *     doubles, the exchange surfel sharding makes too); every rank solves the same 5 x 5 / 4 x 4 systems and cfactor cells;
 *   - bahip_pcg_iteration sweeps this rank's classes of the PCG surfel block's keyframe classes (world must not exceed the count of
 *     bahip_context_set_pcg_sum_classes); the class partials of r and M after the init sweep and of g after every step-1 sweep are
 *     summed over the ranks as BAHIP_SUM_I64 over their bit patterns (C x 2 x (1 or 3) and C x (1 or 3) binary32 values per surfel),
 *     the exact accumulators as under surfel sharding; the normals update before it (bahip_update_surfel_normals) exchanges its
 *     class partials like the geometry step's normals pass (world must not exceed bahip_context_set_sum_classes);
 *   - the batched surfel lifecycle deals the image reads out by owner and runs the order-dependent rest on every rank, every
 *     exchange an integer sum (BAHIP_SUM_I64) of zero-filled partials or counts:
 *       bahip_create_surfels_for_keyframes: every keyframe of the batch takes the creation chain (the last one and a batch of one
 *         too, so the caller's supporting planes end EMPTY, as a merge batch leaves them); one exchange of the owners' occupancy at
 *         the batch's begin, candidates and their raw depth / normal words (n x (cells + padded pixels + 4 cells) bytes), one of the
 *         outlier filter's counts over each rank's co-visible keyframes (n x cells x 8 bytes, when filtering), one of the owners'
 *         records (36 bytes per candidate), then ONE exchange per keyframe of the chain: the next keyframe's occupancy (cells bytes);
 *       bahip_merge_surfels_for_bound_keyframes (inside a lifecycle batch that knows its keyframes): the per-(keyframe, cell) counts
 *         (n x cells x 4 bytes) and the cells' members (12 bytes per associated pair);
 *       bahip_delete_surfels_and_update_radii: per surfel the observation and violation counts and one minimum-radius word per rank
 *         ((2 + world) x 4 bytes);
 *     compaction and the spatial order read no image and run as they are;
 *   - bahip_observed_covisibility, bahip_keyframe_observer_histogram and bahip_surfel_observations build the tile mask table (per
 *     tile of 64 surfels the (keyframe, 64-bit ballot) entries with a non-zero ballot; DESIGN.md section 3, "The tile mask table")
 *     from every rank's own keyframes with two integer sums of zero-filled partials -- the per-tile entry counts (T x ceil(world / 4)
 *     int64 words, T = ceil(surfels / 64)) and the E entries (10 bytes each, in slices of at most 1 600 000 entries; none when
 *     E = 0) -- and reduce it on every rank: the matrix and the histogram over the tiles t % world == rank, summed over the ranks (one
 *     exchange of K x K or K x bins int64 words); the lists on every rank from the whole table, the payload planes from this rank's
 *     keyframes, summed as bit patterns (4 bytes per depth_raw word, 8 per descriptor_raw pair, per plane in slices of at most
 *     4 000 000 words).  Every argument of such a call, the capacity and the planes asked for included, is the same on every rank;
 *   - everything ends with the bits of the unsharded run (with the same class counts) on every rank.
 * The PCG stage entry points (bahip_pcg_begin ...), bahip_assign_colors and the one-keyframe lifecycle entry points
 * (bahip_create_surfels_for_keyframe, bahip_determine_supporting_surfels) and bahip_merge_surfels_for_keyframes (a frame does not
 * say which rank owns it) are refused in this mode.  A hook or an RCCL communicator must be installed when world > 1.  Surfel and
 * keyframe sharding exclude each other on one context. */
int bahip_context_set_keyframe_sharding(bahip_context* ctx, int rank, int world);
/* Dealing the surfel lifecycle over the ranks of a SURFEL partition (ours; off by default).  Under surfel sharding the
 * lifecycle runs inside a whole-cloud phase: bahip_gather_surfel_shards gives every rank the whole cloud, and every rank holds every
 * keyframe's images.  With the mode on, the lifecycle calls between a gather of world >= 2 ranks (a power of two) and the following
 * bahip_extract_surfel_shard deal their sweeps over that partition -- bound keyframe k belongs to rank k % world, surfel i of the
 * gathered cloud to rank (i / chunk) % world -- and exchange what they computed as integer sums (BAHIP_SUM_I64) of zero-filled
 * partials or counts, so every rank ends with the bits of the replicated call.  Sizes at BASELINE configs[2] (640 x 480 pixels,
 * 320 x 240 = 76 800 sparse cells, 3 M surfels), per call:
 *   bahip_create_surfels_for_keyframes (a batch of n >= 2 keyframes inside a lifecycle batch that knows them): the keyframes but the
 *     last are the chain's; their owners sweep the occupancy at the batch's begin, the candidates and their raw depth / normal words ->
 *     ONE exchange of (n - 1) x (cells + padded pixels + 4 cells) bytes, each part rounded up to 256 (691 200 bytes per keyframe); the outlier filter's counts over
 *     each rank's co-visible keyframes -> ONE exchange of (n - 1) x cells x 8 bytes (614 400 bytes per keyframe; only when filtering
 *     with co-visibility lists); the owners' records -> ONE exchange of 36 bytes per candidate (none without candidates).  The chain
 *     (create_chain_kernel) and the last keyframe then run on every rank as in the replicated call, with no exchange per keyframe, so
 *     the caller's supporting planes end as the replicated call leaves them.  A batch of one keyframe, or one the lifecycle batch does
 *     not know, is not dealt;
 *   bahip_merge_surfels_for_bound_keyframes (inside a lifecycle batch that knows its keyframes): the owners' association and fill
 *     sweeps -> TWO exchanges, the per-(keyframe, cell) counts (n x cells x 4 bytes: 307 200 bytes per keyframe) and the cells'
 *     members (12 bytes per associated pair); the scan and the decisions stay on every rank.  bahip_merge_surfels_for_keyframes is
 *     not dealt (a frame does not say which keyframe it is);
 *   bahip_delete_surfels_and_update_radii: dealt by SURFEL chunk, not by keyframe -- each rank decides its own chunks over all
 *     keyframes -> ONE exchange of 8 bytes per surfel + 8 (24 MB for 3 M surfels; keyframe dealing would take (2 + world) x 4 bytes
 *     per surfel).  The data rows end as delete_update's; the scratch rows it fills are not written;
 *   compaction and the spatial order read no image and run as they are.
 * Only calls on the cloud the gather filled (the same surfels->data) are dealt: the gather and the extract must come in pairs.
 * More bytes move than in the replicated call: on a 16-keyframe 640 x 480 drop-in call the mode moved 72 MB per rank, 12.8 MB
 * without it (the merge members at 12 bytes per pair dominate).  Whether it pays depends on the links.
 * With the mode off, or at world 1, every call takes the replicated path and its exchanges (none inside the phase).  Valid with or
 * without a hook / communicator installed (a gather of world >= 2 needs one); refused under keyframe sharding, which deals its own
 * lifecycle by keyframe (and bahip_context_set_keyframe_sharding with world > 1 is refused while the mode is on). */
int bahip_context_set_lifecycle_dealing(bahip_context* ctx, int enabled);
/* What this rank swept of the dealt lifecycle since the last reset: [0] creation keyframes whose up-front sweeps it ran, [1] the sum of
 * (their bound index + 1), [2] merge keyframes whose association / fill sweeps it ran, [3] the sum of (their bound index + 1), [4]
 * surfels whose deletion it decided, [5] calls that took the dealt path, [6] creation candidates whose records were exchanged, [7] merge
 * (surfel, keyframe) pairs whose cell members were exchanged.  stats_out: 8 words. */
int bahip_debug_lifecycle_deal_stats(bahip_context* ctx, long long* stats_out, int reset);
/* The number of interleaved partial sums (keyframe classes) the per-surfel sums of the normals and geometry passes are DEFINED
 * over: 4 (default) or 8.  In exact arithmetic both are the reference's sum (B/kernel_opt_geometry.cu: keyframe after keyframe);
 * in binary32 they differ in the last bits like any reordering.  The oracle takes the same parameter (orc_set_sum_classes), and
 * both class counts are held against it bit for bit.  Takes effect at once (no re-binding needed). */
int bahip_context_set_sum_classes(bahip_context* ctx, int classes);
/* The number of keyframe classes C the 34 global sums of the intrinsics step (A, b1, colour H, colour b) are DEFINED over: 1
 * (default), 2, 4 or 8.  Keyframe k (bound index) belongs to class k % C; per surfel and class a binary32 chain over the class's
 * keyframes in ascending order, per 64-surfel tile and class the xor butterfly, then binary64 over all (tile, class) values
 * (kernels_intrinsics.hip).  C = 1 is the one chain over all keyframes.  Keyframe sharding over `world` ranks needs C >= world, and
 * the single-GPU run it is compared with the same C.  The per-cell sums do not depend on it.  Takes effect with the next step. */
int bahip_context_set_intrinsics_sum_classes(bahip_context* ctx, int classes);
/* The number of keyframe classes C the surfel block of the PCG scheme's r, M (PCGInit) and g (PCGStep1) is DEFINED over: 1 (default),
 * 2, 4 or 8.  Keyframe k (bound index) belongs to class k % C; per surfel entry and class a binary32 chain over the class's keyframes
 * in ascending order, p_c, and the entry is ((p0 + p1) + p2) + ... (the combination rule of the normals / geometry passes).  C = 1
 * is the one chain over all keyframes.  Keyframe sharding of bahip_pcg_iteration over `world` ranks needs C >= world, and the
 * single-GPU run it is compared with the same C.  The dense head (poses, intrinsics, cfactor cells) and the dot products are exact
 * sums and do not depend on it.  Takes effect with the next call. */
int bahip_context_set_pcg_sum_classes(bahip_context* ctx, int classes);
/* Order in which the surfels a keyframe creates are appended: 0 (default) = by tiles of 8 x 8 sparse cells of the creating
 * keyframe, row-major inside a tile -- the 64 surfels of a wavefront form a compact patch, which is what the sweeps' culling wants;
 * 1 = row-major over the whole image, the reference's order (B/kernel_create_surfels.cu:357-390).  The same surfels either way;
 * their indices differ inside each keyframe's block, and with them which of two mergeable surfels survives (the lower index:
 * B/kernel_supporting_surfels.cu:60-86).  Takes effect for the creations that follow. */
int bahip_context_set_creation_order(bahip_context* ctx, int row_major);
/* Arithmetic flavour of the sweeps over (surfel, keyframe) pairs -- activation, normals / geometry step, pose normal equations,
 * intrinsics sweep, PCG init and step-1 sweeps -- of this context:
 *   BAHIP_ARITHMETIC_EXACT (default)  correctly rounded reciprocal / square root / division, defined exp, no contraction beyond the
 *                                     spelled fused multiply-adds: every bit is the CPU oracle's (what the parity tests hold);
 *   BAHIP_ARITHMETIC_FAST             v_rcp_f32 / v_sqrt_f32 / v_exp_f32 (<= 1 ulp), contraction at the compiler's discretion, binary32
 *                                     denormals flushed -- the arithmetic of the reference's own build (nvcc -use_fast_math,
 *                                     applications/badslam/CMakeLists.txt:74); held to the reference's kernels by tolerance
 *                                     (tests/test_gpu_fast_flavour.py: poses within 1e-5 m, association flips <= 0.1 %).
 * The order of every sum is the same in both (fixed trees, fixed-point pose sums, exact PCG sums), so either flavour is
 * deterministic and invariant under surfel / keyframe sharding; preprocessing, the surfel lifecycle, the pose solve and the PCG
 * vector kernels exist once (exact).  Takes effect at once.  The environment variable BAHIP_ARITHMETIC=fast|exact sets the default
 * of contexts created afterwards (A/B runs of unmodified callers). */
enum { BAHIP_ARITHMETIC_EXACT = 0, BAHIP_ARITHMETIC_FAST = 1 };
int bahip_context_set_arithmetic(bahip_context* ctx, int arithmetic);
int bahip_context_get_arithmetic(bahip_context* ctx);
/* A hint, for callers that write the surfel buffer themselves (an upload, a permutation of their own): which surfels share a tile has
 * changed, so the run order the sweeps derive from a census of the tiles ("heavy work first", rebuilt on its own only every 32nd pose
 * phase or when the number of tiles changes) is stale -- the next pose phase takes the census again.  The backend's own movers
 * (bahip_compact_surfels, bahip_sort_surfels_spatially) do this themselves.  Results never depend on the run order. */
int bahip_context_surfels_rearranged(bahip_context* ctx);
#define BAHIP_RCCL_UNIQUE_ID_BYTES 128
int bahip_rccl_get_unique_id(char unique_id_out[BAHIP_RCCL_UNIQUE_ID_BYTES]);
int bahip_context_init_rccl(bahip_context* ctx, const char unique_id[BAHIP_RCCL_UNIQUE_ID_BYTES], int rank, int world_size);
/* The first exchange of a run, as a probe: every rank contributes 1 through the context's transport (hook or native RCCL) on the
 * context's stream; the host waits for the sum at most timeout_ms (<= 0: for ever) and returns the number of ranks that took
 * part.  A job whose first collective cannot complete fails here with a message instead of hanging inside the first BA iteration.
 * Every rank must call it at the same point.  1 rank / no transport: *ranks_out = 1. */
int bahip_context_count_ranks(bahip_context* ctx, int timeout_ms, int* ranks_out);

/* Device memory helpers (what libvis CUDABuffer does with cudaMallocPitch / cudaMemcpy2DAsync,
 * libvis/src/libvis/cuda/cuda_buffer_inl.h:36-186). */
int bahip_malloc_pitch(void** ptr, size_t* pitch_bytes, size_t width_bytes, size_t height);
int bahip_free(void* ptr);
int bahip_memcpy_2d(bahip_context* ctx, void* dst, size_t dst_pitch, const void* src, size_t src_pitch,
                    size_t width_bytes, size_t height, int kind /* 1 = H2D, 2 = D2H, 3 = D2D */);
int bahip_memset_2d(bahip_context* ctx, void* dst, size_t pitch, int value, size_t width_bytes, size_t height);

/* Stream-level helpers used by the host-side CUDABuffer<T> (libvis/src/libvis/cuda/cuda_buffer_inl.h:
 * UploadAsync / DownloadAsync / UploadPartAsync / DownloadPartAsync / Clear / SetTo all take the
 * stream per call).  kind: 1 = H2D, 2 = D2H, 3 = D2D.  All asynchronous on `hip_stream`. */
int bahip_context_set_stream(bahip_context* ctx, void* hip_stream);
int bahip_stream_create(void** hip_stream_out);
int bahip_stream_destroy(void* hip_stream);
int bahip_stream_synchronize(void* hip_stream);
int bahip_memcpy_2d_async(void* hip_stream, void* dst, size_t dst_pitch, const void* src, size_t src_pitch,
                          size_t width_bytes, size_t height, int kind);
int bahip_memcpy_async(void* hip_stream, void* dst, const void* src, size_t bytes, int kind);
int bahip_memset_async(void* hip_stream, void* dst, int value, size_t bytes);
/* Page-locked host memory, and the question CUDABuffer<T>::UploadAsync / DownloadAsync ask before they return: a transfer to or from
 * page-locked memory is left in flight on the stream, as cudaMemcpy2DAsync leaves it (libvis/src/libvis/cuda/cuda_buffer_inl.h:73-90);
 * for pageable memory the call waits, which is what the CUDA runtime does there too (the copy is staged, a download has completed
 * when the call returns).  bahip_host_is_pinned: 1 if both ends of [ptr, ptr + bytes) are page-locked host memory
 * (bahip_host_alloc, hipHostMalloc, hipHostRegister), else 0. */
int bahip_host_alloc(void** ptr, size_t bytes);
int bahip_host_free(void* ptr);
int bahip_host_is_pinned(const void* ptr, size_t bytes);
/* CUDABuffer<T>::Clear(value, stream) (libvis/src/libvis/cuda/cuda_buffer.cu:41-60) for 1/2/4-byte T. */
int bahip_fill_2d(void* hip_stream, void* data, size_t pitch_bytes, int elem_bytes, uint32_t value_bits, int width, int height);

/* ---- frame preprocessing (BadSlam::PreprocessFrame, B/bad_slam.cc:643-765) --------------------- */
/* B/cuda_depth_processing.cu:42-128 BilateralFilteringAndDepthCutoffCUDA: raw depth 0 or > max_depth -> 65535 (unknown),
 * else the bilateral filter in inverse depth over a disc of radius int(radius_factor * sigma_xy + 0.5) <= 8 pixels.
 * Not in place. */
int bahip_bilateral_filtering_and_depth_cutoff(bahip_context* ctx, float sigma_xy, float sigma_value, float radius_factor,
                                               uint16_t max_depth, float raw_to_float_depth, const uint16_t* in_depth,
                                               uint32_t in_pitch_bytes, uint16_t* out_depth, uint32_t out_pitch_bytes, int width,
                                               int height);
/* What PreprocessFrame does ahead of that filter when the BA runs at a pyramid level (B/bad_slam.cc:657-689; the reference runs these
 * on the CPU).  Integer rules, the reference's results bit for bit, the same under either arithmetic flavour.  All three: ordered on
 * the context's stream, not in place, pitches in bytes; a refused call returns non-zero (bahip_last_error) and writes nothing.
 * The median rule: of n non-zero values sorted ascending, s[n/2] for odd n; for even n, with low = s[n/2 - 1], high = s[n/2] and
 * average = float(sum) / float(n) in binary32, low if |average - low| < |average - high| and high otherwise (a tie gives high).
 *
 * One iteration of MedianFilterAndDensifyDepthMap (B/preprocessing.cc:40-85): the rule on the non-zero values of the 3 x 3 window
 * clipped to the image; with fewer than 2 of them the pixel is copied.  A zero pixel with two valid neighbours is filled. */
int bahip_median_filter_and_densify(bahip_context* ctx, const uint16_t* in_depth, uint32_t in_pitch_bytes, uint16_t* out_depth,
                                    uint32_t out_pitch_bytes, int width, int height);
/* Image<u16>::DownscaleUsingMedianWhileExcluding(0, ...) (L/image.h:1003-1053): output pixel (x, y) is the rule on the non-zero values of
 * input columns [(W x) / ow, (W (x + 1)) / ow) and rows [(H y) / oh, (H (y + 1)) / oh) (unsigned division), 0 if there are none.
 * Refused unless 1 <= ow <= W, 1 <= oh <= H, W, H <= 65535 and ceil(W / ow), ceil(H / oh) <= 9: at most 81 values, whose binary32
 * sum is exact (81 * 65535 < 2^24) and so does not depend on the order of summation. */
int bahip_downscale_depth_median(bahip_context* ctx, const uint16_t* in_depth, uint32_t in_pitch_bytes, int in_width, int in_height,
                                 uint16_t* out_depth, uint32_t out_pitch_bytes, int out_width, int out_height);
/* Image<Vec3u8>::DownscaleToHalfSize (L/image.h:929-948) applied `levels` times (1 .. 3), as ImagePyramid does: per channel
 * a / 4 + b / 4 + c / 4 + d / 4, every quotient truncated (four 3s give 0, four 255s give 252).  The output is (width >> levels) x
 * (height >> levels); refused unless width and height are divisible by 2^levels. */
int bahip_downscale_rgb_half(bahip_context* ctx, const uint8_t* rgb_in, uint32_t in_pitch_bytes, int width, int height, int levels,
                             uint8_t* rgb_out, uint32_t out_pitch_bytes);

/* ---- keyframe preprocessing (Keyframe ctor #2, B/keyframe.cc:96-144) ------------------------- */
/* B/cuda_image_processing.cu:165-193 ComputeBrightnessCUDA: uchar3 RGB -> uchar4 (R,G,B,luma). */
int bahip_compute_brightness(bahip_context* ctx, const uint8_t* rgb, uint32_t rgb_pitch_bytes,
                             uint8_t* rgba, uint32_t rgba_pitch_bytes, int width, int height);
/* B/cuda_depth_processing.cu:134-287 ComputeNormalsCUDA. */
int bahip_compute_normals(bahip_context* ctx, const bahip_camera* depth_camera, const bahip_depth_params* dp,
                          const uint16_t* in_depth, uint32_t in_pitch, uint16_t* out_depth, uint32_t out_pitch,
                          uint16_t* out_normals, uint32_t normals_pitch);
/* B/cuda_depth_processing.cu:289-388 ComputePointRadiiAndRemoveIsolatedPixelsCUDA. */
int bahip_compute_point_radii_and_remove_isolated_pixels(
    bahip_context* ctx, const bahip_camera* depth_camera, float raw_to_float_depth,
    const uint16_t* depth, uint32_t depth_pitch, uint16_t* radius, uint32_t radius_pitch,
    uint16_t* out_depth, uint32_t out_pitch);
/* B/cuda_depth_processing.cu:391-465 ComputeMinMaxDepthCUDA (synchronises; results on host). */
int bahip_compute_min_max_depth(bahip_context* ctx, const uint16_t* depth, uint32_t depth_pitch, int width,
                                int height, float raw_to_float_depth, float* min_depth, float* max_depth);

/* ---- scene binding ----------------------------------------------------------------------------
 * The reference passes cameras, DepthParameters and the keyframe vector to every *_CUDA call.
 * Here they are bound once per BA call and kept in a device-side keyframe table so that one
 * launch can sweep all keyframes (the per-keyframe launch granularity of B/kernel_*.cc is what
 * this backend removes). */
int bahip_set_intrinsics(bahip_context* ctx, const bahip_camera* color_camera, const bahip_camera* depth_camera,
                         const bahip_depth_params* dp);
/* Maintenance, like compaction: reorders surfels [0, surfels_size) along a Morton curve over a world grid of
 * `grid_cell_size` metres (stable; deleted surfels last).  Moves the 8 data rows and the active flags.  Surfels that
 * one image region shows become neighbours in the buffer, which is what the sweeps' L2 behaviour wants;
 * no result depends on the order.  Not part of the reference: call it when convenient (after keyframes were added).
 * Round 6: ordered on the context's stream like a kernel launch -- no allocation and no host wait (a scratch block of the context
 * holds keys, indices and a dense copy of the rows; it grows when the cloud does). */
int bahip_sort_surfels_spatially(bahip_context* ctx, const bahip_surfels* surfels, float grid_cell_size);

/* BA planes of one frame: create for the given image sizes, refresh from the frame's images (on the context
 * stream), destroy.  The Keyframe constructor (B/keyframe.cc:81-158) is where the reference derives normals, radii
 * and luma from its inputs; the planes are one more derived product of the same step. */
int bahip_frame_planes_create(bahip_context* ctx, int depth_width, int depth_height, int color_width, int color_height,
                              bahip_frame_planes** out);
int bahip_frame_planes_update(bahip_context* ctx, bahip_frame_planes* planes, const bahip_frame* frame);
void bahip_frame_planes_destroy(bahip_frame_planes* planes);

int bahip_set_keyframes(bahip_context* ctx, const bahip_keyframe* keyframes, int num_keyframes);
/* Read back the poses of the bound keyframes (7 floats each); synchronises. */
int bahip_get_keyframe_poses(bahip_context* ctx, float* global_T_frame_out, int num_keyframes);

/* ---- optimisation stages ---------------------------------------------------------------------- */
/* B/kernels.h UpdateSurfelActivationCUDA (B/kernel_surfel_activation.cc:39-67): surfels
 * [0, surfels_size) become active iff associated with >= 1 keyframe whose activation is kActive. */
int bahip_update_surfel_activation(bahip_context* ctx, const bahip_surfels* surfels, uint32_t surfels_size);
/* B/kernels.h:301-308 AssignColorsCUDA (B/kernel_assign_colors.cc:39-80), behind DirectBA::AssignColors
 * (B/direct_ba.cc:456-459): the colour of every surfel becomes the mean of the bilinear RGBA samples at its colour pixel
 * in all bound keyframes it is associated with (any activation); surfels seen by none keep their colour. */
int bahip_assign_colors(bahip_context* ctx, const bahip_surfels* surfels);
/* B/kernels.h UpdateSurfelNormalsCUDA (B/kernel_opt_geometry.cc:39-77). */
int bahip_update_surfel_normals(bahip_context* ctx, const bahip_surfels* surfels);
/* B/kernels.h OptimizeGeometryIterationCUDA (B/kernel_opt_geometry.cc:80-201). */
int bahip_optimize_geometry_iteration(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                      const bahip_surfels* surfels);
/* UpdateSurfelActivationCUDA for surfels [0, activation_surfels_size) followed by OptimizeGeometryIterationCUDA, as ONE
 * sweep: a surfel is active iff it is associated with a kActive keyframe, and the normals pass of the geometry step tests
 * exactly those associations anyway (B/direct_ba_alternating.cc:441-487 calls the two back to back).  Same flags and the same
 * surfels, bit for bit, as the two separate calls. */
int bahip_update_activation_and_optimize_geometry(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                                  const bahip_surfels* surfels, uint32_t activation_surfels_size);
/* B/kernels.h AccumulatePoseEstimationCoeffsCUDA (B/kernel_opt_pose.cc:39-97): one frame, one
 * linearisation point.  H = 21 floats (row-major upper triangle), b = 6 floats, on the host;
 * synchronises like the reference does (B/kernel_opt_pose.cc:94-96). */
int bahip_accumulate_pose_estimation_coeffs(bahip_context* ctx, int use_depth_residuals,
                                            int use_descriptor_residuals, const bahip_frame* frame,
                                            const float frame_T_global[12], const bahip_surfels* surfels,
                                            float* H, float* b);
/* DirectBA::EstimateFramePose (B/direct_ba_alternating.cc:42-283) for an arbitrary frame:
 * <= 30 Gauss-Newton steps, each = accumulate + double-precision LDLT + T <- T*exp(-x), entirely
 * on the device; one read-back at the end.  Outputs on the host. */
int bahip_estimate_frame_pose(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                              const bahip_frame* frame, const float global_T_frame_initial[7],
                              const bahip_surfels* surfels, float global_T_frame_out[7],
                              int* iterations_done, int* converged);
/* The pose phase of one alternating-BA iteration (B/direct_ba_alternating.cc:545-577): every
 * bound keyframe that is not kInactive gets its own EstimateFramePose, all keyframes batched per
 * Gauss-Newton round (they are mutually independent: surfels are frozen during this phase).
 * Updated poses stay in the device keyframe table (fetch with bahip_get_keyframe_poses) and are
 * also returned here.  iterations_done / converged: per keyframe (0 / 1 for skipped ones).
 * rounds_out: number of batched rounds (= max iterations over keyframes). */
int bahip_estimate_keyframe_poses(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                  const bahip_surfels* surfels, float* global_T_frame_out,
                                  int* iterations_done, int* converged, int* rounds_out);

/* The same pose phase, followed on the device by the activation update of B/direct_ba_alternating.cc:556-577: a keyframe
 * whose pose moved (log(old^-1 * new) fails the convergence test of B/convergence_analysis.h:43-51) becomes kActive, one
 * that did not becomes kInactive.  The device keyframe table (and its host mirror inside the context) then carries the new
 * poses AND activations, so the next iteration's sweeps need no bahip_set_keyframes.  moved: per bound keyframe 1 / 0 (0 for
 * keyframes that were kInactive); num_converged_out: keyframes that were kInactive or did not move. */
int bahip_estimate_keyframe_poses_and_update_activation(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                                        const bahip_surfels* surfels, float* global_T_frame_out,
                                                        int* iterations_done, int* converged, int* moved, int* rounds_out,
                                                        int* num_converged_out);
/* The whole loop of the alternating scheme (B/direct_ba_alternating.cc:345-718) over poses and geometry for a FIXED surfel set,
 * driven by the device: up to max_iterations iterations -- [activation window | co-visible propagation], activation + geometry
 * sweep, pose phase -- are queued back to back; the last solve launch of every pose phase evaluates the loop's stopping rule
 * (every keyframe counts as converged and iteration >= min_iterations - 1, :693-701) and raises a device word that turns
 * every launch queued behind it into a no-op.  The host waits ONCE, for the last launch, instead of after every Gauss-Newton
 * round.  A pose phase that needs more rounds than were queued for it raises the word too; the host then finishes that phase
 * round by round and queues the rest again -- results never depend on how many rounds were queued.  Needs bahip_set_keyframes,
 * bahip_set_covisibility and (fixed_window) bahip_set_activation_window; the device keyframe table carries the new poses and
 * activations afterwards (without the co-visible propagation that follows an iteration that did not end the loop: the caller
 * applies DetermineCovisibleActiveKeyframes itself when *converged_out == 0).
 * *handled_out = 0 and nothing done when the configuration is not covered (keyframe sharding, more keyframes than one launch of
 * the pose sums takes): the caller then drives the iterations through the stage functions above.
 * global_T_frame_out: 7 floats per bound keyframe; activation_out: BAHIP_KF_* per bound keyframe; not_converged_out: pose
 * estimations that hit BAHIP_MAX_POSE_ITERATIONS. */
typedef struct {
  int use_depth_residuals, use_descriptor_residuals;
  int fixed_window;              /* apply the bound activation window at the top of every iteration */
  int activate_in_geometry;      /* 1: UpdateSurfelActivation is part of the geometry sweep (full window); 0: flags as they are */
  uint32_t activation_surfels_size;
  int min_iterations, max_iterations;
} bahip_alternating_options;
int bahip_alternating_iterations(bahip_context* ctx, const bahip_alternating_options* options, const bahip_surfels* surfels,
                                 float* global_T_frame_out, int* activation_out, int* handled_out, int* iterations_done_out,
                                 int* converged_out, int* pose_rounds_out, int* pose_steps_out, int* not_converged_out);
/* Co-visibility lists of the bound keyframes in CSR form over bound indices (offsets: num_keyframes + 1 entries); call after
 * bahip_set_keyframes.  bahip_propagate_covisible_activation is DirectBA::DetermineCovisibleActiveKeyframes
 * (B/direct_ba.cc:549-564) on the device table: kInactive keyframes co-visible with a kActive one become kCovisibleActive.
 * Asynchronous on the context stream. */
int bahip_set_covisibility(bahip_context* ctx, const int* offsets, const int* indices, int num_keyframes);
int bahip_propagate_covisible_activation(bahip_context* ctx);
/* Fixed active window of the alternating scheme (B/direct_ba_alternating.cc:353-371): in_window[k] != 0 for the bound
 * keyframes inside it.  bahip_apply_activation_window sets those kActive, all others kInactive, and then propagates the
 * co-visible activation -- the top of every iteration, on the device table; asynchronous. */
int bahip_set_activation_window(bahip_context* ctx, const uint8_t* in_window, int num_keyframes);
int bahip_apply_activation_window(bahip_context* ctx);

/* ---- surfel lifecycle --------------------------------------------------------------------------- */
/* B/kernels.h DetermineSupportingSurfelsCUDA / ...AndMergeSurfelsCUDA
 * (B/kernel_supporting_surfels.cc:112-165).  supporting: BAHIP_MERGE_BUFFER_COUNT device planes
 * of height x width u32 with the given pitch.  merged_count_out (host, may be NULL when
 * merge == 0) receives the number of surfels deleted by merging; synchronises when merging.
 * Deterministic: slots are claimed by the lowest surfel index (atomicMin), not by arrival. */
int bahip_determine_supporting_surfels(bahip_context* ctx, int merge, float merge_dist_factor,
                                       const bahip_frame* frame, const float frame_T_global[12],
                                       const bahip_surfels* surfels, uint32_t* const* supporting,
                                       uint32_t supporting_pitch_bytes, uint32_t* merged_count_out);
/* merged_count_out == NULL in bahip_determine_supporting_surfels(merge = 1, ...) defers the count: no read-back and no stream
 * synchronisation per keyframe; the surfels merged by all such calls since the last bahip_take_merged_count are returned (and
 * the counter cleared) here -- one synchronisation per batch of keyframes instead of one per keyframe. */
int bahip_take_merged_count(bahip_context* ctx, uint32_t* merged_count_out);
/* The merges of a BATCH of keyframes in one call (DirectBA's merge pass of a BA iteration and of the end tasks,
 * B/direct_ba_alternating.cc:491-540, B/direct_ba.cc:566-620): bahip_determine_supporting_surfels(merge = 1) for frames[0],
 * frames[1], ... in this order, with the same deletions -- but two dependent launches per keyframe instead of three: the sweep that
 * applies keyframe j's decisions runs beside the one that inserts keyframe j + 1's surfels (they alternate between the caller's planes
 * and a second set the context owns).  frame_T_global_3x4: 12 floats per frame.  Inside bahip_lifecycle_batch_begin / _set_frames
 * each keyframe's sweeps run over the tiles it can see.  Both sets of planes end EMPTY (the lists are not an output of a merge batch).
 * Round 6, second form: when the lifecycle batch knows every frame of the call, the planes are not used at all -- which surfels share
 * a sparse cell of frame j does not change while a batch merges, so the members of every (frame, cell) are listed up front for all
 * frames at once and every frame costs ONE launch of one thread per cell (the three lowest indices still alive, the decisions of
 * B/kernel_supporting_surfels.cu:60-86 in ascending order); the same deletions (bahip_debug_set_merge_cells selects the form).
 * merged_count_out: NULL defers the count to bahip_take_merged_count. */
int bahip_merge_surfels_for_keyframes(bahip_context* ctx, float merge_dist_factor, const bahip_frame* frames, const float* frame_T_global_3x4,
                                      int num_frames, const bahip_surfels* surfels, uint32_t* const* supporting, uint32_t supporting_pitch_bytes,
                                      uint32_t* merged_count_out);
/* The same merges for BOUND keyframes named by index (bahip_set_keyframes): their packed entries and poses, in the order given; the
 * same deletions as bahip_merge_surfels_for_keyframes with those keyframes' frames and frame_T_global (no repacking into a slot of the
 * context).  Inside a lifecycle batch that knows the keyframes (bahip_lifecycle_batch_set_keyframes) it runs by cell lists.  Under
 * keyframe sharding it is the merging entry point: the batch must know its keyframes, each rank lists the members of the keyframes it
 * owns, the counts and members are summed over the ranks, the decisions run on every rank. */
int bahip_merge_surfels_for_bound_keyframes(bahip_context* ctx, float merge_dist_factor, const int* keyframe_indices, int num_keyframes,
                                            const bahip_surfels* surfels, uint32_t* const* supporting, uint32_t supporting_pitch_bytes,
                                            uint32_t* merged_count_out);
/* A batch of keyframes creating or merging surfels on one cloud (the BA loop's creation pass, its merge pass, the merges of the
 * end tasks): bahip_lifecycle_batch_begin takes the bounding spheres of the cloud's 64-surfel tiles once; until
 * bahip_lifecycle_batch_end the per-keyframe sweeps of bahip_determine_supporting_surfels / bahip_create_surfels_for_keyframe over
 * the same buffer skip, per wavefront, the tiles the keyframe cannot see.  Results do not depend on the bracket (the test is the
 * conservative one of the BA sweeps); surfels may be appended and marked deleted inside it, not moved: compaction, the spatial
 * sort and the geometry step end the batch by themselves.  Ours: the reference sweeps the whole cloud per keyframe
 * (B/kernel_supporting_surfels.cu:36-60). */
int bahip_lifecycle_batch_begin(bahip_context* ctx, const bahip_surfels* surfels);
/* Optional, after _begin: the frames of the batch -- frame_T_global as 3x4 row-major matrices, exactly the 12 coefficients the
 * per-keyframe calls will be given (bahip_determine_supporting_surfels), or bound keyframe indices (bahip_create_surfels_for_
 * keyframe[s]).  The batch then knows which tiles each frame can see and that frame's sweeps run over those tiles only (a launch of a
 * few hundred workgroups instead of one over the whole cloud).  A frame that is not found sweeps with the per-tile test as before.
 * From here to _end the supporting planes passed to the MERGING calls (bahip_determine_supporting_surfels with merge != 0) belong to
 * the backend: every such call leaves them empty (all slots kInvalidIndex) instead of holding the keyframe's lists, which spares the
 * next keyframe of the batch its fill launch; the surfel buffer and the merged counts are what they are without the bracket. */
int bahip_lifecycle_batch_set_frames(bahip_context* ctx, const float* frame_T_global_3x4, int num_frames);
int bahip_lifecycle_batch_set_keyframes(bahip_context* ctx, const int* keyframe_indices, int num_keyframes);
int bahip_lifecycle_batch_end(bahip_context* ctx);
/* B/kernels.h CreateSurfelsForKeyframeCUDA (B/kernel_create_surfels.cc:40-183), including the
 * DetermineSupportingSurfelsCUDA call that DirectBA::CreateSurfelsForKeyframe issues first
 * (B/direct_ba.cc:345-355).  keyframe_index selects the bound keyframe; covis / n_covis: indices
 * of bound keyframes used for the new-surfel outlier filter.  new_surfel_count_out on the host;
 * synchronises.  Deterministic: the lowest linear pixel index wins a sparse cell. */
int bahip_create_surfels_for_keyframe(bahip_context* ctx, int keyframe_index, int filter_new_surfels,
                                      int min_observation_count, const int* covis, int n_covis,
                                      const bahip_surfels* surfels, uint32_t* const* supporting,
                                      uint32_t supporting_pitch_bytes, uint32_t* new_surfel_count_out);
/* A batch of keyframes, in the order given, each seeing what the ones before it appended -- n calls of
 * bahip_create_surfels_for_keyframe without the host in between (the cloud's size stays on the device during the batch; one host
 * wait at the end instead of two per keyframe).  covis_offsets[num_keyframes + 1] / covis_indices: the co-visibility lists of the
 * keyframes, concatenated, as indices into the bound keyframe list.  new_surfel_count_out: the surfels all of them appended; the
 * caller adds it to surfels_size.  A keyframe that does not fit the capacity creates nothing and raises the flag of
 * bahip_context_take_capacity_exceeded, the others go on (B/kernel_create_surfels.cc:162-165 per keyframe).
 * Round 6: inside a lifecycle batch that knows the keyframes (bahip_lifecycle_batch_set_keyframes) the keyframes do not wait for each
 * other's sweeps: what the cloud at the batch's begin occupies, which pixel of a free cell would create a surfel and whether it passes
 * the filter are found for ALL keyframes up front (three launches); each keyframe but the last then costs ONE launch -- its candidates
 * whose cell is still free are counted, scanned and appended, what it appends is pushed into the next keyframe's occupancy, what the
 * batch appended earlier is pulled into it.  The last keyframe takes the four-launch path, so the supporting planes end as a
 * one-keyframe call leaves them.  The same surfels at the same indices (bahip_debug_set_creation_chain selects the form). */
int bahip_create_surfels_for_keyframes(bahip_context* ctx, const int* keyframe_indices, int num_keyframes, int filter_new_surfels,
                                       int min_observation_count, const int* covis_offsets, const int* covis_indices,
                                       const bahip_surfels* surfels, uint32_t* const* supporting, uint32_t supporting_pitch,
                                       uint32_t* new_surfel_count_out);
/* 1 if the last bahip_create_surfels_for_keyframe on this context created nothing because the surfels would not have fit
 * into `capacity` (the reference's soft failure, B/kernel_create_surfels.cc:162-165); reading clears the flag. */
int bahip_context_take_capacity_exceeded(bahip_context* ctx);
/* B/kernels.h DeleteSurfelsAndUpdateRadiiCUDA (B/kernel_delete_surfels.cc:40-120); synchronises. */
int bahip_delete_surfels_and_update_radii(bahip_context* ctx, int min_observation_count,
                                          const bahip_surfels* surfels, uint32_t* deleted_count_out);
/* B/kernels.h CompactSurfelsCUDA (B/kernel_compact_surfels.cu:159-279): surfel_count valid
 * surfels end up in [0, surfel_count).  surfels->active may be NULL. */
int bahip_compact_surfels(bahip_context* ctx, uint32_t surfel_count, const bahip_surfels* surfels);

/* ---- intrinsics (B/kernels.h OptimizeIntrinsicsCUDA, B/kernel_opt_intrinsics.cc:39-281) --------- */
int bahip_optimize_intrinsics(bahip_context* ctx, int optimize_depth_intrinsics, int optimize_color_intrinsics,
                              const bahip_surfels* surfels, bahip_camera* out_color_camera,
                              bahip_camera* out_depth_camera, float* out_a);

/* ---- PCG solver (B/direct_ba_pcg.cc:229-646 over B/kernels.h PCG*CUDA) -------------------------- */
typedef struct bahip_pcg_options {
  int optimize_poses, optimize_geometry, optimize_depth_intrinsics, optimize_color_intrinsics;
  int use_depth_residuals, use_descriptor_residuals;
  int max_inner_iterations;     /* 30 */
  int gauge_keyframe;           /* index of the keyframe held fixed (reference: rand() % K) */
} bahip_pcg_options;
/* One outer Gauss-Newton iteration of the PCG scheme: builds and solves the full normal
 * equations matrix-free, applies the update to poses (device table), surfels, intrinsics and
 * cfactors.  Outputs new intrinsics on the host; inner_steps_out = PCG steps used. */
int bahip_pcg_iteration(bahip_context* ctx, const bahip_pcg_options* opt, const bahip_surfels* surfels,
                        bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a,
                        int* inner_steps_out, int* num_converged_out /* keyframes whose pose update is below the
                        convergence threshold, gauge keyframe included (B/direct_ba_pcg.cc:556-575) */);
/* The same outer iteration over the active keyframe window (ours; B/direct_ba_pcg.cc:125,140 refuse windows).  The system
 * (kernels_pcg_window.hip: "DEFINITION of the windowed system"): keyframes whose activation in the device table is not
 * BAHIP_KF_INACTIVE are swept in bound order (a kInactive one is not read at all); 6 pose unknowns per BAHIP_KF_ACTIVE keyframe;
 * BAHIP_KF_COVISIBLE_ACTIVE keyframes contribute residuals with fixed poses and then anchor the gauge -- without any, the gauge
 * is opt->gauge_keyframe (a bound index) if it is kActive, else the first kActive keyframe; surfel unknowns are the surfels with
 * the active bit (the layout stays 1 or 3 per surfel; inactive surfels keep zero rows and are left bit-identical).  The epsilon
 * terms of alpha_d count once per swept keyframe.  Poses of keyframes that are not unknowns are not touched, and count as
 * converged in num_converged_out.  With every keyframe kActive and every surfel active: the system of bahip_pcg_iteration.
 * Surfel sharding: the exchanges of bahip_pcg_iteration, the same bits as one GPU.  Refused (error text, context usable) under
 * keyframe sharding and with bahip_context_set_pcg_sum_classes(c > 1).  No kActive keyframe or no unknowns: returns 0 with every
 * keyframe counted as converged. */
int bahip_pcg_iteration_windowed(bahip_context* ctx, const bahip_pcg_options* opt, const bahip_surfels* surfels,
                                 bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a,
                                 int* inner_steps_out, int* num_converged_out);
/* Size of the window of the last bahip_pcg_iteration_windowed call that got as far as building it: swept keyframes and 64-surfel
 * tiles with an active surfel on this rank (diagnostics). */
int bahip_pcg_window_size(bahip_context* ctx, int* swept_keyframes_out, uint32_t* tiles_out);

/* ---- PCG solver, stage by stage (B/kernels.h:397-491): the entry points a caller that keeps the reference's own PCG driver
 * (B/direct_ba_pcg.cc:229-646) binds -- one bahip_ function per *CUDA function, same call sequence:
 *     r = M = 0; bahip_pcg_begin; for each keyframe bahip_pcg_init; bahip_pcg_init2;
 *     per inner step: g = 0 (from the second step on); for each keyframe bahip_pcg_step1; bahip_pcg_step2; read beta_n;
 *     bahip_pcg_step3; ... ; bahip_update_surfels_from_pcg_delta; bahip_update_cfactors_from_pcg_delta.
 * All vectors (unknown_count floats) and the three scalars are DEVICE pointers owned by the caller (the reference's
 * CUDABuffer_<PCGScalar>).  What the reference adds to the vectors with float atomics -- the entries of the poses, of the
 * intrinsics and of the cfactor cells, and the three dot products -- is summed exactly in accumulators inside the context
 * (badslam_amd/csrc/exact_sum.h) and written by the next stage that reads it: bahip_pcg_init2 writes those entries of r and
 * M, bahip_pcg_step2 those of g and *alpha_d (so r, M, g hold only their per-surfel entries between the keyframe loop and the
 * stage that follows it).  The per-surfel entries are read-modify-written per keyframe call exactly like the reference's.
 * Same bits as bahip_pcg_iteration, which runs the keyframe loops as single sweeps. */
typedef struct bahip_pcg_layout {   /* unknown layout (B/direct_ba_pcg.cc:232-307) */
  int optimize_poses, optimize_geometry, optimize_depth_intrinsics, optimize_color_intrinsics;
  int use_depth_residuals, use_descriptor_residuals;
  uint32_t unknown_count;
  uint32_t surfel_unknown_start_index;              /* valid if optimize_geometry */
  uint32_t depth_intrinsics_unknown_start_index;    /* valid if optimize_depth_intrinsics; a_unknown_index = this + 4 */
  uint32_t color_intrinsics_unknown_start_index;    /* valid if optimize_color_intrinsics */
} bahip_pcg_layout;
/* Sizes and clears the context's accumulators for a system with this layout over surfels_size surfels; before the first
 * bahip_pcg_init of an outer iteration. */
int bahip_pcg_begin(bahip_context* ctx, const bahip_pcg_layout* layout, uint32_t surfels_size);
/* PCGInitCUDA (B/kernels.h:397-416) for one keyframe: r -= J^T W F, M += diag(J^T W J).  kf_pose_unknown_index: first of the
 * keyframe's 6 pose unknowns; optimize_pose_of_keyframe = 0 for the gauge keyframe. */
int bahip_pcg_init(bahip_context* ctx, const bahip_pcg_layout* layout, const bahip_frame* frame, const float frame_T_global[12],
                   uint32_t kf_pose_unknown_index, int optimize_pose_of_keyframe, const bahip_surfels* surfels, float* pcg_r, float* pcg_M);
/* PCGInit2CUDA (B/kernels.h:418-428) */
int bahip_pcg_init2(bahip_context* ctx, const bahip_pcg_layout* layout, uint32_t surfels_size, float a, float* pcg_r, float* pcg_M,
                    float* pcg_delta, float* pcg_g, float* pcg_p, float* pcg_alpha_n);
/* PCGStep1CUDA (B/kernels.h:430-453) for one keyframe: g += J^T W J p; the keyframe's share of alpha_d is kept in the context
 * until bahip_pcg_step2 (pcg_alpha_d is not touched here). */
int bahip_pcg_step1(bahip_context* ctx, const bahip_pcg_layout* layout, const bahip_frame* frame, const float frame_T_global[12],
                    uint32_t kf_pose_unknown_index, int optimize_pose_of_keyframe, const bahip_surfels* surfels, const float* pcg_p,
                    float* pcg_g);
/* PCGStep2CUDA (B/kernels.h:455-466); writes *pcg_alpha_d (the sum over the bahip_pcg_step1 calls since the last step 2,
 * epsilon terms included once per call like the reference's AddAlphaDEpsilonTerms) and *pcg_beta_n. */
int bahip_pcg_step2(bahip_context* ctx, const bahip_pcg_layout* layout, uint32_t surfels_size, float* pcg_r, const float* pcg_M,
                    float* pcg_delta, float* pcg_g, const float* pcg_p, const float* pcg_alpha_n, float* pcg_alpha_d, float* pcg_beta_n);
/* PCGStep3CUDA (B/kernels.h:468-474) */
int bahip_pcg_step3(bahip_context* ctx, const bahip_pcg_layout* layout, uint32_t surfels_size, const float* pcg_g, float* pcg_p,
                    const float* pcg_alpha_n, const float* pcg_beta_n);
/* UpdateSurfelsFromPCGDeltaCUDA (B/kernels.h:484-490), UpdateCFactorsFromPCGDeltaCUDA (B/kernels.h:492-496; the cfactor image is
 * the one of bahip_set_intrinsics) */
int bahip_update_surfels_from_pcg_delta(bahip_context* ctx, const bahip_surfels* surfels, int use_descriptor_residuals,
                                        uint32_t surfel_unknown_start_index, const float* pcg_delta);
int bahip_update_cfactors_from_pcg_delta(bahip_context* ctx, uint32_t cfactor_unknown_start_index, const float* pcg_delta);

/* ---- the value of the BA objective (kernels_cost.hip) ---------------------------------------------------------
 * Over every associated (surfel, keyframe) pair, activation flags ignored: with use_depth the depth term 1 * TukeyCost(raw, 10) (one
 * residual), with use_desc -- for the pairs whose depth-to-colour transform is valid -- the two descriptor terms 1e-2 * HuberCost(raw, 10)
 * (one pair).  Each sum is the exact sum of its binary32 terms rounded once to binary64: it does not depend on the launch shape, the
 * tile order, the surfel order or the sharding.  A non-finite term makes its keyframe's sum (and the total) NaN.
 * bahip_evaluate_cost: every bound keyframe (bahip_set_keyframes) x surfels [0, surfels_size); per_keyframe: NULL or num_keyframes
 * entries in bound order; the total is resolved from the summed limbs, not from the per-keyframe doubles.  Surfel sharding: the
 * rows of all ranks are summed as int64 (one exchange of K x 30 words; a rank with an empty shard takes part too); keyframe sharding: each rank sweeps its own keyframes and
 * the rows are summed the same way.  Every rank returns the same bits.  bahip_evaluate_frame_cost: one arbitrary frame at
 * frame_T_global (as bahip_accumulate_pose_estimation_coeffs takes it; an exchange under surfel sharding only).  Synchronise. */
typedef struct bahip_cost {
  double depth, descriptor_1, descriptor_2;
  uint64_t depth_residuals, descriptor_pairs;
} bahip_cost;
int bahip_evaluate_cost(bahip_context* ctx, int use_depth, int use_desc, const bahip_surfels* surfels, bahip_cost* total,
                        bahip_cost* per_keyframe);
int bahip_evaluate_frame_cost(bahip_context* ctx, int use_depth, int use_desc, const bahip_frame* frame, const float frame_T_global[12],
                              const bahip_surfels* surfels, bahip_cost* out);
/* Launch shape of the cost sweep (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1, keyframes
 * per launch 1 .. 256, tile_order 0 = buffer order, 1 = the sweeps' heavy-first order when there is one; 0 / -1 = the default. */
int bahip_debug_set_cost_shape(int waves, int workgroups, int slice, int tile_order);

/* ---- the value of the BA objective per surfel (kernels_surfel_cost.hip; DESIGN.md section 3, "The objective per surfel") -----------
 * For every surfel i < surfels_size: the pairs (i, k) over the bound keyframes k that bahip_evaluate_cost takes (the production
 * association rule; activation flags of surfels and keyframes ignored) and its terms.  depth, descriptor_1, descriptor_2: each the
 * exact sum of the surfel's binary32 terms rounded once to binary64 -- no dependence on the keyframe order, the launch shape, the tile
 * order or the sharding; depth_residuals, descriptor_pairs: the surfel's depth terms and descriptor pairs (0 when the residual type is
 * off).  A non-finite term makes that surfel's three sums NaN (its counts still count; no other surfel is touched).  A surfel without
 * a term -- deleted (NaN position), outside every frustum -- gets +0.0, +0.0, +0.0, 0, 0: every entry [0, surfels_size) of every
 * non-NULL plane is written by every successful call.  No bound keyframe, or both switches off: the planes are zero-filled, nothing is
 * swept.  The planes are device memory, borrowed for the call.
 * Asynchronous on the context's stream.  Surfel sharding: the call covers the shard it is given and exchanges nothing.  Keyframe
 * sharding: each rank sweeps its own keyframes; the integer words of the surfels (30 per surfel) are summed over the ranks in slices of
 * 65 536 surfels (one exchange per slice, as many on every rank; the hook's waits apply) and resolved on the device: every rank gets
 * the unsharded bits.  A failing exchange fails the call and leaves the context usable. */
typedef struct bahip_surfel_costs {      /* device pointers, borrowed; surfels_size entries each; any may be NULL */
  double *depth, *descriptor_1, *descriptor_2;
  uint32_t *depth_residuals, *descriptor_pairs;
} bahip_surfel_costs;
int bahip_evaluate_surfel_costs(bahip_context* ctx, int use_depth, int use_desc, const bahip_surfels* surfels, const bahip_surfel_costs* out);
/* Launch shape of that sweep (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1, surfels per
 * exchange under keyframe sharding (a multiple of 64), tile_order 0 = buffer order, 1 = the sweeps' heavy-first order when there is
 * one; 0 / -1 = the default. */
int bahip_debug_set_surfel_cost_shape(int waves, int workgroups, int slice_surfels, int tile_order);

/* ---- rendered views of the map (kernels_render.hip; DESIGN.md section 3, "Rendered views of the map") ------------------------------
 * The surfel buffer seen from the camera `view` at frame_T_global (3 x 4 row-major, as bahip_evaluate_frame_cost takes it): per pixel
 * the nearest surfel.  `view` follows the depth camera's conventions (pixel-corner projection; pixel-centre unprojection with
 * fx_inv = 1 / fx, cx_inv = -(cx - 0.5) / fx); it need not be a camera of the context.  Activation flags are ignored.
 * Per surfel i with a finite position (binary32, nothing contracted, either arithmetic flavour of the context): local = F p, nl = R n,
 * local.z > 0; nd = nl . local < 0 (the surfel faces the camera); pxx = fx local.x / local.z + cx, pxy likewise, both below 1e6 in
 * magnitude; (px, py) = their floors.  mode BAHIP_RENDER_POINT: the one candidate pixel (px, py) if inside the image, at depth
 * t = local.z.  mode BAHIP_RENDER_DISC (r^2 finite and > 0): rs2 = radius_factor^2 r^2, half-width h = min(max_radius_px,
 * (int)(max(fx, fy) sqrt(rs2) / local.z) + 1); the candidates are the pixels of [px - h, px + h] x [py - h, py + h] inside the image
 * (the centre pixel itself may lie outside); candidate (x, y) with the ray d through its centre is covered when den = nl . d < 0 and
 * the point t d of the surfel's plane, t = nd / den, lies within sqrt(rs2) of the surfel: |t d - local|^2 <= rs2.  A pixel outside the
 * box is not covered: max_radius_px (0 .. 16) is part of the definition.  cull_backfaces = 0 drops the two sign tests and requires
 * t > 0 instead.  A candidate with min_depth <= t <= max_depth contributes the key (bits(t) << 32) | (index_base + i); a pixel holds the
 * minimum key over its candidates -- the nearest surfel, the lower index among equal depths, whatever the launch shape, the surfel
 * order or the order of arrival -- and all ones when it has none.
 * Output planes: device memory, dense row-major width x height, borrowed for the call, any may be NULL.  key: as above; depth: t
 * (+0.0 where empty); index: index_base + i (0xFFFFFFFF where empty); normal: three floats per pixel, the winner's nl (0, 0, 0 where
 * empty); color: four bytes per pixel, the winner's colour row as stored (0 where empty; aligned to 4 bytes).  Every entry of every
 * non-NULL plane is written by every successful call; with no surfels every pixel is empty.
 * The call fails when width or height < 1, width * height > 2^26, mode is neither, max_radius_px is outside 0 .. 16, radius_factor is
 * not > 0, min_depth > max_depth, or index_base + surfels_size would reach 0xFFFFFFFF; a failed call launches nothing.
 * Asynchronous on the context's stream.  Needs no bound keyframe and no bahip_set_intrinsics.  Either sharding: nothing is exchanged;
 * a surfel shard renders the shard it is given.  Shards (or several clouds) are combined by the caller: render each with its own
 * index_base and take the elementwise minimum of the key planes. */
#define BAHIP_RENDER_POINT 0
#define BAHIP_RENDER_DISC 1
typedef struct bahip_render_options {
  int32_t mode, max_radius_px, cull_backfaces;
  float radius_factor, min_depth, max_depth;
  uint32_t index_base;
} bahip_render_options;
typedef struct bahip_render_out {        /* device pointers, borrowed; width * height pixels each; any may be NULL */
  uint64_t* key;
  float* depth;
  uint32_t* index;
  float* normal;
  uint8_t* color;
} bahip_render_out;
int bahip_render_surfels(bahip_context* ctx, const bahip_surfels* surfels, const bahip_camera* view, const float frame_T_global[12],
                         const bahip_render_options* options, const bahip_render_out* out);
/* Launch shape of the splat (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1; 0 = the default. */
int bahip_debug_set_render_shape(int waves, int workgroups);
/* The kernels bahip_render_surfels launches (scripts/render_eval.py takes their times by difference): 1 clear, 2 splat, 4 resolve,
 * or-ed; 0 = all.  With a stage missing the planes are not a rendered view. */
int bahip_debug_set_render_stages(int stages);
/* One clear and one counting splat of the same view, then a wait: counts_out = candidate tests, candidates that contributed a key
 * (one atomic each), covered pixels. */
int bahip_debug_render_census(bahip_context* ctx, const bahip_surfels* surfels, const bahip_camera* view, const float frame_T_global[12],
                              const bahip_render_options* options, unsigned long long counts_out[3]);

/* ---- residual images (kernels_residual_image.hip; DESIGN.md section 3, "Residual images") ------------------------------------------
 * The objective in image space: for one frame at frame_T_global, per pixel of the depth image, which surfel the BA associates with it
 * and with what residuals.  Not a rendered view: the association rule is the sweeps' own (depth gate, normal tests, the
 * cfactor-calibrated depth), evaluated with the context's intrinsics, depth parameters and cfactor plane (bahip_set_intrinsics).  The
 * frame is a bahip_frame with or without packed planes, handled as bahip_evaluate_frame_cost handles it.
 * For every surfel i < surfels_size the pair (i, frame) is evaluated with the production association rule (the device functions of
 * bahip_debug_evaluate_pairs and of the cost sweep, in their order); activation flags are ignored, a NaN position is never associated.
 * An associated pair has its pixel (px, py) and raw = inv_std * dot(nl, u - local).  With m = bits(raw) & 0x7fffffff the pair's key is
 * (m << 32) | (index_base + i) under BAHIP_RESIDUAL_BEST and ((0x7fffffff - m) << 32) | (index_base + i) under BAHIP_RESIDUAL_WORST.
 * A pixel's value is the MINIMUM key over its pairs, all ones when it has none: the smallest |raw| under BEST, the largest under WORST
 * (a NaN residual counts as largest), equal magnitudes to the lower index under both.  Nothing depends on the launch shape, the surfel
 * order or the order in which atomics arrive.
 * The kernels exist once, in the exact arithmetic flavour: a context set to BAHIP_ARITHMETIC_FAST launches the same code, so the image
 * is the exact flavour's association and residuals.
 * Output planes: device memory, dense row-major width x height of the depth camera, borrowed for the call, any may be NULL.
 *   key            u64   as above                                                             all ones where empty
 *   pairs          u32   associated pairs at the pixel (all of them, not only the winner)     0
 *   index          u32   the winner's index_base + i                                          0xFFFFFFFF
 *   depth_residual f32   the winner's raw, signed, in standard deviations                     +0.0
 *   inv_stddev     f32   the winner's inv_std (raw / inv_std is metres)                       +0.0
 *   color_valid    u8    1 when the winner's depth-to-colour transform is valid               0
 *   desc_residual  2 f32 the winner's r1, r2 where color_valid, else +0.0                     +0.0
 * The float planes hold, word for word, what bahip_debug_evaluate_pairs reports for (winner, frame) at [5], [7], [3], [14..15]; the
 * pixel is what it reports at [1], [2].  Every entry of every non-NULL plane is written by every successful call.
 * The call is refused when the frame, the options or the out struct is NULL, select is neither, index_base + surfels_size would reach
 * 0xFFFFFFFF, or no intrinsics are set; a refused call writes nothing and launches nothing, and the context stays usable.
 * Asynchronous on the context's stream.  Either sharding: nothing is exchanged; a surfel shard gives the planes of the shard it holds.
 * Shards are composited by the caller: the elementwise minimum of key, the sum of pairs, and per pixel the other planes of the shard
 * whose key won (the key's low word is the index). */
#define BAHIP_RESIDUAL_BEST 0
#define BAHIP_RESIDUAL_WORST 1
typedef struct bahip_residual_image_options {
  int32_t select;
  uint32_t index_base;
} bahip_residual_image_options;
typedef struct bahip_residual_image_out {   /* device pointers, borrowed; width * height pixels each; any may be NULL */
  uint64_t* key;
  uint32_t *pairs, *index;
  float *depth_residual, *inv_stddev, *desc_residual;
  uint8_t* color_valid;
} bahip_residual_image_out;
int bahip_frame_residual_image(bahip_context* ctx, const bahip_frame* frame, const float frame_T_global[12], const bahip_surfels* surfels,
                               const bahip_residual_image_options* options, const bahip_residual_image_out* out);
/* Launch shape of the sweep (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1; 0 = the default. */
int bahip_debug_set_residual_image_shape(int waves, int workgroups);
/* The kernels bahip_frame_residual_image launches (scripts/residual_image_eval.py takes their times by difference): 1 clear, 2 sweep,
 * 4 resolve, or-ed; 0 = all.  With a stage missing the planes are not a residual image. */
int bahip_debug_set_residual_image_stages(int stages);

/* ---- observed co-visibility (kernels_covisibility.hip; DESIGN.md section 3, "Observed co-visibility") ------------------------------
 * The objective as a graph over the keyframes: how many surfels the BA's own association rule pairs with both keyframe i and keyframe
 * j.  counts: device memory, borrowed for the call, K rows of pitch_words >= K words, K the number of bound keyframes
 * (bahip_set_keyframes); rows and columns in bound order, as per_keyframe of bahip_evaluate_cost.  After a successful call, for all
 * i, j < K, counts[i * pitch_words + j] is the number of surfels s < surfels_size associated with both keyframe i and keyframe j, where
 * "associated" is the pair population of bahip_evaluate_cost with the depth term on: the production association rule, a finite
 * position, activation flags of surfels and keyframes ignored.  Both triangles are written; the diagonal is the keyframe's own pair
 * count (per_keyframe[i].depth_residuals of bahip_evaluate_cost(use_depth = 1)).  The words [K, pitch_words) of a row are never
 * touched.  K = 0 succeeds and writes nothing; surfels_size = 0 writes zeros.  Sums of integers: nothing depends on the launch shape,
 * the tile order, the surfel order or the order in which atomics arrive.  The kernels exist once, in the exact arithmetic flavour: a
 * context set to BAHIP_ARITHMETIC_FAST launches the same code, so the matrix is the exact flavour's association.
 * The call is refused -- error text, nothing written, nothing launched, the context still usable -- when ctx, surfels or counts is NULL,
 * pitch_words < K, no intrinsics are set, 65 536 or more keyframes are bound, or the context is keyframe-sharded without a transport.
 * Keyframe sharding (with an all-reduce hook or an RCCL communicator): the ranks build the tile mask table with 1 + ceil(E / 1 600 000)
 * exchanges (bahip_context_set_keyframe_sharding), every rank sums the pairs of the tiles t % world == rank, and one exchange of K x K
 * int64 words gives every rank the unsharded matrix; the call then waits for the stream.  A failing exchange fails the call with a
 * message that names it ("tile mask counts", "tile mask entries", "co-visibility words"), writes nothing into counts and leaves the
 * context usable.
 * Asynchronous on the context's stream.  Surfel sharding: the call covers the shard it is given; with an all-reduce hook or an RCCL
 * communicator installed the K x K words are summed over the ranks as int64 (one exchange of K x K words; a rank with an empty shard
 * takes part too; the hook's waits apply) and every rank ends with the unsharded matrix; without one the shards' matrices are summed by
 * the caller.  A failing exchange fails the call, writes nothing into counts and leaves the context usable. */
int bahip_observed_covisibility(bahip_context* ctx, const bahip_surfels* surfels, uint32_t* counts, int pitch_words);
/* Launch shape of the sweep (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1, list_capacity
 * 1 .. 512 = the (keyframe, mask) entries a wavefront keeps in LDS before a tile is walked in passes (the overflow path), tile_order
 * 0 = buffer order, 1 = the sweeps' heavy-first order when there is one; 0 / -1 = the default. */
int bahip_debug_set_covisibility_shape(int waves, int workgroups, int list_capacity, int tile_order);
/* What bahip_observed_covisibility launches (scripts/covisibility_eval.py takes the stages' times by difference): 1 clear, 2 traversal
 * (the lists are built), 4 pair stage (the atomics and the copy of the lower triangle into the upper one; needs 2), or-ed; 0 = all.  With a stage missing the words are not the matrix. */
int bahip_debug_set_covisibility_stages(int stages);
/* Of the last bahip_observed_covisibility of this context (this rank's shard), after a wait: out[0] = (tile, keyframe) entries with a
 * non-zero mask, out[1] = atomic adds issued into counts, out[2] = tiles that took the overflow path. */
int bahip_debug_covisibility_census(bahip_context* ctx, uint64_t out[3]);

/* ---- observation lists (kernels_observations.hip; DESIGN.md section 3, "Observation lists") -----------------------------------------
 * The sparse object every form of the objective reduces: the associated (surfel, keyframe) pairs themselves, in compressed rows by
 * surfel.  A pair (s, k), s < surfels_size, k a bound keyframe, is in the table when it is in the pair population of
 * bahip_evaluate_cost with the depth term on: the production association rule, a finite position, activation flags of surfels and
 * keyframes ignored -- the matrix A of bahip_observed_covisibility.  All pointers are device memory, borrowed for the call:
 *   surfel_first    surfels_size + 1 words: surfel_first[0] = 0, surfel_first[s + 1] - surfel_first[s] = the keyframes paired with s,
 *                   surfel_first[surfels_size] = P, the number of pairs
 *   keyframes       entries [surfel_first[s], surfel_first[s + 1]): the bound-order indices of s's keyframes, ascending
 *   depth_raw       entry for entry with keyframes: the pair's raw depth residual, the word bahip_debug_evaluate_pairs reports
 *   descriptor_raw  two words per entry: r1, r2 of the pair; both 0x7fc00000 where the pair's colour pixel is not valid
 * A deleted surfel (NaN position) and a surfel no keyframe sees have an empty list.  Nothing depends on the launch shape, the tile
 * order or the staging; the surfel order moves lists with their surfels.  The kernels exist once, in the exact arithmetic flavour: a
 * context set to BAHIP_ARITHMETIC_FAST launches the same code and gets the exact flavour's association and residual bits.
 * Every successful call writes all of surfel_first, stores P (summed in 64 bits) in *pairs and waits for the stream.  The entry planes
 * are filled only when keyframes is not NULL and P <= capacity (capacity entries per plane, 2 * capacity words of descriptor_raw);
 * otherwise not a word of them is touched and the call still returns 0: compare *pairs with the capacity, allocate, call again.
 * keyframes NULL with both payload planes NULL is a count-only call.  Words of a plane beyond P are never touched.  No bound keyframe:
 * an all-zero surfel_first and P = 0.
 * The call is refused -- error text, nothing written, nothing launched, the context still usable -- when ctx, surfels, out,
 * out->surfel_first or pairs is NULL, a payload plane is given without keyframes, no intrinsics are set, 65 536 or more keyframes are
 * bound, or the context is keyframe-sharded without a transport.  A P above the pair
 * limit (2^32 - 1) fails the call after the count and before a word of surfel_first or of a plane is written.
 * Surfel sharding: the call covers the shard it is given and exchanges nothing.
 * Keyframe sharding (with an all-reduce hook or an RCCL communicator): the ranks build the tile mask table with 1 + ceil(E / 1 600 000)
 * exchanges; every rank computes P, surfel_first and keyframes from it without a further exchange; the payload planes asked for are
 * zero-filled, written by every rank for the pairs of its own keyframes and summed over the ranks as bit patterns, per plane in slices
 * of at most 4 000 000 words (P words of depth_raw, 2 P of descriptor_raw).  P is the same on every rank, and so is what the call does:
 * out->capacity and the planes asked for MUST be the same on every rank, like every argument of a keyframe-sharded call.  A failing
 * exchange ("tile mask counts", "tile mask entries", "observation payload") fails the call, leaves *pairs unwritten and the context
 * usable. */
typedef struct bahip_observations {
  uint32_t* surfel_first;   /* surfels_size + 1 words, required */
  uint16_t* keyframes;      /* capacity entries, or NULL: count only */
  float* depth_raw;         /* capacity entries or NULL */
  float* descriptor_raw;    /* 2 * capacity entries or NULL */
  uint64_t capacity;
} bahip_observations;
int bahip_surfel_observations(bahip_context* ctx, const bahip_surfels* surfels, const bahip_observations* out, uint64_t* pairs);
/* Launch shape (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1; stage_entries selects the
 * fill: -1 = direct (each lane stores into its own list), n > 0 = staged (of the entries of a 64-surfel tile, one contiguous range of
 * every plane, the first n are assembled in LDS per wavefront and written with coalesced stores, the entries beyond are stored at once;
 * waves * n * bytes per entry (2 + 4 + 8 for the planes asked for) is held to 64 KB by a smaller n), -2 = staged with the default
 * window; tile_order 0 = buffer order, 1 = the sweeps' heavy-first order when there is one; pair_limit = the largest P a call
 * accepts (at most 2^32 - 1).  0 (tile_order: -1) = the default. */
int bahip_debug_set_observations_shape(int waves, int workgroups, int stage_entries, int tile_order, uint64_t pair_limit);
/* What bahip_surfel_observations launches (scripts/surfel_observations_eval.py takes the stages' times by difference): 1 = the count
 * alone, 3 = count and scan, 7 or 0 = all (the scan needs the count, the fill needs both).  With a stage missing the words are not the
 * table; *pairs is still P. */
int bahip_debug_set_observations_stages(int stages);

/* ---- keyframe redundancy (kernels_redundancy.hip; DESIGN.md section 3, "Keyframe redundancy") ---------------------------------------
 * What a front end culls redundant keyframes by: per bound keyframe, its surfels by the number of OTHER keyframes that observe them.
 * With A the matrix of the observed co-visibility (A[k][s] = 1 when (surfel s, bound keyframe k) is in the pair population of
 * bahip_evaluate_cost with the depth term on: the production association rule, a finite position, activation flags of surfels and
 * keyframes ignored), c_s = sum over k of A[k][s] for s < surfels_size, and o = c_s - 1 the other observers of a surfel with
 * A[k][s] = 1:  hist[k * pitch_words + j] = the number of s with A[k][s] = 1 and min(o, bins - 1) = j, for j < bins, 1 <= bins <= 64.
 * hist: device memory, borrowed for the call, K rows in bound order of pitch_words >= bins words; the words [bins, pitch_words) of a
 * row are never touched.  K = 0 succeeds and writes nothing; surfels_size = 0 writes zeros.  A row's sum is the keyframe's own pair
 * count (per_keyframe[k].depth_residuals of bahip_evaluate_cost(use_depth = 1), the diagonal of bahip_observed_covisibility); for
 * j < bins - 1 column j sums to (j + 1) times the number of surfels with j + 1 observers; hist[k][0] counts the surfels only k sees.
 * Sums of integers: nothing depends on the launch shape, the tile order, the surfel order, the list capacity or the order in which
 * atomics arrive.  The kernels exist once, in the exact arithmetic flavour: a context set to BAHIP_ARITHMETIC_FAST launches the same code.
 * The call is refused -- error text, nothing written, nothing launched, the context still usable -- when ctx, surfels or hist is NULL,
 * bins is outside 1 .. 64, pitch_words < bins, no intrinsics are set, or the context is keyframe-sharded without a transport.
 * Keyframe sharding (with an all-reduce hook or an RCCL communicator; fewer than 65 536 bound keyframes): the ranks build the tile mask
 * table with 1 + ceil(E / 1 600 000) exchanges, so every rank knows every c_s; every rank attributes the tiles t % world == rank, and one
 * exchange of K x bins int64 words gives every rank the unsharded table.  A failing exchange fails the call with a message that names
 * it ("tile mask counts", "tile mask entries", "observer histogram words"), writes nothing into hist and leaves the context usable.
 * Waits for the context's stream.  Surfel sharding: a surfel lives in one shard with all its observers, so the table of a shard is
 * exact for that shard; with an all-reduce hook or an RCCL communicator installed the K x bins words are summed over the ranks as int64
 * (one exchange; a rank with an empty shard takes part too; the hook's waits apply) and every rank ends with the unsharded table;
 * without one the shards' tables are summed by the caller.  A failing exchange fails the call, writes nothing into hist and leaves
 * the context usable. */
int bahip_keyframe_observer_histogram(bahip_context* ctx, const bahip_surfels* surfels, int bins, uint32_t* hist, int pitch_words);
/* Launch shape of the sweep (test hook; results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1, list_capacity
 * 1 .. 448 = the (keyframe, mask) entries a wavefront keeps in LDS before a tile is traversed a second time (the overflow path),
 * tile_order 0 = buffer order, 1 = the sweeps' heavy-first order when there is one; 0 / -1 = the default. */
int bahip_debug_set_redundancy_shape(int waves, int workgroups, int list_capacity, int tile_order);
/* What bahip_keyframe_observer_histogram launches (scripts/keyframe_redundancy_eval.py takes the stages' times by difference): 1 clear,
 * 2 traversal (the counts and the lists are built), 4 attribution (the atomics and the second traversals; needs 2), or-ed; 0 = all.
 * With a stage missing the words are not the table. */
int bahip_debug_set_redundancy_stages(int stages);
/* Of the last bahip_keyframe_observer_histogram of this context (this rank's shard): out[0] = (tile, keyframe) entries with a non-zero
 * mask, out[1] = atomic adds issued into hist, out[2] = tiles that took a second traversal. */
int bahip_debug_redundancy_census(bahip_context* ctx, uint64_t out[3]);

/* ---- the tile mask table (kernels_tile_masks.hip; DESIGN.md section 3, "The tile mask table"): test hooks ---------------------------
 * The route of the three calls above: 0 (default) = their own kernels wherever those are allowed, the table under keyframe sharding;
 * 1 = the table on an unsharded or surfel-sharded context too: no owner filter, no exchange of the table, all tiles on this rank,
 * then the surfel shards' sum as on route 0.  The words never depend on the route. */
int bahip_debug_set_observed_structure_route(int route);
/* Launch shape of the table's kernels (results never depend on it): wavefronts per workgroup 1 .. 8, workgroups >= 1, tile_order
 * 0 = buffer order, 1 = the sweeps' heavy-first order when there is one; entry_slice = the entries, payload_slice = the 32-bit payload
 * words one exchange carries at most.  0 (tile_order: -1) = the default. */
int bahip_debug_set_tile_mask_shape(int waves, int workgroups, int tile_order, uint32_t entry_slice, uint32_t payload_slice);
/* What a call on the table route launches (scripts/observed_structure_table_eval.py takes the stages' times by difference): 1 = the
 * count sweep (with its exchange, the scan and the read-back of E), 3 = + the fill sweep (with its exchange), 7 = + the merge, 15 or
 * 0 = all.  With a stage missing the words are not the results and no table can be read back. */
int bahip_debug_set_tile_mask_stages(int stages);
/* The table the last of the three calls of this context built (host memory): tile_first ceil(surfels / 64) + 1 words, and, when the
 * E entries fit into `capacity`, keyframes and masks, E entries each, the entries of a tile contiguous and ascending by keyframe.
 * *entries = E.  Any of the three pointers may be NULL.  Refused when that call built none (route 0 without keyframe sharding, no
 * surfels, a failed exchange). */
int bahip_debug_read_tile_masks(bahip_context* ctx, uint32_t* tile_first, uint32_t* keyframes, uint64_t* masks, uint64_t capacity, uint64_t* entries);
/* Of the last call of this context on the table route: out[0] = entries this rank listed, out[1] = entries of the merged table,
 * out[2] = exchanges the call made, out[3] = tiles whose reduction this rank ran, out[4] = atomic adds it issued, out[5] = payload
 * words it wrote.  On that route the census hooks of the co-visibility and the redundancy report [0] the merged entries, [1] this
 * rank's adds, [2] 0. */
int bahip_debug_tile_mask_stats(bahip_context* ctx, uint64_t out[6]);

/* ---- the reduced camera system (kernels_rcs.hip; DESIGN.md section 3, "The reduced camera system") --------------------------------
 * The second-order structure of the joint problem over the bound keyframes: the 6K x 6K matrix S and the vector g that remain of the
 * Gauss-Newton system over poses and surfels when every surfel's unknowns are eliminated (the Schur complement on the poses).  The
 * pairs are those of bahip_evaluate_cost with the same use_depth / use_desc, at the current state; nothing is written to the state,
 * activation flags play no part.  6 unknowns per bound keyframe in bound order, in the tangent convention of the pose phase
 * (T <- T exp(-x)); no gauge is removed.  Per surfel 3 unknowns with descriptors (offset along the normal, the two descriptors), 1
 * without.  A surfel whose 3 x 3 factor is not finite or has a pivot that is not positive is degenerate: counted, held fixed.
 * S_kl = delta_kl A_k - M_kl and g_k = b_k - v_k in binary64, where A_k, b_k are the keyframe's pose equations -- the fixed-point sums
 * bahip_accumulate_pose_estimation_coeffs rounds to binary32, here as binary64 -- and M, v are sums over the surfels with the same
 * definition (fixed tile tree, two-limb fixed point): no word depends on the launch shape, the tile order, the list capacity or the
 * order atomics arrive in, and S equals its transpose bit for bit.
 * S: device memory, 6K rows of pitch_doubles >= 6K doubles (the words [6K, pitch_doubles) of a row are never touched); g: device,
 * 6K doubles; A_diag (K x 36, row-major 6 x 6 blocks) and b (K x 6): device, optional, a NULL plane is skipped.  marginalise = 0:
 * S = blockdiag(A), g = b, the surfel stage does not run.  stats: host memory, optional.  invalid != 0: a tile total or a sum was
 * beyond the fixed point's range and is missing from the words.  The call waits for the stream.
 * Refused -- error text, nothing written -- when ctx, surfels, S or g is NULL, no keyframe is bound, neither term is selected,
 * pitch_doubles < 6K, no intrinsics are set, or the context is keyframe-sharded (a rank lacks the other ranks' pairs).  Surfel
 * sharding: the call covers the shard it is given; with an all-reduce hook or an RCCL communicator the integer sums are added over
 * the ranks (one exchange) and every rank ends with the unsharded words and statistics; a failing exchange fails the call by name
 * and writes nothing.  The kernels exist once, in the exact arithmetic flavour. */
typedef struct {
  uint64_t list_entries;        /* (tile, keyframe) entries with an associated surfel */
  uint64_t pairs_visited;       /* pairs a <= b of a tile's entries that share a surfel */
  uint64_t atomics_issued;      /* 64-bit limb adds due: 12 per entry, 72 per pair a < b, 42 per pair a = b */
  uint64_t degenerate_surfels;
  uint64_t overflow_tiles;      /* tiles with more entries than the list holds: walked in passes */
  uint64_t invalid;
} bahip_rcs_stats;
int bahip_reduced_camera_system(bahip_context* ctx, int use_depth, int use_desc, int marginalise, const bahip_surfels* surfels, double* S,
                                size_t pitch_doubles, double* g, double* A_diag, double* b, bahip_rcs_stats* stats);
/* Launch shape of the sweep (test hooks; results never depend on it): wavefronts per workgroup 1 .. 4, workgroups >= 1, list_capacity
 * 1 .. 32 = the entries (keyframe, mask, Y) a wavefront keeps in LDS before a tile is walked in passes, tile_order 0 = buffer order,
 * 1 = the sweeps' heavy-first order when there is one; 0 / -1 = the default.  Refused when waves x list_capacity entries with
 * descriptors (4 620 bytes each) exceed 160 KB. */
int bahip_debug_set_rcs_shape(int waves, int workgroups, int list_capacity, int tile_order);
int bahip_debug_set_rcs_list_capacity(int list_capacity);
/* What bahip_reduced_camera_system launches (scripts/reduced_camera_system_eval.py takes the stages' times by difference): 1 the pose
 * sums, 2 the factor traversal of the surfel stage, 4 its pair stage (needs 2), 8 the resolution into the caller's planes, or-ed;
 * 0 = all.  With a stage missing the words are not the system. */
int bahip_debug_set_rcs_stages(int stages);

/* ---- step control for the PCG scheme (ours: the reference applies every update; kernels_pcg_trial.hip) --------
 * Damping.  A factor lambda >= 0 per context (default 0), Marquardt-scaled by the diagonal M the scheme assembles: for unknown u, with
 * e = 1e-8 + prior(u) as before and t = lambda * M[u] (one binary32 product), the preconditioner divides by ((M[u] + 1e-8) + prior(u))
 * + t and the matrix-free product adds (e + t) * p on the diagonal.  It holds for bahip_pcg_iteration, bahip_pcg_iteration_windowed
 * and the stage entry points (bahip_pcg_init2, bahip_pcg_step2; bahip_pcg_step3 needs none: its p does not depend on it), which stay
 * one system.  lambda = 0 launches the undamped kernels: every bit as before, in both arithmetic flavours.  Rows with M = 0 (gauge,
 * fixed poses, inactive surfels) stay untouched. */
int bahip_context_set_pcg_damping(bahip_context* ctx, float lambda);
float bahip_context_get_pcg_damping(bahip_context* ctx);
typedef struct bahip_pcg_step_control {
  float lambda_initial;           /* first damping factor (for the caller's *lambda_inout; not read here) */
  float lambda_up, lambda_down;   /* factor after a rejected / an accepted step (up >= 1, 0 < down <= 1) */
  float lambda_min, lambda_max;   /* 0 <= min <= max, finite */
  int max_trials;                 /* trial steps per outer iteration, >= 1 */
} bahip_pcg_step_control;
/* One outer iteration that does not raise the objective:
 *  1. *cost_before = bahip_evaluate_cost of the current state -- or, with have_cost_before != 0, taken as the caller gives it (the
 *     previous call's *cost_after, if nothing touched the state in between);
 *  2. everything an iteration may write is saved (surfel rows x, y, z, the normal row, the descriptor rows with descriptor residuals
 *     -- under a window the 64-surfel tiles with an active surfel only --, the keyframe table, the cfactor plane, the context's
 *     intrinsics and a), then one trial: bahip_update_surfel_normals when update_normals != 0 (the call the reference's driver makes
 *     ahead of each outer iteration, here inside the trial so that it is undone with it), bahip_pcg_iteration (windowed != 0:
 *     bahip_pcg_iteration_windowed) with damping *lambda_inout, the new intrinsics put into the context (bahip_set_intrinsics), and
 *     *cost_after = bahip_evaluate_cost;
 *  3. with f(c) = (c.depth + c.descriptor_1) + c.descriptor_2 in binary64: the trial is accepted iff f(*cost_after) is finite and
 *     f(*cost_after) < f(*cost_before).  Then lambda <- max(lambda * lambda_down, lambda_min) (binary32) and the call returns;
 *  4. else the saved words are written back -- every bit as before the call --, lambda <- min(lambda * lambda_up, lambda_max), and
 *     the next trial runs, at most max_trials.  Without an accepted trial: *accepted_out = 0, *cost_after = *cost_before, the
 *     out_* intrinsics are the context's, and *num_converged_out is what the last trial reported.
 * *trials_out: trials run; *inner_steps_out: inner steps of all of them.  Unlike bahip_pcg_iteration, an accepted step leaves the
 * new intrinsics in the context.  The context's own damping factor is not changed.
 * The objective counts associated pairs only, so a step can lower it by losing associations: compare depth_residuals and
 * descriptor_pairs of the two costs, which is what they are returned for.  No correction is made for it.
 * Sharding: the decision is taken from the total of bahip_evaluate_cost, which has the same bits on every rank, so every rank takes
 * the same branch; surfel sharding gives the accept / reject sequence, lambda and bits of one GPU.  Keyframe sharding: refused
 * (error text, context usable), windowed or not.  An error inside a trial restores the state first.  Synchronises. */
int bahip_pcg_iteration_controlled(bahip_context* ctx, const bahip_pcg_options* opt, const bahip_pcg_step_control* control, int windowed,
                                   int update_normals, const bahip_surfels* surfels, float* lambda_inout, bahip_camera* out_color_camera,
                                   bahip_camera* out_depth_camera, float* out_a, int* inner_steps_out, int* num_converged_out,
                                   int have_cost_before, bahip_cost* cost_before, bahip_cost* cost_after, int* trials_out,
                                   int* accepted_out);

/* ---- step control for the pose phase of the alternating scheme (ours: the reference takes every Gauss-Newton step;
 * kernels_pose_trial.hip) ---------------------------------------------------------------------------------------
 * Work items: every bound keyframe that is not kInactive.  Per item: the pose T, a damping factor lambda (binary32, >= 0), the
 * objective c at T and the normal equations (H, b) at T.  The objective of an item is f = (depth + descriptor_1) + descriptor_2 in
 * binary64 of its per-keyframe entry exactly as bahip_evaluate_cost(..., per_keyframe) reports it with that pose in the table.  The
 * damped step is the plain phase's solve with diagonal entry i replaced by (double)H_ii + (double)lambda * (double)H_ii; lambda = 0
 * gives every bit of the plain step.  Round 0 evaluates (H, b, c) at T; every later round computes T' = T * exp(-x(lambda)) from the
 * stored (H, b), evaluates (H', b', c') at T' in ONE fused sweep, and accepts iff f(c') is finite and f(c') < f(c).  Accepted: T, H,
 * b, c <- T', H', b', c', lambda <- max(lambda * lambda_down, lambda_min); the item is done (converged) if x passed the convergence
 * test, done (not converged) after BAHIP_MAX_POSE_ITERATIONS accepted steps.  Rejected: T, H, b, c stay word for word, lambda <-
 * min(lambda * lambda_up, lambda_max); done (not converged) after max_trials consecutive rejections.  The argument checks are those
 * of bahip_pcg_step_control. */
typedef struct bahip_pose_step_control {
  float lambda_up, lambda_down;   /* factor after a rejected / an accepted step (up >= 1, 0 < down <= 1) */
  float lambda_min, lambda_max;   /* 0 <= min <= max, finite */
  int max_trials;                 /* consecutive rejected candidates after which an item gives up, >= 1 */
} bahip_pose_step_control;
/* The pose phase under that control.  Arrays have num_keyframes entries in bound order; every output may be NULL.  lambda_inout: the
 * damping factor of every keyframe, in and out (finite, >= 0).  iterations_done: accepted steps; trials_out: candidates evaluated;
 * rejected_out: candidates rejected; cost_before_out / cost_after_out: the keyframe's cost at its pose before / after the call, the
 * bits of bahip_evaluate_cost's per-keyframe entry.  update_activation != 0: moved[] and the table's activations follow the rule of
 * bahip_estimate_keyframe_poses_and_update_activation on the pose before and after the call, and *num_converged_out counts as there.
 * A kInactive keyframe: pose and lambda untouched, both costs zeros, converged = 1.  A keyframe without an accepted step keeps every
 * word of its pose, in the table and in global_T_frame_out.  *rounds_out: sweeps made (round 0 included).
 * Surfel sharding: the cost rows travel as int64 with the normal equations (one exchange per round); every rank takes the same
 * decisions and ends with the same bits.  Keyframe sharding: refused (error text, context usable).  A non-finite or out-of-range
 * total of the normal equations fails the call as in the plain phase.  The host waits once per round. */
int bahip_estimate_keyframe_poses_controlled(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                             const bahip_pose_step_control* control, const bahip_surfels* surfels, int update_activation,
                                             float* lambda_inout, float* global_T_frame_out, int* iterations_done, int* converged, int* moved,
                                             int* trials_out, int* rejected_out, bahip_cost* cost_before_out, bahip_cost* cost_after_out,
                                             int* rounds_out, int* num_converged_out);
/* bahip_debug_pose_step with the damped diagonal (lambda = 0: its 25 words bit for bit). */
int bahip_debug_pose_step_damped(bahip_context* ctx, const float* H21_b6, const float* global_T_frame, float lambda, float* out_25);

/* ---- step control for the geometry phase of the alternating scheme (ours: the reference applies every Gauss-Newton step;
 * kernels_geometry_trial.hip, DESIGN.md section 3, "Step control of the geometry phase") -------------------------------------------------
 * With the poses frozen a surfel's cost depends on that surfel alone, so the step is kept or undone PER SURFEL, exactly.  One call:
 *  1. Normals, activation and sums: phases 1 and 2 of the three-phase geometry step (the keyframe-sharded form of
 *     bahip_update_activation_and_optimize_geometry; unsharded this rank owns every class and nothing is exchanged, under keyframe
 *     sharding the two exchanges of that form are made).  Afterwards the flags and normals are those of the plain step, bit for bit, and
 *     the class partials of the position pass hold each surfel's sums: 2 depth-only, or the 8 values a0 a1 a2 a3 a5 a6 a7 a8.  The
 *     normals update is NOT part of the trial: the controlled objective is the cost after it.
 *  2. c0 = bahip_evaluate_surfel_costs of that state (flavour and sharding as the context has them).
 *  3. The five words x, y, z, descriptor_1, descriptor_2 of every surfel are saved; every live surfel (in range, active, position not
 *     NaN) is open.
 *  4. Trials t = 0 .. max_trials - 1 with a scalar lambda_t, the same for every surfel: lambda_0 = lambda_initial, lambda_{t+1} =
 *     min(max(lambda_t * lambda_up, lambda_min), lambda_max) in binary32.  The trial solve (one thread per surfel, in the exact
 *     arithmetic whatever the flavour of the sweeps) forms the totals (p0 + p1) + p2 ... from the class partials and restates the plain
 *     solve with the diagonal damped as one binary32 product and then one add: H_ii = (a_ii + 1e-6f) + lambda * a_ii for a0, a3 and a5;
 *     depth-only the gate stays H > 1e-6f and t = -b / (H + lambda * H).  lambda = 0 gives every bit of the plain step in the exact
 *     flavour.  The candidate goes into the rows of open surfels only, under the plain step's own write conditions; at t = 0 an open
 *     surfel whose candidate equals its words bit for bit is closed with outcome 0.
 *  5. c1 = bahip_evaluate_surfel_costs of the candidate state.
 *  6. With f(c) = (depth + descriptor_1) + descriptor_2 in binary64: an open surfel is accepted iff its five candidate words are all
 *     finite, f(c1) is finite and f(c1) < f(c0) -- and, with guard_pairs, depth_residuals and descriptor_pairs of c1 are not below those
 *     of c0 (the objective counts associated pairs only: without the guard a surfel is rewarded for drifting out of sight).  Accepted:
 *     the words stay, outcome 1 + t, closed.  Rejected: the five saved words are written back, every bit, and the surfel stays open.  A
 *     non-finite candidate is rejected without looking at c1 (a NaN position would read as a deleted surfel of cost 0).
 *  7. The host reads one word per trial, the count of open surfels, and stops at 0 or after max_trials.  Surfels still open: outcome
 *     255, their saved words.  Surfels that are not live: outcome 0, none of their words touched.  Every entry of a non-NULL `outcome`
 *     (device memory, surfels_size bytes) is written by every successful call.
 * Argument checks as for bahip_pcg_step_control (error text, context usable); max_trials <= 254.  activation_surfels_size: the range
 * whose flags the normals pass decides, -1 = the flags are kept (bahip_optimize_geometry_iteration).  An error inside the loop writes the
 * saved words back before it returns.  Surfel sharding: the call covers its shard and exchanges nothing; the ranks may run different
 * numbers of trials.  Keyframe sharding: every decision is taken from bits that are equal on every rank, so every rank takes the same
 * branches, the open count needs no exchange, and every rank ends with the unsharded bits at the same class count.  The host waits
 * once per trial. */
typedef struct bahip_geometry_step_control {
  float lambda_initial;  /* damping of trial 0; finite, >= 0; 0 = the plain Gauss-Newton step */
  float lambda_up;       /* finite, > 1 */
  float lambda_min;      /* finite, > 0: the first non-zero rung */
  float lambda_max;      /* finite, >= lambda_min */
  int   max_trials;      /* >= 1 */
  int   guard_pairs;     /* != 0: a trial that loses a depth residual or a descriptor pair is rejected */
} bahip_geometry_step_control;
typedef struct bahip_geometry_step_stats {
  uint32_t candidates;      /* live surfels whose trial-0 candidate differs from their words */
  uint32_t accepted;        /* ... that ended with an accepted candidate */
  uint32_t restored;        /* ... that ended with their old words */
  uint32_t rejected_cost;   /* rejections (over all trials) by the cost test or a non-finite candidate */
  uint32_t rejected_pairs;  /* rejections whose cost test passed but the pair guard failed */
  int      trials;          /* trials run (cost sweeps made after the first one) */
} bahip_geometry_step_stats;
int bahip_optimize_geometry_iteration_controlled(bahip_context* ctx, int use_depth_residuals, int use_descriptor_residuals,
                                                 const bahip_geometry_step_control* control, const bahip_surfels* surfels,
                                                 long long activation_surfels_size, uint8_t* outcome, bahip_geometry_step_stats* stats);
/* The totals the last controlled call consumed, combined from its class partials in the defined order: host_out[q * surfels_size + i],
 * q < 2 (depth-only) or 8.  Fails when no controlled call has run on this context. */
int bahip_debug_read_geometry_sums(bahip_context* ctx, float* host_out);
/* Host wall-clock split of the last controlled call, in milliseconds, when on (off by default; each part is then followed by a wait
 * for the stream): out[0] phases 1-2, [1] the cost sweeps, [2] snapshot, solve and decide launches, [3] the per-trial read-backs. */
int bahip_debug_geometry_trial_timing(bahip_context* ctx, int enable, double out[4]);

/* ---- step control for the intrinsics step of the alternating scheme (ours: the reference applies every update;
 * kernels_intrinsics_trial.hip, DESIGN.md section 3, "Step control of the intrinsics step") ---------------------------------------------
 * The objective is exactly bahip_evaluate_cost, as in the PCG control: it counts associated pairs only, both counts are returned, no
 * correction is made.
 * The ladder of damping factors, in binary32: up(l) = l == 0 ? lambda_first : min(l * lambda_up, lambda_max); down(l): t = l / lambda_up,
 * t < lambda_first ? 0 : t.  Argument checks: lambda_first > 0, lambda_up > 1, lambda_first <= lambda_max, all finite, max_trials >= 1
 * (error text, context usable).  Defaults of the upper layers: first 1, up 4, max 1e4, 4 trials.
 * The damped system for lambda >= 0.  Per sparse cell, from the binary32-rounded cell record, D' = D + lambda * D (one product, one
 * add, not contracted); everything the plain Schur complement does with D is done with D': the test 1 / D' < 1e12, D'^-1 b2, D'^-1 B,
 * the 20 partial sums, the xor butterfly per wavefront and the ordered chain of wavefront partials added to the rounded global sums.
 * On the host, after the prior on a has been added as in the plain step, M_ii <- M_ii + (double)lambda * M_ii for the five diagonal
 * entries of the reduced 5 x 5 system and the four of the colour 4 x 4 system; then the plain step's LDL^T solves, its update formulas
 * for the cameras and a, and the back-substitution cfactor = saved_cfactor - (D'^-1 b2 - sum_c D'^-1 B_c x_c), zero where a cell's
 * observation count is 0.  lambda = 0: every output word equals the plain step's.
 * One call:
 *  1. *cost_before = bahip_evaluate_cost(use_depth, use_desc) of the current state -- or, with have_cost_before != 0, taken as the
 *     caller gives it.
 *  2. The plain step's sweep, once (its slices, its record buffers, its exchange over the ranks).  The binary64 sums stay in the
 *     context's scratch (bahip_debug_read_intrinsics_sums); the trials read them and do not change them.
 *  3. The cfactor plane is saved device to device (its cf_width x cf_height words, whatever the pitch), the cameras and a on the host.
 *  4. Trials with l = *lambda_inout, then up(l), ...: the damped Schur complement and the read-back of 34 floats, the host solves, the
 *     back-substitution from the SAVED plane into the live plane, the candidate cameras and a put into the context as
 *     bahip_set_intrinsics does, and *cost_after = bahip_evaluate_cost.
 *  5. With f(c) = (c.depth + c.descriptor_1) + c.descriptor_2 in binary64: the trial is accepted iff f(*cost_after) is finite and
 *     f(*cost_after) < f(*cost_before).  Then *lambda_inout = down(l), *lambda_accepted_out = l, the out_* arguments hold the new values,
 *     the context keeps them (unlike bahip_optimize_intrinsics, which leaves them to the caller), and the call returns.
 *  6. Otherwise the plane and the context's intrinsics are written back bit for bit and the next rung runs; the call stops after
 *     max_trials, or after a rejection at lambda_max.
 *  7. Without an accepted trial: *accepted_out = 0, *cost_after = *cost_before, the out_* arguments are the context's unchanged values
 *     and *lambda_inout = up(last l tried).
 * An error inside a trial (a failed exchange, say) restores the state before it returns.  No bound keyframe, or surfels_size == 0
 * without sharding: nothing is swept, *accepted_out = 0, *trials_out = 0.  Depth and colour updates of one call are accepted or rejected
 * together.  Synchronises.
 * Surfel sharding: the sums and the cost total have the same bits on every rank, so every rank takes the same branch and ends with one
 * GPU's bits.  Keyframe sharding: under the plain step's own condition (bahip_context_set_intrinsics_sum_classes >= ranks).
 * The sweep and the cost run in the context's arithmetic flavour; the per-cell kernels of the trials exist once, exact. */
typedef struct bahip_intrinsics_step_control {
  float lambda_first;   /* the first non-zero rung; finite, > 0 */
  float lambda_up;      /* finite, > 1 */
  float lambda_max;     /* finite, >= lambda_first */
  int   max_trials;     /* >= 1 */
} bahip_intrinsics_step_control;
int bahip_optimize_intrinsics_controlled(bahip_context* ctx, int optimize_depth_intrinsics, int optimize_color_intrinsics,
                                         int use_depth_residuals, int use_descriptor_residuals,
                                         const bahip_intrinsics_step_control* control, const bahip_surfels* surfels, float* lambda_inout,
                                         bahip_camera* out_color_camera, bahip_camera* out_depth_camera, float* out_a, int have_cost_before,
                                         bahip_cost* cost_before, bahip_cost* cost_after, int* trials_out, int* accepted_out,
                                         float* lambda_accepted_out);
/* The damped solves from the sums the last intrinsics step (plain or controlled) left in the context, at the context's intrinsics:
 * x1_out the update of the reduced 5 x 5 system, xc_out of the colour system (zeros for a system that is not optimised),
 * cells_after_out (NULL or 8 S floats; depth only) the per-cell table after the damped Schur complement {D'^-1 B0..B4, D'^-1 b2 or NaN,
 * b2, observation count}.  Nothing is applied. */
int bahip_debug_intrinsics_solve_damped(bahip_context* ctx, int optimize_depth_intrinsics, int optimize_color_intrinsics, float lambda,
                                        float x1_out[5], float xc_out[4], float* cells_after_out);
/* Host wall-clock split of the last controlled call, in milliseconds, when on (off by default; each part is then followed by a wait
 * for the stream): out[0] the sweep, [1] the cost sweeps, [2] Schur complement, solves, back-substitution and restore, [3] the waits
 * for the per-trial read-backs. */
int bahip_debug_intrinsics_trial_timing(bahip_context* ctx, int enable, double out[4]);

/* ---- test hook --------------------------------------------------------------------------------------
 * Per-pair evaluation with the production device functions (association, the three raw residuals,
 * weights, pose Jacobians, image gradients) for `count` surfel indices against one frame; 40 floats
 * per index, layout documented in badslam_amd/csrc/kernels_pose.hip.  Host in / host out. */
int bahip_debug_evaluate_pairs(bahip_context* ctx, const bahip_frame* frame, const float frame_T_global[12],
                               const bahip_surfels* surfels, const uint32_t* surfel_indices, int count, float* out);

/* Reads `count` entries of one of the PCG vectors left by the last bahip_pcg_iteration
 * (which: 0 = r, 1 = M, 2 = delta, 3 = g, 4 = p).  With max_inner_iterations = 0 that call only
 * assembles r = -J^T W F and M = diag(J^T W J) and applies no update. */
int bahip_debug_read_pcg_vector(bahip_context* ctx, int which, size_t offset, size_t count, float* out);

/* The exact sum of `count` binary32 values, rounded once to binary64 (nearest, ties to even; NaN if a value is not finite),
 * through the device code the PCG scheme's dense sums and dot products use (badslam_amd/csrc/exact_sum.h).  mode 0: every
 * term with 64-bit integer atomics on the accumulator's limbs; mode 1: per-thread limb columns in workgroup memory, folded
 * per workgroup (the path of the per-unknown kernels).  Tests compare it with math.fsum. */
int bahip_debug_exact_sum(bahip_context* ctx, const float* values, size_t count, int mode, double* out);

/* Work census of one sweep of the bound keyframes over the surfels: counts[0] = (wavefront, keyframe)
 * candidates left by frustum culling, [1] = of those with >= 1 association, [2] = associated
 * (surfel, keyframe) pairs, [3] = pairs projecting into the image. */
/* Launch shapes of the surfel sweeps, process-wide; 0 = chosen from the surfel count (default).  tile_waves (1 | 4):
 * wavefronts per 64-surfel tile in the normals / geometry passes - results are bit-identical for both (the per-surfel
 * sums are defined as four interleaved partial sums).  pose_parts (1 | 2 | 4 | 8): wavefronts sharing a
 * tile's keyframes in the pose kernel (sums merged by float atomics in any case).
 * tile_waves = 5: the geometry step's HYBRID shape (round 6; the default below 8192 tiles once the sweeps have a run order with its
 * heavy list): the heavy tiles take four wavefronts (a keyframe class each), every other tile one -- in one launch; same bits.
 * bahip_debug_geometry_hybrid_launches: how many geometry steps have run in that shape so far. */
int bahip_debug_set_launch_shapes(int tile_waves, int pose_parts);
int bahip_debug_geometry_hybrid_launches(long long* launches_out);
/* tile_waves = 6: the geometry step's FUSED route at any size (the default from the sixth iteration of a bahip_alternating_iterations
 * call on, where the one-wavefront shape runs: no forcing, >= 8192 tiles, descriptor residuals in use -- the first five iterations of a
 * call, in which nearly every normal moves, and the single-step entry points keep the classic kernel, as does the depth-only step): one walk over a tile's candidates with the old
 * normals gives the sums of the normals AND of the position pass; a surfel whose packed normal does not change is solved from them.
 * Per tile, with c changed live surfels: c = 0 held; c >= threshold: the position pass runs again in the kernel; otherwise the changed
 * surfels are left to a fix-up launch, which takes them from windows of `window` consecutive tiles, 64 at a time.  Same bits as the
 * classic shapes.  threshold 1 .. 65 (1: nothing is deferred, no fix-up launch; 65: everything is), window >= 1; 0 = the default.
 * bahip_debug_geometry_fused_stats: out = tiles held, tiles run again, tiles with deferred surfels, deferred surfels, of the context's
 * last geometry step that took the route (zeros if none did); synchronises. */
int bahip_debug_set_geometry_fused(int threshold, int window);
int bahip_debug_geometry_fused_stats(bahip_context* ctx, long long out[4]);
/* Form of the pose sweep, process-wide; results are bit-identical for all of them.  0 = chosen from the sizes (default);
 * 1 = one wavefront per surfel tile, tile totals added to the normal equations with global 64-bit integer atomics (the only form
 * for shards and for more work items than fit the table); 2 = persistent workgroups, one per compute unit, that keep the normal
 * equations of every work item in LDS and flush them once (whenever the table fits 128 KB: up to 292 work items). */
int bahip_debug_set_pose_form(int form);
/* Test / experiment hook: 0 = the sweeps take their surfel tiles in buffer order; 1 (default; BAHIP_TILE_ORDER=0 in the
 * environment switches it off too) = heavy work first, from the candidate counts of an earlier pose phase (wave_cull.h:
 * scheduled_tile).  A scheduling hint: results are bit-identical either way. */
int bahip_debug_set_tile_order(int enabled);
/* The schedule in use (test hook): *padded_tiles_out = the grid size it is valid for (0: none yet); words_out (may be NULL)
 * receives up to max_words of it: [0] heavy tiles, [8 .. 8 + 1024) their list, then one tile per regular position (padded_tiles
 * words, a permutation of the tiles), then one flag per tile (non-zero = in the heavy list). */
int bahip_debug_read_tile_schedule(bahip_context* ctx, uint32_t* padded_tiles_out, uint32_t* words_out, size_t max_words);
/* The intrinsics sweep appends its per-cell records to buffers that keep their size unless a call overflows them (the next call
 * then takes that call's largest demand + 25 %; the first call an estimate) (kernels_intrinsics.hip); records that do not fit go
 * out as atomics, with the same result.  records_per_block >= 0 fixes the size (0: no buffers, < 0:
 * automatic again) -- for the tests of the overflow path and for A/B timing.  bahip_debug_intrinsics_bin_stats: capacity and the
 * largest / total demand of the last call. */
int bahip_debug_set_intrinsics_bin_capacity(bahip_context* ctx, int records_per_block);
int bahip_debug_intrinsics_bin_stats(bahip_context* ctx, uint32_t* capacity_out, uint32_t* most_out, uint64_t* total_out);
/* The sums of the last bahip_optimize_intrinsics call, after the exchange over the ranks, rounded to binary32 as the step rounds
 * them before it forms the Schur complement: out[34] the global sums (A 0..14, b1 15..19, colour H 20..29, colour b 30..33),
 * cells_out (NULL or 8 S floats) the per-cell table {B0..B4, D, b2, observation count} per sparse cell.  These are the sums the
 * oracle's orc_intrinsics_accumulate defines (the 5 x 5 system adds the Schur complement to the first 20). */
int bahip_debug_read_intrinsics_sums(bahip_context* ctx, float out[34], float* cells_out);
/* The intrinsics step's sweep runs in slices of its schedule when the cloud is large (the per-pair records of a slice are reduced on a
 * second stream while the next slice sweeps; two buffer sets of one slice's records each): 1 .. 16 fixes the number of slices (tests on
 * small scenes), 0 = by the size of the sweep (default).  The sums do not depend on it. */
int bahip_debug_set_intrinsics_slices(bahip_context* ctx, int slices);
/* The creation batch's scan + append launch (bahip_create_surfels_for_keyframes) runs a grid handshake and therefore never launches more
 * workgroups than the device holds at once (occupancy x compute units, at most 256).  groups > 0 lowers that limit (tests: the path a
 * partitioned or masked device takes), 0 restores it.  The created surfels do not depend on it. */
int bahip_debug_set_append_groups(int groups);
/* The creation batch as a chain of one launch per keyframe (bahip_create_surfels_for_keyframes inside a lifecycle batch that knows the
 * keyframes): 1 (default; environment BAHIP_CREATION_CHAIN=0 switches it off) or 0 = four launches per keyframe as in round 5; the same
 * surfels either way.  ..._batches: how many calls have taken the chain so far (tests assert the route). */
int bahip_debug_set_creation_chain(int enabled);
int bahip_debug_creation_chain_batches(long long* batches_out);
/* A merge batch by cell lists (bahip_merge_surfels_for_keyframes inside a lifecycle batch that knows the frames; frames without BA
 * planes are allowed up to 64 per batch, each packed into a slot of its own that no bound keyframe uses, so the bound keyframes' planes
 * are never touched; a longer batch with such frames takes the pipelined form): 1 (default; BAHIP_MERGE_CELLS=0 switches it off) or
 * 0 = the pipelined insert / decide / apply sweeps of round 6's first version; the same deletions either way.  ..._batches: how many
 * calls have gone by cell lists. */
int bahip_debug_set_merge_cells(int enabled);
int bahip_debug_merge_cells_batches(long long* batches_out);
/* The LDS form holds the normal equations of at most 292 work items; longer lists are cut into slices, one launch each.  items > 0
 * makes the slices that small (tests: 200 keyframes in slices of 64), 0 restores the default. */
int bahip_debug_set_pose_lds_items(int items);
/* Shape of the LDS form (test hooks; 0 / -1 restore the defaults): wavefronts per workgroup (1 .. 16, default 16), and
 * parts_shift: 2^parts_shift wavefronts share a tile's work items (0 .. 3; -1: chosen from the grid size -- small grids, i.e.
 * shards of a multi-GPU run, split their tiles).  Integer sums: every shape gives the same bits. */
int bahip_debug_set_pose_lds_shape(int waves, int parts_shift);
/* Gauss-Newton rounds queued ahead per host wait (bahip_estimate_*: the later rounds of a phase read the number of work items
 * still iterating from device memory and do nothing when it is zero, so the host need not wait for a round before it queues
 * the next): 0 = as many as the previous phase needed (default; in bahip_alternating_iterations: what the last phases needed,
 * one less per following iteration down to two), n >= 1 = exactly n (1: wait after every round, the round-3 behaviour).  Results
 * do not depend on it. */
int bahip_debug_set_pose_rounds_ahead(int rounds);
/* 1: in bahip_alternating_iterations the launch that ends an iteration's pose phase also opens the next iteration (activation
 * window / propagation, work items) when the keyframe table has at most 1024 entries; 0 (default -- the fused launch measured
 * slower): a launch of its own does.  Results do not depend on it. */
int bahip_debug_set_fused_iteration_begin(int enabled);
/* The activation field (BAHIP_KF_*) of every entry of the DEVICE keyframe table, after waiting for the context stream: what
 * bahip_apply_activation_window, bahip_propagate_covisible_activation, the pose phase's activation update and
 * bahip_alternating_iterations left there.  num_keyframes: the number of bound keyframes.  Host code only (one copy). */
int bahip_debug_read_keyframe_activations(bahip_context* ctx, int* activation_out, int num_keyframes);
/* How the binned per-cell records of the intrinsics step are added (kernels_intrinsics.hip): 0 = into a table in LDS by
 * binary64 LDS atomics, 1 = sorted by cell in LDS and added by the thread that owns the cell, -1 = the default.  Same sums (binary64 sums of
 * binary32 terms, rounded to binary32 afterwards). */
int bahip_debug_set_intrinsics_reduce_form(int form);
/* 0: bahip_alternating_iterations reports "not handled" and callers drive the loop through the stage functions, one host wait
 * per Gauss-Newton round (BAHIP_DEVICE_LOOP=0 in the environment does the same); 1 (default): the device-driven loop.  Same bits. */
int bahip_debug_set_device_loop(int enabled);
/* Calls of bahip_alternating_iterations since the process started that the device-driven loop handled / declined (handled_out = 0:
 * switched off, keyframe sharding, a host all-reduce hook, more work items than one launch of the pose sweep takes).  bench.py prints
 * both; the test suite checks that the default configuration is handled. */
int bahip_debug_alternating_loop_calls(long long* handled_out, long long* declined_out);
/* 0: the step-1 sweep of the PCG scheme always runs one tile per wavefront with global atomics on the exact accumulators; 1
 * (default): persistent workgroups that keep the pose block of the dense head in LDS when it fits (up to ~295 keyframes) and
 * the grid fills the chip; 2: that form whenever the table fits (tests on small scenes).  Exact (integer) sums: the same bits. */
int bahip_debug_set_pcg_lds_form(int mode);
/* launches of the pose accumulation in either form since the last reset (process-wide); bench.py names the dominant kernel by it */
int bahip_debug_pose_form_launches(long long* global_form, long long* lds_form, int reset);
/* Kernel dispatches of the pose accumulate sweep since the process started (each slice of a sliced launch counts; never reset).
 * A profile of a bench run uses it to pick the dispatches of the timed region out of rocprofv3's per-dispatch rows. */
int bahip_debug_pose_kernel_dispatches(long long* dispatches_out);
/* Blocks of device and page-locked memory the library holds for itself in this process at the moment (all contexts, frame planes from
 * bahip_frame_planes_create, the scratch of a running test hook) and their bytes; memory handed to the caller (bahip_malloc_pitch,
 * bahip_host_alloc) is not counted.  A context that is destroyed gives back exactly what it took: a test reads this before and after. */
int bahip_debug_live_allocations(long long* count_out, long long* bytes_out);
/* launches of the PCG scheme's step-1 sweep by form since the process started: one tile per wavefront with global atomics on the
 * exact accumulators / persistent workgroups with the pose block of the dense head in LDS (bench.py names the kernel it measured) */
int bahip_debug_pcg_step1_form_launches(long long* tile_form, long long* lds_form);
/* The fixed-point representation of a tile total of the pose normal equations (badslam_amd/csrc/ba_device.h: hb_split):
 * out[3 i .. 3 i + 2] = limb 0 (weight 2^-32), limb 1 (weight 1), valid (0: not finite or 2^52 and beyond -- such a total is
 * not added and fails the pose estimation). */
int bahip_debug_pose_limbs(bahip_context* ctx, const float* values, size_t count, long long* out);
/* The residual Jacobian functions of the kernels (ba_device.h: jac_*) on explicit inputs, for the golden vectors of
 * tests/golden/jacobians.json.  kind: 0 depth/pose (in: nl[3] u[3] inv_std; out 6), 1 descriptor/pose (ls[3] gx gy; 6),
 * 2 descriptor/surfel (rn[3] lp[3] gx gy cfx cfy; 1), 3 depth/intrinsics (px py depth inv_std n.Frow0 n.Frow1 dot cfactor
 * raw_inv_depth exp_inv_depth corrected_inv_depth; 6), 4 descriptor/colour intrinsics (gx gy nx ny; 4). */
int bahip_debug_jacobian(bahip_context* ctx, int kind, const float* in, int n_in, float* out, int n_out);
/* One wavefront: in = 64 lanes x 28 floats; out[0..27] = totals from the halving reduction used by the pose kernel
 * (wave_reduce.h), out[28..55] = the same totals from the xor-butterfly wave_sum, out[56..63] / out[64..79] = totals of the
 * first 8 / 16 columns from the small halving reductions the PCG sweeps use (wave_reduce_small<8>, <16>). */
int bahip_debug_wave_reduce(bahip_context* ctx, const float* in_64x28, float* out_80);
/* One Gauss-Newton pose update with the device code of the pose solve (binary64 LDLT of the binary32 H (21) | b (6), x as
 * binary32, T <- T * exp(-x) with the defined sin / cos): out = x[6] | T_next[7] | frame_T_global(T_next)[12]. */
/* Counter calibration (tooling): reads a zero-filled device buffer of `bytes` with 4-byte loads, `repeats` launches of
 * read_pattern_kernel.  pattern 0: every dword once, coalesced; 1: one dword per 128-byte line.  Run under
 * `rocprofv3 --pmc FETCH_SIZE` to learn what the counter reports for a known amount of data at this access width
 * (scripts/profile_round.sh). */
int bahip_debug_read_pattern(bahip_context* ctx, size_t bytes, int pattern, int repeats);
/* rcp_exact (kind 0) / sqrt_exact (kind 1) of the device code on n host values (ba_device.h: the few-instruction exact
 * reciprocal and square root the sweeps use instead of the compiler's IEEE sequences); checked exhaustively by the tests.
 * kind 2 / 3 / 4: the defined sin / cos / atan of the SE(3) exponential and logarithm (se3_device.h). */
int bahip_debug_exact_math(bahip_context* ctx, int kind, const float* in, float* out, size_t n);
int bahip_debug_pose_step(bahip_context* ctx, const float* H21_b6, const float* global_T_frame, float* out_25);
int bahip_debug_count_pairs(bahip_context* ctx, const bahip_surfels* surfels, uint64_t* counts_out);
/* The tile cull every surfel sweep begins with (badslam_amd/csrc/wave_cull.h), as the device compiles it in the context's arithmetic
 * flavour.  Per 64-entry tile of the buffer, in buffer order (ceil(surfels_size / 64) tiles, the last one ragged): bounds_out[4 t ..
 * 4 t + 3] = the bounding sphere (centre x, y, z, inflated radius; 0, 0, 0, -1 for a tile without a live entry) of the entries whose
 * x is not NaN, and bit k % 64 of masks_out[t * ceil(K / 64) + k / 64] = may the sphere project into the depth image of bound keyframe
 * k of K, at its bound pose (the bits beyond K are zero).  Activation flags of surfels and keyframes are ignored.  Host pointers;
 * bounds_out may be NULL.  Refused, with nothing written: a NULL context, surfel struct or masks_out, intrinsics not set, no keyframe
 * bound. */
int bahip_debug_tile_cull(bahip_context* ctx, const bahip_surfels* surfels, float* bounds_out, uint64_t* masks_out);

/* ---- instrumentation ---------------------------------------------------------------------------- */
/* Time (ms, hipEvent on the context stream) and launch count of the kernels issued by the last
 * call of each stage; used by bench.py for the roofline line.  stage: 0 activation, 1 geometry,
 * 2 pose accumulate, 3 pose solve, 4 intrinsics (accumulation sweep + reduction of the binned records + Schur complement),
 * 5 the step-1 sweeps of the PCG scheme, 6 the intrinsics sweep alone, 7 the reduction of the binned records alone. */
int bahip_last_stage_time_ms(bahip_context* ctx, int stage, float* ms_out, int* launches_out);
/* enabled: 0 off; 1 = the counters cover the last call of each stage; 2 = cumulative since this call; 3 = cumulative,
 * stage 2 only (two event records per pose round instead of ten per BA iteration). */
int bahip_set_profiling(bahip_context* ctx, int enabled);
/* Work units of the launches counted above (stage 2: sum over launches of the keyframes still
 * iterating in that Gauss-Newton round; other stages: launches). */
int bahip_stage_work_units(bahip_context* ctx, int stage, long long* units_out);
/* ---- surfel shards <-> the whole cloud ------------------------------------------------------------------------------------------
 * Under surfel sharding rank r of `world` owns every world-th chunk of `chunk` consecutive surfels of ONE cloud (local surfel l is
 * global surfel ((l / chunk) * world + r) * chunk + l % chunk).  The per-surfel work of an iteration needs no other rank's
 * surfels; the surfel LIFECYCLE does -- whether a pixel is already supported, which surfels of a cell merge, where compaction
 * moves the last surfels -- and is not worth a distributed algorithm: it runs a few times per BundleAdjustment call.  For those
 * phases every rank assembles the whole cloud, runs the unsharded lifecycle code on it (identical work, identical result on
 * every rank) and takes its shard back out, so a sharded run with surfel updates ends with the bits of the unsharded run.
 *
 * bahip_gather_surfel_shards: cloud := the union of all ranks' shards.  `cloud` must have room for the sum of the shard sizes;
 * rows 0 .. 7 and the active flags travel (one int64 all-reduce per row: bit patterns are preserved), the scratch rows do not.
 * Returns the cloud's size and surfel count (the sums over the ranks) and checks that the shard sizes are those of the
 * chunk-cyclic partition.  bahip_extract_surfel_shard: shard := this rank's surfels of a cloud of cloud->surfels_size; returns
 * the shard's size.  Without a communicator / hook (one GPU) both are plain copies.  The gather's (size, count) table is summed in a
 * buffer the context keeps and travels through its page-locked stage (no allocation per call, one wait on the stream).  A gather over
 * world >= 2 ranks opens the whole-cloud phase that bahip_context_set_lifecycle_dealing deals over; the extract closes it.  The two
 * come in pairs: a host that gathers only to read the cloud should extract (or gather again) before it drives the lifecycle on other
 * buffers -- calls on any buffer other than the gathered cloud are never dealt, but the phase stays open for that cloud. */
int bahip_gather_surfel_shards(bahip_context* ctx, const bahip_surfels* shard, uint32_t shard_surfel_count, int rank, int world, uint32_t chunk,
                               bahip_surfels* cloud, uint32_t* cloud_surfels_size_out, uint32_t* cloud_surfel_count_out);
int bahip_extract_surfel_shard(bahip_context* ctx, const bahip_surfels* cloud, int rank, int world, uint32_t chunk, bahip_surfels* shard,
                               uint32_t* shard_surfels_size_out);

/* Multi-GPU accounting: how many sums over the ranks this context has requested (through the hook or RCCL) since the last
 * reset, and the bytes of the buffers summed (per rank, one direction).  A single-GPU context reports zeros. */
int bahip_exchange_stats(bahip_context* ctx, long long* calls_out, long long* bytes_out, int reset);

#ifdef __cplusplus
}
#endif
#endif  /* BADSLAM_HIP_H_ */
