// ba_tum.cc -- direct bundle adjustment of a TUM-format RGB-D sequence with given initial poses.
//
// What BadSlam does around DirectBA for every keyframe (B/bad_slam.cc: PreprocessFrame, CreateKeyframe, AddKeyframe,
// RunBundleAdjustment), without the odometry front-end: the initial keyframe poses come from a trajectory file of the
// dataset (as with the reference's --import_poses).  Reads <dataset>/{calibration.txt, associated.txt, <trajectory>},
// makes every <interval>-th frame a keyframe, runs <iterations> BA calls of up to 10 iterations each with surfel
// updates, lets the frames in between follow their keyframes (trajectory deformation) and writes <out>.poses.txt (TUM
// trajectory lines of all frames, relative to the first), <out>.*_intrinsics.txt,
// <out>.deformation.txt and <out>.ply.
//
//   ba_tum <dataset_dir> <trajectory_file> <out_prefix> [--interval N] [--iterations N] [--cell N] [--max_depth M]
//          [--raw_to_float_depth S] [--pcg] [--intrinsics] [--incremental | --parallel_ba] [--save_state F] [--load_state F]
//          [--ba_call_iterations N] [--baseline_fx F] [--spatial_sort_cell C] [--row_major_creation]
//          [--bilateral_sigma_xy S] [--bilateral_sigma_inv_depth S] [--bilateral_radius_factor R] [--report_cost]
//          [--pcg_step_control] [--pose_step_control] [--geometry_step_control] [--intrinsics_step_control]
//          [--render_dir DIR [--render_mode point|disc] [--render_max_radius N] [--render_radius_factor F]]
//          [--residual_dir DIR [--residual_select best|worst]] [--covisibility_file F] [--observations_file F]
//          [--redundancy_file F [--redundancy_bins B]] [--cull_redundant_keyframes M,FRACTION]
//          [--pyramid_level_for_depth N] [--pyramid_level_for_color N] [--median_filter_and_densify_iterations N]
//          [--pose_information_file F [--pose_information_gauge ID]]
//
// --pose_information_file F [--pose_information_gauge ID]: after the keyframe redundancy, the reduced camera system of the final state
// (DirectBA::ComputeReducedCameraSystem) as a text file: one line per keyframe but the gauge keyframe ID (default: the first existing
// one), id and the six marginal standard deviations of its pose unknowns (DirectBA::PoseCovariancesOf; 17 digits), then one line per pair
// of keyframes i < j in id order: id_i id_j and the Frobenius norm of the block S_ij.  Nothing acts on the values.
// --pyramid_level_for_depth N / --pyramid_level_for_color N (0 .. 3): the BA runs on depth / colour images of 2^-N the dataset's size, with
// the dataset's cameras Scaled(1 / 2^N) (B/main.cc:457-460); every frame's depth goes through the median downscale and its colour through
// N halvings on the GPU (CreateKeyframeFromFrame).  --median_filter_and_densify_iterations N: that many rounds of the 3 x 3 median
// filter and densification on the raw depth first; not together with a depth level > 0 (as in the reference).  The calibration files
// are written from the BA cameras as they are, i.e. at the pyramid level (as B/io.cc does).  A run resumed with --load_state needs the
// options of the run that saved.
// --render_dir DIR: after the last BA call the map as every keyframe sees it (DirectBA::RenderKeyframeView: the depth camera at the
// keyframe's final pose; discs of at most 4 px unless the --render_* options say otherwise), two files per keyframe id in the existing
// directory DIR: render_%06d_color.ppm (binary P6: the surfels' colours, black where no surfel is seen) and render_%06d_depth.pgm (binary
// P5, 16 bit, big-endian, in the unit of the input depth images: min(65534, (int)(depth / raw_to_float_depth + 0.5f)), 0 = no surfel).
// --residual_dir DIR: after the last BA call (and after the saved state, the output files and the rendered views) every keyframe's residual
// image (DirectBA::KeyframeResidualImage: per pixel the associated surfel with the smallest |depth residual|, or the largest with
// --residual_select worst), in the existing directory DIR: residual_%06d_depth.pgm (binary P5, 16 bit, big-endian: 0 = no pair, else
// clamp(32768 + (int)floorf(raw * 1024 + 0.5f), 1, 65535), raw in standard deviations), residual_%06d_pairs.pgm (binary P5, 8 bit:
// min(pairs, 255)) and residuals.txt, one line per keyframe: id, explained pixels, pairs, pixels with two or more pairs, mean and RMS of
// the winners' raw (accumulated in binary64 in row-major order, printed with 17 digits).
// --covisibility_file F: after the last BA call (and after the saved state, the output files, the rendered views and the residual images)
// the observed co-visibility of the final state (DirectBA::ComputeObservedCovisibility: the surfels the association rule pairs with both
// keyframes) as a text file, one line per pair of keyframes i <= j in id order: id_i id_j shared frustum -- frustum = 1 if j is in i's
// co-visibility list (the frustum test's), else 0 -- and one summary line on the output: the pairs i < j with shared > 0, the pairs of
// the lists with shared == 0, and the pairs with shared > 0 that are in no list.  Nothing acts on the values.
// --observations_file F: after the co-visibility file, the observation lists of the final state (DirectBA::ComputeSurfelObservations: per
// surfel the keyframes the association rule pairs it with) as a text file, one line per surfel with at least one pair: surfel_index count
// id ... (the keyframe ids ascending), and one summary line on the output: the number of pairs, the histogram of the list lengths and
// the surfels whose list is shorter than min_observation_count (what the next deletion pass would remove).  Nothing acts on the lists.
// --redundancy_file F [--redundancy_bins B]: after the observation lists, the keyframe redundancy of the final state
// (DirectBA::ComputeKeyframeRedundancy with B bins, 1 .. 64, default 16) as a text file, one line per keyframe in id order: id total
// and the B words -- word j the keyframe's surfels that min(o, B - 1) = j other keyframes observe as well, total their sum.
// --cull_redundant_keyframes M,FRACTION: before the final BA call (not with --incremental), DirectBA::CullRedundantKeyframes deletes,
// one by one, the keyframes of whose surfels at least FRACTION have M (0 .. 15) or more other observers -- never the first keyframe nor
// the newest -- and the deleted ids are printed.  Off unless given: nothing else deletes a keyframe by this rule.
// --report_cost: prints the value of the BA objective (DirectBA::ComputeCost: total and the depth / descriptor sums and counts) before
// the first and after the last BA call.
// --pose_step_control: without --pcg, damped pose steps kept per keyframe only if its cost falls (DirectBA::SetPoseStepControl, its defaults)
// --geometry_step_control: without --pcg, damped geometry steps kept per surfel only if its cost falls (DirectBA::SetGeometryStepControl, its
// defaults)
// --intrinsics_step_control: with --intrinsics and without --pcg, damped intrinsics steps kept only if the objective falls
// (DirectBA::SetIntrinsicsStepControl, its defaults); the trials, the accepted steps and the damping factor are printed per BA call.
// --pcg_step_control: with --pcg, damped steps that are kept only if the objective falls (DirectBA::SetPCGStepControl, its defaults);
// the trial steps and the undone ones of the last BA call are printed at the end.
// --ba_call_iterations N: every BA call runs exactly N iterations (min = max = N) instead of 1 .. 10; the remaining options set
// what B/bad_slam_config.h makes configurable (and the two order switches of this backend): together they let a TUM-format copy of
// a test scene go through exactly the chain of tests/e2e_vga.py (tests/test_gpu_tum_pipeline.py holds the result against the
// reference's own kernels).
//
// --incremental / --parallel_ba feed the keyframes one at a time through vis::BAScheduler (ba_scheduler.h), the way
// BadSlam::ProcessFrame does: each keyframe arrives with its pose relative to the previous keyframe (taken from the
// trajectory file), plans max_num_ba_iterations_per_keyframe iterations, and these run either right away (sequential) or
// on the BA thread while the next keyframe is being prepared.  --save_state writes the backend state after BA;
// --load_state starts from such a file instead of creating keyframes and surfels (checkpoint / resume, rgbd_io.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "ba_scheduler.h"
#include "rgbd_io.h"

using namespace vis;

// ba_tum --check-dataset <dataset_dir> <trajectory_file>: parse and decode only (no GPU): prints what was read.
static int CheckDataset(const char* dataset, const char* trajectory) {
  RGBDVideo<Vec3u8, u16> video;
  if (!ReadTUMRGBDDatasetAssociatedAndCalibrated(dataset, (trajectory && *trajectory) ? trajectory : nullptr, &video)) return 1;
  const float* c = video.depth_camera()->parameters();
  printf("frames %zu width %d height %d camera %.9g %.9g %.9g %.9g\n", (size_t)video.frame_count(), video.depth_camera()->width(),
         video.depth_camera()->height(), c[0], c[1], c[2], c[3]);
  for (usize f = 0; f < video.frame_count(); ++f) {
    shared_ptr<Image<u16>> depth = video.depth_frame_mutable(f)->GetImage();
    shared_ptr<Image<Vec3u8>> color = video.color_frame_mutable(f)->GetImage();
    if (!depth || !color) return 1;
    unsigned long long depth_sum = 0, color_sum = 0;
    for (usize i = 0; i < (usize)depth->width() * depth->height(); ++i) depth_sum += depth->data()[i];
    for (usize i = 0; i < (usize)color->width() * color->height(); ++i) color_sum += color->data()[i].v[0] + 2 * color->data()[i].v[1] + 3 * color->data()[i].v[2];
    const float* v = video.depth_frame(f)->global_T_frame().data();
    printf("frame %zu %s %s depth_sum %llu color_sum %llu pose %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", (size_t)f,
           video.color_frame(f)->timestamp_string().c_str(), video.depth_frame(f)->timestamp_string().c_str(), depth_sum, color_sum, v[0], v[1],
           v[2], v[3], v[4], v[5], v[6]);
  }
  return 0;
}

// ba_tum --decode-png <file.png> <rgb|depth> <out.raw>: decodes one PNG the way the dataset reader does (8-bit colour / grey as
// RGB triples, 8- or 16-bit grey as 16-bit depth) and writes "width height\n" + the samples (u8 x 3 or native-endian u16).
// Exit code 3 = the decoder refused the file (unsupported format or malformed), 0 = decoded.
static int DecodePng(const char* path, const char* kind, const char* out_path) {
  FILE* out = nullptr;
  if (!strcmp(kind, "rgb")) {
    Image<Vec3u8> image;
    if (!ReadPNG(path, &image)) return 3;
    if (!(out = fopen(out_path, "wb"))) return 1;
    fprintf(out, "%d %d\n", image.width(), image.height());
    fwrite(image.data(), 3, (size_t)image.width() * image.height(), out);
  } else if (!strcmp(kind, "depth")) {
    Image<u16> image;
    if (!ReadPNG(path, &image)) return 3;
    if (!(out = fopen(out_path, "wb"))) return 1;
    fprintf(out, "%d %d\n", image.width(), image.height());
    fwrite(image.data(), 2, (size_t)image.width() * image.height(), out);
  } else {
    return 2;
  }
  fclose(out);
  return 0;
}

// One binary PNM file (rgbd_io has no PNG encoder): "P5" (grey) or "P6" (RGB) with the samples as given -- one byte each for max_value
// 255, two bytes big-endian for 65535.
static bool WritePNM(const std::string& path, const char* magic, int width, int height, int max_value, const vector<unsigned char>& samples) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  fprintf(f, "%s\n%d %d\n%d\n", magic, width, height, max_value);
  const bool ok = fwrite(samples.data(), 1, samples.size(), f) == samples.size();
  return (fclose(f) == 0) && ok;
}

// --render_dir: the two PNM files of one rendered keyframe view
static bool WriteRenderedView(const std::string& dir, int id, const DirectBA::RenderedView& view, float raw_to_float_depth) {
  const size_t n = (size_t)view.width * view.height;
  char name[64];
  snprintf(name, sizeof(name), "/render_%06d_color.ppm", id);
  vector<unsigned char> rgb(3 * n);
  for (size_t p = 0; p < n; ++p)
    for (int c = 0; c < 3; ++c) rgb[3 * p + c] = view.color[4 * p + c];
  if (!WritePNM(dir + name, "P6", view.width, view.height, 255, rgb)) return false;
  snprintf(name, sizeof(name), "/render_%06d_depth.pgm", id);
  vector<unsigned char> depth(2 * n);
  for (size_t p = 0; p < n; ++p) {
    unsigned value = 0;
    if (view.index[p] != 0xFFFFFFFFu) {
      const float units = view.depth[p] / raw_to_float_depth + 0.5f;
      value = units >= 65534.f ? 65534u : (unsigned)(int)units;
    }
    depth[2 * p] = (unsigned char)(value >> 8);
    depth[2 * p + 1] = (unsigned char)(value & 0xff);
  }
  return WritePNM(dir + name, "P5", view.width, view.height, 65535, depth);
}

// --residual_dir: the two PGM files of one keyframe's residual image and its line of residuals.txt -- the keyframe id, the explained
// pixels, the pairs, the pixels with two or more pairs, and the mean and RMS of the winners' raw (binary64, row-major order)
static bool WriteResidualImage(const std::string& dir, int id, const DirectBA::ResidualImage& image, FILE* summary) {
  const size_t n = (size_t)image.width * image.height;
  vector<unsigned char> depth(2 * n), pairs(n);
  unsigned long long explained = 0, total_pairs = 0, multi = 0;
  double sum = 0, sum_sq = 0;
  for (size_t p = 0; p < n; ++p) {
    unsigned value = 0;
    if (image.index[p] != 0xFFFFFFFFu) {
      const float raw = image.depth_residual[p];
      const float scaled = floorf(raw * 1024 + 0.5f);
      // (a NaN or a value beyond the int range would not convert: clamped as floats first)
      value = !(scaled > -32767.f) ? 1u : (scaled >= 32767.f ? 65535u : (unsigned)(32768 + (int)scaled));
      ++explained;
      sum += (double)raw;
      sum_sq += (double)raw * (double)raw;
    }
    depth[2 * p] = (unsigned char)(value >> 8);
    depth[2 * p + 1] = (unsigned char)(value & 0xff);
    pairs[p] = (unsigned char)std::min<uint32_t>(image.pairs[p], 255u);
    total_pairs += image.pairs[p];
    multi += image.pairs[p] >= 2 ? 1 : 0;
  }
  char name[64];
  snprintf(name, sizeof(name), "/residual_%06d_depth.pgm", id);
  if (!WritePNM(dir + name, "P5", image.width, image.height, 65535, depth)) return false;
  snprintf(name, sizeof(name), "/residual_%06d_pairs.pgm", id);
  if (!WritePNM(dir + name, "P5", image.width, image.height, 255, pairs)) return false;
  const double mean = explained ? sum / (double)explained : 0.0, rms = explained ? sqrt(sum_sq / (double)explained) : 0.0;
  return fprintf(summary, "%d %llu %llu %llu %.17g %.17g\n", id, explained, total_pairs, multi, mean, rms) > 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "--check-dataset")) return CheckDataset(argv[2], argc > 3 ? argv[3] : nullptr);
  if (argc == 5 && !strcmp(argv[1], "--decode-png")) return DecodePng(argv[2], argv[3], argv[4]);
  if (argc < 4) {
    fprintf(stderr, "usage: ba_tum <dataset_dir> <trajectory_file> <out_prefix> [--interval N] [--iterations N] [--cell N] [--max_depth M]"
                    " [--raw_to_float_depth S] [--pcg] [--intrinsics]\n");
    return 2;
  }
  const std::string dataset = argv[1], trajectory = argv[2], out = argv[3];
  int interval = 1, iterations = 10, cell = 4;
  float raw_to_float_depth = 1.0f / 5000;   // TUM RGB-D depth PNGs: 5000 units per metre
  float baseline_fx = 40.f, spatial_sort_cell = -1.f;
  int ba_call_iterations = 0;
  bool row_major_creation = false, report_cost = false, pcg_step_control = false, pose_step_control = false, geometry_step_control = false;
  bool intrinsics_step_control = false;
  bool use_pcg = false, intrinsics = false, incremental = false, parallel_ba = false;
  std::string save_state, load_state, render_dir, residual_dir, covisibility_file, observations_file, redundancy_file;
  std::string pose_information_file;
  int pose_information_gauge = -1;
  int redundancy_bins = 16, cull_min_other_observers = -1;
  double cull_min_fraction = 0.0;
  DirectBA::RenderOptions render_options;
  DirectBA::ResidualImageOptions residual_options;
  PreprocessConfig config;
  for (int i = 4; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--interval" && i + 1 < argc) interval = atoi(argv[++i]);
    else if (a == "--iterations" && i + 1 < argc) iterations = atoi(argv[++i]);
    else if (a == "--cell" && i + 1 < argc) cell = atoi(argv[++i]);
    else if (a == "--max_depth" && i + 1 < argc) config.max_depth = (float)atof(argv[++i]);
    else if (a == "--raw_to_float_depth" && i + 1 < argc) raw_to_float_depth = (float)atof(argv[++i]);
    else if (a == "--ba_call_iterations" && i + 1 < argc) ba_call_iterations = atoi(argv[++i]);
    else if (a == "--baseline_fx" && i + 1 < argc) baseline_fx = (float)atof(argv[++i]);
    else if (a == "--spatial_sort_cell" && i + 1 < argc) spatial_sort_cell = (float)atof(argv[++i]);
    else if (a == "--row_major_creation") row_major_creation = true;
    else if (a == "--report_cost") report_cost = true;
    else if (a == "--pcg_step_control") pcg_step_control = true;
    else if (a == "--pose_step_control") pose_step_control = true;
    else if (a == "--geometry_step_control") geometry_step_control = true;
    else if (a == "--intrinsics_step_control") intrinsics_step_control = true;
    else if (a == "--bilateral_sigma_xy" && i + 1 < argc) config.bilateral_filter_sigma_xy = (float)atof(argv[++i]);
    else if (a == "--bilateral_sigma_inv_depth" && i + 1 < argc) config.bilateral_filter_sigma_inv_depth = (float)atof(argv[++i]);
    else if (a == "--bilateral_radius_factor" && i + 1 < argc) config.bilateral_filter_radius_factor = (float)atof(argv[++i]);
    else if (a == "--pcg") use_pcg = true;
    else if (a == "--intrinsics") intrinsics = true;
    else if (a == "--incremental") incremental = true;
    else if (a == "--parallel_ba") incremental = parallel_ba = true;
    else if (a == "--save_state" && i + 1 < argc) save_state = argv[++i];
    else if (a == "--load_state" && i + 1 < argc) load_state = argv[++i];
    else if (a == "--render_dir" && i + 1 < argc) render_dir = argv[++i];
    else if (a == "--render_mode" && i + 1 < argc && (!strcmp(argv[i + 1], "point") || !strcmp(argv[i + 1], "disc"))) render_options.disc = !strcmp(argv[++i], "disc");
    else if (a == "--render_max_radius" && i + 1 < argc) render_options.max_radius_px = atoi(argv[++i]);
    else if (a == "--render_radius_factor" && i + 1 < argc) render_options.radius_factor = (float)atof(argv[++i]);
    else if (a == "--residual_dir" && i + 1 < argc) residual_dir = argv[++i];
    else if (a == "--residual_select" && i + 1 < argc && (!strcmp(argv[i + 1], "best") || !strcmp(argv[i + 1], "worst"))) residual_options.worst = !strcmp(argv[++i], "worst");
    else if (a == "--covisibility_file" && i + 1 < argc) covisibility_file = argv[++i];
    else if (a == "--observations_file" && i + 1 < argc) observations_file = argv[++i];
    else if (a == "--redundancy_file" && i + 1 < argc) redundancy_file = argv[++i];
    else if (a == "--redundancy_bins" && i + 1 < argc) redundancy_bins = atoi(argv[++i]);
    else if (a == "--pose_information_file" && i + 1 < argc) pose_information_file = argv[++i];
    else if (a == "--pose_information_gauge" && i + 1 < argc) pose_information_gauge = atoi(argv[++i]);
    else if (a == "--cull_redundant_keyframes" && i + 1 < argc) {
      char* rest = nullptr;
      cull_min_other_observers = (int)strtol(argv[++i], &rest, 10);
      if (rest == argv[i] || *rest != ',' || cull_min_other_observers < 0 || cull_min_other_observers > 15) {
        fprintf(stderr, "--cull_redundant_keyframes takes M,FRACTION with M in 0 .. 15\n");
        return 2;
      }
      cull_min_fraction = atof(rest + 1);
    }
    else if (a == "--pyramid_level_for_depth" && i + 1 < argc) config.pyramid_level_for_depth = atoi(argv[++i]);
    else if (a == "--pyramid_level_for_color" && i + 1 < argc) config.pyramid_level_for_color = atoi(argv[++i]);
    else if (a == "--median_filter_and_densify_iterations" && i + 1 < argc) config.median_filter_and_densify_iterations = atoi(argv[++i]);
    else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  if (intrinsics_step_control && (!intrinsics || use_pcg)) {
    fprintf(stderr, "--intrinsics_step_control needs --intrinsics and the alternating scheme (no --pcg)\n");
    return 2;
  }
  if (redundancy_bins < 1 || redundancy_bins > 64) {
    fprintf(stderr, "--redundancy_bins takes 1 .. 64\n");
    return 2;
  }
  if (cull_min_other_observers >= 0 && incremental) {
    fprintf(stderr, "--cull_redundant_keyframes runs before the final BA call of the batch mode: not with --incremental or --parallel_ba\n");
    return 2;
  }
  if (render_options.max_radius_px < 0 || render_options.max_radius_px > 16 || !(render_options.radius_factor > 0.f)) {
    fprintf(stderr, "--render_max_radius takes 0 .. 16, --render_radius_factor a factor > 0\n");
    return 2;
  }
  std::string refusal;
  if (!ValidatePreprocessConfig(config, &refusal)) {
    fprintf(stderr, "%s\n", refusal.c_str());
    return 2;
  }
  if (bahip_device_count() <= 0) { fprintf(stderr, "no HIP device (there is no CPU fallback)\n"); return 99; }

  RGBDVideo<Vec3u8, u16> video;
  if (!ReadTUMRGBDDatasetAssociatedAndCalibrated(dataset.c_str(), trajectory.c_str(), &video)) return 1;
  printf("read %zu frames, %d x %d\n", (size_t)video.frame_count(), video.depth_camera()->width(), video.depth_camera()->height());
  if (video.frame_count() == 0) return 1;
  // B/main.cc:457-460, B/bad_slam.cc:125-142: the BA's cameras are the video's at the pyramid levels
  const PinholeCamera4f ba_depth_camera = video.depth_camera()->Scaled(1.0 / (1 << config.pyramid_level_for_depth));
  const PinholeCamera4f ba_color_camera = video.color_camera()->Scaled(1.0 / (1 << config.pyramid_level_for_color));
  printf("BA resolution: depth %d x %d (pyramid level %d), colour %d x %d (pyramid level %d)\n", ba_depth_camera.width(), ba_depth_camera.height(),
         config.pyramid_level_for_depth, ba_color_camera.width(), ba_color_camera.height(), config.pyramid_level_for_color);

  hipStream_t stream = nullptr;
  BAHIP_CHECKED_CALL(bahip_stream_create(&stream));
  const int kMinObservationCount = 2;
  {
    // B/bad_slam.cc:125-142 with the defaults of B/bad_slam_config.h
    DirectBA ba(/*max_surfel_count*/ 25 * 1000 * 1000, raw_to_float_depth, baseline_fx, cell, /*surfel_merge_dist_factor*/ 0.8f,
                /*min_observation_count_while_bootstrapping_1*/ 1, /*min_observation_count_while_bootstrapping_2*/ 2, kMinObservationCount,
                ba_color_camera, ba_depth_camera, config.pyramid_level_for_color, /*use_depth_residuals*/ true,
                /*use_descriptor_residuals*/ true, nullptr, SE3f());
    if (spatial_sort_cell >= 0.f) ba.SetSpatialSortCellSize(spatial_sort_cell);
    if (row_major_creation) ba.SetRowMajorCreation(true);
    if (pose_step_control) {
      const DirectBA::PoseStepControl control;
      if (!ba.SetPoseStepControl(&control)) return 2;
    }
    if (geometry_step_control) {
      const DirectBA::GeometryStepControl control;
      if (!ba.SetGeometryStepControl(&control)) return 2;
    }
    if (intrinsics_step_control) {
      const DirectBA::IntrinsicsStepControl control;
      if (!ba.SetIntrinsicsStepControl(&control)) return 2;
    }
    if (pcg_step_control) {
      const DirectBA::PCGStepControl control;
      if (!ba.SetPCGStepControl(&control)) return 2;
    }
    vector<SE3f> original_keyframe_T_global;
    auto print_cost = [&](const char* when) {
      if (!report_cost) return;
      DirectBA::BACost c;
      ba.ComputeCost(stream, &c);
      printf("cost %s: %.9g (depth %.9g over %llu residuals, descriptor %.9g + %.9g over %llu pairs)\n", when,
             c.depth + c.descriptor_1 + c.descriptor_2, c.depth, (unsigned long long)c.depth_residuals, c.descriptor_1, c.descriptor_2,
             (unsigned long long)c.descriptor_pairs);
    };
    if (incremental) {
      BASchedulerConfig scheduler_config;
      scheduler_config.parallel_ba = parallel_ba;
      scheduler_config.use_pcg = use_pcg;
      scheduler_config.optimize_intrinsics = intrinsics;
      scheduler_config.max_num_ba_iterations_per_keyframe = iterations;
      BAScheduler scheduler(scheduler_config, &ba, &video, stream);
      SE3f previous_keyframe_pose;
      for (usize f = 0; f < video.frame_count(); f += interval) {
        // what an odometry front-end would hand over: the pose relative to the previous keyframe
        const SE3f initial_pose = video.depth_frame(f)->global_T_frame();
        const SE3f last_kf_tr_this_kf = (f == 0) ? SE3f() : previous_keyframe_pose.inverse() * initial_pose;
        previous_keyframe_pose = initial_pose;
        shared_ptr<Keyframe> kf = CreateKeyframeFromFrame(stream, config, ba, video, (int)f);
        if (!kf) return 2;
        const u32 newest_frame = (u32)std::min<usize>(f + interval - 1, video.frame_count() - 1);
        scheduler.SetLastFrameIndex((int)newest_frame);
        scheduler.AddKeyframe(kf, last_kf_tr_this_kf);
        scheduler.RunPlannedIterations(newest_frame);
      }
      scheduler.WaitForQueuedWork();
      scheduler.StopBAThreadAndWaitForIt();
      print_cost("after the last BA call");
      printf("%zu keyframes through the scheduler (%s), %d parallel iteration(s), %u surfels\n", ba.keyframes().size(),
             parallel_ba ? "BA thread" : "sequential", scheduler.parallel_iterations_done(), ba.surfel_count());
    } else {
      if (!load_state.empty()) {
        if (!LoadState(stream, config, &video, &ba, load_state)) { fprintf(stderr, "cannot load state %s\n", load_state.c_str()); return 1; }
        printf("loaded %s: %zu keyframes, %u surfels, BA iteration count %d\n", load_state.c_str(), ba.keyframes().size(), ba.surfel_count(),
               ba.ba_iteration_count());
      } else {
        for (usize f = 0; f < video.frame_count(); f += interval) {
          shared_ptr<Keyframe> kf = CreateKeyframeFromFrame(stream, config, ba, video, (int)f);
          if (!kf) return 2;
          ba.AddKeyframe(kf);
        }
      }
      printf("%zu keyframes\n", ba.keyframes().size());
      RememberKeyframePoses(&ba, &original_keyframe_T_global);   // B/bad_slam.cc:1230 (before the BA that moves them)
      print_cost("before the first BA call");
      auto cull = [&]() {
        vector<int> deleted;
        ba.CullRedundantKeyframes(stream, cull_min_other_observers, cull_min_fraction, /*max_deletions*/ (int)ba.keyframes().size(), /*protect_newest*/ 1,
                                  &deleted);
        printf("culled %zu redundant keyframe(s) (at least %g of the surfels with %d or more other observers):", deleted.size(), cull_min_fraction,
               cull_min_other_observers);
        for (int id : deleted) printf(" %d", id);
        printf("\n");
      };
      if (cull_min_other_observers >= 0 && iterations <= 0) cull();
      for (int i = 0; i < iterations; ++i) {
        if (cull_min_other_observers >= 0 && i == iterations - 1) cull();
        int done = 0;
        bool converged = false;
        ba.BundleAdjustment(stream, /*optimize_depth_intrinsics*/ intrinsics, /*optimize_color_intrinsics*/ intrinsics, /*do_surfel_updates*/ true,
                            /*optimize_poses*/ true, /*optimize_geometry*/ true, /*min_iterations*/ ba_call_iterations > 0 ? ba_call_iterations : 1,
                            /*max_iterations*/ ba_call_iterations > 0 ? ba_call_iterations : 10, use_pcg, 0,
                            (int)ba.keyframes().size() - 1, /*increase_ba_iteration_count*/ true, &done, &converged);
        printf("BA call %d: %d iteration(s)%s, %u surfels\n", i + 1, done, converged ? ", converged" : "", ba.surfel_count());
        if (pose_step_control && !use_pcg)
          printf("  pose step control: %d candidate(s), %d rejected\n", ba.last_pose_trials(), ba.last_pose_rejected_steps());
        if (geometry_step_control && !use_pcg)
          printf("  geometry step control: %lld candidate(s), %lld accepted, %lld restored, %d trial(s)\n", ba.last_geometry_candidates(),
                 ba.last_geometry_accepted(), ba.last_geometry_restored(), ba.last_geometry_trials());
        if (intrinsics_step_control)
          printf("  intrinsics step control: %d trial(s), %d accepted step(s), last accepted lambda %g, next lambda %g, objective lowered by %.9g "
                 "(smallest drop %.9g)\n", ba.last_intrinsics_trials(), ba.last_intrinsics_accepted(), (double)ba.last_intrinsics_lambda(),
                 (double)ba.intrinsics_lambda(), ba.last_intrinsics_cost_drop(), ba.last_intrinsics_smallest_drop());
        if (pcg_step_control && use_pcg)
          printf("  step control: %d trial step(s), %d undone, lambda %g\n", ba.last_pcg_trials(), ba.last_pcg_rejected_steps(), (double)ba.last_pcg_lambda());
      }
      print_cost("after the last BA call");
    }
    // keyframe poses back into the video (the reference shares the pose object between keyframe and video frame), then the
    // frames in between follow their keyframes (B/bad_slam.cc:1259-1269; the scheduler has done that after every BA)
    for (const shared_ptr<Keyframe>& kf : ba.keyframes()) {
      if (!kf) continue;
      video.depth_frame_mutable(kf->frame_index())->SetGlobalTFrame(kf->global_T_frame());
      video.color_frame_mutable(kf->frame_index())->SetGlobalTFrame(kf->global_T_frame());
    }
    if (!incremental) ExtrapolateAndInterpolateKeyframePoseChanges(0, (u32)video.frame_count() - 1, &ba, original_keyframe_T_global, &video);
    if (!save_state.empty()) {
      if (!SaveState(stream, video, ba, save_state)) { fprintf(stderr, "cannot write state %s\n", save_state.c_str()); return 1; }
      printf("wrote %s\n", save_state.c_str());
    }
    if (!SavePoses(video, /*use_depth_timestamps*/ true, /*start_frame*/ 0, out + ".poses.txt")) return 1;
    if (!SaveCalibration(stream, ba, out)) return 1;
    if (!SavePointCloudAsPLY(stream, ba, out + ".ply")) return 1;
    printf("wrote %s.{poses.txt,depth_intrinsics.txt,color_intrinsics.txt,deformation.txt,ply}\n", out.c_str());
    if (!render_dir.empty()) {
      int views = 0;
      for (const shared_ptr<Keyframe>& kf : ba.keyframes()) {
        if (!kf) continue;
        DirectBA::RenderedView view;
        ba.RenderKeyframeView(stream, (int)kf->id(), render_options, &view);
        if (!WriteRenderedView(render_dir, (int)kf->id(), view, raw_to_float_depth)) { fprintf(stderr, "cannot write the rendered views to %s\n", render_dir.c_str()); return 1; }
        ++views;
      }
      printf("wrote %d rendered view(s) (%s, at most %d px) to %s\n", views, render_options.disc ? "discs" : "points", render_options.max_radius_px,
             render_dir.c_str());
    }
    if (!residual_dir.empty()) {
      FILE* summary = fopen((residual_dir + "/residuals.txt").c_str(), "w");
      if (!summary) { fprintf(stderr, "cannot write the residual images to %s\n", residual_dir.c_str()); return 1; }
      int images = 0;
      bool ok = true;
      for (const shared_ptr<Keyframe>& kf : ba.keyframes()) {
        if (!kf || !ok) continue;
        DirectBA::ResidualImage image;
        ba.KeyframeResidualImage(stream, (int)kf->id(), residual_options, &image);
        ok = WriteResidualImage(residual_dir, (int)kf->id(), image, summary);
        ++images;
      }
      ok = (fclose(summary) == 0) && ok;
      if (!ok) { fprintf(stderr, "cannot write the residual images to %s\n", residual_dir.c_str()); return 1; }
      printf("wrote %d residual image(s) (%s pair per pixel) to %s\n", images, residual_options.worst ? "worst" : "best", residual_dir.c_str());
    }
    if (!covisibility_file.empty()) {
      vector<uint32_t> counts;
      vector<int> ids;
      ba.ComputeObservedCovisibility(stream, &counts, &ids);
      const size_t K = ids.size();
      FILE* file = fopen(covisibility_file.c_str(), "w");
      if (!file) { fprintf(stderr, "cannot write the observed co-visibility to %s\n", covisibility_file.c_str()); return 1; }
      size_t shared_pairs = 0, list_pairs_without = 0, shared_pairs_unlisted = 0;
      for (size_t i = 0; i < K; ++i) {
        const vector<int>& list = ba.keyframes()[ids[i]]->co_visibility_list();
        for (size_t j = i; j < K; ++j) {
          const uint32_t shared = counts[i * K + j];
          const bool listed = std::find(list.begin(), list.end(), ids[j]) != list.end();
          fprintf(file, "%d %d %u %d\n", ids[i], ids[j], shared, listed ? 1 : 0);
          if (i == j) continue;
          if (shared > 0) ++shared_pairs;
          if (listed && shared == 0) ++list_pairs_without;
          if (!listed && shared > 0) ++shared_pairs_unlisted;
        }
      }
      if (fclose(file) != 0) { fprintf(stderr, "cannot write the observed co-visibility to %s\n", covisibility_file.c_str()); return 1; }
      printf("wrote the observed co-visibility of %zu keyframe(s) to %s: %zu pair(s) share surfels, %zu pair(s) of the lists share none, %zu sharing pair(s) "
             "are in no list\n", K, covisibility_file.c_str(), shared_pairs, list_pairs_without, shared_pairs_unlisted);
    }
    if (!observations_file.empty()) {
      DirectBA::SurfelObservations table;
      ba.ComputeSurfelObservations(stream, &table);
      FILE* file = fopen(observations_file.c_str(), "w");
      if (!file) { fprintf(stderr, "cannot write the observation lists to %s\n", observations_file.c_str()); return 1; }
      vector<size_t> histogram;
      size_t below = 0;
      for (size_t s = 0; s + 1 < table.first.size(); ++s) {
        const uint32_t begin = table.first[s], count = table.first[s + 1] - begin;
        if (count >= histogram.size()) histogram.resize(count + 1, 0);
        ++histogram[count];
        if (count == 0) continue;
        if ((int)count < kMinObservationCount) ++below;
        fprintf(file, "%zu %u", s, count);
        for (uint32_t e = begin; e < begin + count; ++e) fprintf(file, " %d", table.keyframe_ids[table.keyframes[e]]);
        fprintf(file, "\n");
      }
      if (fclose(file) != 0) { fprintf(stderr, "cannot write the observation lists to %s\n", observations_file.c_str()); return 1; }
      printf("wrote the observation lists of %zu surfel(s) to %s: %zu pair(s), list lengths", table.first.size() - 1, observations_file.c_str(),
             table.keyframes.size());
      for (size_t c = 0; c < histogram.size(); ++c) printf(" %zu:%zu", c, histogram[c]);
      printf(", %zu observed surfel(s) below min_observation_count %d\n", below, kMinObservationCount);
    }
    if (!redundancy_file.empty()) {
      vector<uint32_t> hist;
      vector<int> ids;
      ba.ComputeKeyframeRedundancy(stream, redundancy_bins, &hist, &ids);
      FILE* file = fopen(redundancy_file.c_str(), "w");
      if (!file) { fprintf(stderr, "cannot write the keyframe redundancy to %s\n", redundancy_file.c_str()); return 1; }
      for (size_t i = 0; i < ids.size(); ++i) {
        unsigned long long total = 0;
        for (int j = 0; j < redundancy_bins; ++j) total += hist[i * (size_t)redundancy_bins + j];
        fprintf(file, "%d %llu", ids[i], total);
        for (int j = 0; j < redundancy_bins; ++j) fprintf(file, " %u", hist[i * (size_t)redundancy_bins + j]);
        fprintf(file, "\n");
      }
      if (fclose(file) != 0) { fprintf(stderr, "cannot write the keyframe redundancy to %s\n", redundancy_file.c_str()); return 1; }
      printf("wrote the keyframe redundancy of %zu keyframe(s) (%d bins) to %s\n", ids.size(), redundancy_bins, redundancy_file.c_str());
    }
    if (!pose_information_file.empty()) {
      DirectBA::ReducedCameraSystem system;
      ba.ComputeReducedCameraSystem(stream, &system);
      const size_t K = system.keyframe_ids.size(), n = 6 * K;
      const int gauge = pose_information_gauge >= 0 ? pose_information_gauge : (K ? system.keyframe_ids[0] : 0);
      DirectBA::PoseCovariances covariances;
      std::string why;
      if (!DirectBA::PoseCovariancesOf(system, gauge, &covariances, nullptr, &why)) { fprintf(stderr, "%s\n", why.c_str()); return 1; }
      FILE* file = fopen(pose_information_file.c_str(), "w");
      if (!file) { fprintf(stderr, "cannot write the pose information to %s\n", pose_information_file.c_str()); return 1; }
      for (size_t q = 0; q < covariances.keyframe_ids.size(); ++q) {
        fprintf(file, "%d", covariances.keyframe_ids[q]);
        for (int i = 0; i < 6; ++i) fprintf(file, " %.17g", sqrt(covariances.marginal[36 * q + 7 * i]));
        fprintf(file, "\n");
      }
      for (size_t i = 0; i < K; ++i)
        for (size_t j = i + 1; j < K; ++j) {
          double squares = 0.0;
          for (size_t r = 0; r < 6; ++r)
            for (size_t c = 0; c < 6; ++c) squares += system.S[(6 * i + r) * n + 6 * j + c] * system.S[(6 * i + r) * n + 6 * j + c];
          fprintf(file, "%d %d %.17g\n", system.keyframe_ids[i], system.keyframe_ids[j], sqrt(squares));
        }
      if (fclose(file) != 0) { fprintf(stderr, "cannot write the pose information to %s\n", pose_information_file.c_str()); return 1; }
      printf("wrote the pose information of %zu keyframe(s) (gauge keyframe %d) to %s: %llu list entries, %llu pairs of entries, %llu degenerate surfel(s)\n", K,
             gauge, pose_information_file.c_str(), (unsigned long long)system.list_entries, (unsigned long long)system.pairs_visited,
             (unsigned long long)system.degenerate_surfels);
    }
  }
  bahip_stream_destroy(stream);
  return 0;
}
