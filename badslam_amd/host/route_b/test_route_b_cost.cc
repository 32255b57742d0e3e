// test_route_b_cost.cc -- the debug outputs of the Route-B shim's AccumulatePoseEstimationCoeffsCUDA (kernels_hip.cc): with debug set
// it fills residual_count and residual_sum by the reference's definition (B/kernel_opt_pose.cu:373-380: one count per associated pair
// and residual type, the depth term plus the FIRST descriptor term), taken from bahip_evaluate_frame_cost; H and b do not change.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../direct_ba.h"
#include "badslam/kernels.h"

using namespace vis;

namespace {
constexpr int W = 320, H = 240, K = 3, CELL = 2;
constexpr float kRawToFloat = 1.f / 5000.f, kBaselineFx = 40.f;

// the textured wall of test_route_b.cc
void Render(const float cam[4], float tx, float ty, Image<u16>* depth, Image<Vec3u8>* rgb) {
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const float d = 2.5f + 0.2f * std::sin(0.01f * x) * std::cos(0.013f * y);
      const float gx = (x - (cam[2] - 0.5f)) / cam[0] * d + tx, gy = (y - (cam[3] - 0.5f)) / cam[1] * d + ty;
      const bool border = x == 0 || y == 0 || x == W - 1 || y == H - 1;
      (*depth)(x, y) = border ? 65535 : (u16)(d / kRawToFloat + 0.5f);
      auto ch = [](float a, float b) { return (u8)(127.5f * (1.f + std::sin(30.f * a + 0.5f * std::sin(50.f * b)))); };
      (*rgb)(x, y) = Vec3u8(ch(gx, gy), ch(gy, d), ch(d, gx));
    }
}
int g_failures = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)
}  // namespace

int main() {
  const float camp[4] = {0.5f * H, 0.5f * H, 0.5f * W - 0.5f, 0.5f * H - 0.5f};
  const PinholeCamera4f camera(W, H, camp);
  hipStream_t stream = nullptr;
  DirectBA ba(400000, kRawToFloat, kBaselineFx, CELL, 0.8f, 1, 1, 1, camera, camera, 0, true, true, nullptr, SE3f());
  vector<shared_ptr<Keyframe>> keyframes;
  for (int k = 0; k < K; ++k) {
    Image<u16> depth(W, H); Image<Vec3u8> rgb(W, H);
    const float shift[7] = {0, 0, 0, 1, 0.15f * k, -0.1f * k, 0};
    Render(camp, shift[4], shift[5], &depth, &rgb);
    shared_ptr<Keyframe> kf(new Keyframe(stream, k, ba.depth_params(), ba.depth_camera(), depth, rgb, SE3f(shift)));
    ba.AddKeyframe(kf);
    keyframes.push_back(kf);
  }
  for (int k = 0; k < K; ++k) ba.CreateSurfelsForKeyframe(stream, /*filter_new_surfels*/ false, keyframes[k]);
  DirectBA::BACost total;
  vector<DirectBA::BACost> per;
  ba.ComputeCost(stream, &total, &per);   // (binds the scene: intrinsics and keyframes on the object's context)
  EXPECT(per.size() == (size_t)K && total.depth_residuals > 20000 && total.descriptor_pairs > 20000 && std::isfinite(total.depth));

  // keyframe 1 at a pose 4 mm off, as test_route_b.cc's pose check
  float shifted[7];
  memcpy(shifted, keyframes[1]->global_T_frame().data(), sizeof(shifted));
  shifted[4] += 0.004f;
  float F[12];
  SE3f(shifted).inverse().matrix3x4(F);
  const u32 surfels_size = ba.surfels_size();
  const CUDABuffer<float>& surfels = *ba.surfels();
  const DepthParameters dp = ba.depth_params();
  for (int kind = 0; kind < 3; ++kind) {
    const bool use_depth = kind != 2, use_desc = kind != 1;
    float H0[21], b0[6], H1[21], b1[6];
    u32 count = 0xdeadbeefu;
    float sum = -1.f;
    AccumulatePoseEstimationCoeffsCUDA(stream, use_depth, use_desc, camera, camera, dp, keyframes[1]->depth_buffer(), keyframes[1]->normals_buffer(),
                                       keyframes[1]->color_texture(), CUDAMatrix3x4(F), surfels_size, surfels, false, nullptr, nullptr, H0, b0, nullptr);
    AccumulatePoseEstimationCoeffsCUDA(stream, use_depth, use_desc, camera, camera, dp, keyframes[1]->depth_buffer(), keyframes[1]->normals_buffer(),
                                       keyframes[1]->color_texture(), CUDAMatrix3x4(F), surfels_size, surfels, true, &count, &sum, H1, b1, nullptr);
    EXPECT(memcmp(H0, H1, sizeof(H0)) == 0 && memcmp(b0, b1, sizeof(b0)) == 0);
    // the same frame through the C ABI on the object's own context
    const bahip_frame frame = keyframes[1]->ToBahipFrame();
    const bahip_surfels s = ba.SurfelsStruct(/*with_active*/ false);
    bahip_cost c;
    BAHIP_CHECKED_CALL(bahip_evaluate_frame_cost(ba.backend_context(), use_depth, use_desc, &frame, F, &s, &c));
    EXPECT(count == (u32)(c.depth_residuals + c.descriptor_pairs));
    EXPECT(sum == (float)(c.depth + c.descriptor_1));
    EXPECT(count > 1000 && sum > 0.f);
    EXPECT(use_depth ? c.depth_residuals > 0 : c.depth_residuals == 0);
    EXPECT(use_desc ? c.descriptor_pairs > 0 : c.descriptor_pairs == 0);
    printf("route B debug outputs (depth %d, descriptors %d): %u residuals, sum %.6g (frame cost: depth %.9g, descriptor 1 %.9g, 2 %.9g)\n",
           (int)use_depth, (int)use_desc, count, sum, c.depth, c.descriptor_1, c.descriptor_2);
  }
  if (g_failures == 0) printf("ROUTE_B_COST_OK\n");
  return g_failures == 0 ? 0 : 1;
}
