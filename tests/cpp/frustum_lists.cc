// The co-visibility lists DirectBA::AddKeyframe builds (badslam_amd/host/direct_ba.cc: DetermineNewKeyframeCoVisibility) for a
// sequence of keyframes, on the CPU: vis::CameraFrustum::Intersects on every pair, lists in ascending order.
// stdin: "<K> <width> <height> <fx> <fy> <cx> <cy>", then per keyframe "<min_depth> <max_depth> <qx qy qz qw tx ty tz>".
// stdout: one line per keyframe with the indices of the keyframes whose frustum intersects its own ("-" for none).
// Built and run by tests/keyframe_activation.py for tests/test_cpu_keyframe_activation.py.
#include <cstdio>
#include <vector>

#include "camera_frustum.h"

using namespace vis;

int main() {
  int K = 0, width = 0, height = 0;
  float params[4];
  if (scanf("%d %d %d %f %f %f %f", &K, &width, &height, params, params + 1, params + 2, params + 3) != 7 || K < 0) return 1;
  const PinholeCamera4f camera(width, height, params);
  std::vector<CameraFrustum> frustums;
  for (int k = 0; k < K; ++k) {
    float min_depth, max_depth, T[7];
    if (scanf("%f %f", &min_depth, &max_depth) != 2) return 1;
    for (int c = 0; c < 7; ++c) if (scanf("%f", T + c) != 1) return 1;
    frustums.emplace_back(camera, min_depth, max_depth, SE3f(T));
  }
  for (int a = 0; a < K; ++a) {
    bool any = false;
    for (int b = 0; b < K; ++b) {
      // (a new keyframe is tested against the ones before it: the pair (a, b), a > b, is decided by a's frustum)
      if (a == b || !(a > b ? frustums[a].Intersects(frustums[b]) : frustums[b].Intersects(frustums[a]))) continue;
      printf("%s%d", any ? " " : "", b);
      any = true;
    }
    printf("%s\n", any ? "" : "-");
  }
  return 0;
}
