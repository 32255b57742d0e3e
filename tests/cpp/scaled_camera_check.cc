// Prints vis::PinholeCamera4f::Scaled(1 / 2^level) (badslam_amd/host/libvis_min.h) for cameras read from stdin, one
// "fx fy cx cy width height level" per line: the four parameters as hexadecimal binary32, then width and height.
// tests/test_cpu_frame_ingest.py compares them with the camera-scaling rule of tests/frame_ingest.py.
#include <cstdio>
#include <cstring>

#include "libvis_min.h"

int main() {
  float p[4];
  int width, height, level;
  while (scanf("%f %f %f %f %d %d %d", &p[0], &p[1], &p[2], &p[3], &width, &height, &level) == 7) {
    const vis::PinholeCamera4f scaled = vis::PinholeCamera4f(width, height, p).Scaled(1.0 / (1 << level));
    for (int i = 0; i < 4; ++i) { unsigned bits; memcpy(&bits, &scaled.parameters()[i], 4); printf("%08x ", bits); }
    printf("%d %d\n", scaled.width(), scaled.height());
  }
  return 0;
}
