// Host AddressSanitizer / UBSan run of the host code of sv_lens_rays and sv_rgbd_cloud_lens: the argument checks and the
// reads of cam_host (4 and 21 doubles), dist_host and color_dist_host (8 doubles each), with every call failing before a
// HIP call is reached (no GPU needed, none touched).  Stand-alone: it links sv_rgbd.hip alone and supplies sv::set_error
// itself.  Run it on a CPU machine only.
//
//   cd markerless-robot-camera-calibration_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -ffp-contract=off \
//         -Xarch_host -fsanitize=address,undefined -x hip ../../tools/rgbd_lens_host_asan.cpp sv_rgbd.hip \
//         -o rgbd_lens_host_asan && ./rgbd_lens_host_asan
//
// The host arrays are heap blocks of exactly the documented sizes, so a read past any of them is reported; the device
// pointers are never dereferenced on the host and point at one small heap block.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "sv_hip.h"

static char g_error[512];
namespace sv {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}
}  // namespace sv

static int g_failed = 0;
#define EXPECT(cond)                                                                    \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_error);      \
      ++g_failed;                                                                       \
    }                                                                                   \
  } while (0)

static bool said(const char* word) { return strstr(g_error, word) != nullptr; }

// an exactly-sized heap copy, or NULL for an empty vector
static double* heap(const std::vector<double>& v) {
  if (v.empty()) return nullptr;
  double* p = (double*)malloc(v.size() * sizeof(double));
  memcpy(p, v.data(), v.size() * sizeof(double));
  return p;
}

static int rays(void* p, std::vector<double> cam, std::vector<double> dist, int64_t H, int64_t W, bool null_out = false) {
  double *c = heap(cam), *d = heap(dist);
  g_error[0] = 0;
  const int rc = sv_lens_rays(c, d, H, W, null_out ? nullptr : (double*)p, nullptr);
  free(c);
  free(d);
  return rc;
}

struct Cloud {
  void* p;
  int64_t Hd = 48, Wd = 64, Hc = 60, Wc = 80;
  std::vector<double> cam{58.0, 58.5, 31.5, 23.5, 52.0, 52.5, 40.2, 29.7, 1, 0, 0, 0.025, 0, 1, 0, 0, 0, 0, 1, 0, 0.001};
  std::vector<double> dist;  // empty = NULL
  int flags = 0;
  bool depth_rays = false, color_rays = false, null_count = false;
  size_t ws_bytes = 0;

  int run() const {
    double *c = heap(cam), *d = heap(dist);
    g_error[0] = 0;
    const int rc = sv_rgbd_cloud_lens(p, SV_DEPTH_U16, Hd, Wd, 2 * Wd, nullptr, Hc, Wc, 0, nullptr, c, 0, 0, flags, nullptr,
                                      nullptr, p, ws_bytes, (float*)p, nullptr, nullptr, nullptr, nullptr,
                                      null_count ? nullptr : (int64_t*)p, depth_rays ? (const double*)p : nullptr,
                                      color_rays ? (const double*)p : nullptr, d, nullptr);
    free(c);
    free(d);
    return rc;
  }
};

int main() {
  void* p = malloc(64);
  const double nan = std::nan(""), inf = INFINITY;
  const std::vector<double> cam4{52.0, 52.5, 40.2, 29.7}, zero8(8, 0.0), kinect{0.159, -0.284, -0.003, 0.003, 0, 0, 0, 0};

  // sv_lens_rays
  EXPECT(rays(p, {}, kinect, 60, 80) == SV_ERR_INVALID && said("null pointer") && said("sv_lens_rays"));
  EXPECT(rays(p, cam4, {}, 60, 80) == SV_ERR_INVALID && said("null pointer"));
  EXPECT(rays(p, cam4, kinect, 60, 80, true) == SV_ERR_INVALID && said("null pointer"));
  EXPECT(rays(p, cam4, kinect, 0, 80) == SV_ERR_INVALID && said("at least 1"));
  EXPECT(rays(p, cam4, kinect, 60, -1) == SV_ERR_INVALID && said("at least 1"));
  EXPECT(rays(p, cam4, kinect, 4097, 4096) == SV_ERR_INVALID && said("2^24"));
  EXPECT(rays(p, cam4, kinect, INT64_MAX, INT64_MAX) == SV_ERR_INVALID && said("2^24"));  // no overflowing product
  for (int k = 0; k < 4; ++k)
    for (double bad : {nan, inf, -inf}) {
      std::vector<double> c = cam4;
      c[k] = bad;
      EXPECT(rays(p, c, kinect, 60, 80) == SV_ERR_INVALID && said("not finite"));
    }
  for (int k = 0; k < 8; ++k)
    for (double bad : {nan, inf, -inf}) {
      std::vector<double> d = kinect;
      d[k] = bad;
      EXPECT(rays(p, cam4, d, 60, 80) == SV_ERR_INVALID && said("not finite"));
    }
  for (int k = 0; k < 2; ++k) {
    std::vector<double> c = cam4;
    c[k] = 0.0;
    EXPECT(rays(p, c, zero8, 60, 80) == SV_ERR_INVALID && said("focal length"));
  }

  // sv_rgbd_cloud_lens: what it adds to sv_rgbd_cloud's checks (tools/rgbd_host_asan.cpp drives those)
  Cloud c{p};
  c.ws_bytes = sv_rgbd_cloud_workspace_bytes(c.Hd, c.Wd, c.Hc, c.Wc);
  {
    Cloud k = c;
    k.dist = kinect;
    EXPECT(k.run() == SV_ERR_INVALID && said("color_rays") && said("sv_rgbd_cloud_lens"));
    k.depth_rays = true;
    EXPECT(k.run() == SV_ERR_INVALID && said("color_rays"));
  }
  {
    Cloud k = c;
    k.Hd = k.Hc;
    k.Wd = k.Wc;
    k.flags = SV_RGBD_ALIGNED;
    k.depth_rays = true;
    EXPECT(k.run() == SV_ERR_INVALID && said("SV_RGBD_ALIGNED"));
    k.depth_rays = false;
    k.color_rays = true;
    k.dist = kinect;
    EXPECT(k.run() == SV_ERR_INVALID && said("SV_RGBD_ALIGNED"));
  }
  for (int i = 0; i < 8; ++i)
    for (double bad : {nan, inf, -inf}) {
      Cloud k = c;
      k.color_rays = true;
      k.dist = kinect;
      k.dist[i] = bad;
      EXPECT(k.run() == SV_ERR_INVALID && said("not finite"));
    }
  {
    Cloud k = c;  // the earlier checks still come first, and with this entry's name
    k.color_rays = true;
    k.null_count = true;
    EXPECT(k.run() == SV_ERR_INVALID && said("null pointer") && said("sv_rgbd_cloud_lens"));
    k.null_count = false;
    k.cam[20] = 0.0;
    EXPECT(k.run() == SV_ERR_INVALID && said("depth_scale"));
    k = c;
    k.color_rays = k.depth_rays = true;
    k.dist = kinect;
    k.ws_bytes -= 1;
    EXPECT(k.run() == SV_ERR_WORKSPACE && said("sv_rgbd_cloud_lens: workspace too small"));
  }
  free(p);
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("rgbd_lens_host_asan: all host-side refusals as documented, no sanitizer report\n");
  return 0;
}
