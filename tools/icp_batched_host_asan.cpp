// Host AddressSanitizer run of sv_icp_batched's host code: the argument checks, the walk over tgt_offsets and the
// workspace carving, with every call failing before a HIP call is reached (no GPU needed, none touched).  Stand-alone:
// it links sv_icp.hip alone and supplies sv::set_error itself.
//
//   cd markerless-robot-camera-calibration_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -ffp-contract=off -Xarch_host -fsanitize=address \
//         -x hip ../../tools/icp_batched_host_asan.cpp sv_icp.hip -o icp_batched_host_asan && ./icp_batched_host_asan
//
// tgt_offsets is heap memory of exactly P + 1 entries, so a read past it is reported; the data pointers are never
// dereferenced on the host and point at one small heap block.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

struct Call {
  int64_t S = 100;
  int P = 3;
  std::vector<int64_t> off{0, 50, 51, 120};
  bool null_off = false, null_src = false, null_tgt = false, null_out = false, null_ws = false, normals = false, pre = false;
  int shared = 0;
  double max_distance = 0.1;
  int max_iterations = 30;
  size_t ws_bytes = 0;
  int run(void* block) const {
    // exactly sized heap copy: the library must read P + 1 entries and no more
    int64_t* o = (int64_t*)malloc(off.size() * sizeof(int64_t));
    memcpy(o, off.data(), off.size() * sizeof(int64_t));
    const float* f = (const float*)block;
    const double* d = (const double*)block;
    int rc = sv_icp_batched(null_src ? nullptr : f, S, pre ? d : nullptr, null_tgt ? nullptr : f, normals ? f : nullptr,
                            null_off ? nullptr : o, P, nullptr, shared, max_distance, max_iterations, 1e-6, 1e-6,
                            null_ws ? nullptr : block, ws_bytes, null_out ? nullptr : (double*)block, nullptr, nullptr);
    free(o);
    return rc;
  }
};

int main() {
  void* block = malloc(64);
  Call ok;
  const size_t need = sv_icp_batched_workspace_bytes(ok.S, ok.P);
  EXPECT(need > 3 * 100 * 8);
  EXPECT(sv_icp_batched_workspace_bytes(100, 4) > need && sv_icp_batched_workspace_bytes(101, 3) >= need);
  EXPECT(sv_icp_batched_workspace_bytes(-1, 3) == 0 && sv_icp_batched_workspace_bytes(100, -1) == 0);

  for (int P : {0, -1, 65, 1 << 20}) {
    Call c = ok;
    c.P = P;
    c.off.assign(1, 0);  // one entry: nothing of it may be read when P is out of range
    EXPECT(c.run(block) == SV_ERR_INVALID && strstr(g_error, "1 to 64 problems"));
  }
  for (int64_t S : {(int64_t)2, (int64_t)0, (int64_t)-1, (int64_t)1 << 24, (int64_t)1 << 40}) {
    Call c = ok;
    c.S = S;
    EXPECT(c.run(block) == SV_ERR_INVALID && strstr(g_error, "source points"));
  }
  {
    Call c = ok;
    c.max_distance = 0.0;
    EXPECT(c.run(block) == SV_ERR_INVALID && strstr(g_error, "bad parameters"));
    c = ok, c.max_distance = __builtin_nan("");
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.max_iterations = -1;
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.shared = 2;
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.null_src = true;
    EXPECT(c.run(block) == SV_ERR_INVALID && strstr(g_error, "null pointer"));
    c = ok, c.null_tgt = true;
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.null_off = true;
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.null_out = true;
    EXPECT(c.run(block) == SV_ERR_INVALID);
    c = ok, c.null_ws = true;
    EXPECT(c.run(block) == SV_ERR_INVALID);
  }
  const std::vector<std::vector<int64_t>> bad = {{1, 50, 51, 120},  {0, 50, 40, 120}, {0, 50, 50, 120}, {0, 0, 51, 120},
                                                 {0, 50, 51, 51},   {-5, 50, 51, 120}, {0, 50, 51, 51 + ((int64_t)1 << 24)},
                                                 {0, 50, 51, INT64_MAX}};
  for (const auto& off : bad) {
    Call c = ok;
    c.off = off;
    EXPECT(c.run(block) == SV_ERR_INVALID && (strstr(g_error, "target points") || strstr(g_error, "start at 0")));
  }
  // the largest batch: 65 offsets read, none beyond
  {
    Call c = ok;
    c.P = 64;
    c.off.resize(65);
    for (int p = 0; p <= 64; ++p) c.off[p] = (int64_t)p * ((1 << 24) - 1);
    c.ws_bytes = 4096;  // less than the 64 state records alone
    EXPECT(c.run(block) == SV_ERR_WORKSPACE && strstr(g_error, "workspace too small"));
  }
  // workspace carving: every size below what the five arrays take fails, for both objectives and both modes
  const auto align = [](size_t n) { return (n + 255) / 256 * 256; };
  const size_t used = align(align(align(align(3 * 152) + 1200) + 1200) + 3 * 32 * 8) + 3 * 2 * 8;
  EXPECT(used <= need);
  for (int mode = 0; mode < 4; ++mode) {
    for (size_t bytes : {(size_t)0, (size_t)1, (size_t)255, (size_t)456, (size_t)512, (size_t)1712, (size_t)2992,
                         (size_t)3072, (size_t)3839, used - 48, used - 1}) {
      Call c = ok;
      c.shared = mode & 1;
      c.normals = c.pre = (mode & 2) != 0;
      c.ws_bytes = bytes;
      EXPECT(c.run(block) == SV_ERR_WORKSPACE && strstr(g_error, "workspace too small"));
    }
  }
  free(block);
  if (g_failed)
    printf("%d check(s) FAILED\n", g_failed);
  else
    printf("sv_icp_batched host checks OK\n");
  return g_failed ? 1 : 0;
}
