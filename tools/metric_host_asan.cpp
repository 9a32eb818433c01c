// Host AddressSanitizer / UBSan run of the host code of sv_ms_mine, sv_triplet_margin and sv_mined_triplet_step: the
// argument checks and the workspace arithmetic of sv_metric_workspace_bytes, with every call failing before a HIP call is
// reached (no GPU needed, none touched).  Stand-alone: it links sv_metric.hip alone and supplies sv::set_error itself.  Run
// it on a CPU machine only.
//
//   cd markerless-robot-camera-calibration_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I../../include -I. -ffp-contract=off \
//         -Xarch_host -fsanitize=address,undefined -x hip ../../tools/metric_host_asan.cpp sv_metric.hip \
//         -o metric_host_asan && ./metric_host_asan
//
// The device pointers are never dereferenced on the host and point at one small heap block.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

struct Args {
  void* p;
  void* x;
  void* labels;
  void* ws;
  void* out;  // every output and list pointer
  int64_t ld = 8, max_pos = -1, max_neg = -1, cap_pos = 12, cap_neg = 12;
  int B = 4, E = 8;
  size_t ws_bytes = (size_t)1 << 40;
  explicit Args(void* q) : p(q), x(q), labels(q), ws(q), out(q) {}

  int mine() const {
    g_error[0] = 0;
    return sv_ms_mine((const float*)x, ld, B, E, (const int64_t*)labels, 0.1, max_pos, max_neg, ws, ws_bytes, (int64_t*)out,
                      (int64_t*)out, cap_pos, (int64_t*)out, (int64_t*)out, cap_neg, (int64_t*)out, (int32_t*)out, nullptr);
  }
  int loss() const {
    g_error[0] = 0;
    return sv_triplet_margin((const float*)x, ld, B, E, (const int64_t*)out, (const int64_t*)out, cap_pos, (const int64_t*)out,
                             (const int64_t*)out, cap_neg, (const int64_t*)labels, 0.05, ws, ws_bytes, (double*)out, nullptr,
                             (int64_t*)out, (int32_t*)out, nullptr);
  }
  int step() const {
    g_error[0] = 0;
    return sv_mined_triplet_step((const float*)x, ld, B, E, (const int64_t*)labels, 0.1, 0.05, max_pos, max_neg, ws, ws_bytes,
                                 (double*)out, nullptr, (int64_t*)out, (int64_t*)out, (int32_t*)out, nullptr);
  }
};

int main() {
  void* p = malloc(64);
  typedef int (Args::*Entry)() const;
  const Entry entries[3] = {&Args::mine, &Args::loss, &Args::step};
  const char* names[3] = {"sv_ms_mine", "sv_triplet_margin", "sv_mined_triplet_step"};
  for (int k = 0; k < 3; ++k) {
    const Entry f = entries[k];
    Args a(p);
    a.B = 0;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("1 to 1024 embeddings") && said(names[k]));
    a.B = SV_MAX_BATCH + 1;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("1 to 1024 embeddings"));
    a.B = INT32_MAX;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("1 to 1024 embeddings"));
    a = Args(p);
    a.E = 0;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("E >= 1"));
    a.E = INT32_MIN;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("E >= 1"));
    a = Args(p);
    a.ld = 7;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("ld >= E"));
    a.ld = INT64_MIN;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("ld >= E"));
    a = Args(p);
    a.x = nullptr;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("null pointer"));
    a = Args(p);
    a.labels = nullptr;  // sv_triplet_margin: its counts pointer
    EXPECT((a.*f)() == SV_ERR_INVALID && said("null pointer"));
    a = Args(p);
    a.out = nullptr;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("null pointer"));
    a = Args(p);
    a.ws = nullptr;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("null pointer"));
    a = Args(p);
    a.ws_bytes = sv_metric_workspace_bytes(a.B, a.E) - 1;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("workspace too small") && said(names[k]));
    a.ws_bytes = 0;
    EXPECT((a.*f)() == SV_ERR_INVALID && said("workspace too small"));
    // the largest shape: the size arithmetic stays inside size_t and the check still refuses one byte less
    a = Args(p);
    a.B = SV_MAX_BATCH;
    a.E = INT32_MAX;
    a.ld = INT32_MAX;
    a.ws_bytes = sv_metric_workspace_bytes(a.B, a.E) - 1;
    EXPECT(sv_metric_workspace_bytes(a.B, a.E) > (size_t)2 * 8 * SV_MAX_BATCH * (size_t)INT32_MAX);
    EXPECT((a.*f)() == SV_ERR_INVALID && said("workspace too small"));
    if (k != 1) {
      a = Args(p);
      a.max_pos = -2;
      EXPECT((a.*f)() == SV_ERR_INVALID && said("caps >= -1"));
      a = Args(p);
      a.max_neg = INT64_MIN;
      EXPECT((a.*f)() == SV_ERR_INVALID && said("caps >= -1"));
    }
    if (k != 2) {
      a = Args(p);
      a.cap_pos = -1;
      EXPECT((a.*f)() == SV_ERR_INVALID && said("capacities"));
      a = Args(p);
      a.cap_neg = INT64_MIN;
      EXPECT((a.*f)() == SV_ERR_INVALID && said("capacities"));
    }
  }
  {
    Args a(p);  // the pair lists of sv_triplet_margin are bounded so that cap_pos + cap_neg cannot overflow
    a.cap_pos = INT64_MAX;
    a.cap_neg = INT64_MAX;
    EXPECT(a.loss() == SV_ERR_INVALID && said("capacities"));
  }
  EXPECT(sv_metric_workspace_bytes(0, 0) == sv_metric_workspace_bytes(1, 1));
  EXPECT(sv_metric_workspace_bytes(-5, -5) == sv_metric_workspace_bytes(1, 1));
  EXPECT(sv_metric_workspace_bytes(INT32_MAX, 8) == sv_metric_workspace_bytes(SV_MAX_BATCH, 8));
  free(p);
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("metric_host_asan: all host-side refusals as documented, no sanitizer report\n");
  return 0;
}
