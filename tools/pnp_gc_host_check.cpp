// The host half of csrc/pnp_gc.hip -- argument checks and scratch sizing -- exercised by a stand-alone program, so that it can be
// built under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc gc_host_check`, then run
// checkerpose_amd/csrc/gc_host_check).  Every call below is refused before any launch: no device is needed, nothing is loaded
// into Python.  Exit status 0 = every refusal and every size as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
  } while (0)

int main() {
  alignas(16) static unsigned char buf[256];
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  int64_t* i64 = (int64_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  const int N = 512;
  // cp_radius_graph_count / _fill
  EXPECT(cp_radius_graph_count(nullptr, nullptr, 1, N, 20.0, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_count(nullptr, f, 0, N, 20.0, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_count(nullptr, f, 1, 4097, 20.0, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_count(nullptr, f, 1, N, -1.0, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_count(nullptr, f, 1, N, NAN, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_count(nullptr, f, 1, N, 20.0, (int32_t*)(buf + 2), i32), CP_ERR_ALIGN);
  EXPECT(cp_radius_graph_fill(nullptr, f, 1, N, 20.0, i32, nullptr, i32, 10), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_fill(nullptr, f, 1, N, 20.0, i32, i64, i32, -1), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_fill(nullptr, f, 2, N, 20.0, i32, i64, i32, 2ll * (1ll << 21) + 1), CP_ERR_INVALID);
  EXPECT(cp_radius_graph_fill(nullptr, f, 1, N, 20.0, i32, (int64_t*)(buf + 4), i32, 10), CP_ERR_ALIGN);
  // cp_graphcut_label
  EXPECT(cp_graphcut_label(nullptr, nullptr, i32, i32, 1, N, 100, 6554, u8, i64, i32, nullptr, buf, 400), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 1, 4097, 100, 6554, u8, i64, i32, nullptr, buf, 400), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 1, N, (1ll << 21) + 1, 6554, u8, i64, i32, nullptr, buf, (size_t)1 << 40), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 1, N, 100, -1, u8, i64, i32, nullptr, buf, 400), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 1, N, 100, (1 << 28) + 1, u8, i64, i32, nullptr, buf, 400), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 2, N, 100, 6554, u8, i64, i32, nullptr, buf, 799), CP_ERR_INVALID);
  EXPECT(cp_graphcut_label(nullptr, i32, i32, i32, 1, N, 100, 6554, u8, (int64_t*)(buf + 4), i32, nullptr, buf, 400), CP_ERR_ALIGN);
  // cp_pnp_gc
  auto gc = [&](int B, int n, int iters, int mi, int M, const int32_t* gid, long long me, long long ni, int32_t w, float thr, double* pose) {
    return cp_pnp_gc(nullptr, f, 0, f, u8, 3, f, 0, i32, i32, i64, gid, M, me, ni, B, n, thr, w, iters, mi, 1u, pose, u8, i32, buf);
  };
  EXPECT(gc(0, N, 400, 6, 1, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, 4097, 400, 6, 1, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 0, 6, 1, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 513, 6, 1, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 3, 1, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 2, nullptr, 100, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, (1ll << 21) + 1, 100, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, -1, 6554, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, 100, -1, 2.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, 100, 6554, 0.f, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, 100, 6554, NAN, d), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, 100, 6554, 2.f, nullptr), CP_ERR_INVALID);
  EXPECT(gc(2, N, 400, 6, 1, nullptr, 100, 100, 6554, 2.f, (double*)(buf + 4)), CP_ERR_ALIGN);
  // the scratch query: hypothesis records + step records + cin + labels (rounded up to 8) + flows
  const long long B = 3, E = 18320;
  const long long head = B * 512 * 14 * 8 + B * 9 * 30 * 8 + B * 9 * N * 4 + B * 9 * N;
  EXPECT(cp_pnp_gc_scratch_bytes((int)B, N, E), (head + 7) / 8 * 8 + B * E * 4);
  EXPECT(cp_pnp_gc_scratch_bytes((int)B, N, 0), (head + 7) / 8 * 8 + B * 4);
  EXPECT(cp_pnp_gc_scratch_bytes(4096, 4096, 1ll << 21), 4096ll * 512 * 14 * 8 + 4096ll * 9 * 30 * 8 + 4096ll * 9 * 4096 * 5 + 4096ll * (1ll << 21) * 4);
  EXPECT(cp_pnp_gc_scratch_bytes(0, N, E), 0);
  EXPECT(cp_pnp_gc_scratch_bytes((int)B, 4097, E), 0);
  EXPECT(cp_pnp_gc_scratch_bytes((int)B, N, (1ll << 21) + 1), 0);
  EXPECT(cp_pnp_gc_scratch_bytes((int)B, N, -1), 0);
  printf("pnp_gc host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
