// The host half of csrc/pnp_refine.hip -- argument checks -- exercised by a stand-alone program, so that it can be built under
// AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc refine_host_check`, then run
// checkerpose_amd/csrc/refine_host_check).  Every call below returns before any launch: no device is needed, nothing is loaded
// into Python.  Exit status 0 = every refusal as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0, refusals = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
    else if ((long long)(want) < 0) ++refusals;                                                     \
  } while (0)

int main() {
  alignas(16) static unsigned char buf[4096];
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  const int N = 512;
  struct A {
    const float* p3d; long long p3d_bs; const float* p2d; const uint8_t* mask; int ms; const float* K; long long K_bs; int B, N;
    const double* pose_in; const int32_t* status_in; int iters; double tol; double* pose_out; int32_t* status_out; double* info; double* rec;
  };
  const A ok = {f, 0, f, u8, 1, f, 0, 2, N, d, nullptr, 20, 1e-10, d, i32, d, nullptr};
  auto call = [](const A& a) {
    return cp_pnp_refine_lm(nullptr, a.p3d, a.p3d_bs, a.p2d, a.mask, a.ms, a.K, a.K_bs, a.B, a.N, a.pose_in, a.status_in, a.iters, a.tol,
                            a.pose_out, a.status_out, a.info, a.rec);
  };
  A a;
  // null pointers (status_in and records may be null)
  a = ok; a.p3d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p2d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.mask = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_in = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_out = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.status_out = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.info = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.B = 0; a.info = nullptr; EXPECT(call(a), CP_ERR_INVALID);          // also with nothing to do
  // shapes
  a = ok; a.B = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = -3; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = 4097; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.ms = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p3d_bs = 3 * N - 1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p3d_bs = -3 * N; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K_bs = 8; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K_bs = -9; EXPECT(call(a), CP_ERR_INVALID);
  // the iteration bound and the step tolerance
  a = ok; a.iters = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = 65; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = 0.0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = -1e-10; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  // alignment
  a = ok; a.pose_in = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.pose_out = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.info = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.rec = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.status_out = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.status_in = (const int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  // pose_out over pose_in: all of it (in place) is allowed, a part of it is not
  a = ok; a.pose_out = d + 12; EXPECT(call(a), CP_ERR_INVALID);                // B = 2: rows 1..2 over rows 0..1
  a = ok; a.pose_out = d + 1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_in = d + 23; EXPECT(call(a), CP_ERR_INVALID);
  // nothing to do: returns without a launch, in place or not, adjacent buffers do not overlap
  a = ok; a.B = 0; EXPECT(call(a), CP_OK);
  a = ok; a.B = 0; a.pose_out = d + 12; EXPECT(call(a), CP_OK);
  EXPECT(cp_pnp_refine_lm_record_doubles(), 17);
  EXPECT(cp_pnp_refine_lm_info_doubles(), 40);
  printf("pnp_refine host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
