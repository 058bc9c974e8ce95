// The host halves of csrc/pnp_refine_w.hip and csrc/code_confidence.hip -- argument checks -- exercised by a stand-alone program, so
// that they can be built under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc wlm_host_check`, then run
// checkerpose_amd/csrc/wlm_host_check).  Every call below returns before any launch: no device is needed, nothing is loaded into
// Python.  Exit status 0 = every refusal as expected.
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
    const float* p3d; long long p3d_bs; const float* p2d; const uint8_t* mask; int ms; const float* scale; const float* K; long long K_bs;
    int B, N; const double* pose_in; const int32_t* status_in; double delta; int iters; double tol; double* pose_out; int32_t* status_out;
    double* info; double* rec;
  };
  const A ok = {f, 0, f, u8, 1, f, f, 0, 2, N, d, nullptr, 2.5, 20, 1e-10, d, i32, d, nullptr};
  auto call = [](const A& a) {
    return cp_pnp_refine_wlm(nullptr, a.p3d, a.p3d_bs, a.p2d, a.mask, a.ms, a.scale, a.K, a.K_bs, a.B, a.N, a.pose_in, a.status_in, a.delta,
                             a.iters, a.tol, a.pose_out, a.status_out, a.info, a.rec);
  };
  A a;
  // null pointers (status_in and records may be null)
  a = ok; a.p3d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p2d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.mask = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.scale = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_in = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_out = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.status_out = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.info = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.B = 0; a.scale = nullptr; EXPECT(call(a), CP_ERR_INVALID);         // also with nothing to do
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
  // the iteration bound, the step tolerance and the Huber threshold
  a = ok; a.iters = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = 65; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = 0.0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = -1e-10; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.tol = INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.delta = 0.0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.delta = -1.0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.delta = NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.delta = -INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  // alignment
  a = ok; a.pose_in = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.pose_out = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.info = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.rec = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.status_out = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.status_in = (const int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  // pose_out over pose_in: all of it (in place) is allowed, a part of it is not
  a = ok; a.pose_out = d + 12; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_out = d + 1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose_in = d + 23; EXPECT(call(a), CP_ERR_INVALID);
  // nothing to do: returns without a launch; +inf is a threshold
  a = ok; a.B = 0; EXPECT(call(a), CP_OK);
  a = ok; a.B = 0; a.delta = INFINITY; EXPECT(call(a), CP_OK);
  a = ok; a.B = 0; a.pose_out = d + 12; EXPECT(call(a), CP_OK);
  EXPECT(cp_pnp_refine_wlm_info_doubles(), 42);

  // cp_code_confidence
  struct Cc { const float* bits; int rows, r; const int32_t* bbox; int B, N, Hc, Wc; double floor; double* out; };
  const Cc cok = {f, 13, 6, i32, 2, N, 64, 64, 1.0 / 12.0, d};
  auto conf = [](const Cc& c) { return cp_code_confidence(nullptr, c.bits, c.rows, c.r, c.bbox, c.B, c.N, c.Hc, c.Wc, c.floor, c.out); };
  Cc c;
  c = cok; c.bits = nullptr; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.bbox = nullptr; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.out = nullptr; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.B = 0; c.out = nullptr; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.B = -1; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.N = 0; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.r = 0; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.r = 31; c.rows = 63; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.rows = 12; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.Hc = 0; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.Wc = -64; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.floor = 0.0; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.floor = -1.0; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.floor = NAN; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.floor = INFINITY; EXPECT(conf(c), CP_ERR_INVALID);
  c = cok; c.bits = (const float*)(buf + 2); EXPECT(conf(c), CP_ERR_ALIGN);
  c = cok; c.bbox = (const int32_t*)(buf + 2); EXPECT(conf(c), CP_ERR_ALIGN);
  c = cok; c.out = (double*)(buf + 4); EXPECT(conf(c), CP_ERR_ALIGN);
  c = cok; c.B = 0; EXPECT(conf(c), CP_OK);
  c = cok; c.B = 0; c.r = 30; c.rows = 61; EXPECT(conf(c), CP_OK);
  printf("wlm host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
