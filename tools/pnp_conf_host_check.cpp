// The host halves of csrc/pnp_conf.hip -- argument checks of cp_rank_correspondences and cp_pnp_conf, the scratch size -- exercised by a
// stand-alone program, so that they can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc conf_host_check`, then run checkerpose_amd/csrc/conf_host_check).  Every call below returns before any
// launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

  // cp_rank_correspondences
  struct Rk { const double* s2; const uint8_t* valid; int vs, B, N; int32_t* order; int32_t* nr; int32_t* nd; };
  const Rk rok = {d, u8, 3, 2, N, i32, i32, i32};
  auto rank = [](const Rk& r) { return cp_rank_correspondences(nullptr, r.s2, r.valid, r.vs, r.B, r.N, r.order, r.nr, r.nd); };
  Rk r;
  r = rok; r.s2 = nullptr; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.valid = nullptr; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.order = nullptr; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.nr = nullptr; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.nd = nullptr; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.B = 0; r.order = nullptr; EXPECT(rank(r), CP_ERR_INVALID);        // also with nothing to do
  r = rok; r.B = -1; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.N = 0; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.N = -5; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.N = 4097; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.vs = 0; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.vs = -3; EXPECT(rank(r), CP_ERR_INVALID);
  r = rok; r.s2 = (const double*)(buf + 4); EXPECT(rank(r), CP_ERR_ALIGN);
  r = rok; r.order = (int32_t*)(buf + 2); EXPECT(rank(r), CP_ERR_ALIGN);
  r = rok; r.nr = (int32_t*)(buf + 2); EXPECT(rank(r), CP_ERR_ALIGN);
  r = rok; r.nd = (int32_t*)(buf + 1); EXPECT(rank(r), CP_ERR_ALIGN);
  r = rok; r.B = 0; EXPECT(rank(r), CP_OK);                                    // nothing to do: returns without a launch
  r = rok; r.B = 0; r.N = 4096; EXPECT(rank(r), CP_OK);

  // cp_pnp_conf
  struct A {
    const float* p3d; long long p3d_bs; const float* p2d; const uint8_t* valid; int vs; const double* s2; const float* K; long long K_bs;
    int B, N; double chi2; int iters; uint32_t seed; int guided; double* pose; uint8_t* inl; int32_t* status; int32_t* order; int32_t* nr;
    int32_t* nd; void* scratch;
  };
  const A ok = {f, 0, f, u8, 3, d, f, 0, 2, N, 5.99, 150, 7u, 1, d, u8, i32, i32, i32, i32, buf};
  auto call = [](const A& a) {
    return cp_pnp_conf(nullptr, a.p3d, a.p3d_bs, a.p2d, a.valid, a.vs, a.s2, a.K, a.K_bs, a.B, a.N, a.chi2, a.iters, a.seed, a.guided, a.pose,
                       a.inl, a.status, a.order, a.nr, a.nd, a.scratch);
  };
  A a;
  // null pointers
  a = ok; a.p3d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p2d = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.valid = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.s2 = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.pose = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.inl = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.status = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.order = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.nr = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.nd = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.scratch = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  // shapes
  a = ok; a.B = 0; EXPECT(call(a), CP_ERR_INVALID);                            // as cp_pnp_ransac: an empty batch is refused
  a = ok; a.B = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = -3; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = 4097; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.vs = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.vs = -1; EXPECT(call(a), CP_ERR_INVALID);
  // iterations
  a = ok; a.iters = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.iters = 257; EXPECT(call(a), CP_ERR_INVALID);
  // strides
  a = ok; a.p3d_bs = 3 * N - 1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.p3d_bs = -3 * N; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K_bs = 8; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.K_bs = -9; EXPECT(call(a), CP_ERR_INVALID);
  // the gate's threshold: finite and > 0
  a = ok; a.chi2 = 0.0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.chi2 = -5.99; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.chi2 = NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.chi2 = INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.chi2 = -INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  // alignment
  a = ok; a.pose = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.scratch = buf + 4; EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.s2 = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.status = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.order = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.nr = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.nd = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  // the scratch: 256 records of 14 doubles per crop, whatever N
  EXPECT(cp_pnp_conf_scratch_bytes(3, 512), 3 * 256 * 14 * 8);
  EXPECT(cp_pnp_conf_scratch_bytes(1, 4096), 256 * 14 * 8);
  EXPECT(cp_pnp_conf_scratch_bytes(0, 512), 0);
  EXPECT(cp_pnp_conf_scratch_bytes(-2, 512), 0);
  printf("conf host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
