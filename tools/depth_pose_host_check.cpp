// The host halves of csrc/pose_depth.hip -- cp_lift_correspondences and cp_pose_depth_ransac: argument checks, scratch sizing --
// exercised by a stand-alone program, so that they can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc depth_pose_host_check`, then run checkerpose_amd/csrc/depth_pose_host_check).  Every call below
// returns before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every answer as expected.
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
  alignas(16) static unsigned char buf[8192];
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  void* odd = buf + 2;

  // ---- cp_lift_correspondences
  struct A {
    const float* p2d; const uint8_t* valid; int vs; const float* K; long long kbs; const float* depth; const int32_t* ids; int I, H, W, B, N;
    float* Q; uint8_t* lifted; int32_t* n;
  };
  const A okA = {f, u8, 3, f, 0, f, nullptr, 1, 80, 96, 2, 64, f, u8, i32};
  auto callA = [](const A& a) {
    return cp_lift_correspondences(nullptr, a.p2d, a.valid, a.vs, a.K, a.kbs, a.depth, a.ids, a.I, a.H, a.W, a.B, a.N, a.Q, a.lifted, a.n);
  };
  A a;
  // null pointers (image_ids may be null)
  a = okA; a.p2d = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.valid = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.depth = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.Q = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.lifted = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.n = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  // sizes and strides
  a = okA; a.B = -1; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.N = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.N = 4097; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.vs = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.kbs = 8; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.kbs = -9; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.W = -3; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.I = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.I = 3; EXPECT(callA(a), CP_ERR_INVALID);                          // 3 images for 2 crops need ids
  // alignment
  a = okA; a.p2d = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.K = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.depth = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.Q = (float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.n = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  // ranges
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(callA(a), CP_ERR_RANGE);       // H * W = 2^31
  a = okA; a.B = 1 << 24; a.ids = i32; EXPECT(callA(a), CP_ERR_RANGE);
  // no crop: nothing to do, no launch
  a = okA; a.B = 0; EXPECT(callA(a), CP_OK);
  a = okA; a.B = 0; a.I = 5; EXPECT(callA(a), CP_OK);

  // ---- cp_pose_depth_ransac
  struct S {
    const float* p3d; long long pbs; const float* p2d; const uint8_t* valid; int vs; const float* K; long long kbs; const float* depth;
    const int32_t* ids; int I, H, W, B, N; double thr; const double* thr_b; int iters; uint32_t seed; double* pose; uint8_t* inl;
    int32_t* status; void* scratch;
  };
  const S okS = {f, 0, f, u8, 3, f, 9, f, nullptr, 2, 80, 96, 2, 512, 5.0, nullptr, 150, 7u, d, u8, i32, buf};
  auto callS = [](const S& s) {
    return cp_pose_depth_ransac(nullptr, s.p3d, s.pbs, s.p2d, s.valid, s.vs, s.K, s.kbs, s.depth, s.ids, s.I, s.H, s.W, s.B, s.N, s.thr, s.thr_b,
                                s.iters, s.seed, s.pose, s.inl, s.status, s.scratch);
  };
  S s;
  // null pointers (image_ids and dist_thresholds may be null)
  s = okS; s.p3d = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.p2d = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.valid = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.K = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.depth = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.pose = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.inl = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.status = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.scratch = nullptr; EXPECT(callS(s), CP_ERR_INVALID);
  // sizes and strides
  s = okS; s.B = -2; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.N = 0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.N = 4097; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.vs = -1; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.pbs = 3 * 512 - 1; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.kbs = 4; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.H = 0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.W = 0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.I = 0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.I = 3; EXPECT(callS(s), CP_ERR_INVALID);                          // several images need ids
  // the iteration bound, the threshold
  s = okS; s.iters = 0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.iters = 257; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.thr = 0.0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.thr = -1.0; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.thr = NAN; EXPECT(callS(s), CP_ERR_INVALID);
  s = okS; s.thr = INFINITY; EXPECT(callS(s), CP_ERR_INVALID);
  // alignment
  s = okS; s.p3d = (const float*)odd; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.p2d = (const float*)odd; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.K = (const float*)odd; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.depth = (const float*)odd; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.ids = (const int32_t*)odd; s.I = 3; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.thr_b = (const double*)(buf + 4); EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.pose = (double*)(buf + 4); EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.status = (int32_t*)odd; EXPECT(callS(s), CP_ERR_ALIGN);
  s = okS; s.scratch = buf + 4; EXPECT(callS(s), CP_ERR_ALIGN);
  // ranges
  s = okS; s.H = 1 << 16; s.W = 1 << 15; EXPECT(callS(s), CP_ERR_RANGE);
  s = okS; s.B = 1 << 24; s.ids = i32; EXPECT(callS(s), CP_ERR_RANGE);
  // no crop: nothing to do, no launch (a per-crop threshold table makes the number irrelevant)
  s = okS; s.B = 0; EXPECT(callS(s), CP_OK);
  s = okS; s.B = 0; s.thr = NAN; s.thr_b = d; EXPECT(callS(s), CP_OK);
  // scratch sizing: B * iterations * 14 and B * 4 * 14 doubles, Q, n_lifted, lifted, rounded up to 8 bytes
  EXPECT(cp_pose_depth_ransac_scratch_bytes(0, 64, 150), 0);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(2, 0, 150), 0);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(2, 4097, 150), 0);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(2, 64, 0), 0);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(2, 64, 257), 0);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(2, 64, 150), 2 * 150 * 112 + 2 * 4 * 112 + 2 * 64 * 12 + 8 + 128);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(1, 3, 1), 112 + 448 + 36 + 4 + 3 + 5);
  EXPECT(cp_pose_depth_ransac_scratch_bytes(3, 4096, 256), 3 * 256 * 112 + 3 * 448 + 3 * 4096 * 12 + 12 + 3 * 4096 + 4);
  EXPECT(cp_pose_depth_record_doubles(), 14);
  EXPECT(cp_version() >= 235, 1);
  printf("depth pose host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
