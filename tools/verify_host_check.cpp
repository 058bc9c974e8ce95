// The host halves of csrc/pose_verify.hip -- cp_verify_poses and cp_select_poses: argument checks, scratch sizing -- exercised by a
// stand-alone program, so that they can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc verify_host_check`, then run checkerpose_amd/csrc/verify_host_check).  Every call below returns before
// any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

  // ---- cp_verify_poses
  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; const float* depth; const int32_t* img; int I, H, W; const double* tau; const int32_t* status; double w; int P, Vmax;
    int32_t* counts; double* score; double* fit; double* den; uint8_t* ok; uint8_t* labels; void* scratch;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, f, nullptr, 1, 80, 96, d, nullptr, 1.0, 3, 64, i32, d, d, d, u8, nullptr, buf};
  auto callA = [](const A& a) {
    return cp_verify_poses(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.depth, a.img, a.I, a.H, a.W, a.tau,
                           a.status, a.w, a.P, a.Vmax, a.counts, a.score, a.fit, a.den, a.ok, a.labels, a.scratch);
  };
  A a;
  // null pointers (mesh_ids, image_ids, status and labels may be null)
  a = okA; a.poses = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.depth = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.tau = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.counts = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.score = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.fit = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.den = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.ok = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.scratch = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  // the mesh table
  a = okA; a.verts = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.v_off = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.faces = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.f_off = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.M = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.M = 2; EXPECT(callA(a), CP_ERR_INVALID);                          // several meshes need ids
  a = okA; a.Vmax = 0; EXPECT(callA(a), CP_ERR_INVALID);
  // the view
  a = okA; a.ks = 3; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.W = -1; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.P = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.P = -4; EXPECT(callA(a), CP_ERR_INVALID);
  // the images
  a = okA; a.I = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.I = 2; EXPECT(callA(a), CP_ERR_INVALID);                          // several images need ids
  // the occlusion weight
  a = okA; a.w = -0.25; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.w = 1.5; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.w = NAN; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.w = INFINITY; EXPECT(callA(a), CP_ERR_INVALID);
  // alignment
  a = okA; a.scratch = buf + 8; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.tau = (const double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.score = (double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.fit = (double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.den = (double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.verts = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.v_off = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.depth = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.img = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.status = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.counts = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  // the order of the classes: INVALID before ALIGN before RANGE
  a = okA; a.H = 0; a.scratch = buf + 8; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.H = 4097; a.W = 4096; a.scratch = buf + 8; EXPECT(callA(a), CP_ERR_ALIGN);
  // sizes: 63 H W must fit an int32
  a = okA; a.H = 4097; a.W = 4096; EXPECT(callA(a), CP_ERR_RANGE);             // H * W = 2^24 + 4096
  a = okA; a.H = 1; a.W = (1 << 24) + 1; EXPECT(callA(a), CP_ERR_RANGE);
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(callA(a), CP_ERR_RANGE);
  a = okA; a.H = 4096; a.W = 4096; a.P = 1 << 12; EXPECT(callA(a), CP_ERR_RANGE);      // H * W = 2^24 is allowed; 2^26 tile blocks are not
  a = okA; a.P = 1 << 20; a.Vmax = 1 << 12; EXPECT(callA(a), CP_ERR_RANGE);            // 2^24 vertex blocks
  EXPECT(cp_verify_poses_scratch_bytes(0, 64), 0);
  EXPECT(cp_verify_poses_scratch_bytes(-1, 64), 0);
  EXPECT(cp_verify_poses_scratch_bytes(3, -1), 0);
  EXPECT(cp_verify_poses_scratch_bytes(3, 64), 384 + 3 * 64 * 16);
  EXPECT(cp_verify_poses_scratch_bytes(1, 0), 128);
  EXPECT(cp_verify_poses_scratch_bytes(5, 3), 640 + 240);

  // ---- cp_select_poses
  struct B { const double* score; const uint8_t* ok; int C, B; int32_t* choice; };
  const B okB = {d, u8, 3, 5, i32};
  auto callB = [](const B& b) { return cp_select_poses(nullptr, b.score, b.ok, b.C, b.B, b.choice); };
  B b;
  b = okB; b.score = nullptr; EXPECT(callB(b), CP_ERR_INVALID);                // (ok may be null)
  b = okB; b.choice = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.C = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.C = 65; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.C = -1; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.B = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.B = -3; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.score = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.choice = (int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.C = 0; b.choice = (int32_t*)odd; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.C = 64; b.B = 1 << 25; EXPECT(callB(b), CP_ERR_RANGE);             // C * B = 2^31
  EXPECT(cp_version() >= 236, 1);
  printf("verify host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
