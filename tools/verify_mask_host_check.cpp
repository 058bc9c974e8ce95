// The host half of csrc/pose_verify_mask.hip -- cp_verify_poses_mask: argument checks, scratch sizing -- exercised by a stand-alone
// program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc verify_mask_host_check`, then run checkerpose_amd/csrc/verify_mask_host_check).  Every call below
// returns before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; const int32_t* full; const int32_t* full_area; const int32_t* vis; const int32_t* vis_area; const int32_t* mask_ids;
    int NM, H, W; const int32_t* status; int P, Vmax; int32_t* counts; int32_t* box; double* score; double* iou; double* cover; uint8_t* ok;
    uint8_t* labels; void* scratch;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, i32, i32, nullptr, nullptr, nullptr, 3, 80, 96, nullptr, 3, 64, i32, i32, d, d, d, u8, nullptr, buf};
  auto call = [](const A& a) {
    return cp_verify_poses_mask(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.full, a.full_area, a.vis,
                                a.vis_area, a.mask_ids, a.NM, a.H, a.W, a.status, a.P, a.Vmax, a.counts, a.box, a.score, a.iou, a.cover, a.ok,
                                a.labels, a.scratch);
  };
  A a;
  // null pointers (mesh_ids, the visible masks, mask_ids, status and labels may be null)
  a = okA; a.poses = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.full = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.full_area = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.counts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.box = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.score = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.iou = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.cover = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.ok = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.scratch = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  // the mesh table
  a = okA; a.verts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.v_off = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.faces = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.f_off = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 2; EXPECT(call(a), CP_ERR_INVALID);                           // several meshes need ids
  a = okA; a.Vmax = 0; EXPECT(call(a), CP_ERR_INVALID);
  // the view
  a = okA; a.ks = 3; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.W = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.P = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.P = -4; EXPECT(call(a), CP_ERR_INVALID);
  // the masks
  a = okA; a.NM = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.NM = -2; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.NM = 2; EXPECT(call(a), CP_ERR_INVALID);                          // NM != P needs mask ids
  a = okA; a.NM = 5; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.vis = i32; EXPECT(call(a), CP_ERR_INVALID);                       // the visible masks without their areas
  a = okA; a.vis_area = i32; EXPECT(call(a), CP_ERR_INVALID);                  // the areas without their masks
  // alignment
  a = okA; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.score = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.iou = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.cover = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.verts = (const float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.v_off = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.full = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.full_area = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis = (const int32_t*)odd; a.vis_area = i32; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis = i32; a.vis_area = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.mask_ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.status = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.counts = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.box = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  // the order of the classes: INVALID before ALIGN before RANGE
  a = okA; a.H = 0; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 4097; a.W = 4096; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  // sizes: the sums are int32
  a = okA; a.H = 4097; a.W = 4096; EXPECT(call(a), CP_ERR_RANGE);              // H * W = 2^24 + 4096
  a = okA; a.H = 1; a.W = (1 << 24) + 1; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 4096; a.W = 4096; a.P = 1 << 12; a.NM = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);      // H * W = 2^24 is allowed; 2^26 tile blocks are not
  a = okA; a.P = 1 << 20; a.NM = 1 << 20; a.Vmax = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);            // 2^24 vertex blocks
  EXPECT(cp_verify_poses_mask_scratch_bytes(0, 64), 0);
  EXPECT(cp_verify_poses_mask_scratch_bytes(-1, 64), 0);
  EXPECT(cp_verify_poses_mask_scratch_bytes(3, -1), 0);
  EXPECT(cp_verify_poses_mask_scratch_bytes(3, 64), 384 + 3 * 64 * 16);
  EXPECT(cp_verify_poses_mask_scratch_bytes(1, 0), 128);
  EXPECT(cp_verify_poses_mask_scratch_bytes(5, 3), 640 + 240);
  EXPECT(cp_version() >= 238, 1);
  printf("verify_mask host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
