// The host half of csrc/scene_verify_mask.hip -- cp_verify_scene_mask: argument checks, scratch sizing -- exercised by a stand-alone
// program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc scene_verify_host_check`, then run checkerpose_amd/csrc/scene_verify_host_check).  Every call below
// returns before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; const int32_t* full; const int32_t* full_area; const int32_t* vis; const int32_t* vis_area; const int32_t* mask_ids;
    int NM, H, W; const int32_t* image_ids; int I; const int32_t* status; double delta; int P, Vmax; int32_t* counts; int32_t* boxes;
    int32_t* slot; double* score; double* iou; double* cover; double* iou_vis; double* fract; uint8_t* ok; int32_t* plane_full;
    int32_t* plane_visib; void* scratch;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, i32, i32, i32, i32, nullptr, 3, 80, 96, i32, 2, nullptr, 15.0, 3, 64, i32, i32,
                 i32, d, d, d, d, d, u8, nullptr, nullptr, buf};
  auto call = [](const A& a) {
    return cp_verify_scene_mask(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.full, a.full_area, a.vis,
                                a.vis_area, a.mask_ids, a.NM, a.H, a.W, a.image_ids, a.I, a.status, a.delta, a.P, a.Vmax, a.counts, a.boxes,
                                a.slot, a.score, a.iou, a.cover, a.iou_vis, a.fract, a.ok, a.plane_full, a.plane_visib, a.scratch);
  };
  A a;
  // null pointers (mesh_ids, mask_ids, status and the two planes may be null)
  a = okA; a.poses = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.full = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.full_area = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.vis = nullptr; EXPECT(call(a), CP_ERR_INVALID);                   // the visible masks are required here
  a = okA; a.vis_area = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.image_ids = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.counts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.boxes = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.slot = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.score = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.iou = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.cover = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.iou_vis = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.fract = nullptr; EXPECT(call(a), CP_ERR_INVALID);
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
  // the masks, the images, the planes, delta
  a = okA; a.NM = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.NM = 2; EXPECT(call(a), CP_ERR_INVALID);                          // NM != P needs mask ids
  a = okA; a.NM = 5; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.I = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.I = -2; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.plane_full = i32; EXPECT(call(a), CP_ERR_INVALID);                // one plane without the other
  a = okA; a.plane_visib = i32; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.delta = -1.0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.delta = (double)NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.delta = (double)INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.delta = 1e39; EXPECT(call(a), CP_ERR_INVALID);                    // no float32
  // alignment
  a = okA; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.score = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.iou = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.cover = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.iou_vis = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.fract = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.verts = (const float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.v_off = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.full = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.full_area = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis_area = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.mask_ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.image_ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.status = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.counts = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.boxes = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.slot = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.plane_full = (int32_t*)odd; a.plane_visib = i32; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.plane_full = i32; a.plane_visib = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  // the order of the classes: INVALID before ALIGN before RANGE
  a = okA; a.H = 0; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 4097; a.W = 4096; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  // sizes: the sums are int32
  a = okA; a.H = 4097; a.W = 4096; EXPECT(call(a), CP_ERR_RANGE);              // H * W = 2^24 + 4096
  a = okA; a.H = 4097; a.W = 4096; a.delta = 0.0; EXPECT(call(a), CP_ERR_RANGE);      // delta = 0 is no refusal
  a = okA; a.H = 1; a.W = (1 << 24) + 1; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 4096; a.W = 4096; a.P = 1 << 12; a.NM = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);      // H * W = 2^24 is allowed; 2^26 blocks are not
  a = okA; a.H = 4096; a.W = 4096; a.I = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);                      // the tile grid is per image
  a = okA; a.P = 1 << 20; a.NM = 1 << 20; a.Vmax = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);            // 2^24 vertex blocks
  EXPECT(cp_verify_scene_mask_scratch_bytes(0, 64, 1), 0);
  EXPECT(cp_verify_scene_mask_scratch_bytes(-1, 64, 1), 0);
  EXPECT(cp_verify_scene_mask_scratch_bytes(3, -1, 1), 0);
  EXPECT(cp_verify_scene_mask_scratch_bytes(3, 64, 0), 0);
  EXPECT(cp_verify_scene_mask_scratch_bytes(3, 64, 2), 576 + 3 * 64 * 16 + 256);
  EXPECT(cp_verify_scene_mask_scratch_bytes(1, 0, 1), 192 + 128);
  EXPECT(cp_verify_scene_mask_scratch_bytes(5, 3, 7), 960 + 240 + 896);
  EXPECT(cp_version() >= 241, 1);
  printf("scene_verify host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
