// The host half of csrc/vis_poses.hip -- argument checks, the CSR checks and scratch sizing of cp_vis_poses and cp_depth_diff_vis --
// exercised by a stand-alone program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc vis_host_check`, then run checkerpose_amd/csrc/vis_host_check).  Every call below is refused before
// any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal and every size as expected.
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

struct Args {
  const double* poses; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off;
  int M; const int32_t* mesh_ids; const float* colors; const float* normals; const double* surf; const int32_t* image_of_pose;
  const int32_t* img_off; const int32_t* pose_order; const int32_t* img_off_host; const int32_t* pose_order_host; const uint8_t* frames;
  int shading; double ambient; const double* light; const double* box; int resolve, draw, H, W, P, I, Vmax;
  uint8_t* vis; uint8_t* ren_rgb; float* ren_depth; int32_t* boxes; uint8_t* ok; void* scratch;
};

static int call(const Args& a) {
  return cp_vis_poses(nullptr, a.poses, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.colors, a.normals, a.surf,
                      a.image_of_pose, a.img_off, a.pose_order, a.img_off_host, a.pose_order_host, a.frames, a.shading, a.ambient, a.light,
                      a.box, a.resolve, a.draw, a.H, a.W, a.P, a.I, a.Vmax, a.vis, a.ren_rgb, a.ren_depth, a.boxes, a.ok, a.scratch);
}

int main() {
  alignas(16) static unsigned char buf[256];      // stands for every device pointer: never dereferenced by a refused call
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  const double vec[3] = {0.3, 0.3, 0.3};
  const int P = 5, I = 3;
  const int32_t off[I + 1] = {0, 2, 2, 5}, order[P] = {0, 3, 1, 2, 4};
  const Args good = {d, d, 0, f, i32, i32, i32, 2, i32, f, f, d, i32, i32, i32, off, order, u8, 1, 0.5, vec, vec, 1, 1, 40, 48, P, I, 12,
                     u8, u8, f, i32, u8, buf};
  Args a;
  // null pointers
#define NULLED(field) a = good; a.field = nullptr; EXPECT(call(a), CP_ERR_INVALID)
  NULLED(poses); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(image_of_pose); NULLED(img_off);
  NULLED(pose_order); NULLED(img_off_host); NULLED(pose_order_host); NULLED(frames); NULLED(light); NULLED(box); NULLED(vis);
  NULLED(ren_rgb); NULLED(ren_depth); NULLED(boxes); NULLED(ok); NULLED(scratch);
  NULLED(normals);                                 // phong needs them
  NULLED(mesh_ids);                                // M == 2
  // shapes and enums
#define WITH(field, value, want) a = good; a.field = value; EXPECT(call(a), want)
  WITH(P, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID);
  WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID); WITH(shading, 2, CP_ERR_INVALID);
  WITH(shading, -1, CP_ERR_INVALID); WITH(resolve, 2, CP_ERR_INVALID); WITH(draw, -1, CP_ERR_INVALID); WITH(ambient, NAN, CP_ERR_INVALID);
  WITH(ambient, INFINITY, CP_ERR_INVALID);
  const double bad_vec[3] = {0.3, NAN, 0.3};
  WITH(light, bad_vec, CP_ERR_INVALID); WITH(box, bad_vec, CP_ERR_INVALID);
  // alignment
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(poses, (const double*)(buf + 4), CP_ERR_ALIGN); WITH(surf, (const double*)(buf + 4), CP_ERR_ALIGN);
  WITH(verts, (const float*)(buf + 2), CP_ERR_ALIGN); WITH(ren_depth, (float*)(buf + 2), CP_ERR_ALIGN);
  WITH(boxes, (int32_t*)(buf + 1), CP_ERR_ALIGN); WITH(img_off, (const int32_t*)(buf + 2), CP_ERR_ALIGN);
  // the CSR
  const int32_t off_first[I + 1] = {1, 2, 2, 5}, off_last[I + 1] = {0, 2, 2, 4}, off_back[I + 1] = {0, 3, 2, 5};
  WITH(img_off_host, off_first, CP_ERR_INVALID); WITH(img_off_host, off_last, CP_ERR_INVALID); WITH(img_off_host, off_back, CP_ERR_INVALID);
  const int32_t order_hi[P] = {0, 3, 1, 2, 5}, order_lo[P] = {0, -1, 1, 2, 4};
  WITH(pose_order_host, order_hi, CP_ERR_INVALID); WITH(pose_order_host, order_lo, CP_ERR_INVALID);
  // sizes: a frame side of 2^24, a batch of 2^31 / 3 bytes, 2^24 workgroups
  WITH(W, 1 << 24, CP_ERR_RANGE);
  a = good; a.H = 4096; a.W = 4096; a.I = 64; { static int32_t big_off[65]; for (int i = 0; i < 65; ++i) big_off[i] = i == 0 ? 0 : P; a.img_off_host = big_off; EXPECT(call(a), CP_ERR_RANGE); }
  {                                                // 2^20 poses of 32 vertex chunks each
    static int32_t many_order[1 << 20];
    const int32_t one_off[2] = {0, 1 << 20};
    a = good; a.P = 1 << 20; a.I = 1; a.Vmax = 1 << 13; a.img_off_host = one_off; a.pose_order_host = many_order;
    EXPECT(call(a), CP_ERR_RANGE);
  }
  // two rules broken at once: INVALID before ALIGN, ALIGN before the CSR's INVALID, the CSR before RANGE
  a = good; a.frames = nullptr; a.verts = (const float*)(buf + 2); EXPECT(call(a), CP_ERR_INVALID);
  a = good; a.boxes = (int32_t*)(buf + 2); a.W = 1 << 24; EXPECT(call(a), CP_ERR_ALIGN);
  a = good; a.poses = (const double*)(buf + 4); a.img_off_host = off_back; EXPECT(call(a), CP_ERR_ALIGN);
  a = good; a.pose_order_host = order_hi; a.W = 1 << 24; EXPECT(call(a), CP_ERR_INVALID);
  // scratch: P headers of 48 words, four float4 tables of (P, Vmax)
  EXPECT(cp_vis_poses_scratch_bytes(5, 12, 3), 5 * 48 * 4 + 4 * 5 * 12 * 16);
  EXPECT(cp_vis_poses_scratch_bytes(3, 7, 1), 3 * 48 * 4 + 4 * 3 * 7 * 16);
  EXPECT(cp_vis_poses_scratch_bytes(0, 12, 3), 0); EXPECT(cp_vis_poses_scratch_bytes(5, -1, 3), 0); EXPECT(cp_vis_poses_scratch_bytes(5, 12, 0), 0);

  // cp_depth_diff_vis
  auto dd = [&](const float* ren, const float* dep, const int32_t* ids, int nd, double delta, double s, int H, int W, int n, uint8_t* out,
                double* stats, uint8_t* okp, void* scratch) {
    return cp_depth_diff_vis(nullptr, ren, dep, ids, nd, delta, s, H, W, n, out, stats, okp, scratch);
  };
  EXPECT(dd(nullptr, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, nullptr, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, nullptr, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, nullptr, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, nullptr, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, nullptr), CP_ERR_INVALID);
  EXPECT(dd(f, f, nullptr, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);      // no map, and neither one image nor one each
  EXPECT(dd(f, f, i32, 0, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 0, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 0, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, NAN, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.0, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd(f, f, i32, 2, 15.0, NAN, 40, 48, 3, u8, d, u8, buf), CP_ERR_INVALID);
  EXPECT(dd((const float*)(buf + 2), f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf), CP_ERR_ALIGN);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, (double*)(buf + 4), u8, buf), CP_ERR_ALIGN);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 40, 48, 3, u8, d, u8, buf + 8), CP_ERR_ALIGN);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 32768, 32768, 1, u8, d, u8, buf), CP_ERR_RANGE);
  EXPECT(dd(f, f, i32, 2, 15.0, 0.8, 1024, 1024, 1 << 14, u8, d, u8, buf), CP_ERR_RANGE);      // 2^24 workgroups
  // scratch: 8 words and 4 doubles per image, one double per (image, 1024 pixels), each part rounded up to 16 bytes
  EXPECT(cp_depth_diff_vis_scratch_bytes(3, 40, 48), 96 + 96 + 48);
  EXPECT(cp_depth_diff_vis_scratch_bytes(1, 31, 33), 32 + 32 + 16);
  EXPECT(cp_depth_diff_vis_scratch_bytes(0, 40, 48), 0); EXPECT(cp_depth_diff_vis_scratch_bytes(3, 0, 48), 0);
  printf("vis_poses host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
